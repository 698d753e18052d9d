// Ray queries (include/distraytracer.h rt_trace_rays / rt_trace_rays_device): closest hit and
// occlusion of the caller's rays. The kernels (query_kernels.h) are the render kernels' traversal
// code without shading, instantiated here, in a translation unit of their own, so that the render
// kernels' register allocation in trace.hip / render_minreg.hip is not disturbed.
// The host plumbing shared with the other units (HIP check, variant lookup, staging) is launch_common.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

// as render_minreg.hip: trace.hip alone holds the kernels trace_kernels.h defines outright
#define RT_MINREG_TU
#include "rt_internal.h"
#include "query_kernels.h"
#include "launch_common.h"

using namespace rt;

static_assert(sizeof(rt_ray) == 56 && sizeof(rt_hit) == 80 && sizeof(rt_trace_params) == 24, "ABI layout");

namespace {

// the kernels never reach the noise textures (no shading), so this unit uploads no copy of the
// per-translation-unit Perlin tables (trace_kernels.h c_perm / c_grad3; launch_common.h perlin_ready)

typedef void (*QueryFn)(SceneD, uint64_t, uint64_t, const rt_ray*, int64_t, rt_hit*, uint8_t*);
struct QueryVariant {
  uint32_t mask;
  QueryFn fn[2][2];  // [lanes][any]
};
#define QV(F)                                                                                      \
  {                                                                                                \
    F, {                                                                                           \
      {dv::query_kernel<F, true, false>, dv::query_kernel<F, true, true>}, {                       \
        dv::query_kernel<F, false, false>, dv::query_kernel<F, false, true>                        \
      }                                                                                            \
    }                                                                                              \
  }
// a query walks the specialised traversal the scene's render runs where one matches exactly, else the generic
// one (launch_common.h variant_for)
const QueryVariant kQueryVariants[] = {RT_VARIANT_MASKS(QV)};
#undef QV

// arguments checked before the scene is read or any device call is made
int check_args(const char* who, const rt_scene* s, const rt_trace_params* p, const rt_ray* rays, int64_t n, const rt_hit* hits,
               const uint8_t* occ) {
  const std::string w(who);
  if (!s) return set_error(RT_E_INVALID, w + ": null scene");
  if (!p) return set_error(RT_E_INVALID, w + ": null params");
  if (n < 0) return set_error(RT_E_INVALID, w + ": negative ray count");
  if (!rays) return set_error(RT_E_INVALID, w + ": null rays");
  if ((p->flags & RT_TRACE_ANY) && !occ) return set_error(RT_E_INVALID, w + ": RT_TRACE_ANY needs the occluded buffer");
  if (!(p->flags & RT_TRACE_ANY) && !hits) return set_error(RT_E_INVALID, w + ": a closest-hit trace needs the hits buffer");
  return RT_OK;
}

// the order entries' arguments, checked as check_args checks a trace's
int check_order_args(const char* who, const rt_scene* s, const rt_trace_params* p, const rt_ray* rays, int64_t n,
                     const uint32_t* order) {
  const std::string w(who);
  if (!s) return set_error(RT_E_INVALID, w + ": null scene");
  if (!p) return set_error(RT_E_INVALID, w + ": null params");
  if (n < 0) return set_error(RT_E_INVALID, w + ": negative ray count");
  if (n >= ((int64_t)1 << 32)) return set_error(RT_E_INVALID, w + ": the order's indices are 32-bit, the ray count must be < 2^32");
  if (!rays) return set_error(RT_E_INVALID, w + ": null rays");
  if (!order) return set_error(RT_E_INVALID, w + ": null order");
  return RT_OK;
}

// rays [0, n) of device buffers, asynchronous on st; ray i's key is firstKey + i
int launch_query(rt_scene* s, uint32_t flags, uint64_t seed, uint64_t firstKey, const rt_ray* d_rays, int64_t n, rt_hit* d_hits,
                 uint8_t* d_occ, hipStream_t st) {
  if (flags & RT_TRACE_SORT) return sorted_query(s, flags, seed, firstKey, d_rays, n, d_hits, d_occ, st);
  const SceneD sd = render_scene_view(s, render_flags_of(flags));
  const bool any = (flags & RT_TRACE_ANY) != 0;
  const QueryVariant& v = variant_for(kQueryVariants, render_variant_mask(s, render_flags_of(flags)));
  const QueryFn fn = v.fn[(flags & RT_TRACE_LANES) ? 1 : 0][any ? 1 : 0];
  constexpr int64_t SLICE = (int64_t)1 << 30;  // rays per launch: 2^24 blocks
  for (int64_t at = 0; at < n; at += SLICE) {
    const int64_t m = std::min(SLICE, n - at);
    hipLaunchKernelGGL(fn, dim3((unsigned)((m + 63) / 64)), dim3(64), dv::LDS_RENDER_BYTES, st, sd, seed, firstKey + (uint64_t)at,
                       d_rays + at, m, any ? nullptr : d_hits + at, any ? d_occ + at : nullptr);
    HIPCHK(hipGetLastError());
  }
  return RT_OK;
}

void stage_free(rt_scene* s) {
  (void)hipFree(s->traceDev);
  if (s->traceStage) (void)hipHostFree(s->traceStage);
  s->traceDev = s->traceStage = nullptr;
  s->traceCap = 0;
}

// the coherence order of device rays [0, n) into d_order, window by window: caller indices, asynchronous on st
int order_windows(rt_scene* s, const rt_ray* d_rays, int64_t n, uint32_t* d_order, hipStream_t st) {
  for (int64_t at = 0; at < n; at += s->sortWindow) {
    const int64_t m = std::min(s->sortWindow, n - at);
    const uint32_t* order = nullptr;
    const int rc = sort_order(s, d_rays + at, m, (uint32_t)at, &order, st);
    if (rc != RT_OK) return rc;
    HIPCHK(hipMemcpyAsync(d_order + at, order, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  }
  return RT_OK;
}

}  // namespace

void rt::trace_init(rt_scene* s) {
  s->traceChunk = (int64_t)1 << 18;  // 34 MB of staging; DISTRAYTRACER_TRACE_CHUNK: a testing knob
  if (const char* e = std::getenv("DISTRAYTRACER_TRACE_CHUNK")) s->traceChunk = std::max<int64_t>(64, std::atoll(e));
  // RT_TRACE_SORT: rays per sorted window (at least 64, a multiple of 64, at most 2^30) and the key's bits
  // per axis of the origin cell (1..10) and of the direction (1..16); testing / tuning knobs
  s->sortWindow = (int64_t)1 << 24;
  if (const char* e = std::getenv("DISTRAYTRACER_SORT_WINDOW"))
    s->sortWindow = std::min<int64_t>((int64_t)1 << 30, std::max<int64_t>(64, std::atoll(e))) / 64 * 64;
  s->sortOrgBits = 6;
  if (const char* e = std::getenv("DISTRAYTRACER_SORT_ORG_BITS")) s->sortOrgBits = std::min(10, std::max(1, std::atoi(e)));
  s->sortDirBits = 12;
  if (const char* e = std::getenv("DISTRAYTRACER_SORT_DIR_BITS")) s->sortDirBits = std::min(16, std::max(1, std::atoi(e)));
}

// the scene's stream and its staging buffers for min(n, chunk) rays: [cap rays][cap hits][cap bytes] on the
// device and pinned on the host (grow-only)
int rt::trace_stage(rt_scene* s, int64_t n, void** stream) {
  HIPCHK(hipSetDevice(s->device));
  hipStream_t st;
  const int rc = scene_stream(s, &st);
  if (rc != RT_OK) return rc;
  const size_t cap = (size_t)std::min<int64_t>(n, s->traceChunk);
  if (cap > s->traceCap) {
    HIPCHK(hipStreamSynchronize(st));
    stage_free(s);
    const size_t bytes = cap * (sizeof(rt_ray) + sizeof(rt_hit) + 1);
    HIPCHK(hipMalloc(&s->traceDev, bytes));
    HIPCHK(hipHostMalloc(&s->traceStage, bytes, hipHostMallocDefault));
    s->traceCap = cap;
  }
  *stream = st;
  return RT_OK;
}

void rt::trace_free(rt_scene* s) {
  stage_free(s);
  sort_free(s);
}

extern "C" {

int rt_trace_rays_device(rt_scene* s, const rt_trace_params* p, const rt_ray* d_rays, int64_t n, rt_hit* d_hits,
                         uint8_t* d_occluded, void* hip_stream) {
  int rc = check_args("rt_trace_rays_device", s, p, d_rays, n, d_hits, d_occluded);
  if (rc || n == 0) return rc;
  HIPCHK(hipSetDevice(s->device));
  return launch_query(s, p->flags, p->seed, p->first_key, d_rays, n, d_hits, d_occluded, (hipStream_t)hip_stream);
}

int rt_trace_order_device(rt_scene* s, const rt_trace_params* p, const rt_ray* d_rays, int64_t n, uint32_t* d_order,
                          void* hip_stream) {
  int rc = check_order_args("rt_trace_order_device", s, p, d_rays, n, d_order);
  if (rc || n == 0) return rc;
  HIPCHK(hipSetDevice(s->device));
  return order_windows(s, d_rays, n, d_order, (hipStream_t)hip_stream);
}

int rt_trace_order(rt_scene* s, const rt_trace_params* p, const rt_ray* rays, int64_t n, uint32_t* order) {
  const int rc = check_order_args("rt_trace_order", s, p, rays, n, order);
  if (rc || n == 0) return rc;
  return staged_chunks(  // each staging chunk is sorted on its own, its order in the chunk's hit slots
      "rt_trace_order", s, n,
      [&](const Staging& g, int64_t at, size_t m, hipStream_t st) {
        Enqueued q = {RT_OK, g.upload(rays + at, m, st)};
        if (q.e == hipSuccess) q.rc = order_windows(s, g.dev.rays, (int64_t)m, (uint32_t*)g.dev.hits, st);
        if (q.e == hipSuccess && q.rc == RT_OK) q.e = hipMemcpyAsync(g.pin.hits, g.dev.hits, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
        return q;
      },
      [&](const Staging& g, int64_t at, size_t m) {
        const uint32_t* sOut = (const uint32_t*)g.pin.hits;
        for (size_t i = 0; i < m; i++) order[at + (int64_t)i] = sOut[i] + (uint32_t)at;  // chunk-relative -> caller index
      });
}

int rt_trace_rays(rt_scene* s, const rt_trace_params* p, const rt_ray* rays, int64_t n, rt_hit* hits, uint8_t* occluded) {
  const int rc = check_args("rt_trace_rays", s, p, rays, n, hits, occluded);
  if (rc || n == 0) return rc;
  const bool any = (p->flags & RT_TRACE_ANY) != 0;  // the chunk's occlusion bytes come back in the pinned hit slots
  return staged_chunks(
      "rt_trace_rays", s, n,
      [&](const Staging& g, int64_t at, size_t m, hipStream_t st) {
        Enqueued q = {RT_OK, g.upload(rays + at, m, st)};
        if (q.e == hipSuccess)
          q.rc = launch_query(s, p->flags, p->seed, p->first_key + (uint64_t)at, g.dev.rays, (int64_t)m, g.dev.hits, g.dev.bytes, st);
        if (q.e == hipSuccess && q.rc == RT_OK)
          q.e = hipMemcpyAsync(g.pin.hits, any ? (const void*)g.dev.bytes : (const void*)g.dev.hits, any ? m : m * sizeof(rt_hit),
                               hipMemcpyDeviceToHost, st);
        return q;
      },
      [&](const Staging& g, int64_t at, size_t m) {
        if (any) std::memcpy(occluded + at, g.pin.hits, m);
        else std::memcpy(hits + at, g.pin.hits, m * sizeof(rt_hit));
      });
}

}  // extern "C"
