// Ray queries (include/distraytracer.h rt_trace_rays / rt_trace_rays_device): closest hit and
// occlusion of the caller's rays. The kernels (query_kernels.h) are the render kernels' traversal
// code without shading, instantiated here, in a translation unit of their own, so that the render
// kernels' register allocation in trace.hip / render_minreg.hip is not disturbed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

// as render_minreg.hip: trace.hip alone holds the kernels trace_kernels.h defines outright
#define RT_MINREG_TU
#include "rt_internal.h"
#include "query_kernels.h"

using namespace rt;

#define HIPCHK(expr)                                                                    \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return set_error(RT_E_HIP, std::string(#expr " failed: ") + hipGetErrorString(e_)); \
  } while (0)

static_assert(sizeof(rt_ray) == 56 && sizeof(rt_hit) == 80 && sizeof(rt_trace_params) == 24, "ABI layout");

namespace {

constexpr uint32_t F_C4 = dv::FT_PRIM | dv::FT_TRANS | dv::FT_TEX | dv::FT_LIGHTX;
// the kernels never reach the noise textures (no shading), so the per-translation-unit Perlin
// tables (trace_kernels.h c_perm / c_grad3), which only trace.hip uploads, are not read here

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
// the masks of the render's counting variants (trace.hip kCountVariants): a query walks the
// specialised traversal the scene's render runs where one matches exactly, else the generic one
const QueryVariant kQueryVariants[] = {QV(0u), QV(F_C4), QV(dv::F_C5), QV((uint32_t)dv::FT_ALL)};
#undef QV

const QueryVariant& query_variant(const rt_scene* s, uint32_t flags) {
  const uint32_t m = render_variant_mask(s, (flags & RT_TRACE_GENERIC) ? RT_RENDER_GENERIC : 0u);
  for (const QueryVariant& v : kQueryVariants)
    if (v.mask == m) return v;
  return kQueryVariants[sizeof(kQueryVariants) / sizeof(kQueryVariants[0]) - 1];
}

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
  const SceneD sd = render_scene_view(s, (flags & RT_TRACE_NOCULL) ? RT_RENDER_NOCULL : 0u);
  const bool any = (flags & RT_TRACE_ANY) != 0;
  const QueryFn fn = query_variant(s, flags).fn[(flags & RT_TRACE_LANES) ? 1 : 0][any ? 1 : 0];
  constexpr int64_t SLICE = (int64_t)1 << 30;  // rays per launch: 2^24 blocks
  for (int64_t at = 0; at < n; at += SLICE) {
    const int64_t m = std::min(SLICE, n - at);
    hipLaunchKernelGGL(fn, dim3((unsigned)((m + 63) / 64)), dim3(64), dv::LDS_RENDER_BYTES, st, sd, seed, firstKey + (uint64_t)at,
                       d_rays + at, m, any ? nullptr : d_hits + at, any ? d_occ + at : nullptr);
    HIPCHK(hipGetLastError());
  }
  return RT_OK;
}

constexpr size_t RAY_B = sizeof(rt_ray), HIT_B = sizeof(rt_hit);

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


// the scene's stream and its staging buffers for min(n, chunk) rays: [cap rays][cap hits][cap bytes] on the
// device and pinned on the host (grow-only)
int stage_ready(rt_scene* s, int64_t n, hipStream_t* out) {
  HIPCHK(hipSetDevice(s->device));
  if (!s->stream) {
    hipStream_t st;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    s->stream = st;
  }
  hipStream_t st = (hipStream_t)s->stream;
  const size_t cap = (size_t)std::min<int64_t>(n, s->traceChunk);
  if (cap > s->traceCap) {
    HIPCHK(hipStreamSynchronize(st));
    stage_free(s);
    const size_t bytes = cap * (RAY_B + HIT_B + 1);
    HIPCHK(hipMalloc(&s->traceDev, bytes));
    HIPCHK(hipHostMalloc(&s->traceStage, bytes, hipHostMallocDefault));
    s->traceCap = cap;
  }
  *out = st;
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

int rt::trace_stage(rt_scene* s, int64_t n, void** stream) {
  hipStream_t st = nullptr;
  const int rc = stage_ready(s, n, &st);
  *stream = st;
  return rc;
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
  int rc = check_order_args("rt_trace_order", s, p, rays, n, order);
  if (rc || n == 0) return rc;
  hipStream_t st;
  if ((rc = stage_ready(s, n, &st)) != RT_OK) return rc;
  const size_t C = s->traceCap;
  char *dev = (char*)s->traceDev, *stg = (char*)s->traceStage;
  rt_ray* dRays = (rt_ray*)dev;
  uint32_t* dOrder = (uint32_t*)(dev + C * RAY_B);  // the chunk's hits buffer
  const uint32_t* sOut = (const uint32_t*)(stg + C * RAY_B);
  for (int64_t at = 0; at < n; at += s->traceChunk) {  // each staging chunk is sorted on its own
    const size_t m = (size_t)std::min<int64_t>(s->traceChunk, n - at);
    std::memcpy(stg, rays + at, m * RAY_B);
    hipError_t e = hipMemcpyAsync(dRays, stg, m * RAY_B, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) rc = order_windows(s, dRays, (int64_t)m, dOrder, st);
    if (e == hipSuccess && rc == RT_OK) e = hipMemcpyAsync((void*)sOut, dOrder, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    const hipError_t se = hipStreamSynchronize(st);
    if (rc != RT_OK) return rc;
    if (e != hipSuccess) return set_error(RT_E_HIP, std::string("rt_trace_order: ") + hipGetErrorString(e));
    if (se != hipSuccess) return set_error(RT_E_HIP, std::string("rt_trace_order kernel: ") + hipGetErrorString(se));
    for (size_t i = 0; i < m; i++) order[at + (int64_t)i] = sOut[i] + (uint32_t)at;  // chunk-relative -> caller index
  }
  return RT_OK;
}

int rt_trace_rays(rt_scene* s, const rt_trace_params* p, const rt_ray* rays, int64_t n, rt_hit* hits, uint8_t* occluded) {
  int rc = check_args("rt_trace_rays", s, p, rays, n, hits, occluded);
  if (rc || n == 0) return rc;
  hipStream_t st;
  if ((rc = stage_ready(s, n, &st)) != RT_OK) return rc;
  const bool any = (p->flags & RT_TRACE_ANY) != 0;
  const size_t C = s->traceCap;
  char *dev = (char*)s->traceDev, *stg = (char*)s->traceStage;
  rt_ray* dRays = (rt_ray*)dev;
  rt_hit* dHits = (rt_hit*)(dev + C * RAY_B);
  uint8_t* dOcc = (uint8_t*)(dev + C * (RAY_B + HIT_B));
  char* sOut = stg + C * RAY_B;  // hits or occlusion bytes of the chunk
  for (int64_t at = 0; at < n; at += s->traceChunk) {
    const size_t m = (size_t)std::min<int64_t>(s->traceChunk, n - at);
    const size_t outB = any ? m : m * HIT_B;
    std::memcpy(stg, rays + at, m * RAY_B);
    hipError_t e = hipMemcpyAsync(dRays, stg, m * RAY_B, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) rc = launch_query(s, p->flags, p->seed, p->first_key + (uint64_t)at, dRays, (int64_t)m, dHits, dOcc, st);
    if (e == hipSuccess && rc == RT_OK)
      e = hipMemcpyAsync(sOut, any ? (const void*)dOcc : (const void*)dHits, outB, hipMemcpyDeviceToHost, st);
    const hipError_t se = hipStreamSynchronize(st);  // the call blocks until the chunk is in the staging buffer
    if (rc != RT_OK) return rc;
    if (e != hipSuccess) return set_error(RT_E_HIP, std::string("rt_trace_rays: ") + hipGetErrorString(e));
    if (se != hipSuccess) return set_error(RT_E_HIP, std::string("rt_trace_rays kernel: ") + hipGetErrorString(se));
    if (any) std::memcpy(occluded + at, sOut, outB);
    else std::memcpy(hits + at, sOut, outB);
  }
  return RT_OK;
}

}  // extern "C"
