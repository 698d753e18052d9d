// Host plumbing shared by the launch code of the HIP translation units (trace.hip, query.hip, ray_sort.hip,
// shade.hip, accum.hip, adaptive.hip, denoise.hip): the HIP error check, variant-table lookup, the mapping
// between RT_TRACE_* and RT_RENDER_* flags, the per-unit upload of the Perlin tables, the scene's stream, and
// the staged round trip of the host-buffer entries. Host code only: nothing here reaches a kernel. Included
// after the unit's kernels header, with `using namespace rt` in effect where HIPCHK is used.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>

#include "rt_internal.h"

#define HIPCHK(expr)                                                                    \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return set_error(RT_E_HIP, std::string(#expr " failed: ") + hipGetErrorString(e_)); \
  } while (0)

// The feature masks every unit outside the render's own table (trace.hip kVariants) specialises its kernels
// for: none, C4's, C5's, all. X is the unit's table-entry macro, so the tables cannot drift apart.
#define RT_VARIANT_MASKS(X) X(0u), X(dv::F_C4), X(dv::F_C5), X((uint32_t)dv::FT_ALL)

namespace rt {
namespace {

// the table entry specialised for exactly `mask`, else the last one (the generic kernel)
template <class V, size_t N>
const V& variant_for(const V (&table)[N], uint32_t mask) {
  for (const V& v : table)
    if (v.mask == mask) return v;
  return table[N - 1];
}

// RT_TRACE_GENERIC / RT_TRACE_NOCULL as the RT_RENDER_* flags render_variant_mask and render_scene_view take, and back
constexpr uint32_t render_flags_of(uint32_t trace_flags) {
  return ((trace_flags & RT_TRACE_GENERIC) ? RT_RENDER_GENERIC : 0u) | ((trace_flags & RT_TRACE_NOCULL) ? RT_RENDER_NOCULL : 0u);
}
constexpr uint32_t trace_flags_of(uint32_t render_flags) {
  return ((render_flags & RT_RENDER_GENERIC) ? RT_TRACE_GENERIC : 0u) | ((render_flags & RT_RENDER_NOCULL) ? RT_TRACE_NOCULL : 0u);
}

#ifdef RT_UNIT_SHADES
// The Perlin tables (trace_kernels.h c_perm / c_grad3) are per translation unit. A unit whose kernels reach the
// noise textures defines RT_UNIT_SHADES and uploads its own copy once per device, before its first launch there
// (the current device is the scene's). The numbers are trace.hip's, which uploads its copy at scene creation.
int perlin_ready(int device) {
  static std::mutex mu;
  static bool done[64] = {};
  std::lock_guard<std::mutex> lk(mu);
  if (device >= 0 && device < 64 && done[device]) return RT_OK;
  const int *perm = nullptr, *grad3 = nullptr;
  perlin_tables(&perm, &grad3);
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(dv::c_perm), perm, sizeof(int) * 256));
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(dv::c_grad3), grad3, sizeof(int) * 36));
  if (device >= 0 && device < 64) done[device] = true;
  return RT_OK;
}
#endif

// the scene's own non-blocking stream, created on first use (the current device is the scene's)
int scene_stream(rt_scene* s, hipStream_t* out) {
  if (!s->stream) {
    hipStream_t st;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    s->stream = st;
  }
  *out = (hipStream_t)s->stream;
  return RT_OK;
}

// The tail of a blocking entry: wait for the stream whatever was enqueued, then report the first of the entry's
// own error (rc, already recorded), the enqueue's (e) and the kernels' (what the wait returned).
int sync_report(hipStream_t st, int rc, hipError_t e, const std::string& enqueueWho, const std::string& kernelWho) {
  const hipError_t se = hipStreamSynchronize(st);
  if (rc != RT_OK) return rc;
  if (e != hipSuccess) return set_error(RT_E_HIP, enqueueWho + hipGetErrorString(e));
  if (se != hipSuccess) return set_error(RT_E_HIP, kernelWho + hipGetErrorString(se));
  return RT_OK;
}

// rt_trace_rays' staging (query.hip trace_stage) as typed pointers: [cap rays][cap hits][cap bytes], cap =
// traceCap, on the device and pinned on the host. The hit slots also carry an order's indices and colours.
struct Staging {
  struct View {
    rt_ray* rays;
    rt_hit* hits;
    uint8_t* bytes;
  } dev, pin;
  static View view(void* base, size_t cap) {
    char* p = (char*)base;
    return {(rt_ray*)p, (rt_hit*)(p + cap * sizeof(rt_ray)), (uint8_t*)(p + cap * (sizeof(rt_ray) + sizeof(rt_hit)))};
  }
  explicit Staging(const rt_scene* s) : dev(view(s->traceDev, s->traceCap)), pin(view(s->traceStage, s->traceCap)) {}
  // the caller's rays into the pinned rays, and those to the device
  hipError_t upload(const rt_ray* rays, size_t m, hipStream_t st) const {
    std::memcpy(pin.rays, rays, m * sizeof(rt_ray));
    return hipMemcpyAsync(dev.rays, pin.rays, m * sizeof(rt_ray), hipMemcpyHostToDevice, st);
  }
};

// what enqueueing one chunk gave: the launch code's own status and the last copy's
struct Enqueued {
  int rc;
  hipError_t e;
};

// The staged round trip of a host-buffer entry `who` over n items, traceChunk at a time on the scene's stream:
// enqueue(g, at, m, st) queues the chunk's input copy, launches and output copies and returns an Enqueued; the
// chunk is waited for (sync_report); deliver(g, at, m) copies it from the pinned staging to the caller.
template <class Enqueue, class Deliver>
int staged_chunks(const char* who, rt_scene* s, int64_t n, Enqueue enqueue, Deliver deliver) {
  void* stv = nullptr;
  int rc = trace_stage(s, n, &stv);
  if (rc != RT_OK) return rc;
  hipStream_t st = (hipStream_t)stv;
  const Staging g(s);
  const std::string w(who);
  for (int64_t at = 0; at < n; at += s->traceChunk) {
    const size_t m = (size_t)std::min<int64_t>(s->traceChunk, n - at);
    const Enqueued q = enqueue(g, at, m, st);
    if ((rc = sync_report(st, q.rc, q.e, w + ": ", w + " kernel: ")) != RT_OK) return rc;
    deliver(g, at, m);
  }
  return RT_OK;
}

}  // namespace
}  // namespace rt
