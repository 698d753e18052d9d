// Radiance queries and camera rays (include/distraytracer.h rt_shade_rays / rt_shade_rays_device,
// rt_camera_rays / rt_camera_rays_device). The kernels (shade_kernels.h) run the render kernel's shading
// tree (trace_sample) on the caller's rays, one ray per lane, and restate its camera code as a ray
// emitter. They are instantiated here, in a translation unit of their own, so that the register allocation
// of the render and query kernels in the other units is not disturbed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>

// as render_minreg.hip: trace.hip alone holds the kernels trace_kernels.h defines outright
#define RT_MINREG_TU
#include "rt_internal.h"
#include "shade_kernels.h"

using namespace rt;

#define HIPCHK(expr)                                                                    \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return set_error(RT_E_HIP, std::string(#expr " failed: ") + hipGetErrorString(e_)); \
  } while (0)

static_assert(sizeof(rt_shade_params) == 24, "ABI layout");
// rt_trace_rays' staging holds, per ray, a ray, a hit record and a byte: a colour fits the hit record's place
static_assert(3 * sizeof(double) <= sizeof(rt_hit), "the staging's hit slots hold the colours");

namespace {

constexpr uint32_t F_C4 = dv::FT_PRIM | dv::FT_TRANS | dv::FT_TEX | dv::FT_LIGHTX;
constexpr uint32_t SHADE_FLAGS = RT_TRACE_NOCULL | RT_TRACE_GENERIC | RT_TRACE_SORT;

typedef void (*ShadeFn)(SceneD, uint64_t, uint64_t, uint32_t, const rt_ray*, int64_t, double*, uint8_t*);
typedef void (*ShadeIdxFn)(SceneD, uint64_t, uint64_t, uint32_t, const rt_ray*, int64_t, double*, uint8_t*, const uint32_t*);
struct ShadeVariant {
  uint32_t mask;
  ShadeFn fn;
  ShadeIdxFn idx;
};
#define SV(F) {F, dv::shade_kernel<F>, dv::shade_kernel_idx<F>}
// the masks of query.hip's kQueryVariants, picked by the same rule: the specialised shading tree the scene's
// render runs where one matches exactly, else the generic one
const ShadeVariant kShadeVariants[] = {SV(0u), SV(F_C4), SV(dv::F_C5), SV((uint32_t)dv::FT_ALL)};
#undef SV

const ShadeVariant& shade_variant(const rt_scene* s, uint32_t flags) {
  const uint32_t m = render_variant_mask(s, (flags & RT_TRACE_GENERIC) ? RT_RENDER_GENERIC : 0u);
  for (const ShadeVariant& v : kShadeVariants)
    if (v.mask == m) return v;
  return kShadeVariants[sizeof(kShadeVariants) / sizeof(kShadeVariants[0]) - 1];
}

// The Perlin tables (trace_kernels.h c_perm / c_grad3) are per translation unit, and this one reaches the
// noise textures: its copy is uploaded once per device, before the first launch there (the current device
// is the scene's). The numbers are trace.hip's.
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

// arguments checked before the scene is read or any device call is made
int check_shade_args(const char* who, const rt_scene* s, const rt_shade_params* p, const rt_ray* rays, int64_t n,
                     const double* rgb) {
  const std::string w(who);
  if (!s) return set_error(RT_E_INVALID, w + ": null scene");
  if (!p) return set_error(RT_E_INVALID, w + ": null params");
  if (n < 0) return set_error(RT_E_INVALID, w + ": negative ray count");
  if (!rays) return set_error(RT_E_INVALID, w + ": null rays");
  if (!rgb) return set_error(RT_E_INVALID, w + ": null rgb");
  if (p->flags & RT_TRACE_ANY) return set_error(RT_E_INVALID, w + ": RT_TRACE_ANY is an occlusion query (rt_trace_rays), not a radiance query");
  if (p->flags & RT_TRACE_LANES)
    return set_error(RT_E_INVALID, w + ": RT_TRACE_LANES is not available, the shading tree is compiled for the packet traversal");
  if (p->flags & ~SHADE_FLAGS) return set_error(RT_E_INVALID, w + ": unknown flag bits");
  return RT_OK;
}

// what every shade call does before its first launch: the scene's device, the photon map a scene that uses
// one needs (built on demand with the call's seed, prepare_render's rule), this unit's noise tables
int shade_ready(rt_scene* s, const rt_shade_params* p) {
  HIPCHK(hipSetDevice(s->device));
  if (s->hs.photonMode && !s->photonsUploaded) {
    const int rc = rt_photons_build(s, p->seed);
    if (rc) return rc;
  }
  return perlin_ready(s->device);
}

// rays [0, n) of device buffers, asynchronous on st; ray i's key is {seed, firstKey + i, sample}
int launch_shade(rt_scene* s, const rt_shade_params* p, uint64_t firstKey, const rt_ray* d_rays, int64_t n, double* d_rgb,
                 uint8_t* d_status, hipStream_t st) {
  const SceneD sd = render_scene_view(s, (p->flags & RT_TRACE_NOCULL) ? RT_RENDER_NOCULL : 0u);
  const ShadeVariant& v = shade_variant(s, p->flags);
  if (p->flags & RT_TRACE_SORT) {
    // windows are independent: indices, keys and results are relative to the window's first ray
    for (int64_t at = 0; at < n; at += s->sortWindow) {
      const int64_t m = std::min(s->sortWindow, n - at);
      const uint32_t* order = nullptr;
      const int rc = sort_order(s, d_rays + at, m, 0u, &order, st);
      if (rc != RT_OK) return rc;
      hipLaunchKernelGGL(v.idx, dim3((unsigned)((m + 63) / 64)), dim3(64), dv::LDS_RENDER_BYTES, st, sd, p->seed,
                         firstKey + (uint64_t)at, p->sample, d_rays + at, m, d_rgb + 3 * at, d_status ? d_status + at : nullptr,
                         order);
      HIPCHK(hipGetLastError());
    }
    return RT_OK;
  }
  constexpr int64_t SLICE = (int64_t)1 << 30;  // rays per launch: 2^24 blocks
  for (int64_t at = 0; at < n; at += SLICE) {
    const int64_t m = std::min(SLICE, n - at);
    hipLaunchKernelGGL(v.fn, dim3((unsigned)((m + 63) / 64)), dim3(64), dv::LDS_RENDER_BYTES, st, sd, p->seed,
                       firstKey + (uint64_t)at, p->sample, d_rays + at, m, d_rgb + 3 * at, d_status ? d_status + at : nullptr);
    HIPCHK(hipGetLastError());
  }
  return RT_OK;
}

// the camera entries' arguments and the frame's kernel parameters (the render's own: prepare_render)
int camera_params(const char* who, rt_scene* s, const rt_render_params* p, int sample, const rt_ray* rays, ParamsD& P) {
  const std::string w(who);
  if (!s) return set_error(RT_E_INVALID, w + ": null scene");
  if (!p) return set_error(RT_E_INVALID, w + ": null params");
  if (!rays) return set_error(RT_E_INVALID, w + ": null rays");
  rt_render_params q = *p;
  q.flags = 0;
  const int rc = prepare_render(s, &q, P);
  if (rc) return set_error(rc, w + ": " + rt_last_error());
  if (P.row0 != 0 || P.nrows != P.H || P.rowStep != 1 || P.band != 1) return set_error(RT_E_INVALID, w + ": whole-frame layouts only");
  if (sample < 0 || sample >= P.spp) return set_error(RT_E_INVALID, w + ": sample index outside [0, spp)");
  return RT_OK;
}

int launch_camera(const rt_scene* s, const ParamsD& P, int sample, int64_t first, int64_t count, rt_ray* d_rays, hipStream_t st) {
  hipLaunchKernelGGL(dv::camera_rays_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, s->dev, P, sample, first,
                     count, d_rays);
  HIPCHK(hipGetLastError());
  return RT_OK;
}

constexpr size_t RAY_B = sizeof(rt_ray), HIT_B = sizeof(rt_hit);
constexpr int64_t CAMERA_SLICE = (int64_t)1 << 30;  // rays per launch: 2^22 blocks

}  // namespace

extern "C" {

int rt_shade_rays_device(rt_scene* s, const rt_shade_params* p, const rt_ray* d_rays, int64_t n, double* d_rgb,
                         uint8_t* d_status, void* hip_stream) {
  int rc = check_shade_args("rt_shade_rays_device", s, p, d_rays, n, d_rgb);
  if (rc || n == 0) return rc;
  if ((rc = shade_ready(s, p)) != RT_OK) return rc;
  return launch_shade(s, p, p->first_key, d_rays, n, d_rgb, d_status, (hipStream_t)hip_stream);
}

int rt_shade_rays(rt_scene* s, const rt_shade_params* p, const rt_ray* rays, int64_t n, double* rgb, uint8_t* status) {
  int rc = check_shade_args("rt_shade_rays", s, p, rays, n, rgb);
  if (rc || n == 0) return rc;
  if ((rc = shade_ready(s, p)) != RT_OK) return rc;
  void* stv = nullptr;
  if ((rc = trace_stage(s, n, &stv)) != RT_OK) return rc;
  hipStream_t st = (hipStream_t)stv;
  const size_t C = s->traceCap;
  char *dev = (char*)s->traceDev, *stg = (char*)s->traceStage;
  rt_ray* dRays = (rt_ray*)dev;
  double* dRgb = (double*)(dev + C * RAY_B);  // the chunk's hits buffer
  uint8_t* dStatus = (uint8_t*)(dev + C * (RAY_B + HIT_B));
  const char* sRgb = stg + C * RAY_B;
  const char* sStatus = stg + C * (RAY_B + HIT_B);
  for (int64_t at = 0; at < n; at += s->traceChunk) {  // with RT_TRACE_SORT each staging chunk is sorted on its own
    const size_t m = (size_t)std::min<int64_t>(s->traceChunk, n - at);
    std::memcpy(stg, rays + at, m * RAY_B);
    hipError_t e = hipMemcpyAsync(dRays, stg, m * RAY_B, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) rc = launch_shade(s, p, p->first_key + (uint64_t)at, dRays, (int64_t)m, dRgb, dStatus, st);
    if (e == hipSuccess && rc == RT_OK) e = hipMemcpyAsync((void*)sRgb, dRgb, m * 3 * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && rc == RT_OK) e = hipMemcpyAsync((void*)sStatus, dStatus, m, hipMemcpyDeviceToHost, st);
    const hipError_t se = hipStreamSynchronize(st);  // the call blocks until the chunk is in the staging buffer
    if (rc != RT_OK) return rc;
    if (e != hipSuccess) return set_error(RT_E_HIP, std::string("rt_shade_rays: ") + hipGetErrorString(e));
    if (se != hipSuccess) return set_error(RT_E_HIP, std::string("rt_shade_rays kernel: ") + hipGetErrorString(se));
    std::memcpy(rgb + 3 * at, sRgb, m * 3 * sizeof(double));
    if (status) std::memcpy(status + at, sStatus, m);
  }
  return RT_OK;
}

int rt_camera_rays_device(rt_scene* s, const rt_render_params* p, int sample, rt_ray* d_rays, void* hip_stream) {
  ParamsD P;
  int rc = camera_params("rt_camera_rays_device", s, p, sample, d_rays, P);
  if (rc) return rc;
  HIPCHK(hipSetDevice(s->device));
  const int64_t n = (int64_t)P.W * P.H;
  for (int64_t at = 0; at < n; at += CAMERA_SLICE)
    if ((rc = launch_camera(s, P, sample, at, std::min(CAMERA_SLICE, n - at), d_rays + at, (hipStream_t)hip_stream)) != RT_OK) return rc;
  return RT_OK;
}

int rt_camera_rays(rt_scene* s, const rt_render_params* p, int sample, rt_ray* rays) {
  ParamsD P;
  int rc = camera_params("rt_camera_rays", s, p, sample, rays, P);
  if (rc) return rc;
  const int64_t n = (int64_t)P.W * P.H;
  void* stv = nullptr;
  if ((rc = trace_stage(s, n, &stv)) != RT_OK) return rc;
  hipStream_t st = (hipStream_t)stv;
  rt_ray* dRays = (rt_ray*)s->traceDev;
  for (int64_t at = 0; at < n; at += s->traceChunk) {
    const size_t m = (size_t)std::min<int64_t>(s->traceChunk, n - at);
    rc = launch_camera(s, P, sample, at, (int64_t)m, dRays, st);
    hipError_t e = hipSuccess;
    if (rc == RT_OK) e = hipMemcpyAsync(s->traceStage, dRays, m * RAY_B, hipMemcpyDeviceToHost, st);
    const hipError_t se = hipStreamSynchronize(st);
    if (rc != RT_OK) return rc;
    if (e != hipSuccess) return set_error(RT_E_HIP, std::string("rt_camera_rays: ") + hipGetErrorString(e));
    if (se != hipSuccess) return set_error(RT_E_HIP, std::string("rt_camera_rays kernel: ") + hipGetErrorString(se));
    std::memcpy(rays + at, s->traceStage, m * RAY_B);
  }
  return RT_OK;
}

}  // extern "C"
