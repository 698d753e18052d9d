// Radiance queries and camera rays (include/distraytracer.h rt_shade_rays / rt_shade_rays_device,
// rt_camera_rays / rt_camera_rays_device). The kernels (shade_kernels.h) run the render kernel's shading
// tree (trace_sample) on the caller's rays, one ray per lane, and restate its camera code as a ray
// emitter. They are instantiated here, in a translation unit of their own, so that the register allocation
// of the render and query kernels in the other units is not disturbed.
// The host plumbing shared with the other units (HIP check, variant lookup, staging) is launch_common.h's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

// as render_minreg.hip: trace.hip alone holds the kernels trace_kernels.h defines outright
#define RT_MINREG_TU
#include "rt_internal.h"
#include "comm.h"
#include "shade_kernels.h"
#define RT_UNIT_SHADES  // the kernels reach the noise textures: this unit uploads its own Perlin tables
#include "launch_common.h"

using namespace rt;

static_assert(sizeof(rt_shade_params) == 24, "ABI layout");
// rt_trace_rays' staging holds, per ray, a ray, a hit record and a byte: a colour fits the hit record's place
static_assert(3 * sizeof(double) <= sizeof(rt_hit), "the staging's hit slots hold the colours");

namespace {

constexpr uint32_t SHADE_FLAGS = RT_TRACE_NOCULL | RT_TRACE_GENERIC | RT_TRACE_SORT;

typedef void (*ShadeFn)(SceneD, uint64_t, uint64_t, uint32_t, const rt_ray*, int64_t, double*, uint8_t*);
typedef void (*ShadeIdxFn)(SceneD, uint64_t, uint64_t, uint32_t, const rt_ray*, int64_t, double*, uint8_t*, const uint32_t*);
struct ShadeVariant {
  uint32_t mask;
  ShadeFn fn;
  ShadeIdxFn idx;
};
#define SV(F) {F, dv::shade_kernel<F>, dv::shade_kernel_idx<F>}
// the specialised shading tree the scene's render runs where one matches exactly, else the generic one
// (launch_common.h variant_for)
const ShadeVariant kShadeVariants[] = {RT_VARIANT_MASKS(SV)};
#undef SV

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
  const SceneD sd = render_scene_view(s, render_flags_of(p->flags));
  const ShadeVariant& v = variant_for(kShadeVariants, render_variant_mask(s, render_flags_of(p->flags)));
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

// pose: the rows of a valid camera pose, or nullptr for the camera as it is (the kernel without one)
int launch_camera(const rt_scene* s, const ParamsD& P, int sample, int64_t first, int64_t count, rt_ray* d_rays, const double* pose,
                  hipStream_t st) {
  const dim3 grid((unsigned)((count + 255) / 256));
  if (pose) {
    hipLaunchKernelGGL(dv::camera_rays_kernel<true>, grid, dim3(256), 0, st, s->dev, P, sample, first, count, d_rays, pose_args(pose));
  } else {
    hipLaunchKernelGGL(dv::camera_rays_kernel<false>, grid, dim3(256), 0, st, s->dev, P, sample, first, count, d_rays);
  }
  HIPCHK(hipGetLastError());
  return RT_OK;
}

// a posed camera entry's pose, checked before the scene is read
int check_pose(const char* who, const double* pose) {
  const char* why = pose_invalid(pose);
  return why ? set_error(RT_E_INVALID, std::string(who) + ": " + why) : RT_OK;
}

constexpr int64_t CAMERA_SLICE = (int64_t)1 << 30;  // rays per launch: 2^22 blocks

// the frame's rays into a device buffer, asynchronous on st
int camera_device(rt_scene* s, const ParamsD& P, int sample, const double* pose, rt_ray* d_rays, hipStream_t st) {
  HIPCHK(hipSetDevice(s->device));
  const int64_t n = (int64_t)P.W * P.H;
  for (int64_t at = 0; at < n; at += CAMERA_SLICE) {
    const int rc = launch_camera(s, P, sample, at, std::min(CAMERA_SLICE, n - at), d_rays + at, pose, st);
    if (rc != RT_OK) return rc;
  }
  return RT_OK;
}

// the frame's rays into a host buffer through the scene's staging, blocking
int camera_host(const char* who, rt_scene* s, const ParamsD& P, int sample, const double* pose, rt_ray* rays) {
  const int64_t n = (int64_t)P.W * P.H;
  return staged_chunks(
      who, s, n,
      [&](const Staging& g, int64_t at, size_t m, hipStream_t st) {
        Enqueued q = {launch_camera(s, P, sample, at, (int64_t)m, g.dev.rays, pose, st), hipSuccess};
        if (q.rc == RT_OK) q.e = hipMemcpyAsync(g.pin.rays, g.dev.rays, m * sizeof(rt_ray), hipMemcpyDeviceToHost, st);
        return q;
      },
      [&](const Staging& g, int64_t at, size_t m) { std::memcpy(rays + at, g.pin.rays, m * sizeof(rt_ray)); });
}

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
  return staged_chunks(  // with RT_TRACE_SORT each staging chunk is sorted on its own; the colours travel in the hit slots
      "rt_shade_rays", s, n,
      [&](const Staging& g, int64_t at, size_t m, hipStream_t st) {
        Enqueued q = {RT_OK, g.upload(rays + at, m, st)};
        if (q.e == hipSuccess)
          q.rc = launch_shade(s, p, p->first_key + (uint64_t)at, g.dev.rays, (int64_t)m, (double*)g.dev.hits, g.dev.bytes, st);
        if (q.e == hipSuccess && q.rc == RT_OK) q.e = hipMemcpyAsync(g.pin.hits, g.dev.hits, m * 3 * sizeof(double), hipMemcpyDeviceToHost, st);
        if (q.e == hipSuccess && q.rc == RT_OK) q.e = hipMemcpyAsync(g.pin.bytes, g.dev.bytes, m, hipMemcpyDeviceToHost, st);
        return q;
      },
      [&](const Staging& g, int64_t at, size_t m) {
        std::memcpy(rgb + 3 * at, g.pin.hits, m * 3 * sizeof(double));
        if (status) std::memcpy(status + at, g.pin.bytes, m);
      });
}

int rt_camera_rays_device(rt_scene* s, const rt_render_params* p, int sample, rt_ray* d_rays, void* hip_stream) {
  ParamsD P;
  const int rc = camera_params("rt_camera_rays_device", s, p, sample, d_rays, P);
  if (rc) return rc;
  return camera_device(s, P, sample, nullptr, d_rays, (hipStream_t)hip_stream);
}

int rt_camera_rays(rt_scene* s, const rt_render_params* p, int sample, rt_ray* rays) {
  ParamsD P;
  const int rc = camera_params("rt_camera_rays", s, p, sample, rays, P);
  if (rc) return rc;
  return camera_host("rt_camera_rays", s, P, sample, nullptr, rays);
}

int rt_camera_rays_pose_device(rt_scene* s, const rt_render_params* p, int sample, const double* pose, rt_ray* d_rays,
                               void* hip_stream) {
  if (!pose) return rt_camera_rays_device(s, p, sample, d_rays, hip_stream);
  ParamsD P;
  int rc = check_pose("rt_camera_rays_pose_device", pose);
  if (rc || (rc = camera_params("rt_camera_rays_pose_device", s, p, sample, d_rays, P)) != RT_OK) return rc;
  DeviceGuard dg;
  return camera_device(s, P, sample, pose, d_rays, (hipStream_t)hip_stream);
}

int rt_camera_rays_pose(rt_scene* s, const rt_render_params* p, int sample, const double* pose, rt_ray* rays) {
  if (!pose) return rt_camera_rays(s, p, sample, rays);
  ParamsD P;
  int rc = check_pose("rt_camera_rays_pose", pose);
  if (rc || (rc = camera_params("rt_camera_rays_pose", s, p, sample, rays, P)) != RT_OK) return rc;
  DeviceGuard dg;
  return camera_host("rt_camera_rays_pose", s, P, sample, pose, rays);
}

}  // extern "C"
