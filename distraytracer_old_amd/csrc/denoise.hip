// The denoise step of a progressive frame (include/distraytracer.h rt_denoise_*): an edge-avoiding a-trous
// wavelet filter over an accumulator's mean, its colour edge-stop scaled by the per-pixel variance of the mean,
// guided by the normal, position, depth and material of exactly the frame's centre rays. The guides come from
// the entries a host would use (rt_camera_rays_device, rt_trace_rays_device); the kernels (denoise_kernels.h)
// live in this translation unit alone, which includes nothing of the render kernels.
// The HIP check and the flag mapping are launch_common.h's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rt_internal.h"
#include "comm.h"
#include "accum_state.h"
#include "denoise_kernels.h"
#include "launch_common.h"

using namespace rt;

// The argument checks of the run entries read nothing of this struct: tests hand them a zeroed host-made one.
struct rt_denoise {
  rt_accum* a;
  int32_t W, H;
  dn::GuideN* gn;     // device [W * H]
  dn::GuideP* gp;     // device [W * H]
  dn::Plane* buf[2];  // device [W * H] each: the ping-pong planes
  float* orgb;        // device [3 * W * H]: rt_denoise_run's frame before its read-back
  int32_t* oargb;     // device [W * H]
  int32_t final_;     // the buffer that holds the last run's planes, -1 before any run
  void* last;         // hipStream_t of the last run
  rt_ray* srays;      // device [W * H] and
  rt_hit* shits;      // device [W * H]: the guide build's staging, kept from the first rt_denoise_rebuild on
  uint64_t pose_gen;  // the accumulator's pose_gen the guides were traced under (rt_accum_set_camera moves it on)
};

// tests/test_denoise_abi.py points a host-made denoiser at a host-made accumulator through this field
static_assert(__builtin_offsetof(rt_denoise, a) == 0, "rt_denoise's checked field");

namespace {

int64_t pixels(const rt_denoise* d) { return (int64_t)d->W * d->H; }
unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

void free_buffers(rt_denoise* d) {
  (void)hipFree(d->gn);
  (void)hipFree(d->gp);
  (void)hipFree(d->buf[0]);
  (void)hipFree(d->buf[1]);
  (void)hipFree(d->orgb);
  (void)hipFree(d->oargb);
  (void)hipFree(d->srays);
  (void)hipFree(d->shits);
}

// Traces the frame's centre rays, under the accumulator's camera pose if it has one, and packs the guides, on
// st and waited for. The ray and hit staging
// (56 + 80 bytes per pixel) lives only for the duration of the build, unless `keep`: then the denoiser's own
// is used, allocated here the first time, so that a host that moves the camera every frame pays for it once.
int build_guides(rt_denoise* d, hipStream_t st, const std::string& w, bool keep) {
  rt_accum* a = d->a;
  rt_scene* s = a->scene;
  const int64_t n = pixels(d);
  rt_ray* rays = d->srays;
  rt_hit* hits = d->shits;
  hipError_t e = rays ? hipSuccess : hipMalloc(&rays, (size_t)n * sizeof(rt_ray));
  if (e == hipSuccess && !hits) e = hipMalloc(&hits, (size_t)n * sizeof(rt_hit));
  if (keep) {
    d->srays = rays;
    d->shits = hits;
  }
  int rc = e == hipSuccess ? RT_OK : set_error(RT_E_HIP, w + ": " + hipGetErrorString(e));
  if (rc == RT_OK) {
    rt_render_params q = a->rp;
    q.spp = 1;  // the un-jittered centre ray; in a scene with a lens the one lens ray of sample 0
    rt_trace_params tp;
    std::memset(&tp, 0, sizeof(tp));
    tp.seed = a->rp.seed;
    tp.first_key = 0;
    tp.flags = trace_flags_of(a->rp.flags);
    rc = rt_camera_rays_pose_device(s, &q, 0, a->has_pose ? a->pose : nullptr, rays, st);
    if (rc == RT_OK) rc = rt_trace_rays_device(s, &tp, rays, n, hits, nullptr, st);
    if (rc != RT_OK) rc = set_error(rc, w + ": " + rt_last_error());
  }
  if (rc == RT_OK) {
    hipLaunchKernelGGL(dn::guide_pack_kernel, dim3(blocks256(n)), dim3(256), 0, st, rays, hits, n, d->gn, d->gp);
    e = hipGetLastError();
    if (e != hipSuccess) rc = set_error(RT_E_HIP, w + ": " + hipGetErrorString(e));
  }
  const hipError_t se = hipStreamSynchronize(st);
  if (!d->srays) (void)hipFree(rays);
  if (!d->shits) (void)hipFree(hits);
  if (rc == RT_OK && se != hipSuccess) rc = set_error(RT_E_HIP, w + ": " + hipGetErrorString(se));
  if (rc == RT_OK) d->pose_gen = a->pose_gen;
  return rc;
}

int check_run(const std::string& w, const rt_denoise* d, const rt_denoise_params* p) {
  if (!d) return set_error(RT_E_INVALID, w + ": null denoiser");
  if (!p) return set_error(RT_E_INVALID, w + ": null params");
  if (p->levels < 0 || p->levels > 8) return set_error(RT_E_INVALID, w + ": levels outside 0 .. 8");
  if (p->normal_log2 < 0 || p->normal_log2 > 10) return set_error(RT_E_INVALID, w + ": normal_log2 outside 0 .. 10");
  if (!(p->sigma_l > 0) || !std::isfinite(p->sigma_l)) return set_error(RT_E_INVALID, w + ": sigma_l must be positive and finite");
  if (!(p->sigma_z > 0) || !std::isfinite(p->sigma_z)) return set_error(RT_E_INVALID, w + ": sigma_z must be positive and finite");
  const rt_accum* a = d->a;
  const int64_t any = (a->flags & RT_ACCUM_COUNTS) ? a->bound : a->done;
  if (any < 1) return set_error(RT_E_INVALID, w + ": no samples accumulated yet");
  if (d->pose_gen != a->pose_gen)
    return set_error(RT_E_INVALID, w + ": the guides are of another camera (rt_accum_set_camera was called since: rt_denoise_rebuild)");
  return RT_OK;
}

// init, the levels and the output conversion on st (the current device is the scene's); nothing is waited for
int launch_run(rt_denoise* d, const rt_denoise_params* p, float* d_rgb, int32_t* d_argb, hipStream_t st, const std::string& w) {
  const rt_accum* a = d->a;
  const int64_t n = pixels(d);
  const int64_t bx = (d->W + dn::ROW_LANES - 1) / dn::ROW_LANES, by = (d->H + dn::TILE_ROWS - 1) / dn::TILE_ROWS;
  if (bx * by > INT32_MAX) return set_error(RT_E_INVALID, w + ": more than 2^31 - 1 blocks");
  // per-pixel counts only once they differ from done: until then the count array is not filled
  const int32_t* cnt = ((a->flags & RT_ACCUM_COUNTS) && a->mixed) ? a->cnt : nullptr;
  hipLaunchKernelGGL(dn::denoise_init_kernel, dim3(blocks256(n)), dim3(256), 0, st, a->sum, a->sq, cnt, a->done, n, d->buf[0]);
  HIPCHK(hipGetLastError());
  int cur = 0;
  for (int i = 0; i < p->levels; ++i, cur ^= 1) {
    auto fn = cnt ? dn::atrous_kernel<true> : dn::atrous_kernel<false>;
    hipLaunchKernelGGL(fn, dim3((unsigned)(bx * by)), dim3(256), 0, st, d->W, d->H, (int)bx, 1 << i, p->normal_log2, p->sigma_l,
                       p->sigma_z, cnt, d->gn, d->gp, d->buf[cur], d->buf[cur ^ 1]);
    HIPCHK(hipGetLastError());
  }
  if (d_rgb || d_argb) {
    hipLaunchKernelGGL(dn::denoise_output_kernel, dim3(blocks256(n)), dim3(256), 0, st, d->buf[cur], n, d_rgb, d_argb);
    HIPCHK(hipGetLastError());
  }
  d->final_ = cur;
  d->last = st;
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_denoise_defaults(rt_denoise_params* p) {
  if (!p) return set_error(RT_E_INVALID, "rt_denoise_defaults: null params");
  p->levels = 5;
  p->normal_log2 = 7;
  p->sigma_l = 4.0;
  p->sigma_z = 0.1;
  return RT_OK;
}

int rt_denoise_create(rt_accum* a, rt_denoise** out) {
  const std::string w("rt_denoise_create");
  if (!a) return set_error(RT_E_INVALID, w + ": null accumulator");
  if (!out) return set_error(RT_E_INVALID, w + ": null out");
  *out = nullptr;
  if (!(a->flags & RT_ACCUM_MOMENTS)) return set_error(RT_E_INVALID, w + ": the accumulator was created without RT_ACCUM_MOMENTS");
  DeviceGuard dg;
  HIPCHK(hipSetDevice(a->scene->device));
  HIPCHK(hipStreamSynchronize((hipStream_t)a->last));  // the trace below counts as the scene's one in-flight render
  rt_denoise* d = new rt_denoise();
  std::memset(d, 0, sizeof(*d));
  d->a = a;
  d->W = a->W;
  d->H = a->H;
  d->final_ = -1;
  d->last = a->scene->stream;
  const size_t n = (size_t)pixels(d);
  hipError_t e = hipMalloc(&d->gn, n * sizeof(dn::GuideN));
  if (e == hipSuccess) e = hipMalloc(&d->gp, n * sizeof(dn::GuideP));
  if (e == hipSuccess) e = hipMalloc(&d->buf[0], n * sizeof(dn::Plane));
  if (e == hipSuccess) e = hipMalloc(&d->buf[1], n * sizeof(dn::Plane));
  if (e == hipSuccess) e = hipMalloc(&d->orgb, n * 3 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&d->oargb, n * sizeof(int32_t));
  int rc = e == hipSuccess ? RT_OK : set_error(RT_E_HIP, w + ": " + hipGetErrorString(e));
  if (rc == RT_OK) rc = build_guides(d, (hipStream_t)a->scene->stream, w, false);
  if (rc != RT_OK) {
    free_buffers(d);
    delete d;
    return rc;
  }
  *out = d;
  return RT_OK;
}

int rt_denoise_rebuild(rt_denoise* d) {
  const std::string w("rt_denoise_rebuild");
  if (!d) return set_error(RT_E_INVALID, w + ": null denoiser");
  rt_accum* a = d->a;
  DeviceGuard dg;
  HIPCHK(hipSetDevice(a->scene->device));
  HIPCHK(hipStreamSynchronize((hipStream_t)a->last));  // as creation: the trace is the scene's one in-flight render
  HIPCHK(hipStreamSynchronize((hipStream_t)d->last));  // a run in flight reads the guides
  d->final_ = -1;  // the planes are of the old guides
  return build_guides(d, (hipStream_t)a->scene->stream, w, true);
}

int rt_denoise_guides(rt_denoise* d, float* normal, float* pos, float* depth, int32_t* material) {
  const std::string w("rt_denoise_guides");
  if (!d) return set_error(RT_E_INVALID, w + ": null denoiser");
  if (!normal && !pos && !depth && !material) return RT_OK;
  DeviceGuard dg;
  HIPCHK(hipSetDevice(d->a->scene->device));
  const size_t n = (size_t)pixels(d);
  std::vector<dn::GuideN> gn(n);
  std::vector<dn::GuideP> gp(n);
  HIPCHK(hipMemcpy(gn.data(), d->gn, n * sizeof(dn::GuideN), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(gp.data(), d->gp, n * sizeof(dn::GuideP), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) {
    if (normal) { normal[3 * i] = gn[i].nx; normal[3 * i + 1] = gn[i].ny; normal[3 * i + 2] = gn[i].nz; }
    if (material) material[i] = gn[i].material;
    if (pos) { pos[3 * i] = gp[i].px; pos[3 * i + 1] = gp[i].py; pos[3 * i + 2] = gp[i].pz; }
    if (depth) depth[i] = gp[i].depth;
  }
  return RT_OK;
}

int rt_denoise_run_device(rt_denoise* d, const rt_denoise_params* p, float* d_rgb, int32_t* d_argb, void* hip_stream) {
  const std::string w("rt_denoise_run_device");
  const int rc = check_run(w, d, p);
  if (rc) return rc;
  DeviceGuard dg;
  HIPCHK(hipSetDevice(d->a->scene->device));
  return launch_run(d, p, d_rgb, d_argb, (hipStream_t)hip_stream, w);
}

int rt_denoise_run(rt_denoise* d, const rt_denoise_params* p, float* rgb, int32_t* argb) {
  const std::string w("rt_denoise_run");
  int rc = check_run(w, d, p);
  if (rc) return rc;
  DeviceGuard dg;
  HIPCHK(hipSetDevice(d->a->scene->device));
  hipStream_t st = (hipStream_t)d->a->last;
  HIPCHK(hipStreamSynchronize(st));
  if ((rc = launch_run(d, p, rgb ? d->orgb : nullptr, argb ? d->oargb : nullptr, st, w)) != RT_OK) return rc;
  const size_t n = (size_t)pixels(d);
  if (rgb) HIPCHK(hipMemcpyAsync(rgb, d->orgb, n * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
  if (argb) HIPCHK(hipMemcpyAsync(argb, d->oargb, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return RT_OK;
}

int rt_denoise_planes(rt_denoise* d, double* colour, double* variance) {
  const std::string w("rt_denoise_planes");
  if (!d) return set_error(RT_E_INVALID, w + ": null denoiser");
  if (d->final_ < 0) return set_error(RT_E_INVALID, w + ": no run was made");
  if (!colour && !variance) return RT_OK;
  DeviceGuard dg;
  HIPCHK(hipSetDevice(d->a->scene->device));
  HIPCHK(hipStreamSynchronize((hipStream_t)d->last));
  const size_t n = (size_t)pixels(d);
  std::vector<dn::Plane> pl(n);
  HIPCHK(hipMemcpy(pl.data(), d->buf[d->final_], n * sizeof(dn::Plane), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) {
    if (colour) { colour[3 * i] = pl[i].r; colour[3 * i + 1] = pl[i].g; colour[3 * i + 2] = pl[i].b; }
    if (variance) variance[i] = pl[i].v;
  }
  return RT_OK;
}

void rt_denoise_destroy(rt_denoise* d) {
  if (!d) return;
  DeviceGuard dg;
  if (hipSetDevice(d->a->scene->device) == hipSuccess) {
    (void)hipStreamSynchronize((hipStream_t)d->last);
    free_buffers(d);
  }
  delete d;
}

}  // extern "C"
