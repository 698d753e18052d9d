// Progressive sample accumulation (include/distraytracer.h rt_accum_*): a frame whose per-pixel sample
// sums live on the scene's device between launches, so a host can add samples in chunks, look at the
// frame so far, ask how noisy it still is, checkpoint it and go on. The kernels (accum_kernels.h) run the
// render kernel's wave layout and shading tree (trace_sample) and are instantiated here, in a translation
// unit of their own, so that the register allocation of the kernels in the other units is not disturbed.
// The host plumbing shared with the other units (HIP check, variant lookup, staging) is launch_common.h's.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

// as render_minreg.hip: trace.hip alone holds the kernels trace_kernels.h defines outright
#define RT_MINREG_TU
#include "rt_internal.h"
#include "comm.h"
#include "accum_state.h"
#include "accum_kernels.h"
#define RT_UNIT_SHADES  // the kernels reach the noise textures: this unit uploads its own Perlin tables
#include "launch_common.h"

using namespace rt;

namespace {

constexpr uint32_t RENDER_FLAGS = RT_RENDER_GENERIC | RT_RENDER_NOCULL;
constexpr uint32_t ACCUM_FLAGS = RT_ACCUM_MOMENTS | RT_ACCUM_COUNTS;

// the kernels without a camera pose; an accumulator that has one launches pose.hip's (pose_launch_accum)
typedef void (*AccumFn)(SceneD, ParamsD, int, double*, double*);
struct AccumVariant {
  uint32_t mask;
  AccumFn fn[2];  // without / with the square sums
};
#define AV(F) {F, {dv::accum_kernel<F, false>, dv::accum_kernel<F, true>}}
// the specialised shading tree the scene's render runs where one matches exactly, else the generic one
// (launch_common.h variant_for)
const AccumVariant kAccumVariants[] = {RT_VARIANT_MASKS(AV)};
#undef AV

size_t sums_bytes(const rt_accum* a) { return (size_t)3 * (size_t)a->W * (size_t)a->H * sizeof(double); }
int64_t pixels(const rt_accum* a) { return (int64_t)a->W * a->H; }

// the host-buffer entries wait for the last add first
int sync_last(rt_accum* a) {
  HIPCHK(hipSetDevice(a->scene->device));
  HIPCHK(hipStreamSynchronize((hipStream_t)a->last));
  return RT_OK;
}

// on the accumulator's stream and waited for: an add on any stream may follow
int zero_sums(rt_accum* a) {
  hipStream_t st = (hipStream_t)a->last;
  HIPCHK(hipMemsetAsync(a->sum, 0, sums_bytes(a), st));
  if (a->sq) HIPCHK(hipMemsetAsync(a->sq, 0, sums_bytes(a), st));
  HIPCHK(hipStreamSynchronize(st));
  return RT_OK;
}

// per-pixel counts that differ from done (RT_ACCUM_COUNTS after a selective add): adaptive.hip's kernels
bool mixed_counts(const rt_accum* a) { return (a->flags & RT_ACCUM_COUNTS) && a->mixed; }
// what the resolve and error entries ask of the samples so far: an accumulator with RT_ACCUM_COUNTS has some
// as soon as one add of any kind happened (a pixel without enough of them resolves black, errs +Inf)
int64_t samples_floor(const rt_accum* a) { return (a->flags & RT_ACCUM_COUNTS) ? (a->bound >= 1 ? 2 : 0) : a->done; }

int launch_resolve(rt_accum* a, float* d_rgb, int32_t* d_argb, hipStream_t st) {
  if (mixed_counts(a)) return adaptive_resolve(a, d_rgb, d_argb, st);
  const int64_t n = pixels(a);
  hipLaunchKernelGGL(dv::resolve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a->sum, n, a->done, d_rgb, d_argb);
  HIPCHK(hipGetLastError());
  return RT_OK;
}

int launch_error(rt_accum* a, float* d_err, hipStream_t st) {
  if (mixed_counts(a) || ((a->flags & RT_ACCUM_COUNTS) && a->done < 2)) return adaptive_error(a, d_err, st);  // +Inf below two
  const int64_t n = pixels(a);
  hipLaunchKernelGGL(dv::error_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a->sum, a->sq, n, a->done, d_err);
  HIPCHK(hipGetLastError());
  return RT_OK;
}

int check_resolve(const char* who, const rt_accum* a) {
  const std::string w(who);
  if (!a) return set_error(RT_E_INVALID, w + ": null accumulator");
  if (samples_floor(a) < 1) return set_error(RT_E_INVALID, w + ": no samples accumulated yet");
  return RT_OK;
}

int check_error(const char* who, const rt_accum* a, const float* err) {
  const std::string w(who);
  if (!a) return set_error(RT_E_INVALID, w + ": null accumulator");
  if (!err) return set_error(RT_E_INVALID, w + ": null err");
  if (!(a->flags & RT_ACCUM_MOMENTS)) return set_error(RT_E_INVALID, w + ": the accumulator was created without RT_ACCUM_MOMENTS");
  if (samples_floor(a) < 2) return set_error(RT_E_INVALID, w + ": needs at least two accumulated samples");
  return RT_OK;
}

// device -> host through a temporary device buffer of `bytes`, filled by `fill` on the accumulator's stream
template <class Fill>
int read_back(rt_accum* a, void* host, size_t bytes, Fill fill) {
  void* d = nullptr;
  HIPCHK(hipMalloc(&d, bytes));
  int rc = fill(d);
  hipError_t e = hipSuccess;
  if (rc == RT_OK) e = hipMemcpyAsync(host, d, bytes, hipMemcpyDeviceToHost, (hipStream_t)a->last);
  rc = sync_report((hipStream_t)a->last, rc, e, "rt_accum read-back: ", "rt_accum kernel: ");
  (void)hipFree(d);
  return rc;
}

}  // namespace

extern "C" {

int rt_accum_create(rt_scene* s, const rt_render_params* p, uint32_t accum_flags, rt_accum** out) {
  const std::string w("rt_accum_create");
  if (!s) return set_error(RT_E_INVALID, w + ": null scene");
  if (!p) return set_error(RT_E_INVALID, w + ": null params");
  if (!out) return set_error(RT_E_INVALID, w + ": null out");
  *out = nullptr;
  if (p->flags & ~RENDER_FLAGS) return set_error(RT_E_INVALID, w + ": only RT_RENDER_GENERIC and RT_RENDER_NOCULL are accepted in flags");
  if (accum_flags & ~ACCUM_FLAGS) return set_error(RT_E_INVALID, w + ": unknown accum_flags bits");
  if (p->width <= 0 || p->height <= 0) return set_error(RT_E_INVALID, w + ": bad image size");
  if ((accum_flags & RT_ACCUM_COUNTS) && (int64_t)p->width * p->height > INT32_MAX)
    return set_error(RT_E_INVALID, w + ": RT_ACCUM_COUNTS needs width * height < 2^31");
  {  // the whole image, by rt_render_pixels_device's rule, from the arguments alone
    const int row1 = p->row1 <= 0 ? p->height : p->row1;
    if (p->row0 != 0 || row1 != p->height || p->row_step > 1 || p->row_band > 1)
      return set_error(RT_E_INVALID, w + ": whole-frame layouts only");
  }
  DeviceGuard dg;
  rt_render_params q = *p;
  q.spp = 2;  // any count: the frame's constants and the photon map do not depend on it
  ParamsD P;
  int rc = prepare_render(s, &q, P);
  if (rc) return set_error(rc, w + ": " + rt_last_error());
  HIPCHK(hipSetDevice(s->device));
  if ((rc = perlin_ready(s->device)) != RT_OK) return rc;
  hipStream_t st;
  if ((rc = scene_stream(s, &st)) != RT_OK) return rc;
  rt_accum* a = new rt_accum();
  a->flags = accum_flags;
  a->W = p->width;
  a->H = p->height;
  a->done = 0;
  a->scene = s;
  a->rp = q;
  a->sum = nullptr;
  a->sq = nullptr;
  a->last = st;
  hipError_t e = hipMalloc(&a->sum, sums_bytes(a));
  if (e == hipSuccess && (accum_flags & RT_ACCUM_MOMENTS)) e = hipMalloc(&a->sq, sums_bytes(a));
  if (e == hipSuccess && (accum_flags & RT_ACCUM_COUNTS) && adaptive_alloc(a) != RT_OK) e = hipErrorOutOfMemory;
  if (e != hipSuccess || zero_sums(a) != RT_OK) {
    const std::string msg = e != hipSuccess ? w + ": " + hipGetErrorString(e) : w + ": " + rt_last_error();
    (void)hipFree(a->sum);
    (void)hipFree(a->sq);
    adaptive_free(a);
    delete a;
    return set_error(RT_E_HIP, msg);
  }
  *out = a;
  return RT_OK;
}

int rt_accum_add(rt_accum* a, int count, void* hip_stream) {
  const std::string w("rt_accum_add");
  if (!a) return set_error(RT_E_INVALID, w + ": null accumulator");
  if (count < 1) return set_error(RT_E_INVALID, w + ": count must be at least 1");
  if ((a->done > a->bound ? a->done : a->bound) + (int64_t)count >= ((int64_t)1 << 31))
    return set_error(RT_E_INVALID, w + ": more than 2^31 - 1 samples per pixel");
  DeviceGuard dg;
  rt_scene* s = a->scene;
  rt_render_params q = a->rp;
  q.spp = count;  // make_params' wave layout for a render of `count` samples: G, tw, th
  ParamsD P;
  int rc = prepare_render(s, &q, P);
  if (rc) return set_error(rc, w + ": " + rt_last_error());
  HIPCHK(hipSetDevice(s->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)s->stream;
  const SceneD sd = render_scene_view(s, a->rp.flags & RT_RENDER_NOCULL);
  if (mixed_counts(a)) {  // samples [cnt[p], cnt[p] + count) of every pixel
    if ((rc = adaptive_add_all(a, P, st)) != RT_OK) return rc;
    a->done += count;
    a->bound += count;
    a->last = st;
    return RT_OK;
  }
  const int64_t tilesX = (P.W + P.tw - 1) / P.tw, tilesY = (P.H + P.th - 1) / P.th;
  if (tilesX * tilesY > INT32_MAX) return set_error(RT_E_INVALID, w + ": more than 2^31 - 1 tiles");
  if (a->has_pose) {
    if ((rc = pose_launch_accum(a, sd, P, (unsigned)(tilesX * tilesY), st)) != RT_OK) return rc;
  } else {
    const AccumVariant& v = variant_for(kAccumVariants, render_variant_mask(s, a->rp.flags));
    hipLaunchKernelGGL(v.fn[a->sq ? 1 : 0], dim3((unsigned)(tilesX * tilesY)), dim3(64), dv::LDS_RENDER_BYTES, st, sd, P, (int)a->done,
                       a->sum, a->sq);
    HIPCHK(hipGetLastError());
  }
  a->done += count;
  if (a->flags & RT_ACCUM_COUNTS) a->bound += count;
  a->last = st;
  return RT_OK;
}

int rt_accum_samples(const rt_accum* a, int64_t* samples) {
  const std::string w("rt_accum_samples");
  if (!a) return set_error(RT_E_INVALID, w + ": null accumulator");
  if (!samples) return set_error(RT_E_INVALID, w + ": null samples");
  *samples = a->done;
  return RT_OK;
}

int rt_accum_resolve_device(rt_accum* a, float* d_rgb, int32_t* d_argb, void* hip_stream) {
  int rc = check_resolve("rt_accum_resolve_device", a);
  if (rc) return rc;
  if (!d_rgb && !d_argb) return RT_OK;
  DeviceGuard dg;
  HIPCHK(hipSetDevice(a->scene->device));
  return launch_resolve(a, d_rgb, d_argb, (hipStream_t)hip_stream);
}

int rt_accum_resolve(rt_accum* a, float* rgb, int32_t* argb) {
  int rc = check_resolve("rt_accum_resolve", a);
  if (rc) return rc;
  if (!rgb && !argb) return RT_OK;
  DeviceGuard dg;
  if ((rc = sync_last(a)) != RT_OK) return rc;
  const size_t npx = (size_t)pixels(a), nrgb = npx * 3 * sizeof(float), nargb = npx * sizeof(int32_t);
  std::string tmp(nrgb + nargb, '\0');
  rc = read_back(a, &tmp[0], nrgb + nargb,
                 [&](void* d) { return launch_resolve(a, (float*)d, (int32_t*)((char*)d + nrgb), (hipStream_t)a->last); });
  if (rc != RT_OK) return rc;
  if (rgb) std::memcpy(rgb, tmp.data(), nrgb);
  if (argb) std::memcpy(argb, tmp.data() + nrgb, nargb);
  return RT_OK;
}

int rt_accum_error_device(rt_accum* a, float* d_err, void* hip_stream) {
  int rc = check_error("rt_accum_error_device", a, d_err);
  if (rc) return rc;
  DeviceGuard dg;
  HIPCHK(hipSetDevice(a->scene->device));
  return launch_error(a, d_err, (hipStream_t)hip_stream);
}

int rt_accum_error(rt_accum* a, float* err) {
  int rc = check_error("rt_accum_error", a, err);
  if (rc) return rc;
  DeviceGuard dg;
  if ((rc = sync_last(a)) != RT_OK) return rc;
  return read_back(a, err, (size_t)pixels(a) * sizeof(float), [&](void* d) { return launch_error(a, (float*)d, (hipStream_t)a->last); });
}

int rt_accum_state(rt_accum* a, int64_t* samples, double* sum, double* sq) {
  const std::string w("rt_accum_state");
  if (!a) return set_error(RT_E_INVALID, w + ": null accumulator");
  if (sq && !(a->flags & RT_ACCUM_MOMENTS)) return set_error(RT_E_INVALID, w + ": sq asked of an accumulator without RT_ACCUM_MOMENTS");
  DeviceGuard dg;
  const int rc = sync_last(a);  // also with no buffer to fill: a host waits for its adds this way
  if (rc != RT_OK) return rc;
  if (samples) *samples = a->done;
  hipStream_t st = (hipStream_t)a->last;
  if (sum) HIPCHK(hipMemcpyAsync(sum, a->sum, sums_bytes(a), hipMemcpyDeviceToHost, st));
  if (sq) HIPCHK(hipMemcpyAsync(sq, a->sq, sums_bytes(a), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return RT_OK;
}

int rt_accum_restore(rt_accum* a, int64_t samples, const double* sum, const double* sq) {
  const std::string w("rt_accum_restore");
  if (!a) return set_error(RT_E_INVALID, w + ": null accumulator");
  if (samples < 0 || samples >= ((int64_t)1 << 31)) return set_error(RT_E_INVALID, w + ": sample count outside [0, 2^31)");
  if (!sum) return set_error(RT_E_INVALID, w + ": null sum");
  if (sq && !(a->flags & RT_ACCUM_MOMENTS)) return set_error(RT_E_INVALID, w + ": sq given to an accumulator without RT_ACCUM_MOMENTS");
  if (!sq && (a->flags & RT_ACCUM_MOMENTS)) return set_error(RT_E_INVALID, w + ": an accumulator with RT_ACCUM_MOMENTS needs sq");
  DeviceGuard dg;
  const int rc = sync_last(a);
  if (rc != RT_OK) return rc;
  hipStream_t st = (hipStream_t)a->last;  // waited for: an add on any stream may follow
  HIPCHK(hipMemcpyAsync(a->sum, sum, sums_bytes(a), hipMemcpyHostToDevice, st));
  if (sq) HIPCHK(hipMemcpyAsync(a->sq, sq, sums_bytes(a), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  a->done = samples;
  if (a->flags & RT_ACCUM_COUNTS) adaptive_uniform(a, samples);
  return RT_OK;
}

int rt_accum_reset(rt_accum* a) {
  if (!a) return set_error(RT_E_INVALID, "rt_accum_reset: null accumulator");
  DeviceGuard dg;
  int rc = sync_last(a);
  if (rc != RT_OK) return rc;
  if ((rc = zero_sums(a)) != RT_OK) return rc;
  a->done = 0;
  if (a->flags & RT_ACCUM_COUNTS) adaptive_uniform(a, 0);
  return RT_OK;
}

int rt_accum_set_camera(rt_accum* a, const double* pose) {
  const std::string w("rt_accum_set_camera");
  if (!a) return set_error(RT_E_INVALID, w + ": null accumulator");
  if (pose) {
    const char* why = pose_invalid(pose);
    if (why) return set_error(RT_E_INVALID, w + ": " + why);
  }
  const int rc = rt_accum_reset(a);  // the sums are of the old camera's rays
  if (rc != RT_OK) return rc;
  a->has_pose = pose ? 1 : 0;
  if (pose) std::memcpy(a->pose, pose, sizeof(a->pose));
  a->pose_gen += 1;
  return RT_OK;
}

int rt_accum_camera(const rt_accum* a, double* pose, int* is_set) {
  const std::string w("rt_accum_camera");
  if (!a) return set_error(RT_E_INVALID, w + ": null accumulator");
  if (!pose) return set_error(RT_E_INVALID, w + ": null pose");
  if (!is_set) return set_error(RT_E_INVALID, w + ": null is_set");
  for (int i = 0; i < 16; ++i) pose[i] = a->has_pose ? a->pose[i] : (i % 5 == 0 ? 1.0 : 0.0);
  *is_set = a->has_pose;
  return RT_OK;
}

void rt_accum_destroy(rt_accum* a) {
  if (!a) return;
  DeviceGuard dg;
  if (hipSetDevice(a->scene->device) == hipSuccess) {
    (void)hipStreamSynchronize((hipStream_t)a->last);
    (void)hipFree(a->sum);
    (void)hipFree(a->sq);
    adaptive_free(a);
  }
  delete a;
}

}  // extern "C"
