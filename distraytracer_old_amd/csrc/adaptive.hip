// Adaptive sampling (include/distraytracer.h rt_accum_select_*, rt_accum_add_selected, rt_accum_counts*): an
// accumulator with RT_ACCUM_COUNTS keeps a sample count per pixel, so a host can select the pixels that are
// still noisy and add samples to those alone. The kernels (adaptive_kernels.h) are instantiated here, in a
// translation unit of their own, so that the register allocation of accum.hip's kernels is not disturbed.
// The host plumbing shared with the other units (HIP check, variant lookup, staging) is launch_common.h's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

// as render_minreg.hip: trace.hip alone holds the kernels trace_kernels.h defines outright
#define RT_MINREG_TU
#include "rt_internal.h"
#include "comm.h"
#include "accum_state.h"
#include "adaptive_kernels.h"
#define RT_UNIT_SHADES  // the kernels reach the noise textures: this unit uploads its own Perlin tables
#include "launch_common.h"

using namespace rt;

namespace {

// the kernels without a camera pose; an accumulator that has one launches pose.hip's (pose_launch_list)
typedef void (*ListFn)(SceneD, ParamsD, const int32_t*, size_t, int32_t*, double*, double*);
struct ListVariant {
  uint32_t mask;
  ListFn fn[2];  // without / with the square sums
};
#define LV(F) {F, {dv::accum_list_kernel<F, false>, dv::accum_list_kernel<F, true>}}
// the variant accum.hip's kAccumVariants gives the same scene (launch_common.h variant_for)
const ListVariant kListVariants[] = {RT_VARIANT_MASKS(LV)};
#undef LV

int64_t pixels(const rt_accum* a) { return (int64_t)a->W * a->H; }
int tiles_x(const rt_accum* a) { return (a->W + dv::SEL_TILE - 1) / dv::SEL_TILE; }
int64_t tiles(const rt_accum* a) { return (int64_t)tiles_x(a) * ((a->H + dv::SEL_TILE - 1) / dv::SEL_TILE); }

int sync_last(rt_accum* a) {
  HIPCHK(hipSetDevice(a->scene->device));
  HIPCHK(hipStreamSynchronize((hipStream_t)a->last));
  return RT_OK;
}

// the device array holds every pixel's count: while the counts are uniform it is filled from done here
int counts_ready(rt_accum* a, hipStream_t st) {
  if (!a->mixed) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)a->cnt, (int)a->done, (size_t)pixels(a), st));
  return RT_OK;
}

// the three steps of a selection into `list`, on st; the list's length is then toff[tiles]
template <int MODE>
int build_list(rt_accum* a, const uint8_t* d_mask, float thr, int maxn, int32_t* list, hipStream_t st) {
  const int64_t nt = tiles(a);
  hipLaunchKernelGGL(dv::select_ballot_kernel<MODE>, dim3((unsigned)nt), dim3(64), 0, st, a->W, a->H, tiles_x(a), d_mask, a->sum,
                     a->sq, a->cnt, thr, maxn, a->tballot, a->toff);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(dv::select_scan_kernel, dim3(1), dim3(256), 0, st, a->toff, nt);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(dv::select_scatter_kernel, dim3((unsigned)nt), dim3(64), 0, st, a->W, a->H, tiles_x(a), a->tballot, a->toff, list);
  HIPCHK(hipGetLastError());
  return RT_OK;
}

// a selection entry's tail: wait, read the length, publish the selection
int finish_select(rt_accum* a, hipStream_t st, int64_t* selected) {
  uint32_t n = 0;
  HIPCHK(hipMemcpyAsync(&n, a->toff + tiles(a), sizeof(n), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  a->nsel = n;
  a->has_sel = 1;
  *selected = n;
  return RT_OK;
}

int launch_list(rt_accum* a, const ParamsD& P, const int32_t* list, int64_t nlist, hipStream_t st, const std::string& w) {
  rt_scene* s = a->scene;
  const int64_t per = 64 / P.G, blocks = (nlist + per - 1) / per;
  if (blocks > INT32_MAX) return set_error(RT_E_INVALID, w + ": more than 2^31 - 1 blocks");
  int rc = perlin_ready(s->device);
  if (rc != RT_OK) return rc;
  const SceneD sd = render_scene_view(s, a->rp.flags & RT_RENDER_NOCULL);
  if (a->has_pose) return pose_launch_list(a, sd, P, list, (size_t)nlist, (unsigned)blocks, st);
  const ListVariant& v = variant_for(kListVariants, render_variant_mask(s, a->rp.flags));
  hipLaunchKernelGGL(v.fn[a->sq ? 1 : 0], dim3((unsigned)blocks), dim3(64), dv::LDS_RENDER_BYTES, st, sd, P, list, (size_t)nlist, a->cnt,
                     a->sum, a->sq);
  HIPCHK(hipGetLastError());
  return RT_OK;
}

// the checks every selective entry starts with
int check_counts(const std::string& w, const rt_accum* a) {
  if (!a) return set_error(RT_E_INVALID, w + ": null accumulator");
  if (!(a->flags & RT_ACCUM_COUNTS)) return set_error(RT_E_INVALID, w + ": the accumulator was created without RT_ACCUM_COUNTS");
  return RT_OK;
}

}  // namespace

namespace rt {

int adaptive_alloc(rt_accum* a) {
  const int64_t np = pixels(a), nt = tiles(a);
  HIPCHK(hipMalloc(&a->cnt, (size_t)np * sizeof(int32_t)));
  HIPCHK(hipMalloc(&a->sel, (size_t)np * sizeof(int32_t)));
  HIPCHK(hipMalloc(&a->all, (size_t)np * sizeof(int32_t)));
  HIPCHK(hipMalloc(&a->tballot, (size_t)nt * sizeof(uint64_t)));
  HIPCHK(hipMalloc(&a->toff, (size_t)(nt + 1) * sizeof(uint32_t)));
  return RT_OK;
}

void adaptive_free(rt_accum* a) {
  (void)hipFree(a->cnt);
  (void)hipFree(a->sel);
  (void)hipFree(a->all);
  (void)hipFree(a->tballot);
  (void)hipFree(a->toff);
}

void adaptive_uniform(rt_accum* a, int64_t n) {
  a->mixed = 0;
  a->bound = n;
  a->has_sel = 0;
  a->nsel = 0;
}

int adaptive_add_all(rt_accum* a, const ParamsD& P, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!a->all_ready) {  // its length is known, so nothing is waited for
    const int rc = build_list<0>(a, nullptr, 0.f, 0, a->all, st);
    if (rc != RT_OK) return rc;
    a->all_ready = 1;
  }
  return launch_list(a, P, a->all, pixels(a), st, "rt_accum_add");
}

int adaptive_resolve(rt_accum* a, float* d_rgb, int32_t* d_argb, void* stream) {
  const int64_t n = pixels(a);
  hipLaunchKernelGGL(dv::resolve_counts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a->sum, a->cnt, n,
                     d_rgb, d_argb);
  HIPCHK(hipGetLastError());
  return RT_OK;
}

int adaptive_error(rt_accum* a, float* d_err, void* stream) {
  const int64_t n = pixels(a);
  const int rc = counts_ready(a, (hipStream_t)stream);
  if (rc != RT_OK) return rc;
  hipLaunchKernelGGL(dv::error_counts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a->sum, a->sq,
                     a->cnt, n, d_err);
  HIPCHK(hipGetLastError());
  return RT_OK;
}

}  // namespace rt

extern "C" {

int rt_accum_select_error(rt_accum* a, float threshold, int max_samples, int64_t* selected) {
  const std::string w("rt_accum_select_error");
  int rc = check_counts(w, a);
  if (rc) return rc;
  if (!selected) return set_error(RT_E_INVALID, w + ": null selected");
  if (!(a->flags & RT_ACCUM_MOMENTS)) return set_error(RT_E_INVALID, w + ": the accumulator was created without RT_ACCUM_MOMENTS");
  if (!(threshold >= 0)) return set_error(RT_E_INVALID, w + ": threshold must be at least 0");
  if (max_samples < 1) return set_error(RT_E_INVALID, w + ": max_samples must be at least 1");
  DeviceGuard dg;
  if ((rc = sync_last(a)) != RT_OK) return rc;
  hipStream_t st = (hipStream_t)a->last;
  if ((rc = counts_ready(a, st)) != RT_OK) return rc;
  if ((rc = build_list<2>(a, nullptr, threshold, max_samples, a->sel, st)) != RT_OK) return rc;
  return finish_select(a, st, selected);
}

int rt_accum_select_mask(rt_accum* a, const uint8_t* mask, int64_t* selected) {
  const std::string w("rt_accum_select_mask");
  int rc = check_counts(w, a);
  if (rc) return rc;
  if (!mask) return set_error(RT_E_INVALID, w + ": null mask");
  if (!selected) return set_error(RT_E_INVALID, w + ": null selected");
  DeviceGuard dg;
  if ((rc = sync_last(a)) != RT_OK) return rc;
  hipStream_t st = (hipStream_t)a->last;
  uint8_t* d = nullptr;
  HIPCHK(hipMalloc(&d, (size_t)pixels(a)));
  hipError_t e = hipMemcpyAsync(d, mask, (size_t)pixels(a), hipMemcpyHostToDevice, st);
  rc = e == hipSuccess ? build_list<1>(a, d, 0.f, 0, a->sel, st) : set_error(RT_E_HIP, w + ": " + hipGetErrorString(e));
  if (rc == RT_OK) rc = finish_select(a, st, selected);
  else (void)hipStreamSynchronize(st);
  (void)hipFree(d);
  return rc;
}

int rt_accum_select_mask_device(rt_accum* a, const uint8_t* d_mask, void* hip_stream, int64_t* selected) {
  const std::string w("rt_accum_select_mask_device");
  int rc = check_counts(w, a);
  if (rc) return rc;
  if (!d_mask) return set_error(RT_E_INVALID, w + ": null mask");
  if (!selected) return set_error(RT_E_INVALID, w + ": null selected");
  DeviceGuard dg;
  if ((rc = sync_last(a)) != RT_OK) return rc;  // an add in flight may still read the list
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)a->last;
  if ((rc = build_list<1>(a, d_mask, 0.f, 0, a->sel, st)) != RT_OK) return rc;
  return finish_select(a, st, selected);
}

int rt_accum_selection(rt_accum* a, int32_t* pixels_out) {
  const std::string w("rt_accum_selection");
  int rc = check_counts(w, a);
  if (rc) return rc;
  if (!pixels_out) return set_error(RT_E_INVALID, w + ": null pixels");
  if (!a->has_sel) return set_error(RT_E_INVALID, w + ": no selection was made");
  if (a->nsel == 0) return RT_OK;
  DeviceGuard dg;
  if ((rc = sync_last(a)) != RT_OK) return rc;
  HIPCHK(hipMemcpy(pixels_out, a->sel, (size_t)a->nsel * sizeof(int32_t), hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_accum_add_selected(rt_accum* a, int count, void* hip_stream) {
  const std::string w("rt_accum_add_selected");
  int rc = check_counts(w, a);
  if (rc) return rc;
  if (count < 1) return set_error(RT_E_INVALID, w + ": count must be at least 1");
  if (!a->has_sel) return set_error(RT_E_INVALID, w + ": no selection was made");
  if (a->bound + (int64_t)count >= ((int64_t)1 << 31)) return set_error(RT_E_INVALID, w + ": more than 2^31 - 1 samples per pixel");
  if (a->nsel == 0) return RT_OK;
  DeviceGuard dg;
  rt_scene* s = a->scene;
  rt_render_params q = a->rp;
  q.spp = count;  // make_params' G for a render of `count` samples
  ParamsD P;
  rc = prepare_render(s, &q, P);
  if (rc) return set_error(rc, w + ": " + rt_last_error());
  HIPCHK(hipSetDevice(s->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)s->stream;
  if ((rc = counts_ready(a, st)) != RT_OK) return rc;
  if ((rc = launch_list(a, P, a->sel, a->nsel, st, w)) != RT_OK) return rc;
  a->mixed = 1;
  a->bound += count;
  a->last = st;
  return RT_OK;
}

int rt_accum_counts_device(rt_accum* a, int32_t* d_cnt, void* hip_stream) {
  const std::string w("rt_accum_counts_device");
  int rc = check_counts(w, a);
  if (rc) return rc;
  if (!d_cnt) return set_error(RT_E_INVALID, w + ": null cnt");
  DeviceGuard dg;
  HIPCHK(hipSetDevice(a->scene->device));
  hipStream_t st = (hipStream_t)hip_stream;
  if (!a->mixed) {
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)d_cnt, (int)a->done, (size_t)pixels(a), st));
    return RT_OK;
  }
  HIPCHK(hipMemcpyAsync(d_cnt, a->cnt, (size_t)pixels(a) * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  return RT_OK;
}

int rt_accum_counts(rt_accum* a, int32_t* cnt) {
  const std::string w("rt_accum_counts");
  int rc = check_counts(w, a);
  if (rc) return rc;
  if (!cnt) return set_error(RT_E_INVALID, w + ": null cnt");
  DeviceGuard dg;
  if ((rc = sync_last(a)) != RT_OK) return rc;
  if (!a->mixed) {
    for (int64_t i = 0, n = pixels(a); i < n; ++i) cnt[i] = (int32_t)a->done;
    return RT_OK;
  }
  HIPCHK(hipMemcpy(cnt, a->cnt, (size_t)pixels(a) * sizeof(int32_t), hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_accum_restore_counts(rt_accum* a, const int32_t* cnt) {
  const std::string w("rt_accum_restore_counts");
  int rc = check_counts(w, a);
  if (rc) return rc;
  if (!cnt) return set_error(RT_E_INVALID, w + ": null cnt");
  int32_t top = 0;
  for (int64_t i = 0, n = pixels(a); i < n; ++i) {
    if (cnt[i] < 0) return set_error(RT_E_INVALID, w + ": a count outside [0, 2^31)");
    top = cnt[i] > top ? cnt[i] : top;
  }
  DeviceGuard dg;
  if ((rc = sync_last(a)) != RT_OK) return rc;
  HIPCHK(hipMemcpy(a->cnt, cnt, (size_t)pixels(a) * sizeof(int32_t), hipMemcpyHostToDevice));
  a->mixed = 1;
  a->bound = top;
  a->has_sel = 0;
  a->nsel = 0;
  return RT_OK;
}

}  // extern "C"
