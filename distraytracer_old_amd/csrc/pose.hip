// The camera pose (include/distraytracer.h rt_camera_pose_check, rt_camera_look_at, rt_accum_set_camera): a
// rigid camera-to-world matrix applied where the camera rays are made, so that a host moves the eye over the
// scene as uploaded. The host-only entries live here, and so do the posed instantiations of the accumulator's
// two shading kernels (accum_kernels.h accum_kernel, adaptive_kernels.h accum_list_kernel), in a translation
// unit of their own: they compile beside accum.hip and adaptive.hip and leave the register allocation of the
// un-posed kernels there alone. The posed camera_rays_kernel, which shades nothing, is shade.hip's.
// The host plumbing shared with the other units (HIP check, variant lookup) is launch_common.h's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

// as render_minreg.hip: trace.hip alone holds the kernels trace_kernels.h defines outright; RT_POSE_TU: and
// accum.hip / adaptive.hip those of their kernel headers
#define RT_MINREG_TU
#define RT_POSE_TU
#include "rt_internal.h"
#include "accum_state.h"
#include "accum_kernels.h"
#include "adaptive_kernels.h"
#define RT_UNIT_SHADES  // the kernels reach the noise textures: this unit uploads its own Perlin tables
#include "launch_common.h"

using namespace rt;

namespace {

typedef void (*AccumPoseFn)(SceneD, ParamsD, int, double*, double*, PoseD);
struct AccumPoseVariant {
  uint32_t mask;
  AccumPoseFn fn[2];  // without / with the square sums
};
#define AV(F) {F, {dv::accum_kernel<F, false, true, PoseD>, dv::accum_kernel<F, true, true, PoseD>}}
// the variant accum.hip's kAccumVariants gives the same scene (launch_common.h variant_for)
const AccumPoseVariant kAccumPoseVariants[] = {RT_VARIANT_MASKS(AV)};
#undef AV

typedef void (*ListPoseFn)(SceneD, ParamsD, const int32_t*, size_t, int32_t*, double*, double*, PoseD);
struct ListPoseVariant {
  uint32_t mask;
  ListPoseFn fn[2];
};
#define LV(F) {F, {dv::accum_list_kernel<F, false, true, PoseD>, dv::accum_list_kernel<F, true, true, PoseD>}}
const ListPoseVariant kListPoseVariants[] = {RT_VARIANT_MASKS(LV)};
#undef LV

struct V3 {
  double x, y, z;
};
V3 cross3(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double norm3(V3 a) { return std::sqrt((a.x * a.x + a.y * a.y) + a.z * a.z); }
bool usable(double n) { return std::isfinite(n) && n > 0; }

}  // namespace

namespace rt {

const char* pose_invalid(const double* m) {
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(m[i])) return "an entry is not finite";
  if (m[12] != 0 || m[13] != 0 || m[14] != 0 || m[15] != 1) return "the last row is not 0 0 0 1";
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double g = (m[4 * i] * m[4 * j] + m[4 * i + 1] * m[4 * j + 1]) + m[4 * i + 2] * m[4 * j + 2];
      if (!(std::fabs(g - (i == j ? 1.0 : 0.0)) <= 1e-9)) return "the upper 3x3 is not orthonormal (|R R^T - I| > 1e-9): a rigid pose has no scale or shear";
    }
  const double det = (m[0] * (m[5] * m[10] - m[6] * m[9]) - m[1] * (m[4] * m[10] - m[6] * m[8])) + m[2] * (m[4] * m[9] - m[5] * m[8]);
  if (!(det > 0)) return "the upper 3x3 is a reflection (det R <= 0)";
  return nullptr;
}

PoseD pose_args(const double* pose) {
  PoseD M;
  for (int i = 0; i < 12; ++i) M.m[i] = pose[i];
  return M;
}

int pose_launch_accum(rt_accum* a, const SceneD& sd, const ParamsD& P, unsigned blocks, void* stream) {
  rt_scene* s = a->scene;
  const int rc = perlin_ready(s->device);
  if (rc != RT_OK) return rc;
  const AccumPoseVariant& v = variant_for(kAccumPoseVariants, render_variant_mask(s, a->rp.flags));
  hipLaunchKernelGGL(v.fn[a->sq ? 1 : 0], dim3(blocks), dim3(64), dv::LDS_RENDER_BYTES, (hipStream_t)stream, sd, P, (int)a->done, a->sum,
                     a->sq, pose_args(a->pose));
  HIPCHK(hipGetLastError());
  return RT_OK;
}

int pose_launch_list(rt_accum* a, const SceneD& sd, const ParamsD& P, const int32_t* list, size_t nlist, unsigned blocks,
                     void* stream) {
  rt_scene* s = a->scene;
  const int rc = perlin_ready(s->device);
  if (rc != RT_OK) return rc;
  const ListPoseVariant& v = variant_for(kListPoseVariants, render_variant_mask(s, a->rp.flags));
  hipLaunchKernelGGL(v.fn[a->sq ? 1 : 0], dim3(blocks), dim3(64), dv::LDS_RENDER_BYTES, (hipStream_t)stream, sd, P, list, nlist, a->cnt,
                     a->sum, a->sq, pose_args(a->pose));
  HIPCHK(hipGetLastError());
  return RT_OK;
}

}  // namespace rt

extern "C" {

int rt_camera_pose_check(const double* pose) {
  const std::string w("rt_camera_pose_check");
  if (!pose) return set_error(RT_E_INVALID, w + ": null pose");
  const char* why = pose_invalid(pose);
  if (why) return set_error(RT_E_INVALID, w + ": " + why);
  return RT_OK;
}

int rt_camera_look_at(const double* eye, const double* target, const double* up, double* pose) {
  const std::string w("rt_camera_look_at");
  if (!eye) return set_error(RT_E_INVALID, w + ": null eye");
  if (!target) return set_error(RT_E_INVALID, w + ": null target");
  if (!up) return set_error(RT_E_INVALID, w + ": null up");
  if (!pose) return set_error(RT_E_INVALID, w + ": null pose");
  V3 f = {target[0] - eye[0], target[1] - eye[1], target[2] - eye[2]};
  const double nf = norm3(f);
  if (!usable(nf)) return set_error(RT_E_INVALID, w + ": |target - eye| is zero or not finite");
  f = {f.x / nf, f.y / nf, f.z / nf};
  V3 r = cross3(f, {up[0], up[1], up[2]});
  const double nr = norm3(r);
  if (!usable(nr)) return set_error(RT_E_INVALID, w + ": |cross(view, up)| is zero or not finite (up parallel to the view?)");
  r = {r.x / nr, r.y / nr, r.z / nr};
  const V3 u = cross3(r, f);
  const double m[16] = {r.x, u.x, -f.x, eye[0], r.y, u.y, -f.y, eye[1], r.z, u.z, -f.z, eye[2], 0, 0, 0, 1};
  // what comes out always passes rt_camera_pose_check: an up so close to the view that the cross product
  // keeps too few digits is refused here
  const char* why = pose_invalid(m);
  if (why) return set_error(RT_E_INVALID, w + ": the result is not a valid pose, " + why);
  for (int i = 0; i < 16; ++i) pose[i] = m[i];
  return RT_OK;
}

}  // extern "C"
