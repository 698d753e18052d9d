// The camera code of the render kernel as one device function, shared by camera_rays_kernel
// (shade_kernels.h) and accum_kernel (accum_kernels.h).
#pragma once
#include "trace_kernels.h"

namespace rt {
namespace dv {

// The ray render_kernel shoots for sample s of pixel (row, col) of a whole-frame layout (pixel key =
// row * W + col): the kernel's camera code operation for operation (myScene.java:1386-1462 FOV / DOF,
// :1562-1622 fisheye, :1690-1745 ortho). jit selects the branches a render of two or more samples takes
// (the jittered FOV, fisheye and ortho rays; the DOF branch draws its lens point either way), !jit the
// un-jittered ones of a 1-spp render. The direction is returned as the kernel hands it to trace_sample
// (not normalised). Returns false for a fisheye sample outside the image circle, which the render does
// not trace. F: the caller's feature mask, which compiles the cameras it cannot reach away as
// render_kernel's does (FT_ALL: every camera).
template <uint32_t F>
__device__ __forceinline__ bool camera_ray(const SceneD& S, const ParamsD& P, int row, int col, int s, bool jit, V& o, V& d) {
  const uint64_t pixel = (uint64_t)row * (uint64_t)P.W + (uint64_t)col;
  const bool dof = (F & FT_DOF) && S.dof && !((F & FT_CAMX) && P.cam != 0);
  const double rayY = (-1 * (row - P.H / 2.0));
  const double rayX = col - P.W / 2.0;
  bool traced = true;
  o = mk(0, 0, 0);
  d = mk(0, 0, 0);
  if ((F & FT_CAMX) && P.cam == 1) {  // myFishEyeScene: draw (1 spp) / shootMultiRays
    double xVal, yVal, rSq;
    if (!jit) {
      yVal = (row + P.yStart) * P.fishMult;
      const double ySq = yVal * yVal;
      xVal = (col + P.xStart) * P.fishMult;
      rSq = xVal * xVal + ySq;
      traced = !(rSq > 1);
    } else {
      yVal = ((row + P.yStart) + rng(P.seed, pixel, (uint32_t)s, 0, SITE_AA_Y, 0, -.5, .5)) * P.fishMult;
      xVal = ((col + P.xStart) + rng(P.seed, pixel, (uint32_t)s, 0, SITE_AA_X, 0, -.5, .5)) * P.fishMult;
      rSq = yVal * yVal + xVal * xVal;
      traced = rSq <= 1;
    }
    const double r = sqrt(rSq), theta = r * P.aperHalf, phi = atan2(-yVal, xVal), sTh = jf::sin(theta);
    o = mk(0, 0, 0);
    d = mk(sTh * jf::cos(phi), sTh * jf::sin(phi), -jf::cos(theta));
  } else if ((F & FT_CAMX) && P.cam == 2) {  // myOrthoScene: draw / shootMultiRays
    const double rayYOffset = P.H / 2.0, rayXOffset = P.W / 2.0;
    double rx, ry;
    if (!jit) {
      ry = P.orthPerRow * (-1 * (row - rayYOffset));
      rx = P.orthPerCol * (col - rayXOffset);
    } else {
      const double yB = P.orthPerRow * ((-1 * (row - rayYOffset)) - .5), xB = P.orthPerCol * (col - rayXOffset - .5);
      ry = yB + (P.orthPerRow * rng(P.seed, pixel, (uint32_t)s, 0, SITE_AA_Y, 0, -.5, .5));
      rx = xB + (P.orthPerCol * rng(P.seed, pixel, (uint32_t)s, 0, SITE_AA_X, 0, -.5, .5));
    }
    o = mk(rx, ry, 0);
    d = mk(0, 0, -1);
  } else if (dof) {  // shootMultiDpthOfFldRays: the pixel's lens centre and focal point, then the lens sample
    const V lc = nrmz(mk(rayX, rayY, P.viewZ));
    const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    V ld = nrmz(nrmz(lc));
    V fo = xpt(I, mk(0, 0, 0)), fd = xvec(I, ld);
    V fN = mk(0, 0, 1);
    double pr = dot(fN, fd);
    double t = -(dot(fN, fo) + S.lensFocal) / pr;
    const V fpt = mk(fd.x * t + fo.x, fd.y * t + fo.y, fd.z * t + fo.z);
    double th = rng(P.seed, pixel, (uint32_t)s, 0, SITE_DOF_ANG, 0, 0, TWO_PI_F);
    V tt = nrmz(rot_axis(mk(0, 1, 0), mk(0, 0, -1), th));
    double mm = rng(P.seed, pixel, (uint32_t)s, 0, SITE_DOF_RAD, 0, 0, S.lensRadius);
    tt = mk(tt.x * mm, tt.y * mm, tt.z * mm);
    o = mk(tt.x + lc.x, tt.y + lc.y, tt.z + lc.z);
    d = sub(fpt, o);
  } else if (!jit) {  // myFOVScene.draw's 1-spp path: no jitter
    o = mk(0, 0, 0);
    d = mk(rayX, rayY, P.viewZ);
  } else {  // shootMultiRays: y jitter drawn before x
    double ry = rayY + rng(P.seed, pixel, (uint32_t)s, 0, SITE_AA_Y, 0, -.5, .5);
    double rx = rayX + rng(P.seed, pixel, (uint32_t)s, 0, SITE_AA_X, 0, -.5, .5);
    o = mk(0, 0, 0);
    d = mk(rx, ry, P.viewZ);
  }
  return traced;
}

// A camera pose applied to the ray camera_ray returned: o as a point, d as a vector (still not normalised),
// by trace_device.h's xpt / xvec operation for operation -- per row a = 0.0, then a += m * x, y, z in turn
// and a += m3 * 1.0 (point) or m3 * 0.0 (vector), every step rounded (the units are built
// -ffp-contract=off). xpt and xvec read rows 0 .. 2 of a matrix only, which is what PoseD holds. The
// matrix is a kernel argument and so wave-uniform: the multiplies take it from scalar registers
// (DESIGN.md section 18 says where it waits between the rounds of a sample loop).
__device__ __forceinline__ void pose_ray(V& o, V& d, const PoseD& M) {
  o = xpt(M.m, o);
  d = xvec(M.m, d);
}
// a kernel instantiated without a pose (its argument pack is empty): the ray as it is
__device__ __forceinline__ void pose_ray(V&, V&) {}
// The posed kernels are the un-posed ones with `bool POSE = false, class... M` behind their template
// parameters and `M... pose` behind their arguments: POSE instantiations take one PoseD there, the others
// nothing, so that an un-posed kernel keeps the argument list, and with it the code, it had before.
#define RT_POSE_PACK_CHECK(POSE, M) \
  static_assert(sizeof...(M) == ((POSE) ? 1 : 0), "a posed kernel takes one PoseD last, an un-posed one nothing")

}  // namespace dv
}  // namespace rt
