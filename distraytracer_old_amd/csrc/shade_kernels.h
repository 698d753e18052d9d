// Radiance queries (rt_shade_rays / rt_shade_rays_device): the caller's rays through the render kernel's
// whole shading tree (trace_kernels.h trace_sample, the reference's reflectRay), and the camera rays of a
// frame as data (rt_camera_rays / rt_camera_rays_device).
#pragma once
#include "camera_ray.h"
#include "trace_kernels.h"

namespace rt {
namespace dv {

// One ray per lane, one wave per block (trace_sample's LDS is per wave, indexed by lane).
// shade_ray is the body both kernels below share: ray i of rays, built and rejected as query_ray
// (query_kernels.h) builds and rejects it, shaded under the key the render gives sample `sample` of
// pixel firstKey + i -- {seed, pixel, sample, node 1, SITE_TIME} -- into rgb[3i..3i+2] as the doubles
// trace_sample returns. trace_sample normalises the direction once (the myRay constructor), so d goes in
// as the caller gave it, as render_kernel hands over its camera directions.
// Tail lanes and rejected rays leave before the first wave-level operation: the ballots of the packet
// traversals and the LDS stash slots of trace_sample belong to the lanes that entered it, as in the
// render kernel, whose invalid pixels and untraced samples stay out of trace_sample.
template <uint32_t F>
__device__ __forceinline__ void shade_ray(const SceneD& S, uint64_t seed, uint64_t firstKey, uint32_t sample,
                                          const rt_ray* __restrict__ rays, int64_t i, double* __restrict__ rgb,
                                          uint8_t* __restrict__ status) {
  const double* r = (const double*)(rays + i);
  const V o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
  const double tmax = r[6];
  // finite: |x| <= DBL_MAX is false for NaN and for +-Inf
  const bool fin = fabs(o.x) <= DMAX && fabs(o.y) <= DMAX && fabs(o.z) <= DMAX && fabs(d.x) <= DMAX && fabs(d.y) <= DMAX &&
                   fabs(d.z) <= DMAX;
  const bool bad = !fin || (d.x == 0 && d.y == 0 && d.z == 0) || tmax != tmax;
  if (bad) {
    rgb[3 * i] = 0; rgb[3 * i + 1] = 0; rgb[3 * i + 2] = 0;
    if (status) status[i] = 2;
    return;
  }
  Key k;
  k.seed = seed; k.pixel = firstKey + (uint64_t)i; k.sample = sample; k.node = 1;
  k.tsite = SITE_TIME;
  Counters ct;
  const V c = trace_sample<false, F>(S, o, d, k, ct);
  rgb[3 * i] = c.x; rgb[3 * i + 1] = c.y; rgb[3 * i + 2] = c.z;
  if (status) status[i] = 0;
}

// the render kernel's launch bounds and occupancy hint: trace_sample is allocated as it is there
template <uint32_t F>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RT_RENDER_WAVES)))
shade_kernel(SceneD S, uint64_t seed, uint64_t firstKey, uint32_t sample, const rt_ray* __restrict__ rays, int64_t n,
             double* __restrict__ rgb, uint8_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  shade_ray<F>(S, seed, firstKey, sample, rays, i, rgb, status);
}

// RT_TRACE_SORT: lane `slot` handles ray order[slot] of the window -- its key, its colour, its status byte.
// order is a permutation of [0, n) (ray_sort.hip sort_order), so every index is in range.
template <uint32_t F>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RT_RENDER_WAVES)))
shade_kernel_idx(SceneD S, uint64_t seed, uint64_t firstKey, uint32_t sample, const rt_ray* __restrict__ rays, int64_t n,
                 double* __restrict__ rgb, uint8_t* __restrict__ status, const uint32_t* __restrict__ order) {
  const int64_t slot = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (slot >= n) return;
  shade_ray<F>(S, seed, firstKey, sample, rays, (int64_t)order[slot], rgb, status);
}

// camera_ray (camera_ray.h) for sample s of pixel first + i of a whole-frame layout (ray index = pixel key), into
// rays[i], tmax = +Inf: jittered when the frame has two samples or more. An untraced fisheye sample gets
// d = 0: every query rejects it. POSE: the ray is posed by the PoseD behind the arguments (camera_ray.h
// pose_ray) before that; the origin of an untraced sample is posed too, its d stays +0.
template <bool POSE = false, class... M>
__global__ void __launch_bounds__(256) camera_rays_kernel(SceneD S, ParamsD P, int s, int64_t first, int64_t count,
                                                          rt_ray* __restrict__ rays, M... pose) {
  RT_POSE_PACK_CHECK(POSE, M);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const int64_t px = first + i;
  const int row = (int)(px / P.W), col = (int)(px % P.W);
  V o, d;
  const bool traced = camera_ray<(uint32_t)FT_ALL>(S, P, row, col, s, P.spp != 1, o, d);
  pose_ray(o, d, pose...);
  if (!traced) d = mk(0, 0, 0);
  double* w = (double*)(rays + i);
  w[0] = o.x; w[1] = o.y; w[2] = o.z;
  w[3] = d.x; w[4] = d.y; w[5] = d.z;
  w[6] = __builtin_huge_val();
}

}  // namespace dv
}  // namespace rt
