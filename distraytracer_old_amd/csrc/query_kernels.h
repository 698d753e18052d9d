// Ray queries (rt_trace_rays / rt_trace_rays_device): the caller's rays through the render kernels'
// closest-hit and any-hit code (trace_kernels.h closest / shadowed / make_hit), without shading.
#pragma once
#include "trace_kernels.h"

namespace rt {
namespace dv {

// One ray per lane, one wave per block (the traversals' LDS is per wave, indexed by lane).
// PK: the packet traversals of the render kernel (union walk, fp32 pre-tests, nearest-first order);
// else every BVH is traversed lane by lane in the reference's order, in fp64 throughout.
// ANY: myScene.calcShadow with dist = tmax into occ[], else myScene.findClosestRayHit into hits[].
// Tail lanes and rejected rays leave before the first wave-level operation: the ballots of the packet
// traversals count the active lanes only (every one is a __ballot under the caller's exec mask, and
// the wave-uniform frames in LDS are written and read by those same lanes), as in the render kernel,
// whose invalid pixels and untraced samples stay out of trace_sample.
// query_ray is the body both kernels below share: ray i of rays, keyed firstKey + i, into hits[i] / occ[i].
template <uint32_t F, bool PK, bool ANY>
__device__ __forceinline__ void query_ray(const SceneD& S, uint64_t seed, uint64_t firstKey, const rt_ray* __restrict__ rays,
                                          int64_t i, rt_hit* __restrict__ hits, uint8_t* __restrict__ occ) {
  const double* r = (const double*)(rays + i);
  const V o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
  const double tmax = r[6];
  // finite: |x| <= DBL_MAX is false for NaN and for +-Inf
  const bool fin = fabs(o.x) <= DMAX && fabs(o.y) <= DMAX && fabs(o.z) <= DMAX && fabs(d.x) <= DMAX && fabs(d.y) <= DMAX &&
                   fabs(d.z) <= DMAX;
  const bool bad = !fin || (d.x == 0 && d.y == 0 && d.z == 0) || tmax != tmax;
  rt_hit h;
  h.t = __builtin_huge_val();
  h.pos[0] = h.pos[1] = h.pos[2] = 0;
  h.normal[0] = h.normal[1] = h.normal[2] = 0;
  h.prim = h.top = h.material = -1;
  h.args = 0;
  h.flags = bad ? RT_HIT_BAD_RAY : 0u;
  h.pad = 0;
  if (bad) {
    if (ANY) occ[i] = 2;
    else hits[i] = h;
    return;
  }
  WRay w;
  w.o = o; w.d = nrmz(d); w.d0 = w.d; w.stable = false; w.moved = false; w.ver = 0;  // myRay ctor
  Key k;
  k.seed = seed; k.pixel = firstKey + (uint64_t)i; k.sample = 0; k.node = 1;
  k.tsite = ANY ? SITE_SHADOW_TIME : SITE_TIME;
  Counters ct;
  if constexpr (ANY) {
    occ[i] = shadowed<false, F, PK, false>(S, w, k, tmax, ct) ? 1 : 0;
  } else {
    const Best b = closest<false, F, PK>(S, w, k, ct);
    if (b.t != DMAX) {
      const HitRec hr = make_hit<F>(S, b, w, k);
      h.t = b.t;
      h.pos[0] = hr.fwd.x; h.pos[1] = hr.fwd.y; h.pos[2] = hr.fwd.z;
      h.normal[0] = hr.nrm.x; h.normal[1] = hr.nrm.y; h.normal[2] = hr.nrm.z;
      h.prim = (int32_t)hr.key;
      h.top = b.top;
      h.material = hr.mat;
      h.args = hr.args;
      // Best.inAcc says which CTM make_hit takes, and is 0 for an instanced primitive; one held by a list
      // (a sierpinski element) is still a list member whose hit reCalcCTMHitNorm rebuilds (PrimD.xfc >= 0)
      bool inAcc = b.inAcc != 0;
      if constexpr ((F & FT_INST) != 0) inAcc = inAcc || (b.inst >= 0 && S.prim[b.inst].xfc >= 0);
      h.flags = RT_HIT_HIT | (((F & FT_INST) && b.inst >= 0) ? RT_HIT_INSTANCE : 0u) | (inAcc ? RT_HIT_IN_ACCEL : 0u);
    }
    hits[i] = h;
  }
}

template <uint32_t F, bool PK, bool ANY>
__global__ void __launch_bounds__(64) query_kernel(SceneD S, uint64_t seed, uint64_t firstKey, const rt_ray* __restrict__ rays,
                                                   int64_t n, rt_hit* __restrict__ hits, uint8_t* __restrict__ occ) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  query_ray<F, PK, ANY>(S, seed, firstKey, rays, i, hits, occ);
}

// RT_TRACE_SORT (ray_sort.hip): lane `slot` handles ray order[slot] of the window -- its key, its record.
// order is a permutation of [0, n) (sorted iota values), so every index is in range whatever the keys were.
template <uint32_t F, bool PK, bool ANY>
__global__ void __launch_bounds__(64) query_kernel_idx(SceneD S, uint64_t seed, uint64_t firstKey,
                                                       const rt_ray* __restrict__ rays, int64_t n, rt_hit* __restrict__ hits,
                                                       uint8_t* __restrict__ occ, const uint32_t* __restrict__ order) {
  const int64_t slot = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (slot >= n) return;
  query_ray<F, PK, ANY>(S, seed, firstKey, rays, (int64_t)order[slot], hits, occ);
}

}  // namespace dv
}  // namespace rt
