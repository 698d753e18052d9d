// Adaptive sampling (rt_accum_select_*, rt_accum_add_selected): the accumulator's sample loop over a list of
// pixels with a sample count of their own each, the kernels that build such a list, and the frame and the
// error map of per-pixel counts.
#pragma once
#include "camera_ray.h"

namespace rt {
namespace dv {

// A selection is a list of pixel indices p = row * W + col in tile-major order: the 8 x 8 tiles row-major
// over the image, inside a tile the 6-bit Morton order (code bit 0 = column bit 0), pixels outside the image
// skipped. Runs of 4, 16 and 64 consecutive entries of a dense selection are 2 x 2, 4 x 4 and 8 x 8 pixel
// blocks, so the 64 / G pixels of a wave are neighbours as accum_kernel's tile is.
static constexpr int SEL_TILE = 8;

// lane (the Morton code) of tile -> its pixel index, -1 outside the image
__device__ __forceinline__ int64_t sel_pixel(int lane, int tile, int tilesX, int W, int H) {
  const int dx = (lane & 1) | ((lane >> 1) & 2) | ((lane >> 2) & 4);
  const int dy = ((lane >> 1) & 1) | ((lane >> 2) & 2) | ((lane >> 3) & 4);
  const int col = (tile % tilesX) * SEL_TILE + dx, row = (tile / tilesX) * SEL_TILE + dy;
  return (col < W && row < H) ? (int64_t)row * W + col : -1;
}

// error_kernel's value for one pixel of n >= 2 samples: the same operations in the same order
__device__ __forceinline__ float pixel_error(const double* __restrict__ sum, const double* __restrict__ sq, size_t o, int n) {
  const double dn = (double)n, dn1 = (double)(n - 1);
  double e = 0;
  for (int c = 0; c < 3; ++c) {
    const double m = sum[3 * o + c] / dn;
    const double mm = m * m;
    double v = sq[3 * o + c] / dn - mm;
    v = v < 0 ? 0 : v;
    const double ec = sqrt(((v * dn) / dn1) / dn);
    e = c == 0 ? ec : (ec > e ? ec : e);
  }
  return (float)e;
}

// Step 1 of a selection: one wave per tile, one lane per pixel; the ballot of the predicate and its
// population count per tile. MODE 0: every pixel of the image; 1: mask[p] != 0; 2: the error rule --
// cnt[p] < maxn and (cnt[p] < 2 or !(e_p <= thr)), e_p the float rt_accum_error gives (a NaN selects).
template <int MODE>
__global__ void __launch_bounds__(64) select_ballot_kernel(int W, int H, int tilesX, const uint8_t* __restrict__ mask,
                                                           const double* __restrict__ sum, const double* __restrict__ sq,
                                                           const int32_t* __restrict__ cnt, float thr, int maxn,
                                                           uint64_t* __restrict__ tballot, uint32_t* __restrict__ tcount) {
  const int tile = (int)blockIdx.x;
  const int64_t p = sel_pixel(threadIdx.x, tile, tilesX, W, H);
  bool pick = false;
  if (p >= 0) {
    if (MODE == 0) pick = true;
    if (MODE == 1) pick = mask[(size_t)p] != 0;
    if (MODE == 2) {
      const int n = cnt[(size_t)p];
      if (n < maxn) pick = n < 2 || !(pixel_error(sum, sq, (size_t)p, n) <= thr);
    }
  }
  const uint64_t b = __ballot(pick);
  if (threadIdx.x == 0) {
    tballot[tile] = b;
    tcount[tile] = (uint32_t)__popcll(b);
  }
}

#ifndef RT_POSE_TU  // the kernels defined outright: adaptive.hip only (pose.hip instantiates the posed accum_list_kernel)
// Step 2: the exclusive scan of the tile counts in place, c[ntiles] = the total. One block: every thread
// sums a contiguous run of counts, the 256 partial sums are scanned in LDS, then every thread writes its
// run's prefixes. No atomics: the list's order does not depend on scheduling.
__global__ void __launch_bounds__(256) select_scan_kernel(uint32_t* __restrict__ c, int64_t ntiles) {
  __shared__ uint32_t part[256];
  const int t = threadIdx.x;
  const int64_t per = (ntiles + 255) / 256;
  const int64_t lo = (int64_t)t * per, hi = lo + per < ntiles ? lo + per : ntiles;
  uint32_t s = 0;
  for (int64_t i = lo; i < hi; ++i) s += c[i];
  part[t] = s;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const uint32_t v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t run = part[t] - s;  // exclusive
  for (int64_t i = lo; i < hi; ++i) {
    const uint32_t v = c[i];
    c[i] = run;
    run += v;
  }
  if (t == 255) c[ntiles] = part[255];
}

// Step 3: the selected lanes of a tile write their pixel at the tile's offset plus the number of selected
// lanes below them (mbcnt of the ballot).
__global__ void __launch_bounds__(64) select_scatter_kernel(int W, int H, int tilesX, const uint64_t* __restrict__ tballot,
                                                            const uint32_t* __restrict__ toff, int32_t* __restrict__ list) {
  const int tile = (int)blockIdx.x;
  const uint64_t b = tballot[tile];
  const int lane = threadIdx.x;
  if (!((b >> lane) & 1)) return;
  const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
  list[(size_t)toff[tile] + below] = (int32_t)sel_pixel(lane, tile, tilesX, W, H);
}
#endif  // RT_POSE_TU

// accum_kernel over a list: one launch shades samples [cnt[p], cnt[p] + P.spp) of every listed pixel p, adds
// them to the carried sums by accum_kernel's rules, and sets cnt[p] += P.spp.
//
// The wave: 64 / G consecutive list entries x G sample lanes (P.G is make_params' for a render of P.spp
// samples). Lane j of slot q traces samples cnt[p] + j, cnt[p] + j + G, ... ; after each round the G colours
// go through LDS (cbuf aliases the traversal stack) and are added in sample order by accum_kernel's summing
// lanes: channel lanes with the sums in registers for G >= 4, the pixel's first lane straight onto HBM for
// G < 4. Every listed pixel belongs to one wave: no atomics.
//
// Nothing of a round's geometry is live across trace_sample: a lane finds its slot, the list entry, the
// pixel's row and column and its count again from the opaque lane index wherever it needs them. cnt[p] is
// written once, by the pixel's first lane after the last barrier, so every such read sees the count the
// launch started with. A slot past the list's end and a tail sample lane stay out of trace_sample and reach
// every barrier (the loop bounds are wave-uniform).
//
// POSE and the last argument: as accum_kernel's.
template <uint32_t F, bool MOM, bool POSE = false, class... M>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RT_RENDER_WAVES)))
accum_list_kernel(SceneD S, ParamsD P, const int32_t* __restrict__ list, size_t nlist, int32_t* cnt, double* __restrict__ sum,
                  double* __restrict__ sq, M... pose) {
  RT_POSE_PACK_CHECK(POSE, M);
  constexpr bool FLAG = (F & FT_CAMX) != 0;
  double* cbuf = rt_lds;  // 64 x 4 doubles (colour, traced)
  const int lane = threadIdx.x;
  const int G = P.G, n = P.spp;
  const int lgG = __builtin_ctz((unsigned)G);
  const size_t slot0 = (size_t)blockIdx.x * (size_t)(64 >> lgG);  // the wave's first list entry
  Key k;
  k.seed = P.seed;
  k.tsite = SITE_TIME;
  k.node = 1;
  double a = 0, a2 = 0;  // G >= 4: the channel lane's carried sums
  if (G >= 4) {
    const size_t slot = slot0 + (size_t)(lane >> lgG);
    const int j = lane & (G - 1);
    if (slot < nlist && j < 3) {
      const size_t at = 3 * (size_t)list[slot] + (size_t)j;
      a = sum[at];
      if (MOM) a2 = sq[at];
    }
  }
  for (int s0 = 0; s0 < n; s0 += G) {
    V cc = mk(0, 0, 0);
    bool traced = false;
    {
      const int l = opaque_lane(lane);
      const size_t slot = slot0 + (size_t)(l >> lgG);
      const int sl = s0 + (l & (G - 1));
      if (slot < nlist && sl < n) {
        const int p = list[slot];
        const int s = cnt[p] + sl;
        const int row = p / P.W, col = p - row * P.W;
        V o, d;
        traced = camera_ray<F>(S, P, row, col, s, true, o, d);
        if (traced) {
          pose_ray(o, d, pose...);
          k.pixel = (uint64_t)p;
          k.sample = (uint32_t)s;
          Counters ct;
          cc = trace_sample<false, F>(S, o, d, k, ct);
        }
      }
    }
    const int ln = opaque_lane(lane);
    cbuf[4 * ln + 0] = cc.x;
    cbuf[4 * ln + 1] = cc.y;
    cbuf[4 * ln + 2] = cc.z;
    if (FLAG) cbuf[4 * ln + 3] = traced ? 1.0 : 0.0;
    __syncthreads();
    const int m = (n - s0) < G ? (n - s0) : G;
    const int jq = ln & (G - 1);
    if (G >= 4) {
      if (jq < 3) {  // sample q's slot is the pixel's lane q: channel jq at b[4q], its flag at f[4q]
        const double* b = cbuf + 4 * (ln - jq) + jq;
        const double* f = cbuf + 4 * (ln - jq) + 3;
        for (int q = 0; q < m; ++q) {
          const double v = b[4 * q];
          if (!FLAG || f[4 * q] != 0) {
            a += v;
            if (MOM) {
              const double v2 = v * v;  // rounded, then added (the unit is built with -ffp-contract=off)
              a2 += v2;
            }
          }
        }
      }
    } else if (jq == 0) {
      const size_t slot = slot0 + (size_t)(ln >> lgG);
      if (slot < nlist) {
        const size_t at = 3 * (size_t)list[slot];
        double sr = sum[at], sg = sum[at + 1], sb = sum[at + 2];
        double qr = 0, qg = 0, qb = 0;
        if (MOM) { qr = sq[at]; qg = sq[at + 1]; qb = sq[at + 2]; }
        for (int q = 0; q < m; ++q) {
          const double* b = cbuf + 4 * (ln + q);
          if (!FLAG || b[3] != 0) {
            sr += b[0]; sg += b[1]; sb += b[2];
            if (MOM) {
              const double r2 = b[0] * b[0], g2 = b[1] * b[1], b2 = b[2] * b[2];
              qr += r2; qg += g2; qb += b2;
            }
          }
        }
        sum[at] = sr; sum[at + 1] = sg; sum[at + 2] = sb;
        if (MOM) { sq[at] = qr; sq[at + 1] = qg; sq[at + 2] = qb; }
      }
    }
    __syncthreads();  // the next round's shading tree reuses cbuf as its stack
  }
  const int l = opaque_lane(lane);
  const size_t slot = slot0 + (size_t)(l >> lgG);
  const int j = l & (G - 1);
  if (slot < nlist) {
    const size_t p = (size_t)list[slot];
    if (G >= 4 && j < 3) {
      sum[3 * p + (size_t)j] = a;
      if (MOM) sq[3 * p + (size_t)j] = a2;
    }
    if (j == 0) cnt[p] += n;  // after the last barrier: the wave's reads of the old count are done
  }
}

#ifndef RT_POSE_TU
// resolve_kernel with a sample count per pixel; a pixel without samples is black
__global__ void __launch_bounds__(256) resolve_counts_kernel(const double* __restrict__ sum, const int32_t* __restrict__ cnt,
                                                             int64_t npix, float* __restrict__ rgb, int32_t* __restrict__ argb) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const size_t o = (size_t)i;
  const int n = cnt[o];
  const double dn = (double)n;
  const V c = n == 0 ? mk(0, 0, 0) : clampc(mk(sum[3 * o] / dn, sum[3 * o + 1] / dn, sum[3 * o + 2] / dn));
  if (rgb) {
    rgb[3 * o + 0] = (float)c.x;
    rgb[3 * o + 1] = (float)c.y;
    rgb[3 * o + 2] = (float)c.z;
  }
  if (argb) {
    uint32_t v = (uint32_t)(255u << 24) + ((uint32_t)jd2i(c.x * 255) << 16) + ((uint32_t)jd2i(c.y * 255) << 8) +
                 (uint32_t)jd2i(c.z * 255);
    argb[o] = (int32_t)v;
  }
}

// error_kernel with a sample count per pixel; +Inf where a pixel has fewer than two samples
__global__ void __launch_bounds__(256) error_counts_kernel(const double* __restrict__ sum, const double* __restrict__ sq,
                                                           const int32_t* __restrict__ cnt, int64_t npix, float* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const size_t o = (size_t)i;
  const int n = cnt[o];
  err[o] = n < 2 ? __builtin_inff() : pixel_error(sum, sq, o, n);
}
#endif  // RT_POSE_TU

}  // namespace dv
}  // namespace rt
