// Progressive sample accumulation (rt_accum_*): the render kernel's sample loop with the per-pixel sums
// carried in HBM between launches, and the kernels that turn the sums into a frame and an error map.
#pragma once
#include "camera_ray.h"

namespace rt {
namespace dv {

// One launch shades samples [done, done + P.spp) of every pixel of a whole frame and adds them to
// sum[3 * W * H] (and, MOM, their squares to sq[3 * W * H]), row-major by pixel.
//
// The wave is render_kernel's: a tw x th pixel tile x G sample lanes (P.G / P.tw / P.th are make_params'
// for a render of P.spp samples, so a chunk of 16 runs the layout of a 16-spp render and a chunk of one
// runs 8 x 8 pixels per wave). Lane j of a pixel traces samples done + j, done + j + G, ... of the
// chunk. Sample s is the ray a render of two or more samples shoots (camera_ray, jittered) under the key
// {seed, pixel, s, node 1, SITE_TIME}; neither depends on the frame's sample count, so the colours are
// the render's. After each round the G colours go through LDS (cbuf aliases the traversal stack, as in
// render_kernel) and are added in sample order, one IEEE add each, onto the carried sum: the chain of
// additions of a render, cut where the launches end. Every pixel belongs to one wave: no atomics.
//
// Who adds: with G >= 4 lane c < 3 of a pixel owns channel c. It loads the channel's carried sum (and
// square sum) before the first round, keeps it in registers across the rounds -- one or two doubles live
// across the shading tree -- and stores it after the last. With G < 4 (a chunk of one, two or three
// samples: at most two rounds) the pixel's first lane adds the three channels of a round straight onto
// HBM; keeping its three or six doubles in registers instead would be paid for by every chunk size, the
// kernel's register allocation being one for all G.
//
// A tail lane (s >= the chunk's end), a lane whose pixel is outside the image and a fisheye sample outside
// the image circle stay out of trace_sample, whose ballots and LDS stash slots belong to the lanes that
// entered; they still run every round's two barriers, the loop bounds being wave-uniform. An untraced
// sample adds nothing (the traced flag in cbuf's fourth slot; only the FT_CAMX masks can have one, the
// others neither store nor test the flag) and is counted by the host in done: the render divides by spp.
//
// POSE: the accumulator has a camera pose (rt_accum_set_camera). The last argument is then the PoseD, applied
// to the ray between camera_ray and trace_sample (camera_ray.h pose_ray); the key does not change. Without
// one the pack is empty, and the kernel is the code it was before there were poses.
template <uint32_t F, bool MOM, bool POSE = false, class... M>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RT_RENDER_WAVES)))
accum_kernel(SceneD S, ParamsD P, int done, double* __restrict__ sum, double* __restrict__ sq, M... pose) {
  RT_POSE_PACK_CHECK(POSE, M);
  constexpr bool FLAG = (F & FT_CAMX) != 0;
  double* cbuf = rt_lds;  // 64 x 4 doubles (colour, traced)
  const int lane = threadIdx.x;
  const int G = P.G, n = P.spp;
  const int tilesX = (P.W + P.tw - 1) >> __builtin_ctz((unsigned)P.tw);
  const int tile = blockIdx.x;  // row-major; the grid is exactly the layout's tiles
  Key k;
  k.seed = P.seed;
  k.tsite = SITE_TIME;
  k.node = 1;
  double a = 0, a2 = 0;  // G >= 4: the channel lane's carried sums
  if (G >= 4) {
    const PixGeo g = pix_geo_shift<0u>(lane, tile, tilesX, P.W, P);
    if (g.valid && g.j < 3) {
      const size_t at = 3 * ((size_t)g.row * (size_t)P.W + (size_t)g.col) + (size_t)g.j;
      a = sum[at];
      if (MOM) a2 = sq[at];
    }
  }
  for (int s0 = 0; s0 < n; s0 += G) {
    V cc = mk(0, 0, 0);
    bool traced = false;
    {
      const PixGeo g = pix_geo_shift<0u>(opaque_lane(lane), tile, tilesX, P.W, P);
      const int sl = s0 + g.j;
      if (g.valid && sl < n) {
        V o, d;
        traced = camera_ray<F>(S, P, g.row, g.col, done + sl, true, o, d);
        if (traced) {
          pose_ray(o, d, pose...);
          k.pixel = (uint64_t)g.row * (uint64_t)P.W + (uint64_t)g.col;
          k.sample = (uint32_t)(done + sl);
          Counters ct;
          cc = trace_sample<false, F>(S, o, d, k, ct);
        }
      }
    }
    // the lane's place is taken again from the opaque lane index, so that nothing of the round's
    // geometry has to stay in registers across the shading tree (render_kernel's wave_fast sums)
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
      const PixGeo g = pix_geo_shift<0u>(ln, tile, tilesX, P.W, P);
      if (g.valid) {
        const size_t at = 3 * ((size_t)g.row * (size_t)P.W + (size_t)g.col);
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
  if (G >= 4) {
    const PixGeo g = pix_geo_shift<0u>(opaque_lane(lane), tile, tilesX, P.W, P);
    if (g.valid && g.j < 3) {
      const size_t at = 3 * ((size_t)g.row * (size_t)P.W + (size_t)g.col) + (size_t)g.j;
      sum[at] = a;
      if (MOM) sq[at] = a2;
    }
  }
}

#ifndef RT_POSE_TU  // the kernels defined outright: accum.hip only (pose.hip instantiates the posed accum_kernel)
// the frame of n accumulated samples, one lane per pixel: render_kernel's epilogue on the carried sums --
// clampc(sum / n), the float conversion and myColor.getInt's packing. rgb or argb may be null.
__global__ void __launch_bounds__(256) resolve_kernel(const double* __restrict__ sum, int64_t npix, int64_t n,
                                                      float* __restrict__ rgb, int32_t* __restrict__ argb) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const size_t o = (size_t)i;
  const double dn = (double)n;
  const V c = clampc(mk(sum[3 * o] / dn, sum[3 * o + 1] / dn, sum[3 * o + 2] / dn));
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

// the standard error of a pixel's mean after n >= 2 samples, the largest of its three channels, as a
// float: in fp64 and in this order m = sum / n, v = sq / n - m * m, v = v < 0 ? 0 : v,
// e = sqrt((v * n / (n - 1)) / n)
__global__ void __launch_bounds__(256) error_kernel(const double* __restrict__ sum, const double* __restrict__ sq, int64_t npix,
                                                    int64_t n, float* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const size_t o = (size_t)i;
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
  err[o] = (float)e;
}
#endif  // RT_POSE_TU

}  // namespace dv
}  // namespace rt
