// The variance-guided a-trous denoiser (include/distraytracer.h rt_denoise_*): the guide pack, the init, one
// filter level and the output conversion. All filter arithmetic is fp64, one IEEE operation per step in the
// order the public header fixes (the unit is built with -ffp-contract=off), so a restatement in numpy gives
// the same bytes. The kernels need nothing of the render kernels' headers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/distraytracer.h"

namespace rt {
namespace dn {

static constexpr double EPS = 1e-10;  // the header's epsilon of d_p and of the plane-distance scale
static constexpr int ROW_LANES = 64;  // a wave is 64 consecutive pixels of one image row
static constexpr int TILE_ROWS = 4;   // a block is 4 such rows: 64 x 4 pixels, 256 threads

// the two 16-byte guide records of a pixel
struct __attribute__((aligned(16))) GuideN {
  float nx, ny, nz;
  int32_t material;
};
struct __attribute__((aligned(16))) GuideP {
  float px, py, pz, depth;
};
// the 32-byte record of a pixel in a ping-pong plane buffer
struct __attribute__((aligned(16))) Plane {
  double r, g, b, v;
};

#define DNI __device__ __forceinline__

// min(1, c) as the render's colour clamp takes it (a NaN stays a NaN)
DNI double clamp1(double c) { return (1.0 <= c) ? 1.0 : c; }
// Java's (int) of a double, as the frame's ARGB packing uses it
DNI int32_t d2i(double v) {
  if (v != v) return 0;
  if (v >= 2147483647.0) return 2147483647;
  if (v <= -2147483648.0) return (int32_t)0x80000000;
  return (int32_t)v;
}
// h = [1/16, 1/4, 3/8, 1/4, 1/16] at offset i in -2 .. 2
DNI double tap_h(int i) { return i == 0 ? 0.375 : ((i == 1 || i == -1) ? 0.25 : 0.0625); }
// [1/4, 1/2, 1/4] at offset i in -1 .. 1
DNI double blur_h(int i) { return i == 0 ? 0.5 : 0.25; }

// rt_hit i of ray i -> the pixel's guide records. depth = (float)|pos - o| in fp64; a miss or a rejected ray
// has material -1 and +0 elsewhere.
__global__ void __launch_bounds__(256) guide_pack_kernel(const rt_ray* __restrict__ rays, const rt_hit* __restrict__ hits, int64_t npix,
                                                         GuideN* __restrict__ gn, GuideP* __restrict__ gp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const size_t o = (size_t)i;
  GuideN a = {0.f, 0.f, 0.f, -1};
  GuideP b = {0.f, 0.f, 0.f, 0.f};
  const rt_hit h = hits[o];
  if (h.flags & RT_HIT_HIT) {
    const double dx = h.pos[0] - rays[o].o[0], dy = h.pos[1] - rays[o].o[1], dz = h.pos[2] - rays[o].o[2];
    a.nx = (float)h.normal[0];
    a.ny = (float)h.normal[1];
    a.nz = (float)h.normal[2];
    a.material = h.material;
    b.px = (float)h.pos[0];
    b.py = (float)h.pos[1];
    b.pz = (float)h.pos[2];
    b.depth = (float)sqrt(((dx * dx) + (dy * dy)) + (dz * dz));
  }
  gn[o] = a;
  gp[o] = b;
}

// The filter's input planes from the accumulator's sums: c = min(1, sum / n) (rt_accum_resolve's double), v
// the largest channel of rt_accum_error's expression without its sqrt for n >= 2, 1 for n < 2; colour 0 at
// n = 0. cnt == nullptr: every pixel has `done` samples.
__global__ void __launch_bounds__(256) denoise_init_kernel(const double* __restrict__ sum, const double* __restrict__ sq,
                                                           const int32_t* __restrict__ cnt, int64_t done, int64_t npix,
                                                           Plane* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const size_t o = (size_t)i;
  const int64_t n = cnt ? (int64_t)cnt[o] : done;
  Plane p = {0.0, 0.0, 0.0, 1.0};
  if (n >= 1) {
    const double dn = (double)n;
    p.r = clamp1(sum[3 * o] / dn);
    p.g = clamp1(sum[3 * o + 1] / dn);
    p.b = clamp1(sum[3 * o + 2] / dn);
  }
  if (n >= 2) {
    const double dn = (double)n, dn1 = (double)(n - 1);
    double e = 0;
    for (int c = 0; c < 3; ++c) {
      const double m = sum[3 * o + c] / dn;
      const double mm = m * m;
      double v = sq[3 * o + c] / dn - mm;
      v = v < 0 ? 0 : v;
      const double ec = ((v * dn) / dn1) / dn;
      e = c == 0 ? ec : (ec > e ? ec : e);
    }
    p.v = e;
  }
  out[o] = p;
}

// One a-trous level at tap stride s: in -> out (the two ping-pong buffers). A block is 4 row segments of 64
// pixels, a wave one of them: lanes are consecutive in x, so every tap row of a wave is a run of consecutive
// records at any stride -- 16-byte-per-lane loads of the guides, two of the plane. The centre pixel's guides,
// colour and d_p stay in registers over the 25 taps. Every tap coordinate is checked against the image before
// its loads; a pixel writes only its own record: no atomics, nothing depends on scheduling.
// COUNTS: cnt[] gives each pixel's samples, and a pixel with none is neither filtered nor a tap.
template <bool COUNTS>
__global__ void __launch_bounds__(256) atrous_kernel(int W, int H, int blocksX, int s, int normal_log2, double sigma_l, double sigma_z,
                                                     const int32_t* __restrict__ cnt, const GuideN* __restrict__ gn,
                                                     const GuideP* __restrict__ gp, const Plane* __restrict__ in,
                                                     Plane* __restrict__ out) {
  const int bx = (int)(blockIdx.x % (unsigned)blocksX), by = (int)(blockIdx.x / (unsigned)blocksX);
  const int64_t x = (int64_t)bx * ROW_LANES + (threadIdx.x & (ROW_LANES - 1));
  const int64_t y = (int64_t)by * TILE_ROWS + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const size_t p = (size_t)y * (size_t)W + (size_t)x;
  const Plane cp = in[p];
  if (COUNTS && cnt[p] == 0) {  // out of the filter: carried through as it is
    out[p] = cp;
    return;
  }
  // g_p: the 3 x 3 [1/4, 1/2, 1/4]^2 blur of v at stride 1, coordinates clamped to the image, row-major from +0.0
  double g = 0.0;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
    int64_t yy = y + dy;
    yy = yy < 0 ? 0 : (yy >= H ? H - 1 : yy);
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      int64_t xx = x + dx;
      xx = xx < 0 ? 0 : (xx >= W ? W - 1 : xx);
      const double w = blur_h(dy) * blur_h(dx);
      g = g + w * in[(size_t)yy * (size_t)W + (size_t)xx].v;
    }
  }
  const double dp = sigma_l * sqrt(g) + EPS;
  const GuideN np_ = gn[p];
  const GuideP pp = gp[p];
  const int mat = np_.material;
  const double nx = (double)np_.nx, ny = (double)np_.ny, nz = (double)np_.nz;
  const double px = (double)pp.px, py = (double)pp.py, pz = (double)pp.pz;
  const double zden = sigma_z * (double)pp.depth + EPS;
  double S = 0.0, Cr = 0.0, Cg = 0.0, Cb = 0.0, V = 0.0;
#pragma unroll 1
  for (int dy = -2; dy <= 2; ++dy) {
    const int64_t qy = y + (int64_t)dy * s;
    if (qy < 0 || qy >= H) continue;
    const double hy = tap_h(dy);
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      const int64_t qx = x + (int64_t)dx * s;
      if (qx < 0 || qx >= W) continue;
      const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
      double w = 1.0;
      Plane cq = cp;
      if (dy != 0 || dx != 0) {
        if (COUNTS && cnt[q] == 0) continue;
        const GuideN nq = gn[q];
        if (nq.material != mat) continue;
        cq = in[q];
        double wn = 1.0, uz = 1.0;
        if (mat != -1) {
          const GuideP pq = gp[q];
          const double dot = ((nx * (double)nq.nx) + (ny * (double)nq.ny)) + (nz * (double)nq.nz);
          wn = dot > 0 ? dot : 0.0;
          for (int i = 0; i < normal_log2; ++i) wn = wn * wn;
          const double ex = (double)pq.px - px, ey = (double)pq.py - py, ez = (double)pq.pz - pz;
          const double t = fabs(((nx * ex) + (ny * ey)) + (nz * ez));
          const double rz = t / zden;
          uz = 1.0 + rz * rz;
        }
        const double ar = fabs(cp.r - cq.r), ag = fabs(cp.g - cq.g), ab = fabs(cp.b - cq.b);
        double m = ar;
        m = ag > m ? ag : m;
        m = ab > m ? ab : m;
        const double rl = m / dp;
        const double ul = 1.0 + rl * rl;
        w = wn / ((uz * uz) * (ul * ul));
      }
      const double k = (hy * tap_h(dx)) * w;
      S = S + k;
      Cr = Cr + k * cq.r;
      Cg = Cg + k * cq.g;
      Cb = Cb + k * cq.b;
      V = V + (k * k) * cq.v;
    }
  }
  Plane o;
  o.r = Cr / S;
  o.g = Cg / S;
  o.b = Cb / S;
  o.v = V / (S * S);
  out[p] = o;
}

// The frame of the final planes: rgb = (float)min(1, c), argb the render's packing of the clamped doubles.
__global__ void __launch_bounds__(256) denoise_output_kernel(const Plane* __restrict__ in, int64_t npix, float* __restrict__ rgb,
                                                             int32_t* __restrict__ argb) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= npix) return;
  const size_t o = (size_t)i;
  const Plane p = in[o];
  const double r = clamp1(p.r), g = clamp1(p.g), b = clamp1(p.b);
  if (rgb) {
    rgb[3 * o + 0] = (float)r;
    rgb[3 * o + 1] = (float)g;
    rgb[3 * o + 2] = (float)b;
  }
  if (argb) {
    const uint32_t v = (uint32_t)(255u << 24) + ((uint32_t)d2i(r * 255) << 16) + ((uint32_t)d2i(g * 255) << 8) + (uint32_t)d2i(b * 255);
    argb[o] = (int32_t)v;
  }
}

#undef DNI

}  // namespace dn
}  // namespace rt
