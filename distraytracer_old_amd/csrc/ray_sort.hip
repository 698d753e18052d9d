// RT_TRACE_SORT (include/distraytracer.h): a batch of caller rays reordered for coherence on the device.
// Per window of rays: the bounds of the valid origins (wave reductions, one vector atomic per wave and
// bound), one sort key per ray (origin cell, then direction), a stable radix sort of (key, index) pairs
// (rocPRIM), and the query kernels' body run through the sorted indices (query_kernels.h
// query_kernel_idx). The indices are sorted iota values: a permutation whatever the keys are. The
// indexed instantiations of the heavy kernels live here, so that query.hip's are not disturbed and the
// two translation units compile in parallel.
// The host plumbing shared with the other units (HIP check, variant lookup, staging) is launch_common.h's.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstdlib>
#include <string>

// as render_minreg.hip: trace.hip alone holds the kernels trace_kernels.h defines outright
#define RT_MINREG_TU
#include "rt_internal.h"
#include "query_kernels.h"
#include "launch_common.h"

using namespace rt;

namespace {

// ---- sort keys -------------------------------------------------------------------------------------
// key = [rejected : 1][origin Morton : 3 x orgBits][direction Morton : 2 x dirBits]
constexpr int DIR_Q = 16;  // the direction is quantised to 16 bits per axis, the key keeps the top dirBits

// the rejection test of query_ray (query_kernels.h)
__device__ __forceinline__ bool ray_rejected(const double* r) {
  const bool fin = fabs(r[0]) <= dv::DMAX && fabs(r[1]) <= dv::DMAX && fabs(r[2]) <= dv::DMAX && fabs(r[3]) <= dv::DMAX &&
                   fabs(r[4]) <= dv::DMAX && fabs(r[5]) <= dv::DMAX;
  return !fin || (r[3] == 0 && r[4] == 0 && r[5] == 0) || r[6] != r[6];
}

// doubles as unsigned integers of the same order (atomic min / max on them); -0 < +0
__device__ __forceinline__ unsigned long long enc(double x) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double dec(unsigned long long c) {
  return __longlong_as_double((long long)((c >> 63) ? (c & 0x7fffffffffffffffull) : ~c));
}

// cell[0..2] = min, cell[3..5] = max of the valid origins (encoded; reset to ~0 / 0 on the stream)
__global__ void __launch_bounds__(256) bounds_kernel(const rt_ray* __restrict__ rays, int64_t n, unsigned long long* cell) {
  double lo[3] = {__builtin_huge_val(), __builtin_huge_val(), __builtin_huge_val()};
  double hi[3] = {-__builtin_huge_val(), -__builtin_huge_val(), -__builtin_huge_val()};
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const double* r = (const double*)(rays + i);
    if (ray_rejected(r)) continue;
    for (int a = 0; a < 3; a++) {
      lo[a] = fmin(lo[a], r[a]);
      hi[a] = fmax(hi[a], r[a]);
    }
  }
  for (int a = 0; a < 3; a++)
    for (int m = 32; m >= 1; m >>= 1) {
      lo[a] = fmin(lo[a], __shfl_xor(lo[a], m, 64));
      hi[a] = fmax(hi[a], __shfl_xor(hi[a], m, 64));
    }
  // every lane holds the wave's bounds; a wave without a valid ray (lo = +Inf > hi) leaves the cell alone
  const int lane = threadIdx.x & 63;
  if (lane < 3 && lo[0] <= hi[0]) {
    atomicMin(cell + lane, enc(lane == 0 ? lo[0] : lane == 1 ? lo[1] : lo[2]));
    atomicMax(cell + 3 + lane, enc(lane == 0 ? hi[0] : lane == 1 ? hi[1] : hi[2]));
  }
}

__device__ __forceinline__ uint32_t part1by1(uint32_t x) {  // 16 bits -> every second bit
  x &= 0xffffu;
  x = (x | (x << 8)) & 0x00ff00ffu;
  x = (x | (x << 4)) & 0x0f0f0f0fu;
  x = (x | (x << 2)) & 0x33333333u;
  x = (x | (x << 1)) & 0x55555555u;
  return x;
}
__device__ __forceinline__ uint32_t part1by2(uint32_t x) {  // 10 bits -> every third bit
  x &= 0x3ffu;
  x = (x | (x << 16)) & 0x030000ffu;
  x = (x | (x << 8)) & 0x0300f00fu;
  x = (x | (x << 4)) & 0x030c30c3u;
  x = (x | (x << 2)) & 0x09249249u;
  return x;
}

// q in [0, cells - 1] of t * cells, total: clamped in floating point before the conversion (NaN gives 0)
__device__ __forceinline__ uint32_t quant(double t, double cells) {
  return (uint32_t)fmin(fmax(t * cells, 0.0), cells - 1.0);
}

__global__ void __launch_bounds__(256) key_kernel(const rt_ray* __restrict__ rays, int64_t n, const unsigned long long* __restrict__ cell,
                                                  int orgBits, int dirBits, uint32_t base, unsigned long long* __restrict__ keys,
                                                  uint32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  idx[i] = base + (uint32_t)i;
  const double* r = (const double*)(rays + i);
  const int keyBits = 3 * orgBits + 2 * dirBits;
  if (ray_rejected(r)) {  // the largest key: rejected rays gather in the window's last waves
    keys[i] = (1ull << keyBits);
    return;
  }
  // origin: cell of a (1 << orgBits)^3 grid over the window's bounds. Halved operands keep hi - lo
  // finite for finite origins; an axis of zero (or, with no valid ray, NaN) extent gives cell 0.
  uint32_t oc = 0;
  for (int a = 0; a < 3; a++) {
    const double lo = dec(cell[a]) * 0.5, ext = dec(cell[3 + a]) * 0.5 - lo;
    const uint32_t q = ext > 0 ? quant((r[a] * 0.5 - lo) / ext, (double)(1 << orgBits)) : 0u;
    oc |= part1by2(q) << a;
  }
  // direction: scaled by its largest component first (no overflow at 1e300, no underflow of denormals:
  // that component is nonzero and finite), then the octahedral map of d / |d|_1 onto [-1, 1]^2
  const double m = fmax(fabs(r[3]), fmax(fabs(r[4]), fabs(r[5])));
  const double x = r[3] / m, y = r[4] / m, z = r[5] / m;
  const double s = fabs(x) + fabs(y) + fabs(z);  // in [1, 3]
  double u = x / s, v = y / s;
  if (z < 0) {
    const double fu = (1.0 - fabs(v)) * (u < 0 ? -1.0 : 1.0), fv = (1.0 - fabs(u)) * (v < 0 ? -1.0 : 1.0);
    u = fu;
    v = fv;
  }
  const uint32_t qu = quant(u * 0.5 + 0.5, (double)(1 << DIR_Q)), qv = quant(v * 0.5 + 0.5, (double)(1 << DIR_Q));
  const uint32_t dc = (part1by1(qu) | (part1by1(qv) << 1)) >> (2 * (DIR_Q - dirBits));
  keys[i] = ((unsigned long long)oc << (2 * dirBits)) | dc;
}

// ---- the indexed query kernels ------------------------------------------------------------------------
typedef void (*QueryIdxFn)(SceneD, uint64_t, uint64_t, const rt_ray*, int64_t, rt_hit*, uint8_t*, const uint32_t*);
struct QueryIdxVariant {
  uint32_t mask;
  QueryIdxFn fn[2][2];  // [lanes][any]
};
#define QV(F)                                                                                      \
  {                                                                                                \
    F, {                                                                                           \
      {dv::query_kernel_idx<F, true, false>, dv::query_kernel_idx<F, true, true>}, {               \
        dv::query_kernel_idx<F, false, false>, dv::query_kernel_idx<F, false, true>                \
      }                                                                                            \
    }                                                                                              \
  }
const QueryIdxVariant kQueryIdxVariants[] = {RT_VARIANT_MASKS(QV)};
#undef QV

// scratch layout for a capacity of C rays: keys[2][C] (8 B), idx[2][C] (4 B), the bounds cell, the temporary storage
constexpr size_t CELL_B = 64;
size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

void rt::sort_free(rt_scene* s) {
  (void)hipFree(s->sortDev);
  s->sortDev = nullptr;
  s->sortCap = s->sortTmpCap = 0;
}

int rt::sort_order(rt_scene* s, const rt_ray* d_rays, int64_t n, uint32_t base, const uint32_t** order, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (n <= 0 || n > s->sortWindow) return set_error(RT_E_INVALID, "sort_order: window size out of range");
  const unsigned endBit = (unsigned)(3 * s->sortOrgBits + 2 * s->sortDirBits + 1);
  size_t tmpB = 0;
  {
    rocprim::double_buffer<unsigned long long> k(nullptr, nullptr);
    rocprim::double_buffer<uint32_t> v(nullptr, nullptr);
    HIPCHK(rocprim::radix_sort_pairs(nullptr, tmpB, k, v, (size_t)n, 0u, endBit, st));
  }
  if ((size_t)n > s->sortCap || tmpB > s->sortTmpCap) {  // grow-only; hipFree waits for the work that used the old scratch
    const size_t cap = std::max((size_t)n, s->sortCap), tmpCap = std::max(round256(tmpB), s->sortTmpCap);
    sort_free(s);
    HIPCHK(hipMalloc(&s->sortDev, round256(cap * 16) + round256(cap * 8) + CELL_B + tmpCap));
    s->sortCap = cap;
    s->sortTmpCap = tmpCap;
  }
  const size_t C = s->sortCap;
  char* p = (char*)s->sortDev;
  unsigned long long* keys = (unsigned long long*)p;
  uint32_t* idx = (uint32_t*)(p + round256(C * 16));
  unsigned long long* cell = (unsigned long long*)(p + round256(C * 16) + round256(C * 8));
  void* tmp = (char*)cell + CELL_B;
  HIPCHK(hipMemsetAsync(cell, 0xff, 24, st));
  HIPCHK(hipMemsetAsync(cell + 3, 0, 24, st));
  // 8 rays per lane and at most 1024 blocks: 4096 waves' atomics on the six words at most
  const unsigned bb = (unsigned)std::min<int64_t>(1024, (n + 2047) / 2048);
  hipLaunchKernelGGL(bounds_kernel, dim3(bb), dim3(256), 0, st, d_rays, n, cell);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(key_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_rays, n, cell, s->sortOrgBits,
                     s->sortDirBits, base, keys, idx);
  HIPCHK(hipGetLastError());
  rocprim::double_buffer<unsigned long long> k(keys, keys + C);
  rocprim::double_buffer<uint32_t> v(idx, idx + C);
  size_t tb = s->sortTmpCap;
  HIPCHK(rocprim::radix_sort_pairs(tmp, tb, k, v, (size_t)n, 0u, endBit, st));
  *order = v.current();
  return RT_OK;
}

int rt::sorted_query(rt_scene* s, uint32_t flags, uint64_t seed, uint64_t firstKey, const rt_ray* d_rays, int64_t n, rt_hit* d_hits,
                     uint8_t* d_occ, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const SceneD sd = render_scene_view(s, render_flags_of(flags));
  const bool any = (flags & RT_TRACE_ANY) != 0;
  const QueryIdxVariant& v = variant_for(kQueryIdxVariants, render_variant_mask(s, render_flags_of(flags)));
  const QueryIdxFn fn = v.fn[(flags & RT_TRACE_LANES) ? 1 : 0][any ? 1 : 0];
  // windows are independent: indices, keys and records are relative to the window's first ray
  for (int64_t at = 0; at < n; at += s->sortWindow) {
    const int64_t m = std::min(s->sortWindow, n - at);
    const uint32_t* order = nullptr;
    const int rc = sort_order(s, d_rays + at, m, 0u, &order, st);
    if (rc != RT_OK) return rc;
    hipLaunchKernelGGL(fn, dim3((unsigned)((m + 63) / 64)), dim3(64), dv::LDS_RENDER_BYTES, st, sd, seed, firstKey + (uint64_t)at,
                       d_rays + at, m, any ? nullptr : d_hits + at, any ? d_occ + at : nullptr, order);
    HIPCHK(hipGetLastError());
  }
  return RT_OK;
}
