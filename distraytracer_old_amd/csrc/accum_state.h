// The accumulator behind rt_accum_* as its two translation units see it: accum.hip (the whole-frame entries)
// and adaptive.hip (per-pixel sample counts, selections and the selective add).
#pragma once
#include <cstdint>

#include "rt_internal.h"

// The argument checks read nothing but the fields of this struct, and read them before anything else is
// touched.
struct rt_accum {
  uint32_t flags;  // RT_ACCUM_*
  int32_t W, H;
  int64_t done;  // samples rt_accum_add gave every pixel
  rt_scene* scene;
  rt_render_params rp;  // the frame: size, seed, flags (spp is set per add)
  double* sum;          // device [3 * W * H]
  double* sq;           // device [3 * W * H], RT_ACCUM_MOMENTS only
  void* last;           // hipStream_t of the last add
  // RT_ACCUM_COUNTS only (all zero otherwise, and in a fresh accumulator)
  int32_t* cnt;       // device [W * H]: the samples of each pixel. While !mixed every pixel has `done` and the
                      // array is filled from it where it is needed (counts_ready)
  int32_t* sel;       // device [W * H]: the current selection, tile-major
  int32_t* all;       // device [W * H]: every pixel, tile-major (rt_accum_add once the counts are mixed)
  uint64_t* tballot;  // device [tiles]: the select kernels' scratch, one ballot per 8 x 8 tile
  uint32_t* toff;     // device [tiles + 1]: per-tile counts, scanned in place; [tiles] = the list's length
  int64_t nsel;       // entries of sel
  int64_t bound;      // >= every pixel's count: done + the selective adds' counts
  int32_t has_sel;    // a selection was made since creation, reset or restore
  int32_t mixed;      // a selective add or rt_accum_restore_counts made the counts differ from done
  int32_t all_ready;  // `all` is filled
  // the camera pose (rt_accum_set_camera), behind everything older code reads
  int32_t has_pose;   // 0: none -- every add runs the un-posed kernels
  uint64_t pose_gen;  // counts the rt_accum_set_camera calls: a denoiser's guides are of one of them
  double pose[16];    // row-major camera -> world, valid by rt_camera_pose_check (has_pose only)
};

// tests/test_accum_abi.py hands the entries a host-made accumulator with these two fields set: the refusals
// it checks must need no device
static_assert(__builtin_offsetof(rt_accum, flags) == 0 && __builtin_offsetof(rt_accum, done) == 16, "rt_accum's checked fields");

namespace rt {

// adaptive.hip, for accum.hip's entries on an accumulator with RT_ACCUM_COUNTS. The current device is the
// scene's; `stream` is a hipStream_t. All return RT_OK or set the error.
int adaptive_alloc(rt_accum* a);                  // the count, selection and scratch buffers (rt_accum_create)
void adaptive_free(rt_accum* a);                  // (rt_accum_destroy)
void adaptive_uniform(rt_accum* a, int64_t n);    // every pixel has n samples again; the selection is gone
int adaptive_add_all(rt_accum* a, const rt::ParamsD& P, void* stream);  // rt_accum_add with mixed counts
int adaptive_resolve(rt_accum* a, float* d_rgb, int32_t* d_argb, void* stream);
int adaptive_error(rt_accum* a, float* d_err, void* stream);

// pose.hip: accum.hip's and adaptive.hip's launches of an accumulator with a camera pose (a->has_pose): the
// posed instantiations of accum_kernel and accum_list_kernel for the scene's variant, with the grid and the
// arguments of the un-posed launch. The current device is the scene's; `stream` is a hipStream_t.
int pose_launch_accum(rt_accum* a, const SceneD& sd, const ParamsD& P, unsigned blocks, void* stream);
int pose_launch_list(rt_accum* a, const SceneD& sd, const ParamsD& P, const int32_t* list, size_t nlist, unsigned blocks,
                     void* stream);

}  // namespace rt
