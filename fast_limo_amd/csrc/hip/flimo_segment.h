// fast_limo_amd/csrc/hip/flimo_segment.h -- map segments: which correction a stored point gets, and the move itself.
//
// A segment is a run of insertion indices [begin[s], begin[s + 1]) (include/flimo_c.h, "Map segments").  The two functions below
// are the ONE definition of a correction, compiled for the host (flimo_seg_move_host) and for the kernel (flimo_segment.hip);
// tests/segments_common.py restates them in numpy and every comparison is bit for bit.
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FLIMO_SEG_HD __host__ __device__ __forceinline__
#else
#define FLIMO_SEG_HD inline
#endif

namespace flimo {

// the largest s in [0, S) with begin[s] <= i (begin[0] = 0, begin ascending, S >= 1): an empty segment is never the answer
// unless every later one starts beyond i as well
FLIMO_SEG_HD uint32_t seg_find(const uint64_t* begin, uint32_t S, uint64_t i) {
  uint32_t lo = 0u, hi = S;                  // begin[lo] <= i, and begin[hi] > i or hi == S
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (begin[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// T: row-major 3 x 4, new world <- old world, applied as given.  float64, one rounding per written operation, nothing contracted;
// then one rounding to float32.
FLIMO_SEG_HD void seg_move(const double* T, float x, float y, float z, float out[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double X = (double)x, Y = (double)y, Z = (double)z;
  const double r0 = T[0] * X + (T[1] * Y + (T[2] * Z + T[3]));
  const double r1 = T[4] * X + (T[5] * Y + (T[6] * Z + T[7]));
  const double r2 = T[8] * X + (T[9] * Y + (T[10] * Z + T[11]));
  out[0] = (float)r0; out[1] = (float)r1; out[2] = (float)r2;
}

}  // namespace flimo

#if defined(__HIPCC__)
#include "flimo_kernels.h"
namespace flimo {

// One corrected point per stored point of in[first, first + n): segment s = seg_find(d_begin, S, i), moved by d_T[s] (both on the
// device: d_begin [S] ascending from 0, d_T [S][12]).  out (may be null: counts and box only) receives point i at out[i - first],
// w = the bits of i.  *changed: points with different bits in x, y or z; *nonfinite: points with a moved component that is not
// finite; bb: the moved points' box (untouched when n == 0).  slab: points per workgroup and step (a multiple of 256), blocks: the
// grid; neither changes a result.  One launch; ends synchronised.
constexpr size_t SEG_SLAB_DEFAULT = 2048, SEG_SLAB_MAX = 16384;
hipError_t seg_move_launch(hipStream_t st, const float4* in, size_t first, size_t n, const uint64_t* d_begin, const double* d_T, uint32_t S,
                           float4* out, size_t slab, int blocks, MapBuildScratch& scratch, size_t* changed, size_t* nonfinite, float bb[6]);

}  // namespace flimo
#endif
