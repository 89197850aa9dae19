// fast_limo_amd/csrc/hip/flimo_region.h
// The predicates of the smooth-surface regions (flimo_map_regions, include/flimo_c.h): which stored points are SMOOTH and which
// pairs of them are joined.  A normal is the float32 row nx ny nz curvature of flimo_map_normals_range.  All float32, uncontracted,
// in the written association, so that region_joined(i, j) == region_joined(j, i) bit for bit.  Host AND device: the link kernel
// (flimo_region.hip) and flimo_region_joined_host run these functions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flimo_math.h"

#pragma clang fp contract(off)

namespace flimo {

constexpr uint32_t REGION_NONE = 0xffffffffu;      // no region / no smooth neighbour: label -1
// the integer words the finish counts into: regions, the largest one, selected regions, ones of the mask, smooth and unassigned points
constexpr int REGION_W_REGIONS = 0, REGION_W_LARGEST = 1, REGION_W_SEL = 2, REGION_W_SEL_PTS = 3, REGION_W_SMOOTH = 4, REGION_W_UNASSIGNED = 5,
              REGION_W_LISTED = 6, REGION_WORDS = 8;

__host__ __device__ inline bool region_finite(float v) { return fabsf(v) < __builtin_inff(); }      // (false for a NaN)
// a point HAS A NORMAL iff all four floats are finite
__host__ __device__ inline bool region_has_normal(float nx, float ny, float nz, float curv) {
  return region_finite(nx) && region_finite(ny) && region_finite(nz) && region_finite(curv);
}
// ... and is SMOOTH iff its curvature is at most max_curv (which may be INFINITY)
__host__ __device__ inline bool region_smooth(float nx, float ny, float nz, float curv, float max_curv) {
  return region_has_normal(nx, ny, nz, curv) && curv <= max_curv;
}
// the angle test of an edge: |n_i . n_j| >= min_cos, the dot product as x + (y + z)
__host__ __device__ inline bool region_aligned(float ax, float ay, float az, float bx, float by, float bz, float min_cos) {
  return fabsf(ax * bx + (ay * by + az * bz)) >= min_cos;
}
// the distance test of an edge: flimo_map_clusters' predicate; r2 = tol * tol, one float32 product
__host__ __device__ inline bool region_near(const float pi[3], const float pj[3], float r2) {
  return sqdist3(pi[0], pi[1], pi[2], pj[0], pj[1], pj[2]) < r2;
}
// both tests of an edge, for two points that have normals (smoothness is the caller's: a border point is joined without it)
__host__ __device__ inline bool region_joined(const float pi[3], const float ni[4], const float pj[3], const float nj[4], float r2, float min_cos) {
  return region_near(pi, pj, r2) && region_aligned(ni[0], ni[1], ni[2], nj[0], nj[1], nj[2], min_cos);
}

}  // namespace flimo
