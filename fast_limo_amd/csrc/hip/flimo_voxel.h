// fast_limo_amd/csrc/hip/flimo_voxel.h
// The voxel of one stored point (flimo_map_voxels, include/flimo_c.h): a lattice anchored at the world origin, so that a voxel is
// the same set of space whatever the map's extent.  inv = 1.0f / leaf, c = floorf(p * inv) per axis -- one float32 product and a
// floor, the cells of pcl::VoxelGrid and of voxelkey_kernel shifted by whole cells --, OUTSIDE where a |c| reaches 2^20, otherwise
// three 21-bit fields (cz, cy, cx) from the top: ascending key is ascending (cz, cy, cx).  Host AND device: the key kernel
// (flimo_voxel.hip) and flimo_voxel_key_host run this one function.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace flimo {

constexpr int VOXEL_RUN = 64;                           // FLIMO_VOXEL_RUN: the slots of a run of the sum's shape
constexpr int VOXEL_KEEP_FIRST = 0, VOXEL_KEEP_NEAREST = 1;      // FLIMO_VOXEL_KEEP_*
constexpr float VOXEL_HALF = 1048576.0f;                // FLIMO_VOXEL_HALF: 2^20 cells either side of the origin
constexpr unsigned long long VOXEL_OUTSIDE = ~0ull;     // the key of an outside point: sorts behind every voxel

// the lane plans of the moments stage (flimo_set_voxel_plan): 0 chooses by the voxel's count
constexpr int VOXEL_PLAN_AUTO = 0, VOXEL_PLAN_G8 = 1, VOXEL_PLAN_G16 = 2, VOXEL_PLAN_G64 = 3, VOXEL_PLAN_RUNS = 4;
constexpr int VOXEL_PLAN_SORTED = 8;                    // + 8: the points are first written in sorted order (no gather in the moments)
// the integer words the launches count into: outside points, the largest count, the four plan lists' lengths, the ones of the mask
constexpr int VOXEL_W_OUTSIDE = 0, VOXEL_W_LARGEST = 1, VOXEL_W_LIST = 2, VOXEL_W_SEL = 6, VOXEL_WORDS = 8;
constexpr unsigned VOXEL_MANY = 1024;                   // automatic plan: a voxel of more points takes the many-runs path

// ijk = (cx, cy, cz); an outside point gets ijk = 0, the all-ones key and false
__host__ __device__ inline bool voxel_key(float x, float y, float z, float inv, int32_t ijk[3], unsigned long long* key) {
  const float c[3] = {floorf(x * inv), floorf(y * inv), floorf(z * inv)};
  bool inside = true;
  for (int a = 0; a < 3; a++) {
    const bool in = fabsf(c[a]) < VOXEL_HALF;           // (false for a NaN)
    inside = inside && in;
    ijk[a] = in ? (int32_t)c[a] : 0;
  }
  if (!inside) { ijk[0] = ijk[1] = ijk[2] = 0; *key = VOXEL_OUTSIDE; return false; }
  const unsigned long long h = 1ull << 20;
  *key = ((unsigned long long)(ijk[2] + (long long)h) << 42) | ((unsigned long long)(ijk[1] + (long long)h) << 21) |
         (unsigned long long)(ijk[0] + (long long)h);
  return true;
}
__host__ __device__ inline void voxel_cell_of_key(unsigned long long key, int32_t ijk[3]) {
  ijk[0] = (int32_t)(key & 0x1fffffull) - (1 << 20);
  ijk[1] = (int32_t)((key >> 21) & 0x1fffffull) - (1 << 20);
  ijk[2] = (int32_t)((key >> 42) & 0x1fffffull) - (1 << 20);
}

}  // namespace flimo
