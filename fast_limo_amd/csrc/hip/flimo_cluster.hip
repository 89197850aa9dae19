// fast_limo_amd/csrc/hip/flimo_cluster.hip -- Euclidean clusters of the stored points (gfx950).
//
// pcl::EuclideanClusterExtraction over the resident map (flimo_map_clusters, include/flimo_c.h): the connected components of the
// graph whose edges are the pairs of stored points with
//     sqdist3(p_i, p_j) < tol * tol            (strict; float32; tol * tol one float32 product)
// -- flimo_radius_search's predicate with a stored point as the query, symmetric bit for bit.  A point's label is the smallest
// insertion index of its component, so that the way the components are found cannot show in the result.
//
// Four launches (the second in chunks of stored points):
//  init     parent[t] = t.
//  link     a group of L lanes per stored point t walks the rows of t's ball (flimo_radius.h: the radius search's box and pruning,
//           radius_plan's lanes and tile walk).  A hit u < t -- every edge is met from both ends; the upper end takes it -- is united
//           with t by the hitting lane: lock-free union-find, hooking by index.
//  flatten  parent[t] = the root of t; count[root] += the points of a wave under that root (one add per wave and root).
//  finish   size, mask, label of the range; the counts of the whole map.
//
// The union-find (flimo_unionfind.h, shared with flimo_region.hip): lock-free, hooking by index, every access to `parent` in the link
// launch a relaxed agent-scope atomic; nothing waits for another workgroup.  The flatten is a launch of its own -- roots no longer
// change in it --, and what it writes (a point's root in the place of its parent) is again an ancestor.
#include <hip/hip_runtime.h>
#include "flimo_types.h"
#include "flimo_math.h"
#include "flimo_kernels.h"

#pragma clang fp contract(off)
#include "flimo_radius.h"
#include "flimo_unionfind.h"

namespace flimo {

// One round (radius_round's walk): lane `sub` of the group holds the range [lo, lo + len) of one row; the group walks the
// concatenated ranges together, consecutive lanes on consecutive candidates, RS_UNROLL loads in flight per lane.  Called by every
// lane of the wave (the shuffles are wave-wide).
template <int L>
__device__ __forceinline__ void cluster_round(const GridView& G, float gx, float gy, float gz, float r2, int lane, uint32_t lo, uint32_t len, uint32_t t,
                                              uint32_t& anchor, cl_gu32* parent) {
  const int sub = lane & (L - 1);
  uint32_t inc = len;
#pragma unroll
  for (int o = 1; o < L; o <<= 1) {
    const uint32_t v = __shfl_up(inc, o, L);
    if (sub >= o) inc += v;
  }
  const uint32_t exc = inc - len;
  const uint32_t total = __shfl(inc, L - 1, L);
  for (uint32_t c0 = 0; __any(c0 < total); c0 += (uint32_t)(L * RS_UNROLL)) {
    float4 p[RS_UNROLL];
    bool in[RS_UNROLL];
#pragma unroll
    for (int u = 0; u < RS_UNROLL; u++) {
      const uint32_t c = c0 + (uint32_t)(u * L + sub);
      in[u] = c < total;
      // the lane whose range holds candidate c: the last one whose exclusive sum is <= c
      int s = 0;
#pragma unroll
      for (int step = L / 2; step >= 1; step >>= 1) {
        const uint32_t e = __shfl(exc, s + step, L);
        if (e <= c) s += step;
      }
      const uint32_t slo = __shfl(lo, s, L), sexc = __shfl(exc, s, L);
      p[u] = in[u] ? G.pts[slo + (c - sexc)] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < RS_UNROLL; u++) {
      const float d = sqdist3(gx, gy, gz, p[u].x, p[u].y, p[u].z);
      const uint32_t ins = __float_as_uint(p[u].w);      // insertion index
      if (in[u] && d < r2 && ins < t) anchor = cl_unite(parent, ins, anchor);
    }
  }
}

__global__ __launch_bounds__(RS_BLOCK) void cluster_init_kernel(uint32_t* __restrict__ parent, uint32_t* __restrict__ count, uint32_t n) {
  const size_t t = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (t < n) { parent[t] = (uint32_t)t; count[t] = 0u; }
}

// stored points first .. first + nq - 1 as queries of their own map
template <int L, bool TILES>
__global__ __launch_bounds__(RS_BLOCK) void cluster_link_kernel(GridView G, const float4* __restrict__ map_raw, uint32_t first, int nq, float tol, float r2,
                                                                uint32_t* parent_) {
  static_assert(!TILES || L == 64, "the directory walk is one wave per point");
  cl_gu32* parent = (cl_gu32*)parent_;
  const int lane = threadIdx.x & 63;
  const int sub = lane & (L - 1);
  const size_t gq = ((size_t)blockIdx.x * RS_BLOCK + threadIdx.x) / (unsigned)L;
  const bool live = gq < (size_t)nq;
  const uint32_t t = first + (live ? (uint32_t)gq : 0u);
  const int maxdim = grid_maxdim(G);
  float gx = 0.f, gy = 0.f, gz = 0.f;
  if (live) { const float4 q = map_raw[t]; gx = q.x; gy = q.y; gz = q.z; }
  RadiusGeo g;
  const bool any_cell = radius_geo(G, maxdim, live ? gx : NAN, gy, gz, tol, g);
  uint32_t anchor = t;      // an index of t's tree, lowered as this lane learns of roots
  if (!TILES) {
    const int nyb = any_cell ? g.y1 - g.y0 + 1 : 0, nzb = any_cell ? g.z1 - g.z0 + 1 : 0;
    const int nrows = nyb * nzb;      // (the host takes this path only when a box has few rows)
    for (int jb = 0; __any(jb < nrows); jb += L) {
      const int j = jb + sub;
      uint32_t lo = 0, len = 0;
      if (j < nrows) radius_row(G, g, g.y0 + j % nyb, g.z0 + j / nyb, lo, len);
      cluster_round<L>(G, gx, gy, gz, r2, lane, lo, len, t, anchor, parent);
    }
  } else if (any_cell) {      // (wave-uniform: one point per wave) -- radius_kernel's walk through the directory
    const int ty0 = (g.y0 + GRID_PAD) >> G.ty, ty1 = (g.y1 + GRID_PAD) >> G.ty, tz0 = (g.z0 + GRID_PAD) >> G.tz, tz1 = (g.z1 + GRID_PAD) >> G.tz;
    const int tx0 = ((g.x0 * G.xs) >> 3) >> G.ts, tx1 = min((((g.x1 + 1) * G.xs) >> 3) >> G.ts, G.ntx - 1);
    const int ntyb = ty1 - ty0 + 1, npairs = ntyb * (tz1 - tz0 + 1);
    for (int pb = 0; pb < npairs; pb += 64) {
      const int pi = pb + lane;
      bool exists = false;
      if (pi < npairs) {
        const int ty_ = ty0 + pi % ntyb, tz_ = tz0 + pi / ntyb;
        const uint16_t* d = G.dir + (size_t)(tz_ * G.nty + ty_) * G.ntx;
        for (int tx = tx0; tx <= tx1; tx++) exists |= d[tx] != 0;
      }
      unsigned long long todo = __ballot(exists);
      while (todo) {
        const int b = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const int p = pb + b;
        const int ty_ = ty0 + p % ntyb, tz_ = tz0 + p / ntyb;
        const int ya = max(g.y0, (ty_ << G.ty) - GRID_PAD), yb = min(g.y1, ((ty_ + 1) << G.ty) - GRID_PAD - 1);
        const int za = max(g.z0, (tz_ << G.tz) - GRID_PAD), zb = min(g.z1, ((tz_ + 1) << G.tz) - GRID_PAD - 1);
        const int nyb = yb - ya + 1, nrows = nyb * (zb - za + 1);
        for (int jb = 0; jb < nrows; jb += 64) {
          const int j = jb + lane;
          uint32_t lo = 0, len = 0;
          if (j < nrows) radius_row(G, g, ya + j % nyb, za + j / nyb, lo, len);
          cluster_round<64>(G, gx, gy, gz, r2, lane, lo, len, t, anchor, parent);
        }
      }
    }
  }
}

// parent[t] = the root of t (its label), count[root] = the component's points.  A launch of its own: no root changes here, and a
// word that another thread has already flattened reads as an ancestor all the same.
__global__ __launch_bounds__(RS_BLOCK) void cluster_flatten_kernel(uint32_t* parent_, uint32_t* __restrict__ count, uint32_t n) {
  cl_gu32* parent = (cl_gu32*)parent_;
  const size_t i = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool todo = i < (size_t)n;
  uint32_t x = todo ? (uint32_t)i : 0u;
  if (todo) {
    uint32_t p = cl_load(parent, x);
    while (p != x) { x = p; p = cl_load(parent, x); }
    if (x != (uint32_t)i) __hip_atomic_store(parent + (uint32_t)i, x, CL_RLX_AGENT);
  }
  // one add per wave and root, not per point: a map that is one component would otherwise queue every point on one word
  unsigned long long rem = __ballot(todo);
  while (rem) {      // (wave-uniform)
    const int leader = __ffsll((long long)rem) - 1;
    const uint32_t r = (uint32_t)__shfl((int)x, leader, 64);
    const unsigned long long same = __ballot(todo && x == r);
    if (lane == leader) atomicAdd(count + r, (uint32_t)__popcll(same));
    if (x == r) todo = false;
    rem &= ~same;
  }
}

__device__ __forceinline__ bool cl_selected(uint32_t size, uint32_t min_size, uint32_t max_size) {
  return size >= min_size && (max_size == 0u || size <= max_size);
}
// thread t < n_map: the counts of the whole map from the roots (words[0] clusters, [1] largest, [2] selected clusters); where t
// is in the range [first, first + n): size / mask / label of point t - first and words[3], the ones of the mask.  Integer atomics,
// one per wave and word.
__global__ __launch_bounds__(RS_BLOCK) void cluster_finish_kernel(const uint32_t* __restrict__ label_all, const uint32_t* __restrict__ count, uint32_t n_map,
                                                                  uint32_t first, uint32_t n, uint32_t min_size, uint32_t max_size,
                                                                  int32_t* __restrict__ label, int32_t* __restrict__ size, unsigned char* __restrict__ mask,
                                                                  uint32_t* __restrict__ words) {
  const size_t gt = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = gt < (size_t)n_map;
  const uint32_t t = live ? (uint32_t)gt : 0u;
  uint32_t lab = 0, sz = 0;
  if (live) { lab = label_all[t]; sz = count[lab]; }
  const bool sel = live && cl_selected(sz, min_size, max_size);
  const bool root = live && lab == t;
  const bool in_range = live && t >= first && t - first < n;
  if (in_range) {
    const uint32_t i = t - first;
    if (label) label[i] = (int32_t)lab;
    if (size) size[i] = (int32_t)sz;
    mask[i] = sel ? 1 : 0;
  }
  const uint32_t n_root = (uint32_t)__popcll(__ballot(root)), n_sel_root = (uint32_t)__popcll(__ballot(root && sel)),
                 n_sel_pts = (uint32_t)__popcll(__ballot(in_range && sel));
  uint32_t big = root ? sz : 0u;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) big = max(big, (uint32_t)__shfl_xor((int)big, o, 64));
  if (lane == 0) {
    if (n_root) { atomicAdd(words + 0, n_root); atomicMax(words + 1, big); }
    if (n_sel_root) atomicAdd(words + 2, n_sel_root);
    if (n_sel_pts) atomicAdd(words + 3, n_sel_pts);
  }
}

hipError_t launch_cluster_init(hipStream_t st, uint32_t* parent, uint32_t* count, size_t n_map) {
  if (n_map == 0) return hipSuccess;
  hipLaunchKernelGGL(cluster_init_kernel, dim3((unsigned)((n_map + RS_BLOCK - 1) / RS_BLOCK)), dim3(RS_BLOCK), 0, st, parent, count, (uint32_t)n_map);
  return hipGetLastError();
}
hipError_t launch_cluster_link(hipStream_t st, const GridView& G, const float4* map_raw, unsigned first, int nq, float tol, uint32_t* parent) {
  const float r2 = tol * tol;      // one float32 product
  if (nq <= 0 || !(r2 > 0.f)) return hipSuccess;      // (d < 0 holds for no pair: no edges)
  int lanes; bool tiles;
  radius_plan(G, tol, lanes, tiles);
  const int L = tiles ? 64 : lanes;
  const unsigned blocks = (unsigned)(((size_t)nq * L + RS_BLOCK - 1) / RS_BLOCK);
  if (tiles) hipLaunchKernelGGL((cluster_link_kernel<64, true>), dim3(blocks), dim3(RS_BLOCK), 0, st, G, map_raw, first, nq, tol, r2, parent);
  else if (L == 8) hipLaunchKernelGGL((cluster_link_kernel<8, false>), dim3(blocks), dim3(RS_BLOCK), 0, st, G, map_raw, first, nq, tol, r2, parent);
  else if (L == 16) hipLaunchKernelGGL((cluster_link_kernel<16, false>), dim3(blocks), dim3(RS_BLOCK), 0, st, G, map_raw, first, nq, tol, r2, parent);
  else hipLaunchKernelGGL((cluster_link_kernel<64, false>), dim3(blocks), dim3(RS_BLOCK), 0, st, G, map_raw, first, nq, tol, r2, parent);
  return hipGetLastError();
}
hipError_t launch_cluster_flatten(hipStream_t st, uint32_t* parent, uint32_t* count, size_t n_map) {
  if (n_map == 0) return hipSuccess;
  hipLaunchKernelGGL(cluster_flatten_kernel, dim3((unsigned)((n_map + RS_BLOCK - 1) / RS_BLOCK)), dim3(RS_BLOCK), 0, st, parent, count, (uint32_t)n_map);
  return hipGetLastError();
}
hipError_t launch_cluster_finish(hipStream_t st, const uint32_t* label_all, const uint32_t* count, size_t n_map, size_t first, size_t n, int min_size,
                                 int max_size, int32_t* label, int32_t* size, unsigned char* mask, uint32_t* words) {
  if (n_map == 0) return hipSuccess;
  hipLaunchKernelGGL(cluster_finish_kernel, dim3((unsigned)((n_map + RS_BLOCK - 1) / RS_BLOCK)), dim3(RS_BLOCK), 0, st, label_all, count, (uint32_t)n_map,
                     (uint32_t)first, (uint32_t)n, (uint32_t)min_size, (uint32_t)max_size, label, size, mask, words);
  return hipGetLastError();
}

}  // namespace flimo
