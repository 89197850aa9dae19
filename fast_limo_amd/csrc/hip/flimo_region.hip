// fast_limo_amd/csrc/hip/flimo_region.hip -- smooth-surface regions of the stored points (gfx950).
//
// pcl::RegionGrowing restated without its seed order over the resident map (flimo_map_regions, include/flimo_c.h): a stored point is
// SMOOTH when it has a normal and its curvature is at most max_curv; two smooth points are joined when they are closer than tol
// (flimo_map_clusters' predicate) and their normals agree, |n_i . n_j| >= min_cos; a region is a connected component of that graph
// and carries the smallest insertion index of its smooth points.  With border != 0 a point that has a normal but is not smooth
// attaches to the region of its nearest smooth neighbour that passes both tests, by the key (distance bits, index), and carries
// nothing further.  The predicates are flimo_region.h's, host and device.
//
// The normals are those of flimo_map_normals_range over the whole map, left on the device (launch_knn_k_normals, flimo_knn_k.hip).
// Then five launches (the second in chunks of stored points):
//  init     parent[t] = t, count[t] = 0 (flimo_cluster.hip's), attach[t] = none.
//  link     cluster_link_kernel's walk: a group of L lanes per stored point t walks the rows of t's ball (flimo_radius.h).  A group
//           whose point has no normal walks nothing.  A smooth t takes the hits u < t as the cluster walk does -- every edge is met
//           from both ends, the upper end takes it --, fetches u's normal BY INSERTION INDEX, and unites where u is smooth and the
//           normals agree (flimo_unionfind.h: lock-free, hooking by index, every access to `parent` a relaxed agent-scope atomic,
//           nothing waits for another workgroup).  A border t looks at every hit, keeps the smallest key (bits of the float32
//           distance << 32 | index) of the smooth ones whose normal agrees, and the group reduces it by shuffles: attach[t], no 64-bit
//           atomics.  The choice depends on geometry, normals and smoothness alone, not on the components, so one walk serves both.
//  flatten  parent[t] = the root of t, for the smooth t.  A launch of its own: no root changes here.
//  count    label[t] (in the place of parent[t]): the root for a smooth t, root[attach[t]] for an attached border point, none
//           otherwise; count[label] += the points of a wave under that label (one add per wave and label); the smooth points.
//  finish   size, mask, label of the range; the counts of the whole map.
// The listing (flimo_map_region_list) keys every member of a selected region with its label (all ones otherwise) and goes through
// flimo_voxel.hip's sort, heads, classes and moments: the float64 sums have the voxels' shape.
//
// Why the gather: only a hit inside the ball whose index is below t (a quarter of the candidates of a ball's box in the mean) needs
// a normal, and the whole map's normals are 16 B a point, read-only during the launch: at 1M points they stay in the L2s and the
// Infinity Cache.  A cell-sorted copy would stream 16 B more for EVERY candidate, and the index's rows have slack between them.
#include <hip/hip_runtime.h>
#include "flimo_types.h"
#include "flimo_math.h"
#include "flimo_kernels.h"
#include "flimo_voxel.h"

#pragma clang fp contract(off)
#include "flimo_radius.h"
#include "flimo_unionfind.h"
#include "flimo_region.h"

namespace flimo {

struct RegionRule {
  float r2, min_cos, max_curv;
  int border;
};
__device__ __forceinline__ bool rg_smooth(const float4& n, float max_curv) { return region_smooth(n.x, n.y, n.z, n.w, max_curv); }

// cluster_round's walk.  own: the group's point is smooth (hits of lower index are united with it) or a border point (the best
// key is kept); a group of neither kind is given no rows.
template <int L>
__device__ __forceinline__ void region_round(const GridView& G, const float4* __restrict__ normal, const RegionRule& R, float gx, float gy, float gz,
                                             const float4& nt, bool own_smooth, int lane, uint32_t lo, uint32_t len, uint32_t t, uint32_t& anchor,
                                             unsigned long long& best, cl_gu32* parent) {
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
      if (in[u] && d < R.r2 && (own_smooth ? ins < t : ins != t)) {
        const float4 nu = normal[ins];
        if (rg_smooth(nu, R.max_curv) && region_aligned(nt.x, nt.y, nt.z, nu.x, nu.y, nu.z, R.min_cos)) {
          if (own_smooth) anchor = cl_unite(parent, ins, anchor);
          else best = min(best, ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)ins);
        }
      }
    }
  }
}

__global__ __launch_bounds__(RS_BLOCK) void region_init_kernel(uint32_t* __restrict__ attach, uint32_t n) {
  const size_t t = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (t < n) attach[t] = REGION_NONE;
}

// stored points first .. first + nq - 1 as queries of their own map
template <int L, bool TILES>
__global__ __launch_bounds__(RS_BLOCK) void region_link_kernel(GridView G, const float4* __restrict__ map_raw, const float4* __restrict__ normal,
                                                               uint32_t first, int nq, float tol, RegionRule R, uint32_t* parent_,
                                                               uint32_t* __restrict__ attach) {
  static_assert(!TILES || L == 64, "the directory walk is one wave per point");
  cl_gu32* parent = (cl_gu32*)parent_;
  const int lane = threadIdx.x & 63;
  const int sub = lane & (L - 1);
  const size_t gq = ((size_t)blockIdx.x * RS_BLOCK + threadIdx.x) / (unsigned)L;
  const bool live = gq < (size_t)nq;
  const uint32_t t = first + (live ? (uint32_t)gq : 0u);
  const int maxdim = grid_maxdim(G);
  float gx = 0.f, gy = 0.f, gz = 0.f;
  float4 nt = make_float4(0.f, 0.f, 0.f, 0.f);
  bool own_smooth = false, own_border = false;
  if (live) {
    const float4 q = map_raw[t];
    gx = q.x; gy = q.y; gz = q.z;
    nt = normal[t];
    own_smooth = rg_smooth(nt, R.max_curv);
    own_border = R.border != 0 && !own_smooth && region_has_normal(nt.x, nt.y, nt.z, nt.w);
  }
  const bool walks = own_smooth || own_border;      // (uniform over the group: one point)
  RadiusGeo g;
  const bool any_cell = radius_geo(G, maxdim, walks ? gx : NAN, gy, gz, tol, g);
  uint32_t anchor = t;      // an index of t's tree, lowered as this lane learns of roots
  unsigned long long best = ~0ull;
  if (!TILES) {
    const int nyb = any_cell ? g.y1 - g.y0 + 1 : 0, nzb = any_cell ? g.z1 - g.z0 + 1 : 0;
    const int nrows = nyb * nzb;      // (the host takes this path only when a box has few rows)
    for (int jb = 0; __any(jb < nrows); jb += L) {
      const int j = jb + sub;
      uint32_t lo = 0, len = 0;
      if (j < nrows) radius_row(G, g, g.y0 + j % nyb, g.z0 + j / nyb, lo, len);
      region_round<L>(G, normal, R, gx, gy, gz, nt, own_smooth, lane, lo, len, t, anchor, best, parent);
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
          region_round<64>(G, normal, R, gx, gy, gz, nt, own_smooth, lane, lo, len, t, anchor, best, parent);
        }
      }
    }
  }
  if (R.border != 0) {      // (uniform over the launch) the smallest key of the group's lanes: two 32-bit shuffles a step
#pragma unroll
    for (int o = 1; o < L; o <<= 1) {
      const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), o, L), lw = (uint32_t)__shfl_xor((int)(uint32_t)best, o, L);
      best = min(best, ((unsigned long long)hi << 32) | (unsigned long long)lw);
    }
    if (own_border && sub == 0 && best != ~0ull) attach[t] = (uint32_t)best;
  }
}

// parent[t] = the root of a smooth t.  A launch of its own: no root changes here, and a word that another thread has already
// flattened reads as an ancestor all the same.  A point that is not smooth was never hooked and nobody's path leads through it.
__global__ __launch_bounds__(RS_BLOCK) void region_flatten_kernel(uint32_t* parent_, const float4* __restrict__ normal, float max_curv, uint32_t n) {
  cl_gu32* parent = (cl_gu32*)parent_;
  const size_t i = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (i >= (size_t)n || !rg_smooth(normal[i], max_curv)) return;
  uint32_t x = (uint32_t)i;
  uint32_t p = cl_load(parent, x);
  while (p != x) { x = p; p = cl_load(parent, x); }
  if (x != (uint32_t)i) __hip_atomic_store(parent + (uint32_t)i, x, CL_RLX_AGENT);
}

// label[t] in the place of parent[t], count[label] = the region's points, words[REGION_W_SMOOTH] = the smooth points (the last
// launch that reads the normals).  The words a thread reads of other points are those of smooth points, which this launch leaves
// as they are.
__global__ __launch_bounds__(RS_BLOCK) void region_count_kernel(uint32_t* label_all, const uint32_t* __restrict__ attach,
                                                                const float4* __restrict__ normal, float max_curv, uint32_t* __restrict__ count,
                                                                uint32_t* __restrict__ words, uint32_t n) {
  const size_t i = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = i < (size_t)n;
  uint32_t x = REGION_NONE;
  bool smooth = false;
  if (live) {
    smooth = rg_smooth(normal[i], max_curv);
    if (smooth) {
      x = label_all[i];
    } else {
      const uint32_t j = attach[i];
      if (j != REGION_NONE) x = label_all[j];
      label_all[i] = x;
    }
  }
  const uint32_t n_smooth = (uint32_t)__popcll(__ballot(smooth));
  if (lane == 0 && n_smooth) atomicAdd(words + REGION_W_SMOOTH, n_smooth);
  bool todo = live && x != REGION_NONE;
  // one add per wave and label, not per point: a map that is one region would otherwise queue every point on one word
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

__device__ __forceinline__ bool rg_selected(uint32_t size, uint32_t min_size, uint32_t max_size) {
  return size >= min_size && (max_size == 0u || size <= max_size);
}
// thread t < n_map: the counts of the whole map (words: flimo_region.h); where t is in the range [first, first + n): size / mask /
// label of point t - first and the ones of the mask.  keys (may be null): the listing's key of every stored point.  Integer
// atomics, one per wave and word.
__global__ __launch_bounds__(RS_BLOCK) void region_finish_kernel(const uint32_t* __restrict__ label_all, const uint32_t* __restrict__ count,
                                                                 uint32_t n_map, uint32_t first, uint32_t n, uint32_t min_size, uint32_t max_size, int32_t* __restrict__ label,
                                                                 int32_t* __restrict__ size, unsigned char* __restrict__ mask,
                                                                 unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals,
                                                                 uint32_t* __restrict__ words) {
  const size_t gt = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = gt < (size_t)n_map;
  const uint32_t t = live ? (uint32_t)gt : 0u;
  uint32_t lab = REGION_NONE, sz = 0;
  if (live) {
    lab = label_all[t];
    if (lab != REGION_NONE) sz = count[lab];
  }
  const bool assigned = live && lab != REGION_NONE;
  const bool sel = assigned && rg_selected(sz, min_size, max_size);
  const bool root = assigned && lab == t;
  const bool in_range = live && t >= first && t - first < n;
  if (in_range) {
    const uint32_t i = t - first;
    if (label) label[i] = (int32_t)lab;      // (none: -1)
    if (size) size[i] = (int32_t)sz;
    if (mask) mask[i] = sel ? 1 : 0;
  }
  if (live && keys) { keys[t] = sel ? (unsigned long long)lab : VOXEL_OUTSIDE; vals[t] = t; }
  const uint32_t n_root = (uint32_t)__popcll(__ballot(root)), n_sel_root = (uint32_t)__popcll(__ballot(root && sel)),
                 n_sel_pts = (uint32_t)__popcll(__ballot(in_range && sel)),
                 n_none = (uint32_t)__popcll(__ballot(live && !assigned)), n_listed = (uint32_t)__popcll(__ballot(sel));
  uint32_t big = root ? sz : 0u;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) big = max(big, (uint32_t)__shfl_xor((int)big, o, 64));
  if (lane == 0) {
    if (n_root) { atomicAdd(words + REGION_W_REGIONS, n_root); atomicMax(words + REGION_W_LARGEST, big); }
    if (n_sel_root) atomicAdd(words + REGION_W_SEL, n_sel_root);
    if (n_sel_pts) atomicAdd(words + REGION_W_SEL_PTS, n_sel_pts);
    if (n_none) atomicAdd(words + REGION_W_UNASSIGNED, n_none);
    if (n_listed) atomicAdd(words + REGION_W_LISTED, n_listed);
  }
}

// the listing: label[r] = the key of region r's segment
__global__ __launch_bounds__(RS_BLOCK) void region_list_label_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ seg,
                                                                     uint32_t nr, int32_t* __restrict__ label) {
  const size_t r = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (r < (size_t)nr) label[r] = (int32_t)(uint32_t)keys[seg[r]];
}

static inline dim3 rg_grid(size_t threads) { return dim3((unsigned)((threads + RS_BLOCK - 1) / RS_BLOCK)); }

hipError_t launch_region_init(hipStream_t st, uint32_t* parent, uint32_t* count, uint32_t* attach, size_t n_map) {
  if (n_map == 0) return hipSuccess;
  const hipError_t e = launch_cluster_init(st, parent, count, n_map);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(region_init_kernel, rg_grid(n_map), dim3(RS_BLOCK), 0, st, attach, (uint32_t)n_map);
  return hipGetLastError();
}
hipError_t launch_region_link(hipStream_t st, const GridView& G, const float4* map_raw, const float4* normal, unsigned first, int nq, float tol,
                              float min_cos, float max_curv, int border, uint32_t* parent, uint32_t* attach) {
  const RegionRule R{tol * tol, min_cos, max_curv, border};      // (r2: one float32 product)
  if (nq <= 0 || !(R.r2 > 0.f)) return hipSuccess;      // (d < 0 holds for no pair: no edges, no border)
  int lanes; bool tiles;
  radius_plan(G, tol, lanes, tiles);
  const int L = tiles ? 64 : lanes;
  const unsigned blocks = (unsigned)(((size_t)nq * L + RS_BLOCK - 1) / RS_BLOCK);
  if (tiles) hipLaunchKernelGGL((region_link_kernel<64, true>), dim3(blocks), dim3(RS_BLOCK), 0, st, G, map_raw, normal, first, nq, tol, R, parent, attach);
  else if (L == 8) hipLaunchKernelGGL((region_link_kernel<8, false>), dim3(blocks), dim3(RS_BLOCK), 0, st, G, map_raw, normal, first, nq, tol, R, parent, attach);
  else if (L == 16) hipLaunchKernelGGL((region_link_kernel<16, false>), dim3(blocks), dim3(RS_BLOCK), 0, st, G, map_raw, normal, first, nq, tol, R, parent, attach);
  else hipLaunchKernelGGL((region_link_kernel<64, false>), dim3(blocks), dim3(RS_BLOCK), 0, st, G, map_raw, normal, first, nq, tol, R, parent, attach);
  return hipGetLastError();
}
hipError_t launch_region_labels(hipStream_t st, uint32_t* parent, const uint32_t* attach, const float4* normal, float max_curv, uint32_t* count,
                                uint32_t* words, size_t n_map) {
  if (n_map == 0) return hipSuccess;
  hipLaunchKernelGGL(region_flatten_kernel, rg_grid(n_map), dim3(RS_BLOCK), 0, st, parent, normal, max_curv, (uint32_t)n_map);
  hipLaunchKernelGGL(region_count_kernel, rg_grid(n_map), dim3(RS_BLOCK), 0, st, parent, attach, normal, max_curv, count, words, (uint32_t)n_map);
  return hipGetLastError();
}
hipError_t launch_region_finish(hipStream_t st, const uint32_t* label_all, const uint32_t* count, size_t n_map,
                                size_t first, size_t n, int min_size, int max_size, int32_t* label, int32_t* size, unsigned char* mask,
                                unsigned long long* keys, uint32_t* vals, uint32_t* words) {
  if (n_map == 0) return hipSuccess;
  hipLaunchKernelGGL(region_finish_kernel, rg_grid(n_map), dim3(RS_BLOCK), 0, st, label_all, count, (uint32_t)n_map, (uint32_t)first,
                     (uint32_t)n, (uint32_t)min_size, (uint32_t)max_size, label, size, mask, keys, vals, words);
  return hipGetLastError();
}
hipError_t launch_region_list_labels(hipStream_t st, const unsigned long long* keys, const uint32_t* seg, unsigned nr, int32_t* label) {
  if (nr == 0) return hipSuccess;
  hipLaunchKernelGGL(region_list_label_kernel, rg_grid(nr), dim3(RS_BLOCK), 0, st, keys, seg, nr, label);
  return hipGetLastError();
}

}  // namespace flimo
