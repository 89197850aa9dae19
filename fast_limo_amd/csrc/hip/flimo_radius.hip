// fast_limo_amd/csrc/hip/flimo_radius.hip -- exact radius search over the resident map (gfx950).
//
// Octree::radiusSearch (reference Objects/Octree.hpp:453-523): every stored point p of a query q with
//     sqdist3(q, p) < radius * radius          (strict; float32; radius * radius one float32 product, Octree.hpp:467)
// Two remarks.
//  * The reference takes every point of an octant whose farthest corner lies inside the ball WITHOUT testing the point
//    (Octree.hpp:485-503).  In exact arithmetic that is the same set; in float32 it could differ by a rounding.
//    tests/test_radius_search_host.py restates that traversal over the oracle's octree and finds no query on which it does.
//    The contract here is the predicate.
//  * The reference's order within a query is its tree's traversal order; it is not reproduced.  Unsorted: the order of the walk
//    below, a function of the map's layout alone (no atomics), so two calls on an unchanged map agree.  Sorted: ascending by
//    (squared-distance bits, insertion index), a total order.
//
// One walk, two uses (radius_kernel<FILL, ..>): the count launch and the fill launch visit the same rows and the same candidates in the
// same order; the fill writes at offsets[q] + results so far + rank of the lane among the hits of its group (a ballot).
//
// The walk.  The ball's box in cells is a set of rows (y, z); a row whose distance to the query in the y-z plane exceeds the radius
// is dropped, of a kept row only the cells |x - qx| <= sqrt(r^2 - d_yz^2) (widened) are read, as ONE range [lo, hi) of `pts`
// (grid_row_range).  All pruning is conservative -- the query's cell and the rounding margin as knn_far_kernel computes them -- and
// the float32 `< r^2` test alone decides membership.  A GROUP of L lanes serves a query (L = 8, 16 or 64, chosen by the host from
// the number of rows the box spans): per round each lane fetches one row's range, then the group walks the concatenated ranges
// together, consecutive lanes on consecutive candidates (16-byte loads, consecutive in memory within a row), RS_UNROLL loads in
// flight per lane.  TILES (one wave per query): a box of many rows is walked through the directory instead -- (y, z) tile columns
// none of whose tiles along x exists are skipped 64 at a time, so a ball of kilometres costs the tiles that exist.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include "flimo_types.h"
#include "flimo_math.h"
#include "flimo_kernels.h"

#pragma clang fp contract(off)
#include "flimo_radius.h"      // the ball's box, a row's pruning, the group mask: shared with flimo_cluster.hip

namespace flimo {

// where the fill puts a result: plain arrays (any may be null) or, for the sorted form, 64-bit keys only
struct RadiusOut {
  int32_t* idx;
  float* sqd;
  float* xyz;
  unsigned long long* keys;      // (distance bits << 32) | insertion index
};

// One round: lane `sub` of the group holds the range [lo, lo + len) of one row (len = 0: none).  The group walks the concatenated
// ranges together.  Called by every lane of the wave (the shuffles and ballots are wave-wide); `live`: this lane's group has a
// query.  Returns with `found` advanced by the group's hits.
template <bool FILL, int L>
__device__ __forceinline__ void radius_round(const GridView& G, float gx, float gy, float gz, float r2, int lane, uint32_t lo, uint32_t len,
                                             unsigned long long base, uint32_t& found, unsigned long long& cand, const RadiusOut& O) {
  const int sub = lane & (L - 1);
  // exclusive prefix sum of the lengths over the group
  uint32_t inc = len;
#pragma unroll
  for (int o = 1; o < L; o <<= 1) {
    const uint32_t v = __shfl_up(inc, o, L);
    if (sub >= o) inc += v;
  }
  const uint32_t exc = inc - len;
  const uint32_t total = __shfl(inc, L - 1, L);
  cand += total;
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
      const bool hit = in[u] && d < r2;
      const unsigned long long b = __ballot(hit);
      uint32_t rank, hits;
      if (L == 64) {
        rank = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        hits = (uint32_t)__popcll(b);
      } else {
        const uint32_t m = group_mask_of<L>(b, lane);
        rank = (uint32_t)__popc(m & ((1u << sub) - 1u));
        hits = (uint32_t)__popc(m);
      }
      if (FILL && hit) {
        const unsigned long long at = base + found + rank;
        const uint32_t ins = __float_as_uint(p[u].w);      // insertion index: flimo_map_points' order, what flimo_knn returns
        if (O.keys) O.keys[at] = ((unsigned long long)__float_as_uint(d) << 32) | ins;
        if (O.idx) O.idx[at] = (int32_t)ins;
        if (O.sqd) O.sqd[at] = d;
        if (O.xyz) { O.xyz[3 * at] = p[u].x; O.xyz[3 * at + 1] = p[u].y; O.xyz[3 * at + 2] = p[u].z; }
      }
      found += hits;
    }
  }
}

template <bool FILL, int L, bool TILES>
__global__ __launch_bounds__(RS_BLOCK) void radius_kernel(GridView G, const float* __restrict__ qxyz, int nq, float radius, float r2,
                                                          const unsigned long long* __restrict__ offsets, uint32_t* __restrict__ cnt,
                                                          unsigned long long* __restrict__ cand_out, RadiusOut O) {
  static_assert(!TILES || L == 64, "the directory walk is one wave per query");
  const int lane = threadIdx.x & 63;
  const int sub = lane & (L - 1);
  const size_t gq = ((size_t)blockIdx.x * RS_BLOCK + threadIdx.x) / (unsigned)L;
  const bool live = gq < (size_t)nq;
  const int q = live ? (int)gq : 0;
  const int maxdim = grid_maxdim(G);
  float gx = 0.f, gy = 0.f, gz = 0.f;
  if (live) { gx = qxyz[3 * q]; gy = qxyz[3 * q + 1]; gz = qxyz[3 * q + 2]; }
  RadiusGeo g;
  const bool any_cell = radius_geo(G, maxdim, live ? gx : NAN, gy, gz, radius, g);
  const unsigned long long base = (FILL && live) ? offsets[q] : 0ull;
  uint32_t found = 0;
  unsigned long long cand = 0;
  if (!TILES) {
    const int nyb = any_cell ? g.y1 - g.y0 + 1 : 0, nzb = any_cell ? g.z1 - g.z0 + 1 : 0;
    const int nrows = nyb * nzb;      // (the host takes this path only when a box has few rows)
    for (int jb = 0; __any(jb < nrows); jb += L) {
      const int j = jb + sub;
      uint32_t lo = 0, len = 0;
      if (j < nrows) radius_row(G, g, g.y0 + j % nyb, g.z0 + j / nyb, lo, len);
      radius_round<FILL, L>(G, gx, gy, gz, r2, lane, lo, len, base, found, cand, O);
    }
  } else if (any_cell) {      // (wave-uniform: one query per wave)
    const int ty0 = (g.y0 + GRID_PAD) >> G.ty, ty1 = (g.y1 + GRID_PAD) >> G.ty, tz0 = (g.z0 + GRID_PAD) >> G.tz, tz1 = (g.z1 + GRID_PAD) >> G.tz;
    const int tx0 = ((g.x0 * G.xs) >> 3) >> G.ts, tx1 = min((((g.x1 + 1) * G.xs) >> 3) >> G.ts, G.ntx - 1);
    const int ntyb = ty1 - ty0 + 1, npairs = ntyb * (tz1 - tz0 + 1);
    for (int pb = 0; pb < npairs; pb += 64) {
      // 64 (y, z) tile columns at a time: does any tile of the column along the box's x extent exist?
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
          radius_round<FILL, 64>(G, gx, gy, gz, r2, lane, lo, len, base, found, cand, O);
        }
      }
    }
  }
  if (!FILL && live && sub == 0) {
    cnt[q] = found;
    if (cand_out) cand_out[q] = cand;
  }
}

// the sorted form: keys (distance bits, insertion index) -> idx / sqd / xyz (gathered from the map in insertion order)
__global__ __launch_bounds__(RS_BLOCK) void radius_unpack_kernel(const unsigned long long* __restrict__ keys, size_t n, const float4* __restrict__ map_raw,
                                                                 int32_t* __restrict__ idx, float* __restrict__ sqd, float* __restrict__ xyz) {
  const size_t i = (size_t)blockIdx.x * RS_BLOCK + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i];
  const uint32_t ins = (uint32_t)k;
  if (idx) idx[i] = (int32_t)ins;
  if (sqd) sqd[i] = __uint_as_float((uint32_t)(k >> 32));
  if (xyz) { const float4 p = map_raw[ins]; xyz[3 * i] = p.x; xyz[3 * i + 1] = p.y; xyz[3 * i + 2] = p.z; }
}

template <bool FILL>
static void radius_launch(hipStream_t st, const GridView& G, const float* q, int nq, float radius, int lanes, bool tiles,
                          const unsigned long long* offsets, uint32_t* cnt, unsigned long long* cand, const RadiusOut& O) {
  const float r2 = radius * radius;      // one float32 product (Octree.hpp:467)
  const int L = tiles ? 64 : lanes;
  const unsigned blocks = (unsigned)(((size_t)nq * L + RS_BLOCK - 1) / RS_BLOCK);
  if (tiles) hipLaunchKernelGGL((radius_kernel<FILL, 64, true>), dim3(blocks), dim3(RS_BLOCK), 0, st, G, q, nq, radius, r2, offsets, cnt, cand, O);
  else if (L == 8) hipLaunchKernelGGL((radius_kernel<FILL, 8, false>), dim3(blocks), dim3(RS_BLOCK), 0, st, G, q, nq, radius, r2, offsets, cnt, cand, O);
  else if (L == 16) hipLaunchKernelGGL((radius_kernel<FILL, 16, false>), dim3(blocks), dim3(RS_BLOCK), 0, st, G, q, nq, radius, r2, offsets, cnt, cand, O);
  else hipLaunchKernelGGL((radius_kernel<FILL, 64, false>), dim3(blocks), dim3(RS_BLOCK), 0, st, G, q, nq, radius, r2, offsets, cnt, cand, O);
}

hipError_t launch_radius_count(hipStream_t st, const GridView& G, const float* q, int nq, float radius, uint32_t* cnt, unsigned long long* cand) {
  if (nq <= 0) return hipSuccess;
  int lanes; bool tiles;
  radius_plan(G, radius, lanes, tiles);
  const RadiusOut none{nullptr, nullptr, nullptr, nullptr};
  radius_launch<false>(st, G, q, nq, radius, lanes, tiles, nullptr, cnt, cand, none);
  return hipGetLastError();
}
hipError_t launch_radius_fill(hipStream_t st, const GridView& G, const float* q, int nq, float radius, const unsigned long long* offsets,
                              int32_t* idx, float* sqd, float* xyz, unsigned long long* keys) {
  if (nq <= 0) return hipSuccess;
  int lanes; bool tiles;
  radius_plan(G, radius, lanes, tiles);
  const RadiusOut O{idx, sqd, xyz, keys};
  radius_launch<true>(st, G, q, nq, radius, lanes, tiles, offsets, nullptr, nullptr, O);
  return hipGetLastError();
}
// offsets[0 .. nq] = exclusive sum of cnt[0 .. nq] (the caller has set cnt[nq] = 0); tmp == nullptr: the scratch's size only
hipError_t radius_offsets(hipStream_t st, void* tmp, size_t& tmp_bytes, uint32_t* cnt, unsigned long long* offsets, size_t nq) {
  return rocprim::exclusive_scan(tmp, tmp_bytes, cnt, offsets, 0ull, nq + 1, rocprim::plus<unsigned long long>(), st);
}
// every segment [offsets[i], offsets[i + 1]) of the keys ascending; tmp == nullptr: the scratch's size only
hipError_t radius_sort_segments(hipStream_t st, void* tmp, size_t& tmp_bytes, const unsigned long long* keys_in, unsigned long long* keys_out,
                                size_t total, size_t nq, const unsigned long long* offsets) {
  return rocprim::segmented_radix_sort_keys(tmp, tmp_bytes, keys_in, keys_out, (unsigned int)total, (unsigned int)nq, offsets, offsets + 1, 0, 64, st);
}
hipError_t launch_radius_unpack(hipStream_t st, const unsigned long long* keys, size_t n, const float4* map_raw, int32_t* idx, float* sqd, float* xyz) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(radius_unpack_kernel, dim3((unsigned)((n + RS_BLOCK - 1) / RS_BLOCK)), dim3(RS_BLOCK), 0, st, keys, n, map_raw, idx, sqd, xyz);
  return hipGetLastError();
}

}  // namespace flimo
