// fast_limo_amd/csrc/hip/flimo_knn_k.hip -- exact k-NN for k up to KNNK_MAX_K, with a distance gate, over the resident map (gfx950).
//
// Octree::knn (reference Objects/Octree.hpp:526-555) takes any k.  flimo_knn (flimo_kernels.hip) answers k <= 5 with a private list
// per lane in registers; that cannot be stretched to 64.  Here the running k-best of a query is ONE LIST DISTRIBUTED OVER THE LANES
// that serve it: lane `sub` of the group holds the sub-th smallest 64-bit key so far,
//     key = (float32 squared-distance bits << 32) | insertion index          (the w of the stored point)
// Distances are non-negative floats, so the key's order is (distance, insertion index): a total order that does not depend on where
// a row lies in the cell-sorted array.  The list starts filled with the GATE'S key, (bits of max_dist * max_dist) << 32 (no gate:
// all ones): `key < k-th key` is then at once the gate's strict float32 `sqd < max_dist * max_dist` (flimo_radius_search's predicate)
// and the test against the k-th best, and a slot that still holds the gate's key at the end is an empty one.
//
// Candidates are walked as radius_round walks them (flimo_radius.hip): every lane fetches one row's range [lo, hi) of `pts`, the
// group walks the concatenated ranges, consecutive lanes on consecutive 16-byte points, KK_UNROLL loads in flight per lane.  A batch
// is FILTERED against the k-th key (a broadcast, a compare, a ballot): once the list is warm most batches have no survivor.  A
// survivor is broadcast to its group, every lane compares it with its own key and the tail moves up by one lane (rank-and-shift).
//
// The search has ONE text, two device functions, and one pair of kernels over a JOB that says where a query comes from and how its
// list ends (kk_search_kernel<L, Job> / kk_walk_kernel<Job>, below): flimo_knn_k is the job that ends in knnk_store (KnnJob); the
// normals, the outliers, FPFH, the keypoints, the scan's fitness and its normal equations are the others.
// knnk_block_search<L> (L = 16 lanes per query for k <= 16, a wave beyond): blocks of rows around the query's cell as
// knn_search does -- ring 1, then straight to the ring that proves exactness once k candidates (or the gate) bound the distance;
// of a later block only the shell beyond the block already walked is read, so no point is met twice.  Rows and the cells of a row
// are pruned by the smaller of the k-th distance and the gate.  A query is PROVEN when that bound is <= the distance to the nearest
// cell face not visited (knn_search's margins), or the block covers the grid.  What would need more than KK_FAR_RING rings goes to
// a worklist and knnk_tile_walk: one wave per query, best-first over the directory's existing tiles, nearest first, until the next
// tile is farther than the bound (knn_far_kernel's scheme with the distributed list): a query kilometres from every point costs a
// look at the directory and the nearest tiles.  All pruning is conservative; the float32 key compare alone decides membership and order.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <type_traits>
#include "flimo_types.h"
#include "flimo_math.h"
#include "flimo_kernels.h"
#include "flimo_jacobi.h"
#include "flimo_sums.h"

#pragma clang fp contract(off)

namespace flimo {

typedef unsigned long long kk_u64;
constexpr int KK_UNROLL = 4;
constexpr int KK_BLOCK = 256;
constexpr int KK_FAR_RING = 4;      // rings the block search tries before the tiles' best-first search takes over (as KNN_FAR_RING)
constexpr kk_u64 KK_NONE = 0xffffffffffffffffull;

template <int L>
__device__ __forceinline__ uint32_t kk_group_mask(unsigned long long ballot, int lane) {
  if (L == 64) return 0;      // (not used)
  return (uint32_t)(ballot >> (lane & ~(L - 1))) & ((1u << L) - 1u);
}
__device__ __forceinline__ int kk_floor_clamped(float v) { return (int)floorf(fminf(fmaxf(v, -1.0e9f), 1.0e9f)); }

// the ball of a squared distance d2 [m^2] in cell units squared, inflated: a point whose float32 distance is <= d2 lies inside it
__device__ __forceinline__ float kk_ball(const GridView& G, float d2) {
  if (!(d2 < 3.0e38f)) return INFINITY;
  const float rc = (fl_sqrt(d2) * (1.f + 1.0e-5f) + 1.0e-6f) * G.inv_cell;
  return rc * rc * (1.f + 1.0e-5f);
}
__device__ __forceinline__ float kk_key_dist(kk_u64 key) { return __uint_as_float((uint32_t)(key >> 32)); }

// One round: lane `sub` of the group holds the range [lo, lo + len) of one row (len = 0: none).  The group walks the concatenated
// ranges together and merges what passes the k-th key into its list (`mine`: this lane's entry).  Called by every lane of the wave
// (the shuffles and ballots are wave-wide); a group without work passes len = 0.
template <int L>
__device__ __forceinline__ void knnk_round(const GridView& G, float gx, float gy, float gz, int lane, int k, uint32_t lo, uint32_t len,
                                           kk_u64& mine, unsigned long long& cand) {
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
  for (uint32_t c0 = 0; __any(c0 < total); c0 += (uint32_t)(L * KK_UNROLL)) {
    float4 p[KK_UNROLL];
    bool in[KK_UNROLL];
#pragma unroll
    for (int u = 0; u < KK_UNROLL; u++) {
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
    for (int u = 0; u < KK_UNROLL; u++) {
      const float d = sqdist3(gx, gy, gz, p[u].x, p[u].y, p[u].z);
      const kk_u64 key = ((kk_u64)__float_as_uint(d) << 32) | __float_as_uint(p[u].w);      // w: insertion index (flimo_map_points' order)
      const kk_u64 kth = __shfl(mine, k - 1, L);
      const unsigned long long b = __ballot(in[u] && key < kth);
      if (b == 0ull) continue;                         // (wave-uniform) the usual case once the list is warm
      if (L == 64) {
        unsigned long long todo = b;
        while (todo) {
          const int s = __ffsll((long long)todo) - 1;
          todo &= todo - 1ull;
          const kk_u64 sk = __shfl(key, s, 64);
          const kk_u64 up = __shfl_up(mine, 1, 64);
          if (mine > sk) mine = (sub == 0 || up < sk) ? sk : up;      // (a survivor the list has outgrown meanwhile falls off lane 63 or beyond k)
        }
      } else {
        uint32_t todo = kk_group_mask<L>(b, lane);
        while (__any(todo != 0u)) {
          const int s = todo ? __ffs((int)todo) - 1 : 0;
          const kk_u64 got = __shfl(key, s, L);
          const kk_u64 sk = todo ? got : KK_NONE;      // (a group with no survivor left: nothing is greater than KK_NONE)
          todo &= todo - 1u;
          const kk_u64 up = __shfl_up(mine, 1, L);
          if (mine > sk) mine = (sub == 0 || up < sk) ? sk : up;
        }
      }
    }
  }
}

// the query in cell units (knn_far_kernel / radius_geo: the query's cell, its place inside it, the rounding margin)
struct KnnkGeo {
  int cx, cy, cz;
  float rx, ry, rz, qcx, qcy, qcz, margin;
};
__device__ __forceinline__ bool knnk_geo(const GridView& G, int maxdim, float gx, float gy, float gz, KnnkGeo& g) {
  const float fx = (gx - G.ox) * G.inv_cell, fy = (gy - G.oy) * G.inv_cell, fz = (gz - G.oz) * G.inv_cell;
  g.cx = g.cy = g.cz = 0; g.rx = g.ry = g.rz = 0.f; g.qcx = g.qcy = g.qcz = 0.f; g.margin = 0.f;
  if (!(fx == fx) || !(fy == fy) || !(fz == fz)) return false;      // NaN query: no neighbours
  const float flx = floorf(fminf(fmaxf(fx, -1.0e9f), 1.0e9f)), fly = floorf(fminf(fmaxf(fy, -1.0e9f), 1.0e9f)),
              flz = floorf(fminf(fmaxf(fz, -1.0e9f), 1.0e9f));
  g.cx = (int)flx - G.six; g.cy = (int)fly - G.siy; g.cz = (int)flz - G.siz;
  g.rx = fminf(fmaxf(fx - flx, 0.f), 1.f); g.ry = fminf(fmaxf(fy - fly, 0.f), 1.f); g.rz = fminf(fmaxf(fz - flz, 0.f), 1.f);
  g.qcx = (float)g.cx + g.rx; g.qcy = (float)g.cy + g.ry; g.qcz = (float)g.cz + g.rz;
  g.margin = 1.0e-3f + 4.0e-7f * fmaxf((float)maxdim, fmaxf(fmaxf(fabsf(g.qcx), fabsf(g.qcy)), fabsf(g.qcz)));
  return true;
}
// the range of `pts` of the cells [x0, x1] of row (yy, zz) (inside the grid) that a ball of bnd2 (cell units squared) can reach
__device__ __forceinline__ void knnk_row(const GridView& G, const KnnkGeo& g, float bnd2, int yy, int zz, int x0, int x1, uint32_t& lo, uint32_t& len) {
  lo = 0; len = 0;
  const float a = fmaxf(fmaxf((float)yy - g.qcy, g.qcy - (float)(yy + 1)) - g.margin, 0.f),
              b = fmaxf(fmaxf((float)zz - g.qcz, g.qcz - (float)(zz + 1)) - g.margin, 0.f);
  const float dyz2 = a * a + b * b;
  if (!(dyz2 <= bnd2)) return;
  if (bnd2 < 1.0e18f) {
    // cells of the row the ball reaches: |x - qcx| <= xr, widened
    const float xr = fl_sqrt(fmaxf(bnd2 - dyz2, 0.f)) * (1.f + 1.0e-6f) + g.margin + 1.0e-4f;
    x0 = max(x0, kk_floor_clamped(g.qcx - xr));
    x1 = min(x1, kk_floor_clamped(g.qcx + xr));
  }
  if (x0 > x1) return;
  uint32_t hi;
  grid_row_range(G, G.dir, yy, zz, x0 * G.xs, (x1 + 1) * G.xs, lo, hi);
  len = hi > lo ? hi - lo : 0u;
}

// lane sub < k writes slot sub of its query: entries below the gate's key are results, the rest padding
template <int L>
__device__ __forceinline__ void knnk_store(int lane, int q, int k, kk_u64 mine, kk_u64 gate_key, bool live,
                                           const float4* __restrict__ map_raw, int32_t* __restrict__ idx, float* __restrict__ sqd,
                                           float* __restrict__ xyz, int32_t* __restrict__ cnt) {
  const int sub = lane & (L - 1);
  const bool has = live && sub < k && mine < gate_key;
  const unsigned long long b = __ballot(has);
  const int c = L == 64 ? __popcll(b) : __popc(kk_group_mask<L>(b, lane));
  if (live && sub < k) {
    const size_t at = (size_t)q * (size_t)k + (size_t)sub;
    const uint32_t ins = (uint32_t)mine;
    idx[at] = has ? (int32_t)ins : -1;
    sqd[at] = has ? kk_key_dist(mine) : 0.f;
    if (xyz) {
      float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
      if (has) p = map_raw[ins];
      xyz[3 * at] = p.x; xyz[3 * at + 1] = p.y; xyz[3 * at + 2] = p.z;
    }
  }
  if (live && sub == 0) cnt[q] = c;
}

// ---- the search: the only copy of its text, run by kk_search_kernel / kk_walk_kernel (below), which end a query as their job
//      says -- flimo_knn_k's in knnk_store.  `cand` counts the points met, for the developer's flimo_knn_k_candidates; every
//      other job lets it die. ----
// The block search of one query by the L lanes of its group (every lane of the wave calls it; a group without a query passes
// live = false): `mine` ends as this lane's entry of the k-best list.  Returns whether the list is proven exact; if not, the tiles'
// walk (knnk_tile_walk) has to finish the query.
template <int L>
__device__ __forceinline__ bool knnk_block_search(const GridView& G, bool live, float gx, float gy, float gz, int lane, int k, float r2,
                                                  kk_u64 gate_key, kk_u64& mine, unsigned long long& cand) {
  const int sub = lane & (L - 1);
  const int maxdim = grid_maxdim(G);
  KnnkGeo g;
  const bool valid = knnk_geo(G, maxdim, live ? gx : NAN, gy, gz, g);
  const float edge = fminf(fminf(fminf(g.rx, 1.f - g.rx), fminf(g.ry, 1.f - g.ry)), fminf(g.rz, 1.f - g.rz));
  mine = gate_key;
  bool done = !valid || gate_key == 0ull, proven = true;      // NaN query / a gate of 0: empty, and that is exact
  // first ring that can reach the grid at all
  int r_prev = -1, r = 1;
  if (!done) {
    const int ox_ = g.cx < 0 ? -g.cx : (g.cx >= G.nx ? g.cx - G.nx + 1 : 0);
    const int oy_ = g.cy < 0 ? -g.cy : (g.cy >= G.ny ? g.cy - G.ny + 1 : 0);
    const int oz_ = g.cz < 0 ? -g.cz : (g.cz >= G.nz ? g.cz - G.nz + 1 : 0);
    r = max(1, max(ox_, max(oy_, oz_)));
    if (r > KK_FAR_RING) { done = true; proven = false; }
  }
  float bound = r2;                          // min(gate, k-th distance so far) [m^2]: no point farther than it can enter the list
  while (__any(!done)) {
    // ---- the block of ring r, of which the block of ring r_prev has been walked: rows clipped to the grid; an inner row has a
    //      part on either side of the old block (two jobs), an outer row is one job ----
    const int y0 = max(g.cy - r, 0), y1 = min(g.cy + r, G.ny - 1), z0 = max(g.cz - r, 0), z1 = min(g.cz + r, G.nz - 1);
    const int nyb = max(y1 - y0 + 1, 0), nzb = max(z1 - z0 + 1, 0);
    const int sides = r_prev >= 0 ? 2 : 1;
    const int njobs = done ? 0 : nyb * nzb * sides;
    float bnd2 = kk_ball(G, bound);
    for (int jb = 0; __any(jb < njobs); jb += L) {
      const int j = jb + sub;
      uint32_t lo = 0, len = 0;
      if (j < njobs) {
        const int row = sides == 2 ? j >> 1 : j, side = sides == 2 ? j & 1 : 0;
        const int yy = y0 + row % nyb, zz = z0 + row / nyb;
        const bool inner = r_prev >= 0 && abs(yy - g.cy) <= r_prev && abs(zz - g.cz) <= r_prev;
        int x0 = g.cx - r, x1 = g.cx + r;
        if (inner) { if (side == 0) x1 = g.cx - r_prev - 1; else x0 = g.cx + r_prev + 1; }
        else if (side == 1) x1 = x0 - 1;
        x0 = max(x0, 0); x1 = min(x1, G.nx - 1);
        if (x0 <= x1) knnk_row(G, g, bnd2, yy, zz, x0, x1, lo, len);
      }
      knnk_round<L>(G, gx, gy, gz, lane, k, lo, len, mine, cand);
      // the ball shrinks with the k-th best
      const float dk = kk_key_dist(__shfl(mine, k - 1, L));
      if (dk < bound) { bound = dk; bnd2 = kk_ball(G, bound); }
    }
    if (!done) {
      // ---- exactness: every point not visited is at least rg away (knn_search) ----
      const float rg = ((float)r + edge - g.margin) * G.cell;
      const bool covers = (g.cx - r <= 0) && (g.cx + r >= G.nx - 1) && (g.cy - r <= 0) && (g.cy + r >= G.ny - 1) && (g.cz - r <= 0) &&
                          (g.cz + r >= G.nz - 1);
      if (covers || (rg > 0.f && bound <= rg * rg * (1.f - 1.0e-6f))) {
        done = true;
      } else {
        // next ring: straight to the one that proves exactness once a bound is known, else double
        int rn = 2 * r;
        if (bound < 3.0e38f) {
          const float need = fl_sqrt(bound) * G.inv_cell * (1.f + 4.0e-6f) - edge + g.margin;
          rn = max(r + 1, (int)ceilf(fminf(need, 1.0e9f)));
        }
        if (rn > KK_FAR_RING) { done = true; proven = false; }
        r_prev = r;
        r = rn;
      }
    }
  }
  return proven;
}

// (the walk of one query by one wave: `bound` [m^2] is the first bound, `mine` ends as this lane's entry of the list)
__device__ __forceinline__ void knnk_tile_walk(const GridView& G, int maxdim, int ndir, int cells_per_xtile, float gx, float gy, float gz, int lane,
                                               int k, float bound, kk_u64 gate_key, kk_u64& mine, unsigned long long& cand) {
  KnnkGeo g;
  (void)knnk_geo(G, maxdim, gx, gy, gz, g);                    // (a NaN query never comes here)
  float bnd2 = kk_ball(G, bound);
  mine = gate_key;
  float last_d = -1.f;
  int last_i = -1;
  for (;;) {
    // ---- the nearest tile not visited yet: (distance, directory index) in ascending order ----
    float best_d = INFINITY;
    int best_i = INT_MAX;
    for (int i = lane; i < ndir; i += 64) {
      if (G.dir[i] == 0) continue;
      const int tx = i % G.ntx, tyz = i / G.ntx, ty_ = tyz % G.nty, tz_ = tyz / G.nty;
      const float x0 = (float)(tx * cells_per_xtile), x1 = (float)((tx + 1) * cells_per_xtile);
      const float y0 = (float)((ty_ << G.ty) - GRID_PAD), y1 = (float)(((ty_ + 1) << G.ty) - GRID_PAD);
      const float z0 = (float)((tz_ << G.tz) - GRID_PAD), z1 = (float)(((tz_ + 1) << G.tz) - GRID_PAD);
      const float ax = fmaxf(fmaxf(x0 - g.qcx, g.qcx - x1) - g.margin, 0.f), ay = fmaxf(fmaxf(y0 - g.qcy, g.qcy - y1) - g.margin, 0.f),
                  az = fmaxf(fmaxf(z0 - g.qcz, g.qcz - z1) - g.margin, 0.f);
      const float d = (ax * ax + ay * ay + az * az) * (1.f - 1.0e-6f);
      const bool after = d > last_d || (d == last_d && i > last_i);
      if (after && (d < best_d || (d == best_d && i < best_i))) { best_d = d; best_i = i; }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float od = __shfl_xor(best_d, o, 64);
      const int oi = __shfl_xor(best_i, o, 64);
      if (od < best_d || (od == best_d && oi < best_i)) { best_d = od; best_i = oi; }
    }
    if (best_i == INT_MAX) break;                              // every tile has been visited
    if (best_d > bnd2) break;                                  // no point of it -- or of any later one -- lies within the bound
    last_d = best_d; last_i = best_i;
    // ---- its rows, one per lane and round ----
    const int tx = best_i % G.ntx, tyz = best_i / G.ntx, ty_ = tyz % G.nty, tz_ = tyz / G.nty;
    const int xt0 = tx * cells_per_xtile, xt1 = min((tx + 1) * cells_per_xtile, G.nx) - 1;
    const int nrows = 1 << (G.ty + G.tz);
    for (int jb = 0; jb < nrows; jb += 64) {
      const int j = jb + lane;
      const int yy = (ty_ << G.ty) + (j & ((1 << G.ty) - 1)) - GRID_PAD, zz = (tz_ << G.tz) + (j >> G.ty) - GRID_PAD;
      uint32_t lo = 0, len = 0;
      if (j < nrows && yy >= 0 && yy < G.ny && zz >= 0 && zz < G.nz && xt0 <= xt1) knnk_row(G, g, bnd2, yy, zz, xt0, xt1, lo, len);
      if (!__any(len != 0u)) continue;
      knnk_round<64>(G, gx, gy, gz, lane, k, lo, len, mine, cand);
      const float dk = kk_key_dist(__shfl(mine, k - 1, 64));
      if (dk < bound) { bound = dk; bnd2 = kk_ball(G, bound); }
    }
  }
}

// ---- one pair of kernels over a JOB, passed by value ---------------------------------------------------------------------------
// A job numbers its queries by SLOTS and says where they come from and how they end:
//   slot<L>(at, x, y, z)   the slot of this lane's group and its query; returns whether there is one (if not: slot 0, no query)
//   total()          the number of slots: the walk clamps a worklist entry by it
//   query(at, x, y, z)     the query of a slot, for the walk (the pairs' costs a division the search's workgroups do not need)
//   k, r2, gate_key
//   finish<L>(lane, at, live, mine, gx, gy, gz)      the end of a query whose list is exact, by the L lanes that hold it; every lane
//                    of the wave calls it, live = false for a group without a query or with one the walk has yet to finish
//   LANES            lanes per query, 0: knnk_plan(k);  PAIRS: the slots are (pose, scan point) pairs (KkPairs below)
//   COUNT, cand      optional (KkCounts): the job keeps the number of points its queries met, cand[slot]
// kk_search_kernel is the block search with that end.  A query it cannot prove goes to the worklist (its slot, its first bound:
// the list's k-th distance, when there is one, bounds the true one) by one atomicAdd of its leading lane on `nwork`, and nothing
// of it is written yet; kk_walk_kernel, one wave per entry, runs the walk over the tiles and the same end.
template <class Job, class = void>
struct KkCounts { static constexpr bool value = false; };
template <class Job>
struct KkCounts<Job, std::void_t<decltype(Job::COUNT)>> { static constexpr bool value = Job::COUNT; };

template <int L>
__device__ __forceinline__ bool kk_flat_slot(int nq, size_t& at) {      // slots 0 .. nq - 1, KK_BLOCK / L of them per workgroup
  const size_t gq = ((size_t)blockIdx.x * KK_BLOCK + threadIdx.x) / (unsigned)L;
  const bool live = gq < (size_t)nq;
  at = live ? gq : 0;
  return live;
}

template <int L, class Job>
__global__ __launch_bounds__(KK_BLOCK) void kk_search_kernel(GridView G, Job J, uint2* __restrict__ work, unsigned* __restrict__ nwork) {
  const int lane = threadIdx.x & 63;
  const int sub = lane & (L - 1);
  size_t at;
  float gx = 0.f, gy = 0.f, gz = 0.f;
  const bool live = J.template slot<L>(at, gx, gy, gz);
  kk_u64 mine;
  unsigned long long cand = 0;
  const bool proven = knnk_block_search<L>(G, live, gx, gy, gz, lane, J.k, J.r2, J.gate_key, mine, cand);
  if (!proven) {
    const kk_u64 kth = __shfl(mine, J.k - 1, L);
    if (live && sub == 0) {
      const unsigned w = atomicAdd(nwork, 1u);
      work[w] = make_uint2((unsigned)at, __float_as_uint(kth < J.gate_key ? kk_key_dist(kth) : J.r2));
    }
  }
  J.template finish<L>(lane, at, live && proven, mine, gx, gy, gz);
  if constexpr (KkCounts<Job>::value) {
    if (live && sub == 0) J.cand[at] = cand;      // (proven or not: the walk adds its part)
  }
}

// (waves per SIMD the walk's register budget is cut for: 5 unless a job whose end needs more registers than that leaves asks for fewer)
template <class Job, class = void>
struct KkWalkWaves { static constexpr int value = 5; };
template <class Job>
struct KkWalkWaves<Job, std::void_t<decltype(Job::WALK_WAVES)>> { static constexpr int value = Job::WALK_WAVES; };

template <class Job>
__global__ __launch_bounds__(KK_BLOCK, KkWalkWaves<Job>::value) void kk_walk_kernel(GridView G, Job J, const uint2* __restrict__ work, const unsigned* __restrict__ nwork) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int maxdim = grid_maxdim(G);
  const int ndir = G.ntx * G.nty * G.ntz;
  const int cells_per_xtile = max(1, (8 << G.ts) / G.xs);
  const size_t total = J.total();
  const unsigned nw = (unsigned)min((size_t)*nwork, total);
  for (unsigned w = blockIdx.x * (KK_BLOCK / 64) + wave; w < nw; w += gridDim.x * (KK_BLOCK / 64)) {
    const uint2 e = work[w];
    const size_t at = min((size_t)e.x, total - 1);
    float gx, gy, gz;
    J.query(at, gx, gy, gz);
    kk_u64 mine;
    unsigned long long cand = 0;
    knnk_tile_walk(G, maxdim, ndir, cells_per_xtile, gx, gy, gz, lane, J.k, __uint_as_float(e.y), J.gate_key, mine, cand);
    J.template finish<64>(lane, at, true, mine, gx, gy, gz);
    if constexpr (KkCounts<Job>::value) {
      if (lane == 0) J.cand[at] += cand;
    }
  }
}

// ---- flimo_knn_k: packed queries, the list ended in the caller's arrays (knnk_store) -------------------------------------------
// COUNT: the developer's counter of the points met (flimo_knn_k_candidates).  It is live through the whole search and costs the
// 16-lane search a wave of occupancy (profiles/knn_k/README.md), so the production call does not instantiate it.
template <bool COUNT_>
struct KnnJob {
  static constexpr int LANES = 0;
  static constexpr bool PAIRS = false;
  static constexpr bool COUNT = COUNT_;
  const float* qxyz;     // [nq][3]
  int nq, k;
  float r2;
  kk_u64 gate_key;
  const float4* map_raw;
  int32_t* idx;          // [nq][k]
  float* sqd;            // [nq][k]
  float* xyz;            // [nq][k][3] or null
  int32_t* cnt;          // [nq]
  unsigned long long* cand;      // [nq] (COUNT)
  template <int L>
  __device__ bool slot(size_t& at, float& x, float& y, float& z) const {
    const bool live = kk_flat_slot<L>(nq, at);
    if (live) query(at, x, y, z);
    return live;
  }
  __host__ __device__ size_t total() const { return (size_t)nq; }
  __device__ void query(size_t at, float& x, float& y, float& z) const { x = qxyz[3 * at]; y = qxyz[3 * at + 1]; z = qxyz[3 * at + 2]; }
  template <int L>
  __device__ void finish(int lane, size_t at, bool live, kk_u64 mine, float, float, float) const {
    knnk_store<L>(lane, (int)at, k, mine, gate_key, live, map_raw, idx, sqd, xyz, cnt);
  }
};

// the stored points of a chunk as slots: query i is stored point first + i (the base of the jobs over stored points)
struct KkStored {
  unsigned first;
  int nq, k;             // queries of the chunk; the list's length
  float r2;
  kk_u64 gate_key;
  const float4* map_raw;
  template <int L>
  __device__ bool slot(size_t& at, float& x, float& y, float& z) const {
    const bool live = kk_flat_slot<L>(nq, at);
    if (live) query(at, x, y, z);
    return live;
  }
  __host__ __device__ size_t total() const { return (size_t)nq; }
  __device__ void query(size_t at, float& x, float& y, float& z) const { const float4 p = map_raw[(size_t)first + at]; x = p.x; y = p.y; z = p.z; }
};

// ---- normals and covariances of the k-NN neighbourhoods (flimo_map_normals) ---------------------------------------------------
// The same search; instead of knnk_store the group finishes its query in registers.  Lane `sub` holds slot sub of the list; it
// loads that stored point and forms r = (double)p - (double)q (exact).  Every sum is a butterfly over the 64 SLOTS of a list,
// slots beyond cnt holding +0.0: a 16-lane group runs the four levels it has and adds the +0.0 of the two it lacks, so the bits
// depend on the list alone -- not on which kernel finished the query, nor on how many lanes served it.  Mean (divided by n), then
// the sums of the six products centred on it (two passes, the values stay in registers): 72 bytes per query go to the chunk's
// scratch, the neighbour list goes nowhere.  A third launch, one THREAD per query, divides by n and runs a cyclic Jacobi on the
// 3 x 3 until the off-diagonal is exactly 0 (measured: run by the search kernel's lanes, each on the same numbers, the float64
// divisions and square roots of the rotations added 70 % to the search's time -- profiles/normals/README.md).
template <int L>
__device__ __forceinline__ double kk_slot_sum(double v) {
#pragma unroll
  for (int o = 1; o < L; o <<= 1) v = v + __shfl_xor(v, o, L);
#pragma unroll
  for (int o = L; o < 64; o <<= 1) v = v + 0.0;      // (the empty upper slots of a 64-slot list: also turns a sum of -0.0 into the wave's +0.0)
  return v;
}

// The plane of a symmetric 3 x 3 covariance: kk_eigen3 (flimo_jacobi.h: a cyclic Jacobi until the off-diagonal is exactly 0, the
// eigenvalues in ascending order, on a tie the lower column first), the smallest one's unit vector, oriented.  has_vp: towards the viewpoint, (tvx, tvy, tvz) being
// viewpoint - query; else the component of largest magnitude (the lowest axis of equal ones) made positive.  Shared by every
// kernel that ends a neighbourhood in a plane: their bits are the same by construction.
__device__ __forceinline__ void kk_plane(double a00, double a01, double a02, double a11, double a12, double a22, bool has_vp, double tvx, double tvy,
                                         double tvz, double& l0, double& l1, double& l2, double& nx, double& ny, double& nz) {
  // (only the smallest eigenvalue's vector is kept)
  double v00, v01, v02, v10, v11, v12, v20, v21, v22;
  kk_eigen3(a00, a01, a02, a11, a12, a22, l0, l1, l2, v00, v01, v02, v10, v11, v12, v20, v21, v22);
  nx = v00; ny = v10; nz = v20;
  bool flip;
  if (has_vp) {
    flip = nx * tvx + ny * tvy + nz * tvz < 0.0;
  } else {
    const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
    const double big = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
    flip = big < 0.0;
  }
  if (flip) { nx = -nx; ny = -ny; nz = -nz; }
}

struct NormalsOut {
  float4* normal;        // [n] nx ny nz curvature
  int32_t* cnt;          // [n]
  double* centroid;      // [n][3] or null
  double* cov;           // [n][6] or null: xx xy xz yy yz zz
  double* eig;           // [n][6] or null: l0 <= l1 <= l2, the unit normal
};
struct NormalsArgs {
  const float* qxyz;     // the chunk's queries, or null: query i is stored point first + i
  unsigned first;
  int nq, k, need;       // need: neighbours below which a query's results are NaN
  float r2;
  kk_u64 gate_key;
  float vx, vy, vz;      // the viewpoint
  int has_vp;
};

__device__ __forceinline__ void knnk_query(const NormalsArgs& A, const float4* __restrict__ map_raw, int q, float& gx, float& gy, float& gz) {
  if (A.qxyz) { gx = A.qxyz[3 * q]; gy = A.qxyz[3 * q + 1]; gz = A.qxyz[3 * q + 2]; }
  else { const float4 p = map_raw[(size_t)A.first + (size_t)q]; gx = p.x; gy = p.y; gz = p.z; }
}

// the group's end of a query whose list is exact: cnt, and the record {mean of r (3), sums of the centred products (6)}
constexpr int KK_MOM = 9;
template <int L>
__device__ __forceinline__ void knnk_moments(int k, kk_u64 gate_key, int lane, int q, bool live, kk_u64 mine, float gx, float gy, float gz,
                                             const float4* __restrict__ map_raw, int32_t* __restrict__ cnt, double* __restrict__ mom) {
  const int sub = lane & (L - 1);
  const bool has = live && sub < k && mine < gate_key;
  const unsigned long long bal = __ballot(has);
  const int c = L == 64 ? __popcll(bal) : __popc(kk_group_mask<L>(bal, lane));
  const double qx = (double)gx, qy = (double)gy, qz = (double)gz;
  double rx = 0.0, ry = 0.0, rz = 0.0;
  if (has) {
    const float4 p = map_raw[(uint32_t)mine];
    rx = (double)p.x - qx; ry = (double)p.y - qy; rz = (double)p.z - qz;
  }
  const double n = (double)c;
  const double mx = kk_slot_sum<L>(rx) / n, my = kk_slot_sum<L>(ry) / n, mz = kk_slot_sum<L>(rz) / n;      // (c == 0: NaN, not used)
  const double dx = has ? rx - mx : 0.0, dy = has ? ry - my : 0.0, dz = has ? rz - mz : 0.0;
  const double s00 = kk_slot_sum<L>(has ? dx * dx : 0.0), s01 = kk_slot_sum<L>(has ? dx * dy : 0.0), s02 = kk_slot_sum<L>(has ? dx * dz : 0.0),
               s11 = kk_slot_sum<L>(has ? dy * dy : 0.0), s12 = kk_slot_sum<L>(has ? dy * dz : 0.0), s22 = kk_slot_sum<L>(has ? dz * dz : 0.0);
  if (live && sub == 0) {
    cnt[q] = c;
    double* M = mom + (size_t)KK_MOM * (size_t)q;
    M[0] = mx; M[1] = my; M[2] = mz; M[3] = s00; M[4] = s01; M[5] = s02; M[6] = s11; M[7] = s12; M[8] = s22;
  }
}

// One thread per query, after both searches: covariance = sums / n, the eigen-decomposition, the orientation, the outputs.  (In
// the search kernels the 64 lanes of a wave would each run this on the same numbers: a wave's time for one query instead of 64.)
__global__ __launch_bounds__(KK_BLOCK) void knnk_normals_finish_kernel(NormalsArgs A, const float4* __restrict__ map_raw, const double* __restrict__ mom,
                                                                       NormalsOut O) {
  const size_t gq = (size_t)blockIdx.x * KK_BLOCK + threadIdx.x;
  if (gq >= (size_t)A.nq) return;
  const int q = (int)gq;
  float gx, gy, gz;
  knnk_query(A, map_raw, q, gx, gy, gz);
  const double qx = (double)gx, qy = (double)gy, qz = (double)gz;
  const int c = O.cnt[q];
  const bool enough = c >= A.need;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double* M = mom + (size_t)KK_MOM * (size_t)q;
  const double n = (double)c;
  double mx = 0.0, my = 0.0, mz = 0.0, a00 = 1.0, a01 = 0.0, a02 = 0.0, a11 = 1.0, a12 = 0.0, a22 = 1.0;      // (too few: nothing to rotate)
  if (enough) {
    mx = M[0]; my = M[1]; mz = M[2];
    a00 = M[3] / n; a01 = M[4] / n; a02 = M[5] / n; a11 = M[6] / n; a12 = M[7] / n; a22 = M[8] / n;
  }
  if (O.centroid) {
    O.centroid[3 * (size_t)q] = enough ? qx + mx : nan; O.centroid[3 * (size_t)q + 1] = enough ? qy + my : nan; O.centroid[3 * (size_t)q + 2] = enough ? qz + mz : nan;
  }
  if (O.cov) {
    double* C = O.cov + 6 * (size_t)q;
    C[0] = enough ? a00 : nan; C[1] = enough ? a01 : nan; C[2] = enough ? a02 : nan; C[3] = enough ? a11 : nan; C[4] = enough ? a12 : nan; C[5] = enough ? a22 : nan;
  }
  double l0, l1, l2, nx, ny, nz;
  kk_plane(a00, a01, a02, a11, a12, a22, A.has_vp != 0, (double)A.vx - qx, (double)A.vy - qy, (double)A.vz - qz, l0, l1, l2, nx, ny, nz);
  const double tr = l0 + l1 + l2;
  const double curv = tr == 0.0 ? 0.0 : l0 / tr;
  const float fn = __int_as_float(0x7fc00000);
  O.normal[q] = enough ? make_float4((float)nx, (float)ny, (float)nz, (float)curv) : make_float4(fn, fn, fn, fn);
  if (O.eig) {
    double* E = O.eig + 6 * (size_t)q;
    E[0] = enough ? l0 : nan; E[1] = enough ? l1 : nan; E[2] = enough ? l2 : nan; E[3] = enough ? nx : nan; E[4] = enough ? ny : nan; E[5] = enough ? nz : nan;
  }
}

// the queries of a chunk, ended in their moments (the arguments above are knnk_normals_finish_kernel's too)
struct NormalsJob : NormalsArgs {
  static constexpr int LANES = 0;
  static constexpr bool PAIRS = false;
  const float4* map_raw;
  int32_t* cnt;
  double* mom;
  template <int L>
  __device__ bool slot(size_t& at, float& x, float& y, float& z) const {
    const bool live = kk_flat_slot<L>(nq, at);
    if (live) query(at, x, y, z);
    return live;
  }
  __host__ __device__ size_t total() const { return (size_t)nq; }
  __device__ void query(size_t at, float& x, float& y, float& z) const { knnk_query(*this, map_raw, (int)at, x, y, z); }
  template <int L>
  __device__ void finish(int lane, size_t at, bool live, kk_u64 mine, float gx, float gy, float gz) const {
    knnk_moments<L>(k, gate_key, lane, (int)at, live, mine, gx, gy, gz, map_raw, cnt, mom);
  }
};

// ---- fitness of the resident scan under pose hypotheses (flimo_scan_fitness) ----------------------------------------------------
// One query per (pose, scan point) pair: the world point is transform_kernel's (flimo_kernels.hip) float32
// c0*x + (c1*y + (c2*z + c3)) from the pose's RT, the search is the one above with k = 1 and the gate.  A workgroup serves
// KK_BLOCK / FIT_L consecutive scan points of ONE pose, so the 12 floats of its RT are uniform over the wave.  The nearest key of a pair goes
// into the pair's slot (sqd, -1.0f when the query is empty; the insertion index beside it when asked for): by the group when the
// block search proves it, by the walk over the tiles otherwise (FitJob).  A third launch, one workgroup
// per pose, counts and sums the pose's n slots in ONE shape: thread t adds slots t, t + FIT_RED, ... in float64, then a tree over
// the FIT_RED partials in shared memory.  No atomics on floating-point values: the bits of a pose's sum depend on its slots alone.
constexpr int FIT_L = 8;                        // lanes per query: a list of one key; measured against 16 (profiles/scan_fitness/README.md)
constexpr int FIT_RED = 256;                    // threads of the reduction's workgroup

// the (pose, scan point) pairs of a chunk of poses as slots: pair (pose, i) is slot pose * n + i
struct KkPairs {
  const float4* scan;    // the resident scan (body frame), [n]
  const float* poses;    // the chunk's poses: [np][12], the upper three rows of RT (pose_from_x26)
  unsigned n, np;        // points of the scan, poses of the chunk: n * np <= 2^31, np < 2^16 (the grid's y)
  unsigned b0;           // the search launch's first workgroup of a pose
  __device__ void world(unsigned pose, unsigned i, float& x, float& y, float& z) const {
    const float4 p = scan[i];
    const float* M = poses + 12 * (size_t)pose;
    x = M[0] * p.x + (M[1] * p.y + (M[2] * p.z + M[3]));
    y = M[4] * p.x + (M[5] * p.y + (M[6] * p.z + M[7]));
    z = M[8] * p.x + (M[9] * p.y + (M[10] * p.z + M[11]));
  }
  template <int L>
  __device__ bool slot(size_t& at, float& x, float& y, float& z) const {      // a workgroup: KK_BLOCK / L points of pose blockIdx.y
    const size_t gi = ((size_t)b0 + blockIdx.x) * (KK_BLOCK / L) + threadIdx.x / (unsigned)L;
    const bool live = gi < (size_t)n;
    at = live ? (size_t)blockIdx.y * (size_t)n + gi : 0;
    if (live) world(blockIdx.y, (unsigned)gi, x, y, z);
    return live;
  }
  __host__ __device__ size_t total() const { return (size_t)n * (size_t)np; }
  __device__ void query(size_t at, float& x, float& y, float& z) const { world((unsigned)(at / n), (unsigned)(at % n), x, y, z); }
};
__device__ __forceinline__ void fit_store(size_t at, bool has, kk_u64 key, float* __restrict__ sqd, int32_t* __restrict__ idx) {
  sqd[at] = has ? kk_key_dist(key) : -1.f;
  if (idx) idx[at] = has ? (int32_t)(uint32_t)key : -1;
}

// the pairs, each ended in its slot of sqd / idx (k = 1: the group's first lane holds the list)
struct FitJob {
  static constexpr int LANES = FIT_L;
  static constexpr bool PAIRS = true;
  static constexpr int k = 1;
  KkPairs P;
  float r2;
  kk_u64 gate_key;
  float* sqd;
  int32_t* idx;
  template <int L>
  __device__ bool slot(size_t& at, float& x, float& y, float& z) const { return P.slot<L>(at, x, y, z); }
  __host__ __device__ size_t total() const { return P.total(); }
  __device__ void query(size_t at, float& x, float& y, float& z) const { P.query(at, x, y, z); }
  template <int L>
  __device__ void finish(int lane, size_t at, bool live, kk_u64 mine, float, float, float) const {
    if (live && (lane & (L - 1)) == 0) fit_store(at, mine < gate_key, mine, sqd, idx);
  }
};

// One workgroup per pose over its n slots: the number of slots that hold a distance and their float64 sum, in one fixed shape.
__global__ __launch_bounds__(FIT_RED) void fit_reduce_kernel(const float* __restrict__ sqd, unsigned n, int32_t* __restrict__ inliers,
                                                             double* __restrict__ sum_sqd) {
  __shared__ double s_sum[FIT_RED];
  __shared__ int s_cnt[FIT_RED];
  const float* s = sqd + (size_t)blockIdx.x * (size_t)n;
  double acc = 0.0;
  int c = 0;
  for (unsigned i = threadIdx.x; i < n; i += FIT_RED) {
    const float v = s[i];
    if (v >= 0.f) { acc = acc + (double)v; c++; }      // (an empty slot holds -1)
  }
  s_sum[threadIdx.x] = acc;
  s_cnt[threadIdx.x] = c;
  __syncthreads();
  for (int o = FIT_RED / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) {
      s_sum[threadIdx.x] = s_sum[threadIdx.x] + s_sum[threadIdx.x + o];
      s_cnt[threadIdx.x] += s_cnt[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { inliers[blockIdx.x] = s_cnt[0]; sum_sqd[blockIdx.x] = s_sum[0]; }
}

// ---- point-to-plane normal equations of the resident scan under pose hypotheses (flimo_scan_linearize) --------------------------
// One query per (pose, scan point) pair, the world point as above.  The search is the normals' for any k, a workgroup serving
// KK_BLOCK / L consecutive scan points of ONE pose as the fitness' does (LinJob); the pair's moments (72 B) and count go to the
// chunk's scratch, a pair the block search cannot prove to the worklist and the walk over the tiles.  A third launch, one THREAD per
// pair, runs kk_plane on the moments -- flimo_map_normals' plane of the query w, bit for bit -- and writes the pair's row
// {J0..J5, d} and its validity; every term is float64 in the association flimo_c.h states.  The sums have the shape of flimo_sums.h,
// a row being a pose and a slot a scan point: a slot adds its 28 products, an invalid one +0.0.
constexpr int LIN_NUM = 28;                     // 21 of H, 6 of g, the cost

// the pairs, each ended in its moments; need and max_curv are lin_finish_kernel's
struct LinJob {
  static constexpr int LANES = 0;
  static constexpr bool PAIRS = true;
  KkPairs P;
  int need;              // neighbours below which a pair has no plane
  double max_curv;
  int k;
  float r2;
  kk_u64 gate_key;
  const float4* map_raw;
  int32_t* cnt;
  double* mom;
  template <int L>
  __device__ bool slot(size_t& at, float& x, float& y, float& z) const { return P.slot<L>(at, x, y, z); }
  __host__ __device__ size_t total() const { return P.total(); }
  __device__ void query(size_t at, float& x, float& y, float& z) const { P.query(at, x, y, z); }
  template <int L>
  __device__ void finish(int lane, size_t at, bool live, kk_u64 mine, float gx, float gy, float gz) const {
    knnk_moments<L>(k, gate_key, lane, (int)at, live, mine, gx, gy, gz, map_raw, cnt, mom);
  }
};

// One thread per pair, after both searches: the plane as knnk_normals_finish_kernel forms it, the validity, the row.
__global__ __launch_bounds__(KK_BLOCK) void lin_finish_kernel(LinJob A, const int32_t* __restrict__ cnt, const double* __restrict__ mom,
                                                              double* __restrict__ rows, unsigned char* __restrict__ ok) {
  const size_t at = (size_t)blockIdx.x * KK_BLOCK + threadIdx.x;
  if (at >= (size_t)A.P.n * (size_t)A.P.np) return;
  const unsigned pose = (unsigned)(at / A.P.n), i = (unsigned)(at % A.P.n);
  float gx, gy, gz;
  A.P.world(pose, i, gx, gy, gz);
  const double wx = (double)gx, wy = (double)gy, wz = (double)gz;
  const int c = cnt[at];
  const bool enough = c >= A.need;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double* M = mom + (size_t)KK_MOM * at;
  const double n = (double)c;
  double mx = 0.0, my = 0.0, mz = 0.0, a00 = 1.0, a01 = 0.0, a02 = 0.0, a11 = 1.0, a12 = 0.0, a22 = 1.0;      // (too few: nothing to rotate)
  if (enough) {
    mx = M[0]; my = M[1]; mz = M[2];
    a00 = M[3] / n; a01 = M[4] / n; a02 = M[5] / n; a11 = M[6] / n; a12 = M[7] / n; a22 = M[8] / n;
  }
  double l0, l1, l2, nx, ny, nz;
  kk_plane(a00, a01, a02, a11, a12, a22, false, 0.0, 0.0, 0.0, l0, l1, l2, nx, ny, nz);
  const double tr = l0 + l1 + l2;
  const double curv = tr == 0.0 ? 0.0 : l0 / tr;
  const bool valid = enough && curv <= A.max_curv;
  const double cx = wx + mx, cy = wy + my, cz = wz + mz;      // the centroid as flimo_map_normals returns it
  const double d = nx * (wx - cx) + (ny * (wy - cy) + nz * (wz - cz));
  const float* R = A.P.poses + 12 * (size_t)pose;
  const double a0 = (double)R[0] * nx + ((double)R[4] * ny + (double)R[8] * nz), a1 = (double)R[1] * nx + ((double)R[5] * ny + (double)R[9] * nz),
               a2 = (double)R[2] * nx + ((double)R[6] * ny + (double)R[10] * nz);
  const float4 p4 = A.P.scan[i];
  const double px = (double)p4.x, py = (double)p4.y, pz = (double)p4.z;
  const double b0 = py * a2 - pz * a1, b1 = pz * a0 - px * a2, b2 = px * a1 - py * a0;
  double* Rw = rows + (size_t)7 * at;
  Rw[0] = valid ? a0 : nan; Rw[1] = valid ? a1 : nan; Rw[2] = valid ? a2 : nan; Rw[3] = valid ? b0 : nan; Rw[4] = valid ? b1 : nan;
  Rw[5] = valid ? b2 : nan; Rw[6] = valid ? d : nan;
  ok[at] = valid ? 1 : 0;
}

// level 1: workgroup (segment, pose) over the slots [seg * SUM_SEG, min(n, (seg + 1) * SUM_SEG)) of its pose
__global__ __launch_bounds__(SUM_RED) void lin_reduce_kernel(const double* __restrict__ rows, const unsigned char* __restrict__ ok, unsigned n,
                                                             unsigned nseg, double* __restrict__ part, int32_t* __restrict__ part_cnt) {
  const unsigned seg = blockIdx.x, pose = blockIdx.y;
  const size_t base = (size_t)pose * (size_t)n;
  const unsigned end = min(n, (seg + 1u) * (unsigned)SUM_SEG);
  double acc[LIN_NUM];
#pragma unroll
  for (int t = 0; t < LIN_NUM; t++) acc[t] = 0.0;
  int c[1] = {0};
  for (unsigned i = seg * (unsigned)SUM_SEG + threadIdx.x; i < end; i += SUM_RED) {
    const bool v = ok[base + i] != 0;
    const double* Rw = rows + (size_t)7 * (base + i);
    double J[7];
#pragma unroll
    for (int t = 0; t < 7; t++) J[t] = Rw[t];
    int t = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int b = a; b < 6; b++) { acc[t] = acc[t] + (v ? J[a] * J[b] : 0.0); t++; }
#pragma unroll
    for (int a = 0; a < 6; a++) acc[21 + a] = acc[21 + a] + (v ? J[a] * J[6] : 0.0);
    acc[27] = acc[27] + (v ? J[6] * J[6] : 0.0);
    c[0] += v ? 1 : 0;
  }
  sum_tail(acc, c, pose, nseg, seg, part, part_cnt);
}

// ---- mean neighbour distances of stored points (flimo_map_outliers) -------------------------------------------------------------
// Query i is stored point first + i, the search is the normals' with a list of k + 1 keys (OutlierJob): the point is its own neighbour
// at distance 0.  The group ends the query in registers: the slot whose insertion index is the point's own is dropped -- when no
// slot holds it and the list is full (more than k exact duplicates of lower index come first), the last one is --, c = the slots
// left, S = kk_slot_sum over the float64 widenings of fl_sqrt(sqd) with the dropped and the empty slots at +0.0: 8 B + 4 B per
// point, the list goes nowhere.  The statistics over a range's mean[] / cnt[] are sums of the shape of flimo_sums.h with one row and
// one number: a slot's term is m (pass 0, which also counts T) or (m - mu) * (m - mu) (pass 1), a slot outside T adds +0.0.
template <int L>
__device__ __forceinline__ void knnk_mean_dist(unsigned first, int k1, kk_u64 gate_key, int lane, int q, bool live, kk_u64 mine,
                                               double* __restrict__ mean, int32_t* __restrict__ cnt) {
  const int sub = lane & (L - 1);
  const bool has = live && sub < k1 && mine < gate_key;
  const bool self = has && (uint32_t)mine == first + (unsigned)q;
  const unsigned long long bs = __ballot(self);
  const bool any_self = L == 64 ? bs != 0ull : kk_group_mask<L>(bs, lane) != 0u;
  const bool keep = has && !self && (any_self || sub != k1 - 1);      // (no own slot: a result in slot k is the full list's last)
  const unsigned long long bk = __ballot(keep);
  const int c = L == 64 ? __popcll(bk) : __popc(kk_group_mask<L>(bk, lane));
  const double s = kk_slot_sum<L>(keep ? (double)fl_sqrt(kk_key_dist(mine)) : 0.0);
  if (live && sub == 0) {
    cnt[q] = c;
    mean[q] = c > 0 ? s / (double)c : __longlong_as_double(0x7ff8000000000000ll);
  }
}

// the stored points of a chunk, ended in their mean neighbour distance
struct OutlierJob : KkStored {      // (k: the neighbours asked for + 1)
  static constexpr int LANES = 0;
  static constexpr bool PAIRS = false;
  double* mean;
  int32_t* cnt;
  template <int L>
  __device__ void finish(int lane, size_t at, bool live, kk_u64 mine, float, float, float) const {
    knnk_mean_dist<L>(first, k, gate_key, lane, (int)at, live, mine, mean, cnt);
  }
};

// level 1 of the statistics: workgroup `seg` over the slots [seg * SUM_SEG, min(n, (seg + 1) * SUM_SEG)) of the range; T: cnt >= need
template <int PASS>
__global__ __launch_bounds__(SUM_RED) void outlier_sum_kernel(const double* __restrict__ mean, const int32_t* __restrict__ cnt, unsigned n, int need,
                                                              double mu, double* __restrict__ part, int32_t* __restrict__ part_cnt) {
  const unsigned seg = blockIdx.x;
  const unsigned end = min(n, (seg + 1u) * (unsigned)SUM_SEG);
  double acc[1] = {0.0};
  int c[1] = {0};
  for (unsigned i = seg * (unsigned)SUM_SEG + threadIdx.x; i < end; i += SUM_RED) {
    const bool in = cnt[i] >= need;
    const double m = mean[i];
    const double d = m - mu;
    acc[0] = acc[0] + (in ? (PASS == 0 ? m : d * d) : 0.0);
    c[0] += in ? 1 : 0;
  }
  sum_tail(acc, c, 0u, 0u, seg, part, part_cnt);      // (one row: its partials are part[seg])
}
// the predicate: few = cnt < min_pts; far = the statistical rule is on, the point is of T and its mean is beyond the threshold
__global__ __launch_bounds__(KK_BLOCK) void outlier_mask_kernel(const double* __restrict__ mean, const int32_t* __restrict__ cnt, unsigned n, int min_pts,
                                                                int need, int stat_on, double threshold, unsigned char* __restrict__ mask,
                                                                unsigned* __restrict__ counts) {
  const size_t g = (size_t)blockIdx.x * KK_BLOCK + threadIdx.x;
  bool few = false, far = false;
  if (g < (size_t)n) {
    const int c = cnt[g];
    few = c < min_pts;
    far = stat_on != 0 && c >= need && mean[g] > threshold;      // (a NaN threshold -- T is empty -- selects nothing)
    mask[g] = (few || far) ? 1 : 0;
  }
  const unsigned long long bf = __ballot(few), ba = __ballot(far);
  if ((threadIdx.x & 63) == 0) {
    if (bf) atomicAdd(&counts[0], (unsigned)__popcll(bf));
    if (ba) atomicAdd(&counts[1], (unsigned)__popcll(ba));
  }
}

// ---- FPFH descriptors of stored points (flimo_map_fpfh) --------------------------------------------------------------------------
// Two more ends of the normals' search with stored points as queries, over the normals of ALL stored points left on the device by
// launch_knn_k_normals (a neighbour can be anywhere).  Every term is float64 in the association flimo_c.h states.
//   SpfhJob  lane `sub` holds slot sub of the list of point j: it loads that stored point and its normal and forms the pair's three
//            angles and their bins (Darboux frame, PCL's computePairFeatures); a slot at distance 0 -- the point itself, its exact
//            duplicates --, a NaN normal on either side or a degenerate frame is no pair.  The 33 counts are popcounts of ballots:
//            integers, so the order of the lanes does not matter.  33 B + 1 B (the list's length c) per point.
//   FpfhJob  searches again (cheaper than 8 B x k per point of the whole map kept between the launches); lane `sub` gathers the row
//            and the length of its slot's point, forms weight * (count * 100 / (c - 1)) per bin, and every bin is one kk_slot_sum:
//            the tree over the 64 slots whose bits depend on the list alone.  Each group of 11 is scaled to a sum of 100.
// No floating-point atomics; both jobs take the worklist and the walk over the tiles as every other job does.
constexpr int FPFH_BINS = 11;                   // per angle
constexpr int FPFH_DIM = 3 * FPFH_BINS;

__device__ __forceinline__ int fpfh_bin(double x) { return (int)fmin(fmax(floor(x), 0.0), (double)(FPFH_BINS - 1)); }

template <int L>
__device__ __forceinline__ void knnk_spfh(unsigned first, int k, kk_u64 gate_key, int lane, size_t at, bool live, kk_u64 mine, float gx, float gy,
                                          float gz, const float4* __restrict__ map_raw, const float4* __restrict__ normals,
                                          unsigned char* __restrict__ spfh, unsigned char* __restrict__ len) {
  const int sub = lane & (L - 1);
  const bool has = live && sub < k && mine < gate_key;
  const unsigned long long bal = __ballot(has);
  const int c = L == 64 ? __popcll(bal) : __popc(kk_group_mask<L>(bal, lane));
  const size_t j = (size_t)first + at;
  bool pair = has && kk_key_dist(mine) != 0.f;
  int h1 = 0, h2 = 0, h3 = 0;
  if (pair) {
    const uint32_t t = (uint32_t)mine;
    const float4 pt = map_raw[t], nt4 = normals[t], ns4 = normals[j];
    pair = ns4.x == ns4.x && ns4.y == ns4.y && ns4.z == ns4.z && nt4.x == nt4.x && nt4.y == nt4.y && nt4.z == nt4.z;
    if (pair) {
      const double nsx = (double)ns4.x, nsy = (double)ns4.y, nsz = (double)ns4.z, ntx = (double)nt4.x, nty = (double)nt4.y, ntz = (double)nt4.z;
      double dx = (double)pt.x - (double)gx, dy = (double)pt.y - (double)gy, dz = (double)pt.z - (double)gz;
      const double f4 = sqrt(dx * dx + (dy * dy + dz * dz));
      const double a1 = (nsx * dx + (nsy * dy + nsz * dz)) / f4, a2 = (ntx * dx + (nty * dy + ntz * dz)) / f4;
      const bool swap = fabs(a1) < fabs(a2);      // the frame sits on the point whose normal is closer to the line (PCL: acos(|a1|) > acos(|a2|))
      const double ux = swap ? ntx : nsx, uy = swap ? nty : nsy, uz = swap ? ntz : nsz;
      const double mx = swap ? nsx : ntx, my = swap ? nsy : nty, mz = swap ? nsz : ntz;
      const double f3 = swap ? -a2 : a1;
      if (swap) { dx = -dx; dy = -dy; dz = -dz; }
      double vx = dy * uz - dz * uy, vy = dz * ux - dx * uz, vz = dx * uy - dy * ux;
      const double vn = sqrt(vx * vx + (vy * vy + vz * vz));
      pair = vn != 0.0;
      if (pair) {
        vx = vx / vn; vy = vy / vn; vz = vz / vn;
        const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
        const double f2 = vx * mx + (vy * my + vz * mz);
        const double f1 = atan2(wx * mx + (wy * my + wz * mz), ux * mx + (uy * my + uz * mz));
        h1 = fpfh_bin(11.0 * ((f1 + M_PI) * (1.0 / (2.0 * M_PI))));
        h2 = fpfh_bin(11.0 * ((f2 + 1.0) * 0.5));
        h3 = fpfh_bin(11.0 * ((f3 + 1.0) * 0.5));
      }
    }
  }
  // bin B of the row belongs to lane B % L of the group
  constexpr int NR = (FPFH_DIM + L - 1) / L;
  int r[NR];
#pragma unroll
  for (int i = 0; i < NR; i++) r[i] = 0;
#pragma unroll
  for (int B = 0; B < FPFH_DIM; B++) {
    const int h = B < FPFH_BINS ? h1 : (B < 2 * FPFH_BINS ? h2 : h3);
    const unsigned long long bb = __ballot(pair && h == B % FPFH_BINS);
    const int n = L == 64 ? __popcll(bb) : __popc(kk_group_mask<L>(bb, lane));
    if (sub == (B & (L - 1))) r[B / L] = n;
  }
  if (live) {
#pragma unroll
    for (int i = 0; i < NR; i++)
      if (sub + i * L < FPFH_DIM) spfh[j * FPFH_DIM + (size_t)(sub + i * L)] = (unsigned char)r[i];
    if (sub == 0) len[j] = (unsigned char)c;
  }
}

// the stored points of a chunk, ended in their SPFH row and the length of their list (both arrays are the whole map's)
struct SpfhJob : KkStored {
  static constexpr int LANES = 0;
  static constexpr bool PAIRS = false;
  static constexpr int WALK_WAVES = 4;      // (the pair's float64 frame and atan2: 132 B a lane spilled at 5)
  const float4* normals; // [map size]: nx ny nz curvature, NaN where there is no plane
  unsigned char* spfh;   // [map size][FPFH_DIM]
  unsigned char* len;    // [map size]
  template <int L>
  __device__ void finish(int lane, size_t at, bool live, kk_u64 mine, float gx, float gy, float gz) const {
    knnk_spfh<L>(first, k, gate_key, lane, at, live, mine, gx, gy, gz, map_raw, normals, spfh, len);
  }
};

template <int L>
__device__ __forceinline__ void knnk_fpfh(int k, kk_u64 gate_key, int lane, size_t at, bool live, kk_u64 mine, const unsigned char* __restrict__ spfh,
                                          const unsigned char* __restrict__ len, float* __restrict__ fpfh, int32_t* __restrict__ cnt) {
  const int sub = lane & (L - 1);
  const bool has = live && sub < k && mine < gate_key;
  const unsigned long long bal = __ballot(has);
  const int c = L == 64 ? __popcll(bal) : __popc(kk_group_mask<L>(bal, lane));
  double w = 0.0, inc = 0.0;
  const unsigned char* row = spfh;
  if (has) {
    const uint32_t t = (uint32_t)mine;
    const float sqd = kk_key_dist(mine);
    w = sqd != 0.f ? 1.0 / (double)sqd : 0.0;
    const int ct = (int)len[t];
    inc = ct >= 2 ? 100.0 / (double)(ct - 1) : 0.0;
    row = spfh + (size_t)t * FPFH_DIM;
  }
#pragma unroll
  for (int g = 0; g < 3; g++) {
    double F[FPFH_BINS];
#pragma unroll
    for (int b = 0; b < FPFH_BINS; b++) F[b] = kk_slot_sum<L>(has ? w * ((double)row[g * FPFH_BINS + b] * inc) : 0.0);
    double S = F[0];
#pragma unroll
    for (int b = 1; b < FPFH_BINS; b++) S = S + F[b];
    double own = 0.0;
#pragma unroll
    for (int b = 0; b < FPFH_BINS; b++) own = sub == b ? F[b] : own;
    const double scale = 100.0 / S;
    if (live && sub < FPFH_BINS) fpfh[at * FPFH_DIM + (size_t)(g * FPFH_BINS + sub)] = S != 0.0 ? (float)(own * scale) : 0.f;
  }
  if (live && sub == 0) cnt[at] = c;
}

// the stored points of a chunk of the range, ended in their FPFH row (the chunk's) from the rows of SpfhJob (the whole map's)
struct FpfhJob : KkStored {
  static constexpr int LANES = 0;
  static constexpr bool PAIRS = false;
  const unsigned char* spfh;
  const unsigned char* len;
  float* fpfh;           // [nq][FPFH_DIM]
  int32_t* cnt;          // [nq]
  template <int L>
  __device__ void finish(int lane, size_t at, bool live, kk_u64 mine, float, float, float) const {
    knnk_fpfh<L>(k, gate_key, lane, at, live, mine, spfh, len, fpfh, cnt);
  }
};

// ---- ISS keypoints of stored points (flimo_map_keypoints) ------------------------------------------------------------------------
// Saliency: NormalsJob's moments with stored points as queries, then one THREAD per point in the place of
// knnk_normals_finish_kernel: the same sums / n, the same kk_plane -- the eigenvalues are flimo_map_normals_range's by
// construction -- and the three strict float64 tests; sal [map size] holds l0 of a salient point and a quiet NaN otherwise (no
// compare with a NaN holds, so a point that is not salient neither beats a neighbour nor survives).  cnt of the points inside the
// range [rfirst, rfirst + rn) goes to rcnt when asked for.
__global__ __launch_bounds__(KK_BLOCK) void iss_saliency_kernel(unsigned first, int nq, int need, double gamma21, double gamma32,
                                                                const int32_t* __restrict__ cnt, const double* __restrict__ mom, double* __restrict__ sal,
                                                                unsigned rfirst, unsigned rn, int32_t* __restrict__ rcnt) {
  const size_t gq = (size_t)blockIdx.x * KK_BLOCK + threadIdx.x;
  if (gq >= (size_t)nq) return;
  const int c = cnt[gq];
  const double* M = mom + (size_t)KK_MOM * gq;
  const double n = (double)c;
  double s = __longlong_as_double(0x7ff8000000000000ll);
  if (c >= need) {
    double l0, l1, l2, nx, ny, nz;
    kk_plane(M[3] / n, M[4] / n, M[5] / n, M[6] / n, M[7] / n, M[8] / n, false, 0.0, 0.0, 0.0, l0, l1, l2, nx, ny, nz);
    if (l0 > 0.0 && l1 < gamma21 * l2 && l0 < gamma32 * l1) s = l0;
  }
  const unsigned j = first + (unsigned)gq;
  sal[j] = s;
  if (rcnt && j >= rfirst && j - rfirst < rn) rcnt[j - rfirst] = c;
}

// Suppression: the search once more with a list of nms_k keys.  Lane `sub` holds slot sub of the list of point j = first + at and
// gathers the saliency of that slot's point: it BEATS j when it is another point (by index: an exact duplicate is at distance 0 too)
// whose saliency is greater, or equal with a lower insertion index.  The group's ballot decides; integers only.
template <int L>
__device__ __forceinline__ void knnk_iss(unsigned first, int k, kk_u64 gate_key, int lane, size_t at, bool live, kk_u64 mine,
                                         const double* __restrict__ sal, unsigned char* __restrict__ mask, unsigned* __restrict__ count) {
  const int sub = lane & (L - 1);
  const bool has = live && sub < k && mine < gate_key;
  const unsigned j = first + (unsigned)at;
  bool beats = false;
  double sj = 0.0;
  if (live) sj = sal[j];
  if (has) {
    const uint32_t t = (uint32_t)mine;
    if (t != j) {
      const double st = sal[t];
      beats = st > sj || (st == sj && t < j);
    }
  }
  const unsigned long long bb = __ballot(beats);
  const bool beaten = L == 64 ? bb != 0ull : kk_group_mask<L>(bb, lane) != 0u;
  const bool key = live && sj == sj && !beaten;
  const unsigned long long bk = __ballot(key && sub == 0);
  if (live && sub == 0) mask[at] = key ? 1 : 0;
  if (lane == 0 && bk) atomicAdd(count, (unsigned)__popcll(bk));
}

// the stored points of a chunk of the range, ended in their mask byte (the chunk's) from the saliency of the whole map
struct IssJob : KkStored {
  static constexpr int LANES = 0;
  static constexpr bool PAIRS = false;
  const double* sal;     // [map size]
  unsigned char* mask;   // [nq]
  unsigned* count;       // the keypoints so far
  template <int L>
  __device__ void finish(int lane, size_t at, bool live, kk_u64 mine, float, float, float) const {
    knnk_iss<L>(first, k, gate_key, lane, at, live, mine, sal, mask, count);
  }
};

// lanes per query from k: a list of k keys needs k lanes
int knnk_plan(int k) { return k <= 16 ? 16 : 64; }

// the gate: r2 [m^2] and the key every list starts filled with
static void kk_gate(float max_dist, float& r2, kk_u64& gate_key) {
  r2 = max_dist * max_dist;                  // one float32 product, as the radius search's (Octree.hpp:467); INFINITY: no gate
  uint32_t r2_bits;
  memcpy(&r2_bits, &r2, sizeof r2_bits);
  gate_key = std::isinf(max_dist) ? KK_NONE : (kk_u64)r2_bits << 32;
}

constexpr unsigned KK_MAX_GRID_X = 1u << 20;    // the pairs' search grid is (workgroups of a pose, poses); a pose of more workgroups takes several launches

template <int L, class Job>
static void kk_launch_search(hipStream_t st, const GridView& G, Job J, uint2* work, unsigned* nwork) {
  constexpr unsigned qpb = KK_BLOCK / L;      // queries per workgroup
  if constexpr (Job::PAIRS) {
    const unsigned bpp = (unsigned)(((size_t)J.P.n + qpb - 1) / qpb);      // workgroups per pose
    for (J.P.b0 = 0; J.P.b0 < bpp; J.P.b0 += KK_MAX_GRID_X)
      hipLaunchKernelGGL((kk_search_kernel<L, Job>), dim3(std::min(bpp - J.P.b0, KK_MAX_GRID_X), J.P.np), dim3(KK_BLOCK), 0, st, G, J, work, nwork);
  } else {
    hipLaunchKernelGGL((kk_search_kernel<L, Job>), dim3((unsigned)((J.total() + qpb - 1) / qpb)), dim3(KK_BLOCK), 0, st, G, J, work, nwork);
  }
}
// the worklist emptied, the block search, the walk over the tiles of what it could not prove
template <class Job>
static hipError_t kk_launch(hipStream_t st, const GridView& G, const Job& J, uint2* work, unsigned* nwork) {
  const hipError_t e = hipMemsetAsync(nwork, 0, sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  if constexpr (Job::LANES != 0) kk_launch_search<Job::LANES>(st, G, J, work, nwork);
  else if (knnk_plan(J.k) == 16) kk_launch_search<16>(st, G, J, work, nwork);
  else kk_launch_search<64>(st, G, J, work, nwork);
  const unsigned walk_blocks = (unsigned)std::min<size_t>(4096, (J.total() + KK_BLOCK / 64 - 1) / (KK_BLOCK / 64));
  hipLaunchKernelGGL(kk_walk_kernel<Job>, dim3(walk_blocks), dim3(KK_BLOCK), 0, st, G, J, work, nwork);
  return hipGetLastError();
}
// the fields every job over a chunk of flat slots has: the chunk, the list's length, the gate, the stored points
template <class Job>
static void kk_fill(Job& J, unsigned first, int nq, int k, float max_dist, const float4* map_raw) {
  J.first = first; J.nq = nq; J.k = k;
  kk_gate(max_dist, J.r2, J.gate_key);
  J.map_raw = map_raw;
}

template <bool COUNT>
static hipError_t knn_k_launch(hipStream_t st, const GridView& G, const float4* map_raw, const float* q, int nq, int k, float max_dist, int32_t* idx,
                               float* sqd, float* xyz, int32_t* cnt, unsigned long long* cand, uint2* work, unsigned* nwork) {
  KnnJob<COUNT> J;
  J.qxyz = q; J.nq = nq; J.k = k;
  kk_gate(max_dist, J.r2, J.gate_key);
  J.map_raw = map_raw; J.idx = idx; J.sqd = sqd; J.xyz = xyz; J.cnt = cnt; J.cand = cand;
  return kk_launch(st, G, J, work, nwork);
}
hipError_t launch_knn_k(hipStream_t st, const GridView& G, const float4* map_raw, const float* q, int nq, int k, float max_dist, int32_t* idx,
                        float* sqd, float* xyz, int32_t* cnt, unsigned long long* cand, uint2* work, unsigned* nwork) {
  if (nq <= 0) return hipSuccess;
  if (k < 1 || k > KNNK_MAX_K) return hipErrorInvalidValue;
  return cand ? knn_k_launch<true>(st, G, map_raw, q, nq, k, max_dist, idx, sqd, xyz, cnt, cand, work, nwork)
              : knn_k_launch<false>(st, G, map_raw, q, nq, k, max_dist, idx, sqd, xyz, cnt, cand, work, nwork);
}

hipError_t launch_knn_k_normals(hipStream_t st, const GridView& G, const float4* map_raw, const float* q, unsigned first, int nq, int k,
                                float max_dist, int min_pts, const float* viewpoint, float4* normal, int32_t* cnt, double* centroid, double* cov,
                                double* eig, double* mom, uint2* work, unsigned* nwork) {
  if (nq <= 0) return hipSuccess;
  if (k < 1 || k > KNNK_MAX_K) return hipErrorInvalidValue;
  NormalsJob J;
  kk_fill(J, first, nq, k, max_dist, map_raw);
  J.qxyz = q; J.need = std::max(3, min_pts);
  J.has_vp = viewpoint != nullptr;
  J.vx = viewpoint ? viewpoint[0] : 0.f; J.vy = viewpoint ? viewpoint[1] : 0.f; J.vz = viewpoint ? viewpoint[2] : 0.f;
  J.cnt = cnt; J.mom = mom;
  const NormalsOut O{normal, cnt, centroid, cov, eig};
  const hipError_t e = kk_launch(st, G, J, work, nwork);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(knnk_normals_finish_kernel, dim3((unsigned)(((size_t)nq + KK_BLOCK - 1) / KK_BLOCK)), dim3(KK_BLOCK), 0, st, static_cast<const NormalsArgs&>(J), map_raw, mom, O);
  return hipGetLastError();
}

hipError_t launch_outlier_search(hipStream_t st, const GridView& G, const float4* map_raw, unsigned first, int nq, int k, float max_dist,
                                 double* mean, int32_t* cnt, uint2* work, unsigned* nwork) {
  if (nq <= 0) return hipSuccess;
  if (k < 1 || k + 1 > KNNK_MAX_K) return hipErrorInvalidValue;
  OutlierJob J;
  kk_fill(J, first, nq, k + 1, max_dist, map_raw);
  J.mean = mean; J.cnt = cnt;
  return kk_launch(st, G, J, work, nwork);
}

hipError_t launch_fpfh_spfh(hipStream_t st, const GridView& G, const float4* map_raw, const float4* normals, unsigned first, int nq, int k,
                            float max_dist, unsigned char* spfh, unsigned char* len, uint2* work, unsigned* nwork) {
  if (nq <= 0) return hipSuccess;
  if (k < 1 || k > KNNK_MAX_K) return hipErrorInvalidValue;
  SpfhJob J;
  kk_fill(J, first, nq, k, max_dist, map_raw);
  J.normals = normals; J.spfh = spfh; J.len = len;
  return kk_launch(st, G, J, work, nwork);
}

hipError_t launch_fpfh_sum(hipStream_t st, const GridView& G, const float4* map_raw, const unsigned char* spfh, const unsigned char* len,
                           unsigned first, int nq, int k, float max_dist, float* fpfh, int32_t* cnt, uint2* work, unsigned* nwork) {
  if (nq <= 0) return hipSuccess;
  if (k < 1 || k > KNNK_MAX_K) return hipErrorInvalidValue;
  FpfhJob J;
  kk_fill(J, first, nq, k, max_dist, map_raw);
  J.spfh = spfh; J.len = len; J.fpfh = fpfh; J.cnt = cnt;
  return kk_launch(st, G, J, work, nwork);
}

hipError_t launch_iss_saliency(hipStream_t st, const GridView& G, const float4* map_raw, unsigned first, int nq, int k, float max_dist, int min_pts,
                               float gamma21, float gamma32, double* sal, unsigned rfirst, unsigned rn, int32_t* rcnt, int32_t* cnt, double* mom,
                               uint2* work, unsigned* nwork) {
  if (nq <= 0) return hipSuccess;
  if (k < 1 || k > KNNK_MAX_K) return hipErrorInvalidValue;
  NormalsJob J;
  kk_fill(J, first, nq, k, max_dist, map_raw);
  J.qxyz = nullptr; J.need = std::max(3, min_pts);
  J.has_vp = 0; J.vx = J.vy = J.vz = 0.f;
  J.cnt = cnt; J.mom = mom;
  const hipError_t e = kk_launch(st, G, J, work, nwork);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(iss_saliency_kernel, dim3((unsigned)(((size_t)nq + KK_BLOCK - 1) / KK_BLOCK)), dim3(KK_BLOCK), 0, st, first, nq, J.need,
                     (double)gamma21, (double)gamma32, cnt, mom, sal, rfirst, rn, rcnt);
  return hipGetLastError();
}

hipError_t launch_iss_suppress(hipStream_t st, const GridView& G, const float4* map_raw, const double* sal, unsigned first, int nq, int k,
                               float max_dist, unsigned char* mask, unsigned* count, uint2* work, unsigned* nwork) {
  if (nq <= 0) return hipSuccess;
  if (k < 1 || k > KNNK_MAX_K) return hipErrorInvalidValue;
  IssJob J;
  kk_fill(J, first, nq, k, max_dist, map_raw);
  J.sal = sal; J.mask = mask; J.count = count;
  return kk_launch(st, G, J, work, nwork);
}

hipError_t launch_outlier_sum(hipStream_t st, const double* mean, const int32_t* cnt, unsigned n, int need, int pass, double mu, double* part,
                              int32_t* part_cnt, unsigned long long* out) {
  if (n == 0) return hipErrorInvalidValue;
  const unsigned nseg = sum_segments(n);
  if (pass == 0) hipLaunchKernelGGL((outlier_sum_kernel<0>), dim3(nseg), dim3(SUM_RED), 0, st, mean, cnt, n, need, mu, part, part_cnt);
  else hipLaunchKernelGGL((outlier_sum_kernel<1>), dim3(nseg), dim3(SUM_RED), 0, st, mean, cnt, n, need, mu, part, part_cnt);
  // (out[0] takes the sum as a float64 -- its bits --, out[1] the count as a 64-bit integer)
  launch_sum_final<1, 1>(st, part, part_cnt, 1u, nseg, reinterpret_cast<double*>(out), reinterpret_cast<long long*>(out + 1));
  return hipGetLastError();
}

hipError_t launch_outlier_mask(hipStream_t st, const double* mean, const int32_t* cnt, unsigned n, int min_pts, int need, bool stat_on,
                               double threshold, unsigned char* mask, unsigned* counts) {
  if (n == 0) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(counts, 0, 2 * sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(outlier_mask_kernel, dim3((unsigned)(((size_t)n + KK_BLOCK - 1) / KK_BLOCK)), dim3(KK_BLOCK), 0, st, mean, cnt, n, min_pts, need,
                     stat_on ? 1 : 0, threshold, mask, counts);
  return hipGetLastError();
}

hipError_t launch_scan_fit_search(hipStream_t st, const GridView& G, const float4* scan, unsigned n, const float* poses, unsigned np, float max_dist,
                                  float* sqd, int32_t* idx, uint2* work, unsigned* nwork) {
  if (n == 0 || np == 0) return hipSuccess;
  if ((unsigned long long)n * np > 0x80000000ull || np > FIT_MAX_POSES) return hipErrorInvalidValue;
  FitJob J;
  J.P = KkPairs{scan, poses, n, np, 0};
  kk_gate(max_dist, J.r2, J.gate_key);
  J.sqd = sqd; J.idx = idx;
  return kk_launch(st, G, J, work, nwork);
}
hipError_t launch_scan_fit_reduce(hipStream_t st, const float* sqd, unsigned n, unsigned np, int32_t* inliers, double* sum_sqd) {
  if (n == 0 || np == 0) return hipSuccess;
  hipLaunchKernelGGL(fit_reduce_kernel, dim3(np), dim3(FIT_RED), 0, st, sqd, n, inliers, sum_sqd);
  return hipGetLastError();
}
hipError_t launch_scan_fitness(hipStream_t st, const GridView& G, const float4* scan, unsigned n, const float* poses, unsigned np, float max_dist,
                               float* sqd, int32_t* idx, uint2* work, unsigned* nwork, int32_t* inliers, double* sum_sqd) {
  const hipError_t e = launch_scan_fit_search(st, G, scan, n, poses, np, max_dist, sqd, idx, work, nwork);
  if (e != hipSuccess) return e;
  return launch_scan_fit_reduce(st, sqd, n, np, inliers, sum_sqd);
}

hipError_t launch_scan_linearize(hipStream_t st, const GridView& G, const float4* map_raw, const float4* scan, unsigned n, const float* poses,
                                 unsigned np, int k, float max_dist, int min_pts, float max_curv, int32_t* cnt, double* mom, uint2* work,
                                 unsigned* nwork, double* rows, unsigned char* ok, double* part, int32_t* part_cnt, double* sums, long long* valid) {
  if (n == 0 || np == 0) return hipSuccess;
  if ((unsigned long long)n * np > 0x10000000ull || np > FIT_MAX_POSES || k < 1 || k > KNNK_MAX_K) return hipErrorInvalidValue;
  LinJob J;
  J.P = KkPairs{scan, poses, n, np, 0};
  J.need = std::max(3, min_pts);
  J.max_curv = (double)max_curv;
  J.k = k;
  kk_gate(max_dist, J.r2, J.gate_key);
  J.map_raw = map_raw; J.cnt = cnt; J.mom = mom;
  const hipError_t e = kk_launch(st, G, J, work, nwork);
  if (e != hipSuccess) return e;
  const size_t pairs = (size_t)n * np;
  hipLaunchKernelGGL(lin_finish_kernel, dim3((unsigned)((pairs + KK_BLOCK - 1) / KK_BLOCK)), dim3(KK_BLOCK), 0, st, J, cnt, mom, rows, ok);
  const unsigned nseg = sum_segments(n);
  hipLaunchKernelGGL(lin_reduce_kernel, dim3(nseg, np), dim3(SUM_RED), 0, st, rows, ok, n, nseg, part, part_cnt);
  launch_sum_final<LIN_NUM, 1>(st, part, part_cnt, np, nseg, sums, valid);
  return hipGetLastError();
}

}  // namespace flimo
