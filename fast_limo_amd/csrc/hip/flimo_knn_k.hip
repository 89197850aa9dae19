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
// The search.  knnk_kernel<L> (L = 16 lanes per query for k <= 16, a wave beyond): blocks of rows around the query's cell as
// knn_search does -- ring 1, then straight to the ring that proves exactness once k candidates (or the gate) bound the distance;
// of a later block only the shell beyond the block already walked is read, so no point is met twice.  Rows and the cells of a row
// are pruned by the smaller of the k-th distance and the gate.  A query is PROVEN when that bound is <= the distance to the nearest
// cell face not visited (knn_search's margins), or the block covers the grid.  What would need more than KK_FAR_RING rings is left
// to knnk_far_kernel: one wave per query, best-first over the directory's existing tiles, nearest first, until the next tile is
// farther than the bound (knn_far_kernel's scheme with the distributed list): a query kilometres from every point costs a look at
// the directory and the nearest tiles.  All pruning is conservative; the float32 key compare alone decides membership and order.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include "flimo_types.h"
#include "flimo_math.h"
#include "flimo_kernels.h"

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
__device__ __forceinline__ void knnk_store(int lane, int q, int k, kk_u64 mine, kk_u64 gate_key, bool proven, bool live,
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
      if (has && proven) p = map_raw[ins];
      xyz[3 * at] = p.x; xyz[3 * at + 1] = p.y; xyz[3 * at + 2] = p.z;
    }
  }
  if (live && sub == 0) cnt[q] = proven ? c : -c - 1;      // (negative: knnk_far_kernel finishes the query)
}

template <int L>
__global__ __launch_bounds__(KK_BLOCK) void knnk_kernel(GridView G, const float* __restrict__ qxyz, int nq, int k, float r2, kk_u64 gate_key,
                                                        const float4* __restrict__ map_raw, int32_t* __restrict__ idx, float* __restrict__ sqd,
                                                        float* __restrict__ xyz, int32_t* __restrict__ cnt, unsigned long long* __restrict__ cand_out) {
  const int lane = threadIdx.x & 63;
  const int sub = lane & (L - 1);
  const size_t gq = ((size_t)blockIdx.x * KK_BLOCK + threadIdx.x) / (unsigned)L;
  const bool live = gq < (size_t)nq;
  const int q = live ? (int)gq : 0;
  const int maxdim = grid_maxdim(G);
  float gx = 0.f, gy = 0.f, gz = 0.f;
  if (live) { gx = qxyz[3 * q]; gy = qxyz[3 * q + 1]; gz = qxyz[3 * q + 2]; }
  KnnkGeo g;
  const bool valid = knnk_geo(G, maxdim, live ? gx : NAN, gy, gz, g);
  const float edge = fminf(fminf(fminf(g.rx, 1.f - g.rx), fminf(g.ry, 1.f - g.ry)), fminf(g.rz, 1.f - g.rz));
  kk_u64 mine = gate_key;
  unsigned long long cand = 0;
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
  knnk_store<L>(lane, q, k, mine, gate_key, proven, live, map_raw, idx, sqd, xyz, cnt);
  if (cand_out && live && sub == 0) cand_out[q] = cand;
}

// What knnk_kernel could not prove within KK_FAR_RING rings, ONE WAVE PER QUERY over the directory of tiles that exist: tiles in
// ascending order of their box's distance to the query (a lower bound of the distance of every point inside) until the next tile
// is farther than the bound -- the smaller of the gate and the k-th best -- or none is left.  The list starts afresh; when the
// block search left k candidates, its k-th distance (an upper bound of the true one) is the first bound.
__global__ __launch_bounds__(KK_BLOCK) void knnk_far_kernel(GridView G, const float* __restrict__ qxyz, int nq, int k, float r2, kk_u64 gate_key,
                                                            const float4* __restrict__ map_raw, int32_t* __restrict__ idx, float* __restrict__ sqd,
                                                            float* __restrict__ xyz, int32_t* __restrict__ cnt, unsigned long long* __restrict__ cand_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int maxdim = grid_maxdim(G);
  const int ndir = G.ntx * G.nty * G.ntz;
  const int cells_per_xtile = max(1, (8 << G.ts) / G.xs);
  for (int q = blockIdx.x * (KK_BLOCK / 64) + wave; q < nq; q += gridDim.x * (KK_BLOCK / 64)) {
    const int c0 = cnt[q];
    if (c0 >= 0) continue;                                       // proven by the block search (wave-uniform)
    const float gx = qxyz[3 * q], gy = qxyz[3 * q + 1], gz = qxyz[3 * q + 2];
    KnnkGeo g;
    (void)knnk_geo(G, maxdim, gx, gy, gz, g);                    // (a NaN query never comes here)
    float bound = r2;
    if (-c0 - 1 == k) bound = fminf(bound, sqd[(size_t)q * k + (k - 1)]);
    float bnd2 = kk_ball(G, bound);
    kk_u64 mine = gate_key;
    unsigned long long cand = 0;
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
    knnk_store<64>(lane, q, k, mine, gate_key, true, true, map_raw, idx, sqd, xyz, cnt);
    if (cand_out && lane == 0) cand_out[q] += cand;
  }
}

// lanes per query from k: a list of k keys needs k lanes
int knnk_plan(int k) { return k <= 16 ? 16 : 64; }

hipError_t launch_knn_k(hipStream_t st, const GridView& G, const float4* map_raw, const float* q, int nq, int k, float max_dist, int32_t* idx,
                        float* sqd, float* xyz, int32_t* cnt, unsigned long long* cand) {
  if (nq <= 0) return hipSuccess;
  if (k < 1 || k > KNNK_MAX_K) return hipErrorInvalidValue;
  const float r2 = max_dist * max_dist;      // one float32 product, as the radius search's (Octree.hpp:467); INFINITY: no gate
  uint32_t r2_bits;
  memcpy(&r2_bits, &r2, sizeof r2_bits);
  const kk_u64 gate_key = std::isinf(max_dist) ? KK_NONE : (kk_u64)r2_bits << 32;
  const int L = knnk_plan(k);
  const unsigned blocks = (unsigned)(((size_t)nq * L + KK_BLOCK - 1) / KK_BLOCK);
  if (L == 16) hipLaunchKernelGGL((knnk_kernel<16>), dim3(blocks), dim3(KK_BLOCK), 0, st, G, q, nq, k, r2, gate_key, map_raw, idx, sqd, xyz, cnt, cand);
  else hipLaunchKernelGGL((knnk_kernel<64>), dim3(blocks), dim3(KK_BLOCK), 0, st, G, q, nq, k, r2, gate_key, map_raw, idx, sqd, xyz, cnt, cand);
  const unsigned far_blocks = (unsigned)std::min<size_t>(4096, ((size_t)nq + KK_BLOCK / 64 - 1) / (KK_BLOCK / 64));
  hipLaunchKernelGGL(knnk_far_kernel, dim3(far_blocks), dim3(KK_BLOCK), 0, st, G, q, nq, k, r2, gate_key, map_raw, idx, sqd, xyz, cnt, cand);
  return hipGetLastError();
}

}  // namespace flimo
