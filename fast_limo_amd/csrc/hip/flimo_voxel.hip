// fast_limo_amd/csrc/hip/flimo_voxel.hip -- voxel statistics and thinning of the stored points (flimo_map_voxels,
// flimo_map_voxel_mask, flimo_map_thin; include/flimo_c.h): what pcl::VoxelGrid computes per leaf, over the map, on a lattice that
// does not move when the map grows, with float64 sums of one fixed shape.
//
//   voxel_key_kernel       one THREAD per stored point: its 64-bit key (voxel_key, flimo_voxel.h), all-ones for an outside point, and
//                          the outside count (a ballot and one integer add per wave).
//   (sort_pairs_u64)       stable: the members of a voxel come out in ascending insertion index.
//   voxel_head_kernel      head flags; an exclusive scan of them numbers the voxels in ascending key.
//   voxel_segment_kernel   per head: the segment start, the cell and the first member.
//   voxel_classify_kernel  one THREAD per voxel: count, the largest count, the lane plan of the voxel (an integer append to the
//                          plan's list: the list's order is free, every result is written by voxel index) and, for the many-runs
//                          path, its number of runs (an exclusive scan of those numbers the run slots).
//   voxel_group_kernel<G>  the hot path: a GROUP of G = 8, 16 or 64 lanes per voxel.  A run is 64 slots; a lane holds 64 / G
//                          neighbouring slots, adds them pairwise in registers and the group finishes the tree by __shfl_xor
//                          (a voxel of at most G points: one slot per lane, the upper levels of the tree would add +0.0 only).  The
//                          centroid pass first, then covariance and nearest in a second pass over the same members.
//   voxel_run_*_kernel     the many-runs path: one WAVE per run of any voxel of the list (the run's voxel by binary search in the
//                          scanned run numbers), the run's sums into a slot; then one wave per voxel chains the slots in ascending
//                          order -- the only serial part of the shape.  Twice: coordinates, then products and nearest.
//   voxel_point_kernel     one THREAD per sorted position: rank = position - segment start, voxel[], the mask, and the count of
//                          ones by one ballot and one integer add per wave.
// No atomics on floating-point values: the bits depend on the stored points and the leaf alone.
#include <algorithm>
#include "flimo_voxel.h"
#include "flimo_prims.h"
#include "flimo_kernels.h"

#pragma clang fp contract(off)

namespace flimo {

__global__ __launch_bounds__(256) void voxel_key_kernel(const float4* __restrict__ map, unsigned n, float inv,
                                                        unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals,
                                                        uint32_t* __restrict__ words) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  bool out = false;
  if (i < n) {
    const float4 p = map[i];
    int32_t ijk[3];
    unsigned long long k;
    out = !voxel_key(p.x, p.y, p.z, inv, ijk, &k);
    keys[i] = k;
    vals[i] = i;
  }
  const unsigned long long b = __ballot(out);
  if ((threadIdx.x & 63u) == 0u && b) atomicAdd(&words[VOXEL_W_OUTSIDE], (unsigned)__popcll(b));
}

__global__ __launch_bounds__(256) void voxel_head_kernel(const unsigned long long* __restrict__ keys, unsigned n, uint32_t* __restrict__ head) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i];
  head[i] = (k != VOXEL_OUTSIDE && (i == 0u || keys[i - 1u] != k)) ? 1u : 0u;
}

// seg [nv + 1]: seg[nv] = the number of inside points (they come first in sorted order)
__global__ __launch_bounds__(256) void voxel_segment_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ perm,
                                                            const uint32_t* __restrict__ head, const uint32_t* __restrict__ pos, unsigned n,
                                                            unsigned nv, unsigned inside, uint32_t* __restrict__ seg,
                                                            int32_t* __restrict__ ijk, int32_t* __restrict__ first) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0u) seg[nv] = inside;
  if (i >= n || !head[i]) return;
  const unsigned v = pos[i];
  seg[v] = i;
  if (ijk) {      // (null: the keys are no cells -- flimo_region.hip's listing)
    int32_t c[3];
    voxel_cell_of_key(keys[i], c);
    ijk[3 * (size_t)v] = c[0]; ijk[3 * (size_t)v + 1] = c[1]; ijk[3 * (size_t)v + 2] = c[2];
  }
  first[v] = (int32_t)perm[i];
}

// lists: [4][nv] (may be null: no moments are wanted), runs: [nv + 1]
__global__ __launch_bounds__(256) void voxel_classify_kernel(const uint32_t* __restrict__ seg, unsigned nv, int plan, int32_t* __restrict__ count,
                                                             uint32_t* __restrict__ runs, uint32_t* __restrict__ lists,
                                                             uint32_t* __restrict__ words) {
  // (atomics on one address are slow on this part: one add per class and one max per WORKGROUP, the places inside it from ballots)
  __shared__ unsigned s_cnt[4][4], s_base[4], s_max[4];
  const unsigned v = blockIdx.x * blockDim.x + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  unsigned c = 0;
  int cls = -1;
  if (v < nv) {
    c = seg[v + 1u] - seg[v];
    count[v] = (int32_t)c;
    if (lists) {
      cls = plan != VOXEL_PLAN_AUTO ? plan - 1 : c <= 8u ? 0 : c <= 16u ? 1 : c <= VOXEL_MANY ? 2 : 3;
      runs[v] = cls == 3 ? (c + 63u) / 64u : 0u;
    }
  } else if (v == nv && lists) {
    runs[nv] = 0u;
  }
  unsigned m = c;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
  unsigned before = 0;                                    // the voxels of this thread's class in the lanes below it
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const unsigned long long b = __ballot(cls == k);
    if (lane == 0u) s_cnt[wave][k] = (unsigned)__popcll(b);
    if (cls == k) before = (unsigned)__popcll(b & ((1ull << lane) - 1ull));
  }
  if (lane == 0u) s_max[wave] = m;
  __syncthreads();
  if (threadIdx.x < 4u) {
    const unsigned tot = (s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x]) + (s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x]);
    s_base[threadIdx.x] = tot ? atomicAdd(&words[VOXEL_W_LIST + threadIdx.x], tot) : 0u;
  } else if (threadIdx.x == 64u) {
    const unsigned mm = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
    if (mm) atomicMax(&words[VOXEL_W_LARGEST], mm);
  }
  __syncthreads();
  if (cls >= 0) {
    unsigned at = s_base[cls] + before;
    for (unsigned w = 0; w < wave; w++) at += s_cnt[w][cls];
    lists[(size_t)cls * nv + at] = v;
  }
}

struct VoxView {
  const float4* pts;         // the stored points, or their copy in sorted order
  const uint32_t* gather;    // sorted position -> index into pts; null: pts is in sorted order
  const uint32_t* perm;      // sorted position -> insertion index
  const uint32_t* seg;       // [nv + 1]
};
__device__ inline float4 vox_point(const VoxView& w, unsigned i) { return w.pts[w.gather ? w.gather[i] : i]; }

// the levels of the run tree that lie across the G lanes of a group: t[s] += t[s ^ o]
template <int G>
__device__ inline double vox_tree(double v) {
#pragma unroll
  for (int o = 1; o < G; o <<= 1) v = v + __shfl_xor(v, o, G);
  return v;
}
// ... and the levels inside a lane: K neighbouring slots, ((u0 + u1) + (u2 + u3)) + ...
template <int K>
__device__ inline double vox_local(double (&u)[K]) {
#pragma unroll
  for (int w = 1; w < K; w <<= 1)
#pragma unroll
    for (int t = 0; t < K; t += 2 * w) u[t] = u[t] + u[t + w];
  return u[0];
}
// the smaller (q, sorted position) of the group: a position is a member's rank, so ties go to the smaller insertion index
template <int G>
__device__ inline void vox_nearest(double& q, unsigned& p) {
#pragma unroll
  for (int o = 1; o < G; o <<= 1) {
    const double q2 = __shfl_xor(q, o, G);
    const unsigned p2 = (unsigned)__shfl_xor((int)p, o, G);
    if (q2 < q || (q2 == q && p2 < p)) { q = q2; p = p2; }
  }
}
__device__ inline double vox_sq(double x, double y, double z) { return x * x + (y * y + z * z); }

template <int G>
__global__ __launch_bounds__(256) void voxel_group_kernel(VoxView w, const uint32_t* __restrict__ list, unsigned nlist, int second,
                                                          double* __restrict__ centroid, double* __restrict__ cov, int32_t* __restrict__ rep) {
  constexpr int K = 64 / G;
  const unsigned g = (blockIdx.x * 256u + threadIdx.x) / (unsigned)G, lane = threadIdx.x & (unsigned)(G - 1);
  if (g >= nlist) return;                                 // (whole groups leave: the shuffles below stay inside a group)
  const unsigned v = list[g], s = w.seg[v], c = w.seg[v + 1u] - s;
  const bool compact = c <= (unsigned)G;                  // one slot per lane, one run
  const unsigned runs = compact ? 1u : (c + 63u) / 64u;
  double S[3] = {0.0, 0.0, 0.0};
  for (unsigned j = 0; j < runs; j++) {
    double u[3][K];
#pragma unroll
    for (int t = 0; t < K; t++) {
      const unsigned slot = compact ? lane : 64u * j + lane * (unsigned)K + (unsigned)t;
      const bool have = (!compact || t == 0) && slot < c;
      float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
      if (have) p = vox_point(w, s + slot);                 // (an absent slot costs no load)
      u[0][t] = have ? (double)p.x : 0.0;
      u[1][t] = have ? (double)p.y : 0.0;
      u[2][t] = have ? (double)p.z : 0.0;
    }
#pragma unroll
    for (int a = 0; a < 3; a++) S[a] = S[a] + vox_tree<G>(vox_local<K>(u[a]));
  }
  const double dc = (double)c;
  const double cen[3] = {S[0] / dc, S[1] / dc, S[2] / dc};
  if (lane == 0u)
    for (int a = 0; a < 3; a++) centroid[3 * (size_t)v + a] = cen[a];
  if (!second) return;
  double C[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double bq = __builtin_inf();
  unsigned bp = 0xffffffffu;
  for (unsigned j = 0; j < runs; j++) {
    double d[3][K];
    double q = __builtin_inf();
    unsigned qp = 0xffffffffu;
#pragma unroll
    for (int t = 0; t < K; t++) {
      const unsigned slot = compact ? lane : 64u * j + lane * (unsigned)K + (unsigned)t;
      const bool have = (!compact || t == 0) && slot < c;
      float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
      if (have) p = vox_point(w, s + slot);                 // (an absent slot costs no load)
      d[0][t] = have ? (double)p.x - cen[0] : 0.0;
      d[1][t] = have ? (double)p.y - cen[1] : 0.0;
      d[2][t] = have ? (double)p.z - cen[2] : 0.0;
      const double qt = vox_sq(d[0][t], d[1][t], d[2][t]);
      if (have && qt < q) { q = qt; qp = s + slot; }      // (ascending slots, strict: the first of equals stays)
    }
    vox_nearest<G>(q, qp);
    if (q < bq) { bq = q; bp = qp; }                       // (ascending runs, strict)
    int k = 0;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = a; b < 3; b++, k++) {
        double pr[K];
#pragma unroll
        for (int t = 0; t < K; t++) pr[t] = d[a][t] * d[b][t];
        C[k] = C[k] + vox_tree<G>(vox_local<K>(pr));
      }
  }
  if (lane == 0u) {
    for (int k = 0; k < 6; k++) cov[6 * (size_t)v + k] = C[k] / dc;
    rep[v] = (int32_t)w.perm[bp == 0xffffffffu ? s : bp];      // (stored points are finite: some q is below infinity)
  }
}

// the voxel of run slot r: the last v with roff[v] <= r (roff [nv + 1] is the exclusive scan of the voxels' run numbers; a voxel
// of no runs shares its offset with the next one that has some, which comes later)
__device__ inline unsigned vox_run_owner(const uint32_t* __restrict__ roff, unsigned nv, unsigned r) {
  unsigned lo = 0, hi = nv;
  while (hi - lo > 1u) {
    const unsigned mid = lo + (hi - lo) / 2u;
    if (roff[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

// rs [R][3]: the coordinate sums of every run
__global__ __launch_bounds__(256) void voxel_run_sum_kernel(VoxView w, const uint32_t* __restrict__ roff, unsigned nv, unsigned R,
                                                            double* __restrict__ rs) {
  const unsigned r = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (r >= R) return;
  const unsigned v = vox_run_owner(roff, nv, r), j = r - roff[v], s = w.seg[v], c = w.seg[v + 1u] - s;
  const unsigned slot = 64u * j + lane;
  const bool have = slot < c;
  const float4 p = vox_point(w, s + (have ? slot : 0u));
  const double x = vox_tree<64>(have ? (double)p.x : 0.0), y = vox_tree<64>(have ? (double)p.y : 0.0), z = vox_tree<64>(have ? (double)p.z : 0.0);
  if (lane == 0u) { rs[3 * (size_t)r] = x; rs[3 * (size_t)r + 1] = y; rs[3 * (size_t)r + 2] = z; }
}
// S = ((+0.0 + R_0) + R_1) + ... per listed voxel: one wave, 64 slots loaded at a time, every lane keeps the same chain
__global__ __launch_bounds__(256) void voxel_run_centroid_kernel(VoxView w, const uint32_t* __restrict__ list, unsigned nlist,
                                                                 const uint32_t* __restrict__ roff, const double* __restrict__ rs,
                                                                 double* __restrict__ centroid) {
  const unsigned g = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (g >= nlist) return;
  const unsigned v = list[g], c = w.seg[v + 1u] - w.seg[v], runs = (c + 63u) / 64u, r0 = roff[v];
  double S[3] = {0.0, 0.0, 0.0};
  for (unsigned base = 0; base < runs; base += 64u) {
    const unsigned lim = min(64u, runs - base);
    double x[3];
    for (int a = 0; a < 3; a++) x[a] = lane < lim ? rs[3 * (size_t)(r0 + base + lane) + a] : 0.0;
    for (unsigned t = 0; t < lim; t++)
      for (int a = 0; a < 3; a++) S[a] = S[a] + __shfl(x[a], (int)t, 64);
  }
  const double dc = (double)c;
  if (lane < 3u) centroid[3 * (size_t)v + lane] = (lane == 0u ? S[0] : lane == 1u ? S[1] : S[2]) / dc;
}
// rc [R][6], rq [R], rp [R]: the product sums, the smallest q and its sorted position of every run
__global__ __launch_bounds__(256) void voxel_run_cov_kernel(VoxView w, const uint32_t* __restrict__ roff, unsigned nv, unsigned R,
                                                            const double* __restrict__ centroid, double* __restrict__ rc,
                                                            double* __restrict__ rq, uint32_t* __restrict__ rp) {
  const unsigned r = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (r >= R) return;
  const unsigned v = vox_run_owner(roff, nv, r), j = r - roff[v], s = w.seg[v], c = w.seg[v + 1u] - s;
  const unsigned slot = 64u * j + lane;
  const bool have = slot < c;
  const float4 p = vox_point(w, s + (have ? slot : 0u));
  const double cen[3] = {centroid[3 * (size_t)v], centroid[3 * (size_t)v + 1], centroid[3 * (size_t)v + 2]};
  const double d[3] = {have ? (double)p.x - cen[0] : 0.0, have ? (double)p.y - cen[1] : 0.0, have ? (double)p.z - cen[2] : 0.0};
  double q = have ? vox_sq(d[0], d[1], d[2]) : __builtin_inf();
  unsigned qp = have ? s + slot : 0xffffffffu;
  vox_nearest<64>(q, qp);
  double C[6];
  int k = 0;
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = a; b < 3; b++, k++) C[k] = vox_tree<64>(d[a] * d[b]);
  if (lane == 0u) {
    for (int t = 0; t < 6; t++) rc[6 * (size_t)r + t] = C[t];
    rq[r] = q;
    rp[r] = qp;
  }
}
__global__ __launch_bounds__(256) void voxel_run_finish_kernel(VoxView w, const uint32_t* __restrict__ list, unsigned nlist,
                                                               const uint32_t* __restrict__ roff, const double* __restrict__ rc,
                                                               const double* __restrict__ rq, const uint32_t* __restrict__ rp,
                                                               double* __restrict__ cov, int32_t* __restrict__ rep) {
  const unsigned g = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (g >= nlist) return;
  const unsigned v = list[g], s = w.seg[v], c = w.seg[v + 1u] - s, runs = (c + 63u) / 64u, r0 = roff[v];
  double S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double bq = __builtin_inf();
  unsigned bp = 0xffffffffu;
  for (unsigned base = 0; base < runs; base += 64u) {
    const unsigned lim = min(64u, runs - base);
    double x[6];
    for (int a = 0; a < 6; a++) x[a] = lane < lim ? rc[6 * (size_t)(r0 + base + lane) + a] : 0.0;
    double q = lane < lim ? rq[r0 + base + lane] : __builtin_inf();
    unsigned qp = lane < lim ? rp[r0 + base + lane] : 0xffffffffu;
    for (unsigned t = 0; t < lim; t++)
      for (int a = 0; a < 6; a++) S[a] = S[a] + __shfl(x[a], (int)t, 64);
    vox_nearest<64>(q, qp);                                // (positions ascend with the runs: the first of equals stays)
    if (q < bq) { bq = q; bp = qp; }
  }
  const double dc = (double)c;
  if (lane == 0u) {
    for (int a = 0; a < 6; a++) cov[6 * (size_t)v + a] = S[a] / dc;
    rep[v] = (int32_t)w.perm[bp == 0xffffffffu ? s : bp];
  }
}

constexpr int VOXEL_POINT_PER = 8;      // sorted positions a thread of the per-point stage

__global__ __launch_bounds__(256) void voxel_sorted_copy_kernel(const float4* __restrict__ map, const uint32_t* __restrict__ perm, unsigned n,
                                                                float4* __restrict__ out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = map[perm[i]];
}

__global__ __launch_bounds__(256) void voxel_point_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ perm,
                                                          const uint32_t* __restrict__ head, const uint32_t* __restrict__ pos,
                                                          const uint32_t* __restrict__ seg, const int32_t* __restrict__ rep, unsigned n,
                                                          unsigned first, unsigned nr, int keep, unsigned max_pts,
                                                          int32_t* __restrict__ voxel, unsigned char* __restrict__ mask,
                                                          uint32_t* __restrict__ words) {
  // VOXEL_POINT_PER positions a thread, one integer add a workgroup (atomics on one address are slow on this part)
  __shared__ unsigned s_cnt[4];
  unsigned cnt = 0;
#pragma unroll
  for (int r = 0; r < VOXEL_POINT_PER; r++) {
    const size_t i64 = ((size_t)blockIdx.x * VOXEL_POINT_PER + (size_t)r) * 256u + threadIdx.x;
    bool sel = false;
    if (i64 < (size_t)n) {
      const unsigned i = (unsigned)i64;
      const unsigned orig = perm[i];
      const bool in_range = orig >= first && orig - first < nr;
      int32_t v = -1;
      bool go = false;
      if (keys[i] != VOXEL_OUTSIDE) {
        v = (int32_t)(pos[i] + head[i] - 1u);             // (the scan is exclusive: a head holds its voxel, a later member one more)
        go = keep == VOXEL_KEEP_FIRST ? i - seg[v] >= max_pts : (int32_t)orig != rep[v];
      }
      if (in_range) {
        if (voxel) voxel[orig - first] = v;
        if (mask) mask[orig - first] = go ? 1 : 0;
        sel = go;
      }
    }
    cnt += (unsigned)__popcll(__ballot(sel));             // (the wave's: uniform)
  }
  if ((threadIdx.x & 63u) == 0u) s_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0u) {
    const unsigned tot = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    if (tot) atomicAdd(&words[VOXEL_W_SEL], tot);
  }
}

static inline dim3 vox_grid(size_t threads) { return dim3((unsigned)((threads + 255) / 256)); }

hipError_t voxel_tmp_bytes(size_t n, size_t* bytes) {
  size_t a = 0, b = 0;
  hipError_t e = sort_pairs_u64(nullptr, a, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr,
                                (uint32_t*)nullptr, n, hipStream_t(0));
  if (e != hipSuccess) return e;
  e = exclusive_sum(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, n + 1, hipStream_t(0));
  if (e != hipSuccess) return e;
  *bytes = std::max(a, b) + 256;
  return hipSuccess;
}

hipError_t launch_voxel_sort(hipStream_t st, const float4* map_raw, unsigned n, float inv, unsigned long long* keys_in, unsigned long long* keys_out,
                             uint32_t* vals_in, uint32_t* vals_out, uint32_t* head, uint32_t* pos, void* tmp, size_t tmp_bytes, uint32_t* words) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(voxel_key_kernel, vox_grid(n), dim3(256), 0, st, map_raw, n, inv, keys_in, vals_in, words);
  return launch_voxel_sort_keys(st, n, keys_in, keys_out, vals_in, vals_out, head, pos, tmp, tmp_bytes);
}
hipError_t launch_voxel_sort_keys(hipStream_t st, unsigned n, unsigned long long* keys_in, unsigned long long* keys_out, uint32_t* vals_in,
                                  uint32_t* vals_out, uint32_t* head, uint32_t* pos, void* tmp, size_t tmp_bytes) {
  if (n == 0) return hipSuccess;
  size_t bytes = tmp_bytes;
  hipError_t e = sort_pairs_u64(tmp, bytes, keys_in, keys_out, vals_in, vals_out, n, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(voxel_head_kernel, vox_grid(n), dim3(256), 0, st, keys_out, n, head);
  bytes = tmp_bytes;
  e = exclusive_sum(tmp, bytes, head, pos, n, st);
  if (e != hipSuccess) return e;
  return hipGetLastError();
}

hipError_t launch_voxel_classify(hipStream_t st, const unsigned long long* keys, const uint32_t* perm, const uint32_t* head, const uint32_t* pos,
                                 unsigned n, unsigned nv, unsigned inside, int plan, uint32_t* seg, int32_t* ijk, int32_t* first, int32_t* count,
                                 uint32_t* runs, uint32_t* roff, uint32_t* lists, void* tmp, size_t tmp_bytes, uint32_t* words) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(voxel_segment_kernel, vox_grid(n), dim3(256), 0, st, keys, perm, head, pos, n, nv, inside, seg, ijk, first);
  hipLaunchKernelGGL(voxel_classify_kernel, vox_grid((size_t)nv + 1), dim3(256), 0, st, seg, nv, plan & 7, count, runs, lists, words);
  if (lists) {
    size_t bytes = tmp_bytes;
    const hipError_t e = exclusive_sum(tmp, bytes, runs, roff, (size_t)nv + 1, st);
    if (e != hipSuccess) return e;
  }
  return hipGetLastError();
}

hipError_t launch_voxel_sorted_copy(hipStream_t st, const float4* map_raw, const uint32_t* perm, unsigned n, float4* out) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(voxel_sorted_copy_kernel, vox_grid(n), dim3(256), 0, st, map_raw, perm, n, out);
  return hipGetLastError();
}

hipError_t launch_voxel_moments(hipStream_t st, const float4* pts, const uint32_t* gather, const uint32_t* perm, const uint32_t* seg, unsigned nv,
                                const uint32_t* lists, const unsigned nlist[4], const uint32_t* roff, unsigned R, int second, double* rs,
                                double* rc, double* rq, uint32_t* rp, double* centroid, double* cov, int32_t* rep) {
  const VoxView w{pts, gather, perm, seg};
  if (nlist[0])
    hipLaunchKernelGGL(voxel_group_kernel<8>, vox_grid((size_t)nlist[0] * 8), dim3(256), 0, st, w, lists, nlist[0], second, centroid, cov, rep);
  if (nlist[1])
    hipLaunchKernelGGL(voxel_group_kernel<16>, vox_grid((size_t)nlist[1] * 16), dim3(256), 0, st, w, lists + (size_t)nv, nlist[1], second, centroid,
                       cov, rep);
  if (nlist[2])
    hipLaunchKernelGGL(voxel_group_kernel<64>, vox_grid((size_t)nlist[2] * 64), dim3(256), 0, st, w, lists + 2 * (size_t)nv, nlist[2], second,
                       centroid, cov, rep);
  if (nlist[3]) {
    const uint32_t* list = lists + 3 * (size_t)nv;
    hipLaunchKernelGGL(voxel_run_sum_kernel, dim3((R + 3u) / 4u), dim3(256), 0, st, w, roff, nv, R, rs);
    hipLaunchKernelGGL(voxel_run_centroid_kernel, dim3((nlist[3] + 3u) / 4u), dim3(256), 0, st, w, list, nlist[3], roff, rs, centroid);
    if (second) {
      hipLaunchKernelGGL(voxel_run_cov_kernel, dim3((R + 3u) / 4u), dim3(256), 0, st, w, roff, nv, R, centroid, rc, rq, rp);
      hipLaunchKernelGGL(voxel_run_finish_kernel, dim3((nlist[3] + 3u) / 4u), dim3(256), 0, st, w, list, nlist[3], roff, rc, rq, rp, cov, rep);
    }
  }
  return hipGetLastError();
}

hipError_t launch_voxel_points(hipStream_t st, const unsigned long long* keys, const uint32_t* perm, const uint32_t* head, const uint32_t* pos,
                               const uint32_t* seg, const int32_t* rep, unsigned n, unsigned first, unsigned nr, int keep, unsigned max_pts,
                               int32_t* voxel, unsigned char* mask, uint32_t* words) {
  if (n == 0 || nr == 0) return hipSuccess;
  hipLaunchKernelGGL(voxel_point_kernel, vox_grid(((size_t)n + VOXEL_POINT_PER - 1) / VOXEL_POINT_PER), dim3(256), 0, st, keys, perm, head, pos, seg, rep, n, first, nr, keep, max_pts, voxel, mask,
                     words);
  return hipGetLastError();
}

}  // namespace flimo
