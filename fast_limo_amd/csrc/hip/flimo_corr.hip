// fast_limo_amd/csrc/hip/flimo_corr.hip -- pose hypotheses from point correspondences (flimo_corr_poses, include/flimo_c.h): what
// pcl::SampleConsensusPrerejective does per sample, for a chunk of the caller's samples at once; and, further down, the consistency
// graph of the correspondences with its core numbers (flimo_corr_graph).
//
//   corr_solve_kernel  one THREAD per hypothesis: the six points of its triplet, corr_solve (flimo_corr.h: edge tests, TRIAD,
//                      Shepperd, the float32 matrix), its status and pose7.  A hypothesis that is not OK gets its final answers
//                      here (inliers 0, sum +0.0); an OK one gets its 12 matrix floats, by hypothesis index, and an entry of the
//                      survivor list (an integer append: the list's order is free, every result is written by hypothesis index).
//   corr_count_kernel  the hot path: one workgroup of CORR_RED threads per CORR_G survivors.  A thread loads src[i] and dst[i] once
//                      per slot i = t, t + CORR_RED, ... and evaluates the pair against all CORR_G matrices (uniform over the
//                      workgroup): transform_kernel's c0*x + (c1*y + (c2*z + c3)), sqdist3, the strict float32 gate -- what
//                      flimo_scan_fitness would see.  Per pose a float64 partial and a count per thread, then fit_reduce_kernel's
//                      tree over the CORR_RED partials in shared memory (partial[t] += partial[t + o], o = 128 .. 1), all CORR_G
//                      trees between the same barriers.  No atomics on floating-point values: the bits of a hypothesis's sum
//                      depend on the two clouds, its matrix and the gate alone -- not on which survivors share its workgroup.
//   corr_fill_kernel   pair_sqd asked for: -1 in every slot of the chunk before the count writes the survivors' rows.
#include <algorithm>
#include "flimo_corr.h"
#include "flimo_kernels.h"
#include "flimo_math.h"

namespace flimo {

constexpr int CORR_RED = 256;      // threads of a count workgroup: the sum's shape (fit_reduce_kernel's FIT_RED)
#ifndef FLIMO_CORR_G      // (the variants of the profile's table are built with -DFLIMO_CORR_G=..)
#define FLIMO_CORR_G 4
#endif
constexpr int CORR_G = FLIMO_CORR_G;      // survivors per count workgroup: the group sizes measured are in profiles/corr_poses/README.md

__global__ __launch_bounds__(256) void corr_solve_kernel(const float* __restrict__ src, const float* __restrict__ dst,
                                                         const int32_t* __restrict__ tri, unsigned nh, float edge_sim, float min_edge,
                                                         int32_t* __restrict__ status, double* __restrict__ pose, float* __restrict__ rt,
                                                         int32_t* __restrict__ surv, unsigned* __restrict__ nsurv,
                                                         int32_t* __restrict__ inliers, double* __restrict__ sum_sqd) {
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nh) return;
  const int32_t a = tri[3 * (size_t)j], b = tri[3 * (size_t)j + 1], c = tri[3 * (size_t)j + 2];      // (the host checked: all in [0, m))
  float s3[9], d3[9];
  const int32_t id[3] = {a, b, c};
  for (int v = 0; v < 3; v++)
    for (int t = 0; t < 3; t++) { s3[3 * v + t] = src[3 * (size_t)id[v] + t]; d3[3 * v + t] = dst[3 * (size_t)id[v] + t]; }
  double p7[7];
  float m12[12];
  int st = corr_solve(s3, d3, edge_sim, min_edge, p7, m12);
  if (a == b || b == c || a == c) {      // (a repeated index: zero edges pass a min_edge of 0)
    st = CORR_DEGENERATE;
    for (int t = 0; t < 7; t++) p7[t] = __builtin_nan("");
  }
  status[j] = st;
  for (int t = 0; t < 7; t++) pose[7 * (size_t)j + t] = p7[t];
  if (st == CORR_OK) {
    for (int t = 0; t < 12; t++) rt[12 * (size_t)j + t] = m12[t];
    surv[atomicAdd(nsurv, 1u)] = (int32_t)j;
  } else {
    inliers[j] = 0;
    sum_sqd[j] = 0.0;
  }
}

__global__ __launch_bounds__(256) void corr_fill_kernel(float* __restrict__ p, size_t n, float v) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

template <int G, bool PAIRS>      // PAIRS: pair_sqd is asked for (its stores stay out of the loop of the call that does not)
__global__ __launch_bounds__(CORR_RED) void corr_count_kernel(const float* __restrict__ src, const float* __restrict__ dst, unsigned m,
                                                              const float* __restrict__ rt, const int32_t* __restrict__ surv,
                                                              const unsigned* __restrict__ nsurv, float gate2,
                                                              int32_t* __restrict__ inliers, double* __restrict__ sum_sqd,
                                                              float* __restrict__ pair_sqd) {
  __shared__ double s_sum[G][CORR_RED];
  __shared__ int s_cnt[G][CORR_RED];
  const unsigned ns = *nsurv;
  const unsigned g0 = blockIdx.x * (unsigned)G;
  if (g0 >= ns) return;                                   // (the grid covers the chunk as if every hypothesis survived)
  const unsigned ng = min((unsigned)G, ns - g0);           // survivors of this workgroup; the slots beyond repeat the last one
  unsigned hyp[G];
  float M[G][12];
#pragma unroll
  for (int g = 0; g < G; g++) {
    hyp[g] = (unsigned)surv[g0 + min((unsigned)g, ng - 1u)];
#pragma unroll
    for (int t = 0; t < 12; t++) M[g][t] = rt[12 * (size_t)hyp[g] + t];
  }
  double acc[G];
  int cnt[G];
#pragma unroll
  for (int g = 0; g < G; g++) { acc[g] = 0.0; cnt[g] = 0; }
  for (unsigned i = threadIdx.x; i < m; i += CORR_RED) {
    const float px = src[3 * (size_t)i], py = src[3 * (size_t)i + 1], pz = src[3 * (size_t)i + 2];
    const float qx = dst[3 * (size_t)i], qy = dst[3 * (size_t)i + 1], qz = dst[3 * (size_t)i + 2];
#pragma unroll
    for (int g = 0; g < G; g++) {
      const float wx = M[g][0] * px + (M[g][1] * py + (M[g][2] * pz + M[g][3]));
      const float wy = M[g][4] * px + (M[g][5] * py + (M[g][6] * pz + M[g][7]));
      const float wz = M[g][8] * px + (M[g][9] * py + (M[g][10] * pz + M[g][11]));
      const float v = sqdist3(wx, wy, wz, qx, qy, qz);
      const bool in = v < gate2;                          // (false for a NaN)
      if (in) { acc[g] = acc[g] + (double)v; cnt[g]++; }
      if (PAIRS && (unsigned)g < ng) pair_sqd[(size_t)hyp[g] * (size_t)m + i] = in ? v : -1.f;
    }
  }
#pragma unroll
  for (int g = 0; g < G; g++) { s_sum[g][threadIdx.x] = acc[g]; s_cnt[g][threadIdx.x] = cnt[g]; }
  __syncthreads();
  for (int o = CORR_RED / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int g = 0; g < G; g++) {
        s_sum[g][threadIdx.x] = s_sum[g][threadIdx.x] + s_sum[g][threadIdx.x + o];
        s_cnt[g][threadIdx.x] += s_cnt[g][threadIdx.x + o];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x < ng) {
    const unsigned h = (unsigned)surv[g0 + threadIdx.x];
    inliers[h] = s_cnt[threadIdx.x][0];
    sum_sqd[h] = s_sum[threadIdx.x][0];
  }
}

hipError_t launch_corr_poses(hipStream_t st, const float* src, const float* dst, unsigned m, const int32_t* tri, unsigned nh, float edge_sim,
                             float min_edge, float max_dist, int32_t* status, double* pose, float* rt, int32_t* surv, unsigned* nsurv,
                             int32_t* inliers, double* sum_sqd, float* pair_sqd) {
  if (nh == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(nsurv, 0, sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(corr_solve_kernel, dim3((nh + 255u) / 256u), dim3(256), 0, st, src, dst, tri, nh, edge_sim, min_edge, status, pose, rt, surv,
                     nsurv, inliers, sum_sqd);
  if (pair_sqd) {
    const size_t n = (size_t)nh * (size_t)m;
    hipLaunchKernelGGL(corr_fill_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 65536)), dim3(256), 0, st, pair_sqd, n, -1.f);
  }
  const float gate2 = max_dist * max_dist;      // one float32 product, as the searches form theirs
  const dim3 grid((nh + CORR_G - 1u) / CORR_G);
  if (pair_sqd)
    hipLaunchKernelGGL((corr_count_kernel<CORR_G, true>), grid, dim3(CORR_RED), 0, st, src, dst, m, rt, surv, nsurv, gate2, inliers, sum_sqd, pair_sqd);
  else
    hipLaunchKernelGGL((corr_count_kernel<CORR_G, false>), grid, dim3(CORR_RED), 0, st, src, dst, m, rt, surv, nsurv, gate2, inliers, sum_sqd, pair_sqd);
  return hipGetLastError();
}

// ---- the consistency graph of the correspondences and its core numbers (flimo_corr_graph, include/flimo_c.h) ----------------------
//   corr_adj_kernel     one launch per call: a workgroup of CG_WAVES waves takes CG_TILE rows i and CG_WAVES words of their bit rows.
//                       A LANE owns a column j and keeps its two points widened in registers; the tile's rows come in uniformly
//                       from shared memory; __ballot of corr_compatible (flimo_corr.h) IS the word of row i.  Lane l keeps the
//                       ballot of the tile's l-th row, and the wave stores its 64 words at the end, one store a word.  The whole
//                       square is computed: the predicate is symmetric bit for bit, so the two triangles agree.
//   corr_degree_kernel  one wave per row: the popcount of its words, to degree and to the first core estimate.
//   corr_core_kernel    one round of the synchronous h-index iteration (Lu, Zhou, Zhang, Stanley 2016: it starts at the degrees and
//                       ends at the core numbers), one wave per vertex v: the largest t <= c(v) with at least t neighbours u of
//                       c(u) >= t.  A scan of the row answers eight thresholds at once, c(v) itself among them -- the common
//                       case ends there --, and the search narrows 9-fold per scan (the count falls as t rises, so the
//                       thresholds that hold are a prefix).  A scan: the lanes load 64 words, the words that hold a bit are
//                       broadcast four at a time, and lane l gathers c of bit l of each.  Integers only; a changed estimate ORs
//                       into the round's flag word.
constexpr int CG_TILE = 64;       // rows of an adjacency tile: one per lane, so that a lane can keep a row's word
constexpr int CG_WAVES = 4;       // waves of a workgroup: adjacent words of the same rows (32 B of every row a workgroup)

__global__ __launch_bounds__(64 * CG_WAVES) void corr_adj_kernel(const float* __restrict__ src, const float* __restrict__ dst, unsigned m,
                                                                 unsigned W, double min2, double tol, double s2,
                                                                 uint64_t* __restrict__ adj) {
  __shared__ double s_row[CG_TILE][6];      // src xyz, dst xyz of the tile's rows (the rows beyond m repeat the last one: never stored)
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned r0 = blockIdx.y * (unsigned)CG_TILE;
  for (unsigned t = threadIdx.x; t < (unsigned)CG_TILE * 6u; t += 64u * CG_WAVES) {
    const unsigned row = t / 6u, k = t % 6u;
    const unsigned i = min(r0 + row, m - 1u);
    s_row[row][k] = (double)(k < 3u ? src[3 * (size_t)i + k] : dst[3 * (size_t)i + (k - 3u)]);
  }
  __syncthreads();
  const unsigned w = blockIdx.x * (unsigned)CG_WAVES + wave;
  if (w >= W) return;      // (whole waves, behind the only barrier)
  const unsigned j = 64u * w + lane;
  const unsigned jc = min(j, m - 1u);      // (a padding column: loaded from the last point, never set)
  const double sj[3] = {(double)src[3 * (size_t)jc], (double)src[3 * (size_t)jc + 1], (double)src[3 * (size_t)jc + 2]};
  const double dj[3] = {(double)dst[3 * (size_t)jc], (double)dst[3 * (size_t)jc + 1], (double)dst[3 * (size_t)jc + 2]};
  unsigned long long mine = 0ull;
  for (unsigned t = 0; t < (unsigned)CG_TILE; t++) {
    const bool e = j < m && r0 + t != j && corr_compatible(&s_row[t][0], sj, &s_row[t][3], dj, min2, tol, s2);
    const unsigned long long word = __ballot(e);
    if (lane == t) mine = word;
  }
  const unsigned i = r0 + lane;
  if (i < m) adj[(size_t)i * W + w] = mine;
}

__global__ __launch_bounds__(256) void corr_degree_kernel(const uint64_t* __restrict__ adj, unsigned m, unsigned W, int32_t* __restrict__ degree,
                                                          int32_t* __restrict__ c0) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned v = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (v >= m) return;
  int cnt = 0;
  for (unsigned w = lane; w < W; w += 64u) cnt += __popcll(adj[(size_t)v * W + w]);
  for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) { degree[v] = cnt; c0[v] = cnt; }
}

// One scan of a row: the neighbours u with c[u] >= t[i], for CG_T thresholds at once (the same CG_T numbers in every lane).  The
// lanes load 64 words; the words that hold a bit are handed round CG_U at a time (a ballot finds them, a shuffle broadcasts them),
// lane l gathers c of bit l of each -- CG_U independent loads of 64 adjacent integers in flight -- and counts in its own registers;
// one shuffle tree per threshold ends the scan.  The thresholds are >= 1: a lane without a bit counts with c = -1.
constexpr int CG_T = 8;       // thresholds a scan answers: the search for the h-index is 9-ary
constexpr int CG_U = 4;       // words in flight
__device__ inline void corr_scan_row(const uint64_t* __restrict__ row, unsigned W, const int32_t* __restrict__ c, unsigned lane,
                                     const int t[CG_T], int n[CG_T]) {
#pragma unroll
  for (int i = 0; i < CG_T; i++) n[i] = 0;
  for (unsigned base = 0; base < W; base += 64u) {
    const unsigned long long mine = base + lane < W ? row[base + lane] : 0ull;
    unsigned long long some = __ballot(mine != 0ull);
    while (some) {
      int cu[CG_U];
#pragma unroll
      for (int q = 0; q < CG_U; q++) {
        const int k = some ? __ffsll(some) - 1 : 0;
        const unsigned long long word = some ? __shfl(mine, k) : 0ull;      // (the list ran out: no bit, no load)
        some &= some - 1ull;
        // (the padding bits are 0: a set bit is a vertex below m)
        cu[q] = ((word >> lane) & 1ull) ? c[64u * (base + (unsigned)k) + lane] : -1;
      }
#pragma unroll
      for (int q = 0; q < CG_U; q++)
#pragma unroll
        for (int i = 0; i < CG_T; i++) n[i] += cu[q] >= t[i] ? 1 : 0;
    }
  }
#pragma unroll
  for (int i = 0; i < CG_T; i++)
    for (int o = 32; o >= 1; o >>= 1) n[i] += __shfl_xor(n[i], o);
}

__global__ __launch_bounds__(256) void corr_core_kernel(const uint64_t* __restrict__ adj, unsigned m, unsigned W, const int32_t* __restrict__ c_in,
                                                        int32_t* __restrict__ c_out, unsigned* __restrict__ changed) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned v = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (v >= m) return;
  const uint64_t* row = adj + (size_t)v * W;
  const int cv = c_in[v];
  // the largest t in [0, cv] with at least t neighbours of c >= t: t = lo holds, the candidates left are lo + 1 .. hi.  A scan
  // tries up to CG_T of them, evenly spaced and hi among them; those that hold are a prefix (the count falls as t rises).
  int lo = 0, hi = cv;
  while (lo < hi) {
    const int step = (hi - lo + CG_T - 1) / CG_T;
    int t[CG_T], n[CG_T];
#pragma unroll
    for (int i = 0; i < CG_T; i++) t[i] = min(lo + (i + 1) * step, hi);
    corr_scan_row(row, W, c_in, lane, t, n);
    bool open = true;
#pragma unroll
    for (int i = 0; i < CG_T; i++) {
      if (!open) continue;
      if (n[i] >= t[i]) lo = t[i];      // (all eight hold: lo = hi -- in the first scan that is c(v) itself, the common case)
      else { hi = t[i] - 1; open = false; }
    }
  }
  if (lane == 0) {
    c_out[v] = lo;
    if (lo != cv) atomicOr(changed, 1u);
  }
}

hipError_t launch_corr_adjacency(hipStream_t st, const float* src, const float* dst, unsigned m, float tol, float min_edge, float edge_sim,
                                 uint64_t* adj, int32_t* degree, int32_t* c0) {
  if (m == 0) return hipSuccess;
  const unsigned W = (m + 63u) / 64u;
  const double min2 = (double)min_edge * (double)min_edge, s2 = (double)edge_sim * (double)edge_sim;
  hipLaunchKernelGGL(corr_adj_kernel, dim3((W + CG_WAVES - 1u) / CG_WAVES, (m + CG_TILE - 1u) / CG_TILE), dim3(64 * CG_WAVES), 0, st, src, dst, m, W,
                     min2, (double)tol, s2, adj);
  hipLaunchKernelGGL(corr_degree_kernel, dim3((m + 3u) / 4u), dim3(256), 0, st, adj, m, W, degree, c0);
  return hipGetLastError();
}

hipError_t launch_corr_core_rounds(hipStream_t st, const uint64_t* adj, unsigned m, int32_t* c[2], int* cur, unsigned* flags, int rounds) {
  if (m == 0) return hipSuccess;
  const unsigned W = (m + 63u) / 64u;
  hipError_t e = hipMemsetAsync(flags, 0, (size_t)rounds * sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  for (int r = 0; r < rounds; r++) {
    hipLaunchKernelGGL(corr_core_kernel, dim3((m + 3u) / 4u), dim3(256), 0, st, adj, m, W, c[*cur], c[*cur ^ 1], flags + r);
    *cur ^= 1;
  }
  return hipGetLastError();
}

}  // namespace flimo
