// fast_limo_amd/csrc/hip/flimo_corr.hip -- pose hypotheses from point correspondences (flimo_corr_poses, include/flimo_c.h): what
// pcl::SampleConsensusPrerejective does per sample, for a chunk of the caller's samples at once.
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

}  // namespace flimo
