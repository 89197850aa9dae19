// fast_limo_amd/csrc/hip/flimo_gicp.hip -- generalized ICP of the resident scan against the stored points (flimo_gicp_build,
// flimo_scan_gicp; include/flimo_c.h): what pcl::GeneralizedIterativeClosestPoint linearises per iteration, for a batch of poses.
//
// The model (behind flimo_map_normals_range's own launches, whose covariances stay on the device):
//   gicp_pack_kernel    one THREAD per stored point of the chunk: gicp_regularize (flimo_gicp.h) of its neighbourhood's covariance
//                       into the model's row, 48 B; a point without a covariance gets six NaN.  The rows that got one are counted
//                       by one integer atomic per wave.
// The passes (per chunk of whole poses, behind flimo_scan_fitness' two search launches -- launch_scan_fit_search):
//   gicp_reduce_kernel  level 1 of the sums in the shape of flimo_sums.h, a row being a pose and a slot a scan point: the slot's
//                       nearest stored point (idx), that point (16 B) and its model row (three 16-byte loads), the scan point's own
//                       row the same way, gicp_term, and its 28 contributions each ONE add onto the thread's accumulators.  The
//                       whole term lives in registers: no pair-sized array but idx, sqd and -- where asked for -- m.
//   sum_final_kernel    level 2 (flimo_sums.h).
// No atomics on floating-point values: the bits depend on the scan, its covariances, the stored points, the model, the pose and
// max_dist alone.
#include "flimo_gicp.h"
#include "flimo_kernels.h"
#include "flimo_sums.h"

#pragma clang fp contract(off)

namespace flimo {

constexpr int GICP_BLOCK = 256;

__global__ __launch_bounds__(GICP_BLOCK) void gicp_pack_kernel(const double* __restrict__ cov, unsigned n, int rule, double eps,
                                                               double* __restrict__ out, unsigned* __restrict__ count) {
  const size_t g = (size_t)blockIdx.x * GICP_BLOCK + threadIdx.x;
  bool has = false;
  if (g < (size_t)n) {
    double c[6], r[6];
#pragma unroll
    for (int t = 0; t < 6; t++) c[t] = cov[6 * g + t];
    has = gicp_regularize(c, rule, eps, r);
#pragma unroll
    for (int t = 0; t < 6; t++) out[6 * g + t] = r[t];
  }
  const unsigned long long b = __ballot(has);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (unsigned)__popcll(b));
}

// a row of six float64 through three 16-byte loads
__device__ __forceinline__ void gicp_load(const double* __restrict__ rows, size_t at, double r[6]) {
  const double2* src = reinterpret_cast<const double2*>(rows + 6 * at);
#pragma unroll
  for (int t = 0; t < 3; t++) { const double2 v = src[t]; r[2 * t] = v.x; r[2 * t + 1] = v.y; }
}

// workgroup (segment, pose) over the slots [seg * SUM_SEG, min(n, (seg + 1) * SUM_SEG)) of its pose
__global__ __launch_bounds__(SUM_RED) void gicp_reduce_kernel(const float4* __restrict__ scan, const float* __restrict__ poses, unsigned n,
                                                              const int32_t* __restrict__ idx, const float4* __restrict__ map_raw,
                                                              const double* __restrict__ model, const double* __restrict__ scan_cov,
                                                              unsigned nseg, double* __restrict__ pair_m, double* __restrict__ part,
                                                              int32_t* __restrict__ part_cnt) {
  const unsigned seg = blockIdx.x, pose = blockIdx.y;
  const size_t base = (size_t)pose * (size_t)n;
  const unsigned end = min(n, (seg + 1u) * (unsigned)SUM_SEG);
  const float* M = poses + 12 * (size_t)pose;
  const float R[9] = {M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10]};
  double acc[GICP_NUM];
#pragma unroll
  for (int t = 0; t < GICP_NUM; t++) acc[t] = 0.0;
  int c[1] = {0};
  for (unsigned i = seg * (unsigned)SUM_SEG + threadIdx.x; i < end; i += SUM_RED) {
    const int32_t at = idx[base + i];
    double out[30];
    bool valid = false;
    if (at >= 0) {
      const float4 p4 = scan[i], b4 = map_raw[at];
      const float p[3] = {p4.x, p4.y, p4.z}, b[3] = {b4.x, b4.y, b4.z};
      const float w[3] = {M[0] * p4.x + (M[1] * p4.y + (M[2] * p4.z + M[3])), M[4] * p4.x + (M[5] * p4.y + (M[6] * p4.z + M[7])),
                          M[8] * p4.x + (M[9] * p4.y + (M[10] * p4.z + M[11]))};      // (transform_kernel's arithmetic)
      double CA[6], CB[6];
      gicp_load(scan_cov, i, CA);
      gicp_load(model, (size_t)at, CB);
      valid = gicp_term(w, b, p, R, CA, CB, out);
    }
#pragma unroll
    for (int t = 0; t < GICP_NUM; t++) acc[t] = acc[t] + (valid ? out[2 + t] : 0.0);
    c[0] += valid ? 1 : 0;
    if (pair_m) pair_m[base + i] = valid ? out[0] : __longlong_as_double(0x7ff8000000000000ll);
  }
  sum_tail(acc, c, pose, nseg, seg, part, part_cnt);
}

hipError_t launch_gicp_pack(hipStream_t st, const double* cov, unsigned n, int rule, double eps, double* out, unsigned* count) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(gicp_pack_kernel, dim3((unsigned)(((size_t)n + GICP_BLOCK - 1) / GICP_BLOCK)), dim3(GICP_BLOCK), 0, st, cov, n, rule, eps, out,
                     count);
  return hipGetLastError();
}

hipError_t launch_scan_gicp(hipStream_t st, const GridView& G, const float4* map_raw, const float4* scan, unsigned n, const float* poses, unsigned np,
                            float max_dist, const double* model, const double* scan_cov, float* sqd, int32_t* idx, uint2* work, unsigned* nwork,
                            double* pair_m, double* part, int32_t* part_cnt, double* sums, long long* valid) {
  if (n == 0 || np == 0) return hipSuccess;
  if ((unsigned long long)n * np > 0x10000000ull || !idx) return hipErrorInvalidValue;
  const hipError_t e = launch_scan_fit_search(st, G, scan, n, poses, np, max_dist, sqd, idx, work, nwork);
  if (e != hipSuccess) return e;
  const unsigned nseg = sum_segments(n);
  hipLaunchKernelGGL(gicp_reduce_kernel, dim3(nseg, np), dim3(SUM_RED), 0, st, scan, poses, n, idx, map_raw, model, scan_cov, nseg, pair_m, part,
                     part_cnt);
  launch_sum_final<GICP_NUM, 1>(st, part, part_cnt, np, nseg, sums, valid);
  return hipGetLastError();
}

}  // namespace flimo
