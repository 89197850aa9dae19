// fast_limo_amd/csrc/hip/flimo_sums.h -- the one fixed shape of the two-level float64 sums behind flimo_scan_linearize,
// flimo_scan_ndt and flimo_map_outliers.  The bits of such a sum depend on the terms and on the number of slots alone -- not on the
// batch, the chunk or the cell size --, so the shape is part of the ABI (include/flimo_c.h) and tests/sums_common.py restates it:
//   level 1  the n slots of a row (a pose; the one range of the outliers) are cut into segments of SUM_SEG; one workgroup of SUM_RED
//            threads per (segment, row): thread t adds the terms of slots t, t + SUM_RED, .. of its segment in ascending order onto
//            +0.0, a slot's own terms in the order its kernel states (a slot without a term adds +0.0) -- that loop is the kernel's
//            own; sum_tail ends it: an xor butterfly over the 64 lanes of each wave, then ((wave 0 + wave 1) + (wave 2 + wave 3))
//   level 2  sum_final_kernel: one thread per (row, number) adds the row's segment partials in ascending order of the segment onto +0.0
// N float64 numbers and C integer counts per row travel together.  No atomics on floating-point values; every addition is written
// a = a + b and nothing here is contracted.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace flimo {

constexpr int SUM_RED = 256;       // threads of a level-1 workgroup
constexpr int SUM_SEG = 4096;      // slots of a segment: 16 per thread
inline unsigned sum_segments(size_t n) { return (unsigned)((n + SUM_SEG - 1) / SUM_SEG); }

// the end of a level-1 workgroup (all SUM_RED threads call it): part [rows * nseg][N], part_cnt [rows * nseg][C]
template <int N, int C>
__device__ __forceinline__ void sum_tail(double (&acc)[N], int (&cnt)[C], unsigned row, unsigned nseg, unsigned seg, double* __restrict__ part,
                                         int32_t* __restrict__ part_cnt) {
  __shared__ double s_sum[SUM_RED / 64][N];
  __shared__ int s_cnt[SUM_RED / 64][C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < N; t++) {
    double v = acc[t];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = v + __shfl_xor(v, o, 64);
    acc[t] = v;
  }
#pragma unroll
  for (int t = 0; t < C; t++)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) cnt[t] += __shfl_xor(cnt[t], o, 64);
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < N; t++) s_sum[wave][t] = acc[t];
#pragma unroll
    for (int t = 0; t < C; t++) s_cnt[wave][t] = cnt[t];
  }
  __syncthreads();
  const size_t slot = (size_t)row * (size_t)nseg + seg;
  const unsigned t = threadIdx.x;
  if (t < (unsigned)N) part[slot * N + t] = (s_sum[0][t] + s_sum[1][t]) + (s_sum[2][t] + s_sum[3][t]);
  if (t < (unsigned)C) part_cnt[slot * C + t] = (s_cnt[0][t] + s_cnt[1][t]) + (s_cnt[2][t] + s_cnt[3][t]);
}

// level 2: sums [rows][N], counts [rows][C].  The threads of the counts start on a wave of their own (sum_count_base): no wave
// walks the segments twice, once per kind.
inline __host__ __device__ size_t sum_count_base(unsigned rows, int N) { return ((size_t)rows * N + 63) / 64 * 64; }
template <int N, int C>
__global__ __launch_bounds__(SUM_RED) void sum_final_kernel(const double* __restrict__ part, const int32_t* __restrict__ part_cnt, unsigned rows,
                                                            unsigned nseg, double* __restrict__ sums, long long* __restrict__ counts) {
  const size_t g = (size_t)blockIdx.x * SUM_RED + threadIdx.x, base = sum_count_base(rows, N);
  if (g < (size_t)rows * N) {
    const size_t row = g / N, t = g % N;
    double v = 0.0;
    for (unsigned s = 0; s < nseg; s++) v = v + part[(row * nseg + s) * N + t];
    sums[g] = v;
  } else if (g >= base && g - base < (size_t)rows * C) {
    const size_t row = (g - base) / C, t = (g - base) % C;
    long long c = 0;
    for (unsigned s = 0; s < nseg; s++) c += part_cnt[(row * nseg + s) * C + t];
    counts[g - base] = c;
  }
}
template <int N, int C>
inline void launch_sum_final(hipStream_t st, const double* part, const int32_t* part_cnt, unsigned rows, unsigned nseg, double* sums, long long* counts) {
  const size_t threads = sum_count_base(rows, N) + (size_t)rows * C;
  hipLaunchKernelGGL((sum_final_kernel<N, C>), dim3((unsigned)((threads + SUM_RED - 1) / SUM_RED)), dim3(SUM_RED), 0, st, part, part_cnt, rows, nseg,
                     sums, counts);
}

}  // namespace flimo
