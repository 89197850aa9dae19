// fast_limo_amd/csrc/hip/flimo_plane.hip -- RANSAC planes of the stored points (flimo_map_planes, include/flimo_c.h): what
// pcl::SACSegmentation(SACMODEL_PLANE / PERPENDICULAR_PLANE, RANSAC) does per sample, for a chunk of the caller's samples at once
// against EVERY stored point; and the mask of one plane (flimo_map_plane_mask, flimo_map_remove_plane).
//
//   plane_solve_kernel   one THREAD per hypothesis: the three points of its triplet, plane_solve (flimo_plane.h), its status and
//                        plane.  A hypothesis that is not OK gets its final answers here (inliers 0, sum +0.0); an OK one gets its
//                        32-byte record {nf, p_a}, by hypothesis index, and an entry of the survivor list (an integer append: the
//                        list's order is free, every result is written by hypothesis index).
//   plane_count_kernel   the hot path: grid (slabs, survivor groups), PLANE_RED threads.  A thread owns the slab's slots T,
//                        T + 256, ...: 32 float4 loads from the stored points, issued together, and the points stay in registers
//                        for every hypothesis the workgroup walks (PLANE_W groups of PLANE_G).  The records are uniform over the
//                        workgroup.  Per hypothesis a thread adds its slots in ascending order into a float64 partial; then
//                        fit_reduce_kernel's tree over the 256 partials in shared memory (partial[t] += partial[t + o],
//                        o = 128 .. 1), the PLANE_G trees between the same barriers.  The count is an integer and takes the
//                        short way: a ballot and a popcount per slot and wave, the four waves' counts added at the end.  One
//                        (int32, double) per (hypothesis, slab).
//                        No atomics on floating-point values: the bits depend on the stored points, the record and the gate
//                        alone -- not on which survivors share the workgroup.
//   plane_finish_kernel  one THREAD per hypothesis of the chunk: the integer sum and the ascending float64 sum over its slabs.
//   plane_mask_kernel    one THREAD per point of the range: the mask byte; the count by one ballot and one integer add per wave.
#include <algorithm>
#include "flimo_plane.h"
#include "flimo_kernels.h"

namespace flimo {

#ifndef FLIMO_PLANE_G      // (the variants of the profile's table are built with -DFLIMO_PLANE_G=.. -DFLIMO_PLANE_W=..)
#define FLIMO_PLANE_G 16
#endif
#ifndef FLIMO_PLANE_W
#define FLIMO_PLANE_W 1
#endif
constexpr int PLANE_G = FLIMO_PLANE_G;      // survivors whose trees share the barriers: the sizes measured are in profiles/planes/README.md
constexpr int PLANE_W = FLIMO_PLANE_W;      // groups a workgroup walks with one load of its slab
constexpr int PLANE_PER = PLANE_SLAB / PLANE_RED;      // slots of a thread: 32
static_assert(PLANE_RED == 256 && PLANE_SLAB % PLANE_RED == 0 && PLANE_G >= 1 && PLANE_G <= PLANE_RED && PLANE_W >= 1, "plane count shape");

__global__ __launch_bounds__(256) void plane_solve_kernel(const float4* __restrict__ map, const int32_t* __restrict__ tri, unsigned nh,
                                                          float min_edge, float min_sin, float ax, float ay, float az, float min_cos,
                                                          int32_t* __restrict__ status, double* __restrict__ plane, float4* __restrict__ rec,
                                                          int32_t* __restrict__ surv, unsigned* __restrict__ nsurv,
                                                          int32_t* __restrict__ inliers, double* __restrict__ sum_sq) {
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nh) return;
  const int32_t a = tri[3 * (size_t)j], b = tri[3 * (size_t)j + 1], c = tri[3 * (size_t)j + 2];      // (the host checked: all in [0, N))
  const float4 pa = map[a], pb = map[b], pc = map[c];
  const float p3[9] = {pa.x, pa.y, pa.z, pb.x, pb.y, pb.z, pc.x, pc.y, pc.z};
  const float axis[3] = {ax, ay, az};
  double p4[4];
  float nf[3];
  int st = plane_solve(p3, min_edge, min_sin, axis, min_cos, p4, nf);
  if (a == b || b == c || a == c) {      // (a repeated index is degenerate whatever the points)
    st = PLANE_DEGENERATE;
    for (int t = 0; t < 4; t++) p4[t] = __builtin_nan("");
  }
  status[j] = st;
  for (int t = 0; t < 4; t++) plane[4 * (size_t)j + t] = p4[t];
  if (st == PLANE_OK) {
    rec[2 * (size_t)j] = make_float4(nf[0], nf[1], nf[2], 0.f);
    rec[2 * (size_t)j + 1] = make_float4(pa.x, pa.y, pa.z, 0.f);
    surv[atomicAdd(nsurv, 1u)] = (int32_t)j;
  } else {
    inliers[j] = 0;
    sum_sq[j] = 0.0;
  }
}

// part_cnt / part_sum: [slabs][k] -- slab-major, so that the finish reads adjacent words from adjacent threads
template <int G, int W>
__global__ __launch_bounds__(PLANE_RED) void plane_count_kernel(const float4* __restrict__ map, unsigned N, const float4* __restrict__ rec,
                                                                const int32_t* __restrict__ surv, const unsigned* __restrict__ nsurv,
                                                                float dist, unsigned k, int32_t* __restrict__ part_cnt,
                                                                double* __restrict__ part_sum) {
  __shared__ double s_sum[G][PLANE_RED];
  __shared__ int s_cnt[G][PLANE_RED / 64];      // per wave: a count is an integer, any order of its additions gives it
  const unsigned ns = *nsurv;
  const unsigned w0 = blockIdx.y * (unsigned)(G * W);
  if (w0 >= ns) return;                                   // (the grid covers the chunk as if every hypothesis survived)
  const unsigned slab = blockIdx.x;
  const unsigned base = slab * (unsigned)PLANE_SLAB + threadIdx.x;      // (N < 2^31: no wrap)
  // the thread's slots: slot r is point base + 256 r; one beyond the map's end reads the last point and becomes NaN (never inside)
  float px[PLANE_PER], py[PLANE_PER], pz[PLANE_PER];
#pragma unroll
  for (int r = 0; r < PLANE_PER; r++) {
    const unsigned i = base + (unsigned)(r * PLANE_RED);
    const float4 p = map[min(i, N - 1u)];
    const bool have = i < N;
    px[r] = have ? p.x : __builtin_nanf("");
    py[r] = p.y;
    pz[r] = p.z;
  }
  for (int w = 0; w < W; w++) {
    const unsigned g0 = w0 + (unsigned)(w * G);
    if (g0 >= ns) break;                                  // (uniform: ns and g0 are the workgroup's)
    const unsigned ng = min((unsigned)G, ns - g0);         // survivors of this group; the slots beyond repeat the last one
#pragma unroll
    for (int g = 0; g < G; g++) {
      const unsigned h = (unsigned)surv[g0 + min((unsigned)g, ng - 1u)];
      const float4 nf = rec[2 * (size_t)h], pa = rec[2 * (size_t)h + 1];
      double acc = 0.0;
      int cnt = 0;
#pragma unroll
      for (int r = 0; r < PLANE_PER; r++) {
        const float t = plane_t(nf.x, nf.y, nf.z, pa.x, pa.y, pa.z, px[r], py[r], pz[r]);
        const bool in = fabsf(t) < dist;                  // (false for a NaN)
        // acc + (double)t * (double)t in ONE instruction: the product of two widened float32 is exact in float64, so the fused
        // form rounds once, to the same bits as the product followed by the add.  A non-inlier adds +0.0 * +0.0, which changes
        // no bit of a partial that starts at +0.0 and is never -0.0.
        const double dt = (double)(in ? t : 0.f);
        acc = __builtin_fma(dt, dt, acc);
        cnt += __popcll(__ballot(in));                    // (the wave's: uniform, on the scalar unit)
      }
      s_sum[g][threadIdx.x] = acc;
      if ((threadIdx.x & 63u) == 0u) s_cnt[g][threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    for (int o = PLANE_RED / 2; o >= 1; o >>= 1) {
      if ((int)threadIdx.x < o) {
#pragma unroll
        for (int g = 0; g < G; g++) s_sum[g][threadIdx.x] = s_sum[g][threadIdx.x] + s_sum[g][threadIdx.x + o];
      }
      __syncthreads();
    }
    if (threadIdx.x < ng) {
      const unsigned h = (unsigned)surv[g0 + threadIdx.x];
      part_cnt[(size_t)slab * k + h] = (s_cnt[threadIdx.x][0] + s_cnt[threadIdx.x][1]) + (s_cnt[threadIdx.x][2] + s_cnt[threadIdx.x][3]);
      part_sum[(size_t)slab * k + h] = s_sum[threadIdx.x][0];
    }
    if (W > 1) __syncthreads();                           // (the next group's partials overwrite slot 0)
  }
}

__global__ __launch_bounds__(256) void plane_finish_kernel(const int32_t* __restrict__ status, unsigned k, unsigned slabs,
                                                           const int32_t* __restrict__ part_cnt, const double* __restrict__ part_sum,
                                                           int32_t* __restrict__ inliers, double* __restrict__ sum_sq) {
  const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k || status[j] != PLANE_OK) return;            // (the others got their answers from the solve)
  int cnt = 0;
  double S = 0.0;
  for (unsigned s = 0; s < slabs; s++) {
    cnt += part_cnt[(size_t)s * k + j];
    S = S + part_sum[(size_t)s * k + j];
  }
  inliers[j] = cnt;
  sum_sq[j] = S;
}

__global__ __launch_bounds__(256) void plane_mask_kernel(const float4* __restrict__ map, unsigned first, unsigned n, float nx, float ny, float nz,
                                                         float ax, float ay, float az, float dist, int side,
                                                         unsigned char* __restrict__ mask, unsigned* __restrict__ count) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  bool in = false;
  if (i < n) {
    const float4 p = map[(size_t)first + i];
    in = plane_side(plane_t(nx, ny, nz, ax, ay, az, p.x, p.y, p.z), dist, side);
    if (mask) mask[i] = in ? 1 : 0;
  }
  const unsigned long long b = __ballot(in);
  if ((threadIdx.x & 63u) == 0u && b) atomicAdd(count, (unsigned)__popcll(b));
}

hipError_t launch_plane_chunk(hipStream_t st, const float4* map_raw, unsigned N, const int32_t* tri, unsigned k, float dist, float min_edge,
                              float min_sin, const float axis[3], float min_cos, int32_t* status, double* plane, int32_t* inliers,
                              double* sum_sq, float4* rec, int32_t* surv, unsigned* nsurv, int32_t* part_cnt, double* part_sum) {
  if (k == 0 || N == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(nsurv, 0, sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(plane_solve_kernel, dim3((k + 255u) / 256u), dim3(256), 0, st, map_raw, tri, k, min_edge, min_sin, axis[0], axis[1], axis[2],
                     min_cos, status, plane, rec, surv, nsurv, inliers, sum_sq);
  const unsigned slabs = plane_slabs(N);
  const unsigned per = (unsigned)(PLANE_G * PLANE_W);
  hipLaunchKernelGGL((plane_count_kernel<PLANE_G, PLANE_W>), dim3(slabs, (k + per - 1u) / per), dim3(PLANE_RED), 0, st, map_raw, N, rec, surv, nsurv,
                     dist, k, part_cnt, part_sum);
  hipLaunchKernelGGL(plane_finish_kernel, dim3((k + 255u) / 256u), dim3(256), 0, st, status, k, slabs, part_cnt, part_sum, inliers, sum_sq);
  return hipGetLastError();
}

hipError_t launch_plane_mask(hipStream_t st, const float4* map_raw, unsigned first, unsigned n, const float normal[3], const float anchor[3],
                             float dist, int side, unsigned char* mask, unsigned* count) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(plane_mask_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, map_raw, first, n, normal[0], normal[1], normal[2], anchor[0],
                     anchor[1], anchor[2], dist, side, mask, count);
  return hipGetLastError();
}

}  // namespace flimo
