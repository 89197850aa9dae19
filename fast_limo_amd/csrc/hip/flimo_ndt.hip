// fast_limo_amd/csrc/hip/flimo_ndt.hip -- the normal distributions transform of the resident scan against a resident cell model
// (flimo_ndt_build, flimo_scan_ndt; include/flimo_c.h): what pcl::NormalDistributionsTransform computes per iteration, without its
// indefinite Hessian terms, for a batch of poses.
//
// The model (behind flimo_map_voxels' own key, sort and moments launches, whose arrays stay on the device):
//   ndt_cell_kernel     one THREAD per voxel: kk_eigen3 (flimo_jacobi.h, the routine of kk_plane) on the voxel's cov where its count
//                       reaches min_pts; flag = count >= min_pts && l2 > 0.  (an exclusive scan of the flags numbers the cells)
//   ndt_pack_kernel     one THREAD per voxel: a cell writes its key, count, eigenvalues and the 128-byte record at its number --
//                       ascending key, because the voxels are.
// The passes (per chunk of whole poses):
//   ndt_lookup_kernel   stage 1, one THREAD per (pair, neighbour slot): the float32 world point, its voxel (voxel_key), the slot's
//                       key, a binary search of the model's keys, m (ndt_m) and e = exp(-0.5 * d2 * m): 12 B a slot (20 B with m).
//   ndt_reduce_kernel   stage 2 and level 1 of the sums in the shape of flimo_sums.h, a row being a pose and a slot a scan point:
//                       inside a slot the neighbour slots ascend; a live term reloads its record (L2-resident: stage 1 just read
//                       it) and ndt_term adds the 28 contributions onto the thread's accumulators, its exp being stage 1's stored
//                       e.  Two counts travel with the sums: the pairs with a live term and the live terms.
//   sum_final_kernel    level 2 (flimo_sums.h).
// No atomics on floating-point values: the bits depend on the scan, the model, the pose, hood and d2 alone.
#include "flimo_ndt.h"
#include "flimo_jacobi.h"
#include "flimo_prims.h"
#include "flimo_kernels.h"
#include "flimo_sums.h"

#pragma clang fp contract(off)

namespace flimo {

constexpr int NDT_BLOCK = 256;

__global__ __launch_bounds__(NDT_BLOCK) void ndt_cell_kernel(const int32_t* __restrict__ count, const double* __restrict__ cov, unsigned nv,
                                                             int min_pts, double* __restrict__ eig, uint32_t* __restrict__ flag) {
  const unsigned v = blockIdx.x * NDT_BLOCK + threadIdx.x;
  if (v > nv) return;
  if (v == nv) { flag[nv] = 0u; return; }      // (the scan runs over nv + 1 flags: its last entry is the number of cells)
  bool cell = false;
  if (count[v] >= min_pts) {
    const double* C = cov + 6 * (size_t)v;
    double l0, l1, l2, v00, v01, v02, v10, v11, v12, v20, v21, v22;
    kk_eigen3(C[0], C[1], C[2], C[3], C[4], C[5], l0, l1, l2, v00, v01, v02, v10, v11, v12, v20, v21, v22);
    cell = l2 > 0.0;
    double* E = eig + 12 * (size_t)v;
    E[0] = l0; E[1] = l1; E[2] = l2;
    E[3] = v00; E[4] = v10; E[5] = v20;      // v0
    E[6] = v01; E[7] = v11; E[8] = v21;      // v1
    E[9] = v02; E[10] = v12; E[11] = v22;    // v2
  }
  flag[v] = cell ? 1u : 0u;
}

__global__ __launch_bounds__(NDT_BLOCK) void ndt_pack_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                             const int32_t* __restrict__ ijk, const int32_t* __restrict__ count,
                                                             const double* __restrict__ centroid, const double* __restrict__ eig, unsigned nv,
                                                             double eig_ratio, unsigned long long* __restrict__ keys, int32_t* __restrict__ cnt,
                                                             double* __restrict__ eval, NdtCell* __restrict__ cells) {
  const unsigned v = blockIdx.x * NDT_BLOCK + threadIdx.x;
  if (v >= nv || !flag[v]) return;
  const unsigned at = pos[v];
  const int32_t c[3] = {ijk[3 * (size_t)v], ijk[3 * (size_t)v + 1], ijk[3 * (size_t)v + 2]};
  unsigned long long key = 0;
  (void)ndt_slot_key(c, 0, &key);
  keys[at] = key;
  cnt[at] = count[v];
  const double* E = eig + 12 * (size_t)v;
  const double floor_l = eig_ratio * E[2];
  NdtCell r;
#pragma unroll
  for (int a = 0; a < 3; a++) r.mean[a] = centroid[3 * (size_t)v + a];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double l = E[k];
    eval[3 * (size_t)at + k] = l;
    r.w[k] = 1.0 / (l < floor_l ? floor_l : l);
#pragma unroll
    for (int a = 0; a < 3; a++) r.v[k][a] = E[3 + 3 * k + a];
  }
  r.pad = 0.0;
  cells[at] = r;
}

// a record through eight 16-byte loads
__device__ __forceinline__ void ndt_load(const NdtCell* __restrict__ cells, int32_t at, NdtCell& r) {
  const double2* src = reinterpret_cast<const double2*>(cells + at);
  double2* dst = reinterpret_cast<double2*>(&r);
#pragma unroll
  for (int t = 0; t < 8; t++) dst[t] = src[t];
}

struct NdtPass {
  const float4* scan;              // the resident scan (body frame), [n]
  const float* poses;              // the chunk's poses: [np][12], the upper three rows of RT (pose_from_x26)
  unsigned n, np;
  int hood;                        // 1 or 7
  float inv;                       // 1.0f / leaf
  double cc, d2;                   // -0.5 * d2, d2
  const unsigned long long* keys;  // the model: ascending keys, records
  const NdtCell* cells;
  unsigned nc;
  __device__ void world(unsigned pose, const float4& p, float w[3]) const {      // (transform_kernel's arithmetic)
    const float* M = poses + 12 * (size_t)pose;
    w[0] = M[0] * p.x + (M[1] * p.y + (M[2] * p.z + M[3]));
    w[1] = M[4] * p.x + (M[5] * p.y + (M[6] * p.z + M[7]));
    w[2] = M[8] * p.x + (M[9] * p.y + (M[10] * p.z + M[11]));
  }
};

// stage 1: cell [pairs][hood] (-1: absent), e [pairs][hood] (0.0 for an absent cell), m [pairs][hood] (may be null; NaN when absent)
__global__ __launch_bounds__(NDT_BLOCK) void ndt_lookup_kernel(NdtPass A, int32_t* __restrict__ cell, double* __restrict__ e_out,
                                                               double* __restrict__ m_out) {
  const size_t g = (size_t)blockIdx.x * NDT_BLOCK + threadIdx.x;
  const size_t total = (size_t)A.n * (size_t)A.np * (size_t)A.hood;
  if (g >= total) return;
  const size_t pair = g / (unsigned)A.hood;
  const int s = (int)(g % (unsigned)A.hood);
  const unsigned pose = (unsigned)(pair / A.n), i = (unsigned)(pair % A.n);
  float w[3];
  A.world(pose, A.scan[i], w);
  int32_t ijk[3];
  unsigned long long key = 0;
  int32_t at = -1;
  if (voxel_key(w[0], w[1], w[2], A.inv, ijk, &key) && ndt_slot_key(ijk, s, &key)) at = ndt_find(A.keys, A.nc, key);
  double m = __longlong_as_double(0x7ff8000000000000ll), e = 0.0;
  if (at >= 0) {
    NdtCell r;
    ndt_load(A.cells, at, r);
    double d[3];
    m = ndt_m(w, r, d);
    e = exp(A.cc * m);
  }
  cell[g] = at;
  e_out[g] = e;
  if (m_out) m_out[g] = m;
}

struct NdtStoredExp {      // stage 2's exp: the value stage 1 stored for this term
  double e;
  __device__ double operator()(double) const { return e; }
};

// stage 2 + level 1: workgroup (segment, pose) over the slots [seg * SUM_SEG, min(n, (seg + 1) * SUM_SEG)) of its pose
__global__ __launch_bounds__(SUM_RED) void ndt_reduce_kernel(NdtPass A, const int32_t* __restrict__ cell, const double* __restrict__ e_in,
                                                             unsigned nseg, double* __restrict__ part, int32_t* __restrict__ part_cnt) {
  const unsigned seg = blockIdx.x, pose = blockIdx.y;
  const size_t base = (size_t)pose * (size_t)A.n;
  const unsigned end = min(A.n, (seg + 1u) * (unsigned)SUM_SEG);
  const float* M = A.poses + 12 * (size_t)pose;
  const float R[9] = {M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10]};
  double acc[NDT_NUM];
#pragma unroll
  for (int t = 0; t < NDT_NUM; t++) acc[t] = 0.0;
  int c[2] = {0, 0};      // pairs with a live term, live terms
  for (unsigned i = seg * (unsigned)SUM_SEG + threadIdx.x; i < end; i += SUM_RED) {
    const float4 p4 = A.scan[i];
    const float p[3] = {p4.x, p4.y, p4.z};
    float w[3];
    A.world(pose, p4, w);
    int live = 0;
    for (int s = 0; s < A.hood; s++) {
      const size_t g = (base + i) * (unsigned)A.hood + (unsigned)s;
      const int32_t at = cell[g];
      const double e = e_in[g];
      if (at < 0 || !(e > 0.0)) continue;
      NdtCell r;
      ndt_load(A.cells, at, r);
      double m, e2;
      live += ndt_term(w, p, R, r, A.cc, A.d2, NdtStoredExp{e}, &m, &e2, acc) ? 1 : 0;
    }
    c[1] += live;
    c[0] += live > 0 ? 1 : 0;
  }
  sum_tail(acc, c, pose, nseg, seg, part, part_cnt);
}

static inline dim3 ndt_grid(size_t threads) { return dim3((unsigned)((threads + NDT_BLOCK - 1) / NDT_BLOCK)); }

hipError_t ndt_tmp_bytes(size_t nv, size_t* bytes) {
  size_t b = 0;
  const hipError_t e = exclusive_sum(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, nv + 1, hipStream_t(0));
  if (e != hipSuccess) return e;
  *bytes = b + 256;
  return hipSuccess;
}
hipError_t launch_ndt_cells(hipStream_t st, const int32_t* count, const double* cov, unsigned nv, int min_pts, double* eig, uint32_t* flag,
                            uint32_t* pos, void* tmp, size_t tmp_bytes) {
  hipLaunchKernelGGL(ndt_cell_kernel, ndt_grid((size_t)nv + 1), dim3(NDT_BLOCK), 0, st, count, cov, nv, min_pts, eig, flag);
  size_t bytes = tmp_bytes;
  const hipError_t e = exclusive_sum(tmp, bytes, flag, pos, (size_t)nv + 1, st);
  if (e != hipSuccess) return e;
  return hipGetLastError();
}
hipError_t launch_ndt_pack(hipStream_t st, const uint32_t* flag, const uint32_t* pos, const int32_t* ijk, const int32_t* count, const double* centroid,
                           const double* eig, unsigned nv, double eig_ratio, unsigned long long* keys, int32_t* cnt, double* eval, void* cells) {
  if (nv == 0) return hipSuccess;
  hipLaunchKernelGGL(ndt_pack_kernel, ndt_grid(nv), dim3(NDT_BLOCK), 0, st, flag, pos, ijk, count, centroid, eig, nv, eig_ratio, keys, cnt, eval,
                     static_cast<NdtCell*>(cells));
  return hipGetLastError();
}

hipError_t launch_scan_ndt(hipStream_t st, const float4* scan, unsigned n, const float* poses, unsigned np, int hood, float inv, double d2,
                           const unsigned long long* keys, const void* cells, unsigned nc, int32_t* cell, double* e, double* m, double* part,
                           int32_t* part_cnt, double* sums, long long* counts) {
  if (n == 0 || np == 0) return hipSuccess;
  const NdtPass A{scan, poses, n, np, hood, inv, -0.5 * d2, d2, keys, static_cast<const NdtCell*>(cells), nc};
  hipLaunchKernelGGL(ndt_lookup_kernel, ndt_grid((size_t)n * np * (size_t)hood), dim3(NDT_BLOCK), 0, st, A, cell, e, m);
  const unsigned nseg = sum_segments(n);
  hipLaunchKernelGGL(ndt_reduce_kernel, dim3(nseg, np), dim3(SUM_RED), 0, st, A, cell, e, nseg, part, part_cnt);
  launch_sum_final<NDT_NUM, 2>(st, part, part_cnt, np, nseg, sums, counts);
  return hipGetLastError();
}

}  // namespace flimo
