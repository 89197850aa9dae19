// fast_limo_amd/csrc/hip/flimo_ieskf_dev.hip  -- gfx950 device code.
//
// Developer entries (include/flimo_dev.h: flimo_ieskf_eval, flimo_ieskf_eval_host): the helpers of flimo_ieskf.h evaluated in batches,
// on the device and -- the same source compiled for the host -- beside it, for tests/test_gpu_ieskf.py and tests/test_ieskf_host.py.
// A translation unit of its own: every non-kernel device function has internal linkage in a device compilation, and one that gains
// a second caller in flimo_ieskf.hip is no longer inlined into ieskf_kernel (the one-wave solve became a call there: other code
// for the shipped kernel).  Here the helpers are instantiated for these kernels alone.  (flimo_ieskf.h's only non-inline global
// exists under IESKF_STAMPS, which tools/ieskf_bench.hip alone defines, and that tool does not link this file.)
#include <hip/hip_runtime.h>
#include "flimo_types.h"
#include "flimo_chain.h"
#include "flimo_ieskf.h"

#pragma clang fp contract(off)

namespace flimo {

static const int IK_OP_IN[10] = {4, 3, 4, 1, 3, 6, 8, 144, 156, 582};
static const int IK_OP_OUT[10] = {3, 9, 4, 2, 6, 2, 4, 145, 13, 299};

// one scalar helper, one item: the device kernel and the host twin both call this
__host__ __device__ inline void ik_eval_item(int op, const double* a, double* o) {
  switch (op) {
    case 0: { const Q4 q{a[0], a[1], a[2], a[3]}; ik_so3_log(q, o); break; }
    case 1: ik_A_T(a, o); break;
    case 2: { const Q4 q = ik_exp_quat(a, a[3]); o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w; break; }
    case 3: ik_cos_sinc_sqrt(a[0], o[0], o[1]); break;
    case 4: ik_s2_Bx(a, o); break;
    case 5: ik_s2_boxminus(a, a + 3, o); break;
    default: ik_s2_J(a, a + 3, a + 6, o); break;
  }
}
__global__ __launch_bounds__(64) void ik_eval_scalar_kernel(int op, int n_in, int n_out, const double* __restrict__ in, int n, double* __restrict__ out) {
  const int i = (int)(blockIdx.x * 64 + threadIdx.x);
  if (i >= n) return;
  double a[8], o[9];
  for (int k = 0; k < n_in; k++) a[k] = in[(size_t)i * n_in + k];
  ik_eval_item(op, a, o);
  for (int k = 0; k < n_out; k++) out[(size_t)i * n_out + k] = o[k];
}
// one wave per 12 x 12 system
__global__ __launch_bounds__(64) void ik_eval_gj_kernel(int solve, const double* __restrict__ in, double* __restrict__ out) {
  __shared__ double T[144], X[144], v[12];
  const int lane = (int)threadIdx.x;
  const double* a = in + (size_t)blockIdx.x * (solve ? 156 : 144);
  double* o = out + (size_t)blockIdx.x * (solve ? 13 : 145);
  for (int e = lane; e < 144; e += 64) { T[e] = a[e]; X[e] = 0.0; }
  if (solve && lane < 12) v[lane] = a[144 + lane];
  __syncthreads();
  const bool ok = solve ? ik_gj12_solve_wave(T, v, X, lane) : ik_gj12_inverse_wave(T, X, lane);
  __syncthreads();
  const int n_res = solve ? 12 : 144;
  for (int e = lane; e < n_res; e += 64) o[e] = X[e];
  if (lane == 0) o[n_res] = ok ? 1.0 : 0.0;
}
// one workgroup per item: ik_pre_block as the extra workgroup of a pass runs it
__global__ __launch_bounds__(256) void ik_eval_pre_kernel(const double* __restrict__ in, double* __restrict__ out) {
  __shared__ double lds[IKL_END];
  const int tid = (int)threadIdx.x;
  const double* a = in + (size_t)blockIdx.x * 582;
  double* o = out + (size_t)blockIdx.x * 299;
  if (tid < 26) { lds[IKL_XC + tid] = a[tid]; lds[IKL_XP + tid] = a[26 + tid]; }
  for (int i = tid; i < 529; i += 256) lds[IKL_P + i] = a[52 + i];
  const double R = a[581];
  __syncthreads();
  ik_pre_block(lds, R, tid);
  if (tid < IK_N) o[tid] = lds[IKL_DXN + tid];
  for (int e = tid; e < 276; e += 256) o[23 + e] = lds[IKL_AI + e];       // A11^-1 and G2: contiguous
}
bool ieskf_op_shape(int op, int* n_in, int* n_out) {
  if (op < 0 || op > 9) return false;
  if (n_in) *n_in = IK_OP_IN[op];
  if (n_out) *n_out = IK_OP_OUT[op];
  return true;
}
void launch_ieskf_eval(hipStream_t st, int op, const double* d_in, int n, double* d_out) {
  if (n <= 0) return;
  if (op <= 6) hipLaunchKernelGGL(ik_eval_scalar_kernel, dim3((n + 63) / 64), dim3(64), 0, st, op, IK_OP_IN[op], IK_OP_OUT[op], d_in, n, d_out);
  else if (op <= 8) hipLaunchKernelGGL(ik_eval_gj_kernel, dim3(n), dim3(64), 0, st, op == 8 ? 1 : 0, d_in, d_out);
  else hipLaunchKernelGGL(ik_eval_pre_kernel, dim3(n), dim3(256), 0, st, d_in, d_out);
}
// the host twin, and which branch an item takes (the helpers' own conditions, on the helpers' own intermediate values)
static int ik_chart(const double g[3]) { return g[0] + IK_S2L > IK_TOL ? 0 : 1; }
bool ieskf_eval_host(int op, const double* in, size_t n, double* out, int* branch) {
  if (op < 0 || op > 9 || op == 8) return false;
  const int ni = IK_OP_IN[op], no = IK_OP_OUT[op];
  for (size_t i = 0; i < n; i++) {
    const double* a = in + i * ni;
    double* o = out + i * no;
    int br = 0;
    if (op <= 6) {
      ik_eval_item(op, a, o);
      if (op == 0) br = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) < IK_TOL;
      else if (op == 1) br = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) < IK_TOL;
      else if (op == 2) br = !(a[3] * a[3] * (a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) >= sqrt(sqrt(2.220446049250313e-16)));
      else if (op == 3) br = !(a[0] >= sqrt(sqrt(2.220446049250313e-16)));
      else if (op == 4) br = ik_chart(a);
      else if (op == 5) {
        double Ha[9], hv[3];
        ik_hat(a, Ha);
        ik_mv3(Ha, a + 3, hv);
        const double v_sin = sqrt(hv[0] * hv[0] + hv[1] * hv[1] + hv[2] * hv[2]);
        const double theta = atan2(v_sin, a[0] * a[3] + a[1] * a[4] + a[2] * a[5]);
        br = (v_sin < IK_TOL ? (fabs(theta) > IK_TOL ? 2 : 1) : 0) + 4 * ik_chart(a + 3);
      } else {
        br = (sqrt(a[6] * a[6] + a[7] * a[7]) < IK_TOL ? 1 : 0) + 2 * ik_chart(a) + 4 * ik_chart(a + 3);
      }
    } else if (op == 7) {
      const bool ok = ik_inverse_gj12_serial(a, o);
      if (!ok) for (int e = 0; e < 144; e++) o[e] = 0.0;
      o[144] = ok ? 1.0 : 0.0;
    } else {
      ik_pre_serial(a, a + 26, a + 52, a[581], o, o + 23, o + 23 + 144);
    }
    if (branch) branch[i] = br;
  }
  return true;
}

}  // namespace flimo
