// fast_limo_amd/csrc/hip/flimo_gicp.h
// Generalized ICP, plane to plane (flimo_gicp_build / flimo_scan_gicp, include/flimo_c.h): the regularised covariance of a
// neighbourhood (gicp_regularize) and the term of one (pose, scan point) pair against its nearest stored point (gicp_term) -- the
// residual weighed by the shape of BOTH surfaces, M = (CB + R CA R^T)^-1.  Host AND device: the kernels (flimo_gicp.hip) and
// flimo_gicp_regularize_host / flimo_gicp_term_host run these functions.  Everything float64 on float32 inputs widened, nothing
// contracted; a covariance is its six numbers xx xy xz yy yz zz.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "flimo_jacobi.h"

#pragma clang fp contract(off)

namespace flimo {

constexpr int GICP_NUM = 28;       // the sums of a pose: 21 of H, 6 of g, the cost
constexpr int GICP_PLANE = 0;      // FLIMO_GICP_PLANE: the eigenvalues become (eps, 1, 1) -- PCL's rule
constexpr int GICP_CLAMP = 1;      // FLIMO_GICP_CLAMP: no eigenvalue below eps * l2 -- the NDT model's rule

__host__ __device__ inline bool gicp_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }      // (false for a NaN)
__host__ __device__ inline double gicp_nan() {
#if defined(__HIP_DEVICE_COMPILE__)
  return __longlong_as_double(0x7ff8000000000000ll);
#else
  return (double)NAN;
#endif
}

// kk_eigen3's pairs of a covariance: l0 <= l1 <= l2 and v[k], the unit vector of lk
__host__ __device__ inline void gicp_eigen(const double cov[6], double l[3], double v[3][3]) {
  kk_eigen3(cov[0], cov[1], cov[2], cov[3], cov[4], cov[5], l[0], l[1], l[2], v[0][0], v[1][0], v[2][0], v[0][1], v[1][1], v[2][1], v[0][2], v[1][2],
            v[2][2]);
}

// C' = sum over k ascending of (lk' * vk[a]) * vk[b], added onto +0.0, from kk_eigen3's l0 <= l1 <= l2 and v0 v1 v2.  No
// covariance -- a non-finite number among the six, or no l2 > 0.0 --: six NaN and false.
__host__ __device__ inline bool gicp_regularize(const double cov[6], int rule, double eps, double out[6]) {
  bool ok = true;
#pragma unroll
  for (int t = 0; t < 6; t++) ok = ok && gicp_finite(cov[t]);
  double l[3], v[3][3];
  if (ok) {
    gicp_eigen(cov, l, v);
    ok = l[2] > 0.0;
  }
  if (!ok) {
#pragma unroll
    for (int t = 0; t < 6; t++) out[t] = gicp_nan();
    return false;
  }
  if (rule == GICP_PLANE) {
    l[0] = eps; l[1] = 1.0; l[2] = 1.0;
  } else {
    const double floor_l = eps * l[2];
#pragma unroll
    for (int k = 0; k < 3; k++) l[k] = l[k] < floor_l ? floor_l : l[k];
  }
  int t = 0;
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = a; b < 3; b++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 3; k++) s = s + (l[k] * v[k][a]) * v[k][b];
      out[t++] = s;
    }
  return true;
}

__host__ __device__ inline double gicp_dot3(const double a[3], const double b[3]) { return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2]); }

// The term of one pair.  w: the float32 world point, b: the float32 nearest stored point, p: the float32 scan point, R: the nine
// float32 rotation entries row-major (all widened); CA: the scan point's covariance (body frame), CB: the stored point's.
//   r = w - b;  T = R CA, S = CB + T R^T (its six numbers);  c = the cofactors of S, det = S00*c00 + (S01*c01 + S02*c02), M = c / det
//   LIVE iff the twelve covariance numbers are finite, det > 0.0 and 1.0 / det is finite
//   y = M r, m = r . y;  J_c = R e_c (c < 3), R (e_(c-3) x p) (c >= 3);  U_c = M J_c
//   H_ab = J_a . U_b (21 upper-triangle entries, row-major), g_a = J_a . y, cost = m
// every three-term sum as x0 + (x1 + x2).  out30 = m, det, the 28; all 0 when the term is not live.
__host__ __device__ inline bool gicp_term(const float w[3], const float b[3], const float p[3], const float R[9], const double CA[6],
                                          const double CB[6], double out[30]) {
  bool live = true;
#pragma unroll
  for (int t = 0; t < 6; t++) live = live && gicp_finite(CA[t]) && gicp_finite(CB[t]);
  const double r[3] = {(double)w[0] - (double)b[0], (double)w[1] - (double)b[1], (double)w[2] - (double)b[2]};
  const double Rd[3][3] = {{(double)R[0], (double)R[1], (double)R[2]}, {(double)R[3], (double)R[4], (double)R[5]},
                           {(double)R[6], (double)R[7], (double)R[8]}};
  const double A[3][3] = {{CA[0], CA[1], CA[2]}, {CA[1], CA[3], CA[4]}, {CA[2], CA[4], CA[5]}};
  double T[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) T[i][j] = Rd[i][0] * A[0][j] + (Rd[i][1] * A[1][j] + Rd[i][2] * A[2][j]);
  const double S00 = CB[0] + gicp_dot3(T[0], Rd[0]), S01 = CB[1] + gicp_dot3(T[0], Rd[1]), S02 = CB[2] + gicp_dot3(T[0], Rd[2]);
  const double S11 = CB[3] + gicp_dot3(T[1], Rd[1]), S12 = CB[4] + gicp_dot3(T[1], Rd[2]), S22 = CB[5] + gicp_dot3(T[2], Rd[2]);
  const double c00 = S11 * S22 - S12 * S12, c01 = S02 * S12 - S01 * S22, c02 = S01 * S12 - S02 * S11;
  const double c11 = S00 * S22 - S02 * S02, c12 = S01 * S02 - S00 * S12, c22 = S00 * S11 - S01 * S01;
  const double det = S00 * c00 + (S01 * c01 + S02 * c02);
  live = live && det > 0.0 && gicp_finite(1.0 / det);
  if (!live) {
#pragma unroll
    for (int t = 0; t < 30; t++) out[t] = 0.0;
    return false;
  }
  const double M[3][3] = {{c00 / det, c01 / det, c02 / det}, {c01 / det, c11 / det, c12 / det}, {c02 / det, c12 / det, c22 / det}};
  const double y[3] = {gicp_dot3(M[0], r), gicp_dot3(M[1], r), gicp_dot3(M[2], r)};
  const double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
  double J[6][3], U[6][3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    J[0][i] = Rd[i][0]; J[1][i] = Rd[i][1]; J[2][i] = Rd[i][2];
    J[3][i] = py * Rd[i][2] - pz * Rd[i][1];
    J[4][i] = pz * Rd[i][0] - px * Rd[i][2];
    J[5][i] = px * Rd[i][1] - py * Rd[i][0];
  }
#pragma unroll
  for (int c = 0; c < 6; c++)
#pragma unroll
    for (int a = 0; a < 3; a++) U[c][a] = gicp_dot3(M[a], J[c]);
  out[0] = gicp_dot3(r, y);
  out[1] = det;
  int t = 2;
#pragma unroll
  for (int a = 0; a < 6; a++)
#pragma unroll
    for (int c = a; c < 6; c++) out[t++] = gicp_dot3(J[a], U[c]);
#pragma unroll
  for (int a = 0; a < 6; a++) out[23 + a] = gicp_dot3(J[a], y);
  out[29] = out[0];
  return true;
}

}  // namespace flimo
