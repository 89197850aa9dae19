// fast_limo_amd/csrc/hip/flimo_jacobi.h -- the eigen-solve of a symmetric 3 x 3 covariance that every kernel ending a neighbourhood
// or a voxel in its principal axes shares: a cyclic Jacobi until the off-diagonal is exactly 0, the eigenvalues in ascending order
// (on a tie the lower column first), the unit vectors as the rotations leave them.  kk_plane (flimo_knn_k.hip) keeps the smallest
// one's vector and orients it; the NDT cell kernel (flimo_ndt.hip) keeps all three.  One text: their bits are the same by construction.
// Host AND device: gicp_regularize (flimo_gicp.h) runs it on both; every operation is an IEEE float64 +, -, *, / or sqrt.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace flimo {

// one Jacobi rotation in the plane (p, q) of a symmetric 3 x 3: app, aqq, apq its 2 x 2; arp, arq the third row's entries of those
// columns; v*p, v*q columns p and q of the accumulated eigenvectors (Rutishauser's update: apq becomes exactly 0)
__host__ __device__ __forceinline__ void kk_jacobi_rot(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                              double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double g = fabs(apq);
  if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) { apq = 0.0; return; }      // below the diagonal's last bit
  const double h = aqq - app;
  double t;
  if (fabs(h) + g == fabs(h)) {
    t = apq / h;
  } else {
    const double theta = 0.5 * h / apq;
    t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
  }
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
  const double hh = t * apq;
  app = app - hh; aqq = aqq + hh; apq = 0.0;
  double a = arp, b = arq;
  arp = a - s * (b + a * tau); arq = b + s * (a - b * tau);
  a = v0p; b = v0q; v0p = a - s * (b + a * tau); v0q = b + s * (a - b * tau);
  a = v1p; b = v1q; v1p = a - s * (b + a * tau); v1q = b + s * (a - b * tau);
  a = v2p; b = v2q; v2p = a - s * (b + a * tau); v2q = b + s * (a - b * tau);
}

constexpr int KK_JACOBI_SWEEPS = 12;
__host__ __device__ __forceinline__ void kk_swap_if(bool c, double& a, double& b) { const double x = c ? b : a, y = c ? a : b; a = x; b = y; }

// The principal axes of a symmetric 3 x 3 covariance: l0 <= l1 <= l2 and the unit vectors as COLUMNS of v (vRC: row R, column C;
// column k belongs to lk), with whatever sign the rotations leave.
__host__ __device__ __forceinline__ void kk_eigen3(double a00, double a01, double a02, double a11, double a12, double a22, double& l0, double& l1, double& l2,
                                          double& v00, double& v01, double& v02, double& v10, double& v11, double& v12, double& v20, double& v21,
                                          double& v22) {
  v00 = 1.0; v01 = 0.0; v02 = 0.0; v10 = 0.0; v11 = 1.0; v12 = 0.0; v20 = 0.0; v21 = 0.0; v22 = 1.0;
  for (int sweep = 0; sweep < KK_JACOBI_SWEEPS; sweep++) {
    if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
    kk_jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
    kk_jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
    kk_jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
  }
  // ascending eigenvalues; on a tie the lower column first
  l0 = a00; l1 = a11; l2 = a22;
  const bool s01 = l1 < l0;
  kk_swap_if(s01, l0, l1); kk_swap_if(s01, v00, v01); kk_swap_if(s01, v10, v11); kk_swap_if(s01, v20, v21);
  const bool s12 = l2 < l1;
  kk_swap_if(s12, l1, l2); kk_swap_if(s12, v01, v02); kk_swap_if(s12, v11, v12); kk_swap_if(s12, v21, v22);
  const bool t01 = l1 < l0;
  kk_swap_if(t01, l0, l1); kk_swap_if(t01, v00, v01); kk_swap_if(t01, v10, v11); kk_swap_if(t01, v20, v21);
}

}  // namespace flimo
