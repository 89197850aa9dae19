// fast_limo_amd/csrc/hip/flimo_corr.h
// The pose of one minimal sample of three point correspondences (flimo_corr_poses, include/flimo_c.h): the edge tests and the
// closed-form TRIAD solve, float64 on the float32 inputs widened, only + - * / sqrt, in the association the header states.  Host AND
// device: the solve kernel (flimo_corr.hip) and flimo_corr_pose_host run this one function, compiled without FMA contraction.
// corr_compatible is the edge predicate of flimo_corr_graph, under the same rules.
#pragma once
#include <hip/hip_runtime.h>
#include "flimo_pose.h"

#pragma clang fp contract(off)

namespace flimo {

constexpr int CORR_OK = 0, CORR_DEGENERATE = 1, CORR_REJECTED = 2;      // FLIMO_CORR_* (flimo_c.h)

__host__ __device__ inline double corr_sq(double x, double y, double z) { return x * x + (y * y + z * z); }
__host__ __device__ inline bool corr_finite(double v) { return v - v == 0.0; }      // (false for NaN and the infinities)

// Two correspondences i and j can both be true (flimo_corr_graph, include/flimo_c.h): the edge i -> j has the same length in both
// clouds to within tol, is not shorter than min_edge in either, and passes corr_solve's polygon test.  The points are the float32
// inputs widened; min2 = (double)min_edge * (double)min_edge, s2 = (double)edge_sim * (double)edge_sim.  i == j is the caller's.
// Host AND device: the adjacency kernel (flimo_corr.hip) and flimo_corr_compatible_host run this one function.
__host__ __device__ inline bool corr_compatible(const double si[3], const double sj[3], const double di[3], const double dj[3], double min2,
                                                double tol, double s2) {
  const double es = corr_sq(sj[0] - si[0], sj[1] - si[1], sj[2] - si[2]);
  const double ed = corr_sq(dj[0] - di[0], dj[1] - di[1], dj[2] - di[2]);
  if (!(es >= min2) || !(ed >= min2)) return false;      // (a NaN coordinate fails here)
  if (!(fabs(sqrt(es) - sqrt(ed)) <= tol)) return false;      // (two infinite edges: inf - inf fails)
  const double lo = es < ed ? es : ed, hi = es < ed ? ed : es;
  return lo >= s2 * hi;
}

// the orthonormal frame of a triangle: u1 along a -> b, u3 along u1 x (c - a), u2 = u3 x u1; U = {u1, u2, u3}
__host__ __device__ inline void corr_frame(const double p[9], double U[9]) {
  const double e1[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]};
  const double e2[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
  const double n1 = sqrt(corr_sq(e1[0], e1[1], e1[2]));
  const double u1[3] = {e1[0] / n1, e1[1] / n1, e1[2] / n1};
  const double cr[3] = {u1[1] * e2[2] - u1[2] * e2[1], u1[2] * e2[0] - u1[0] * e2[2], u1[0] * e2[1] - u1[1] * e2[0]};
  const double n3 = sqrt(corr_sq(cr[0], cr[1], cr[2]));
  const double u3[3] = {cr[0] / n3, cr[1] / n3, cr[2] / n3};
  const double u2[3] = {u3[1] * u1[2] - u3[2] * u1[1], u3[2] * u1[0] - u3[0] * u1[2], u3[0] * u1[1] - u3[1] * u1[0]};
  for (int i = 0; i < 3; i++) { U[i] = u1[i]; U[3 + i] = u2[i]; U[6 + i] = u3[i]; }
}

// src3 / dst3: the three points a, b, c of either cloud, packed xyz.  Returns CORR_*; for CORR_OK pose7 = (t, x, y, z, w) and rt12 =
// the upper three rows of the float32 matrix pose_from_x26 forms from it; both NaN otherwise.
__host__ __device__ inline int corr_solve(const float src3[9], const float dst3[9], float edge_sim, float min_edge, double pose7[7],
                                          float rt12[12]) {
  const double nan = __builtin_nan("");
  for (int i = 0; i < 7; i++) pose7[i] = nan;
  for (int i = 0; i < 12; i++) rt12[i] = __builtin_nanf("");
  double s[9], d[9];
  for (int i = 0; i < 9; i++) { s[i] = (double)src3[i]; d[i] = (double)dst3[i]; }
  // edges a -> b, b -> c, c -> a of both clouds
  double es[3], ed[3];
  for (int e = 0; e < 3; e++) {
    const int a = 3 * e, b = 3 * ((e + 1) % 3);
    es[e] = corr_sq(s[b] - s[a], s[b + 1] - s[a + 1], s[b + 2] - s[a + 2]);
    ed[e] = corr_sq(d[b] - d[a], d[b + 1] - d[a + 1], d[b + 2] - d[a + 2]);
  }
  const double min2 = (double)min_edge * (double)min_edge;
  for (int e = 0; e < 3; e++)
    if (!(es[e] >= min2) || !(ed[e] >= min2)) return CORR_DEGENERATE;      // (a NaN coordinate fails here)
  const double s2 = (double)edge_sim * (double)edge_sim;
  for (int e = 0; e < 3; e++) {
    const double lo = es[e] < ed[e] ? es[e] : ed[e], hi = es[e] < ed[e] ? ed[e] : es[e];
    if (!(lo >= s2 * hi)) return CORR_REJECTED;
  }
  double Us[9], Ud[9], R[9], t[3];
  corr_frame(s, Us);
  corr_frame(d, Ud);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) R[3 * r + c] = Ud[r] * Us[c] + (Ud[3 + r] * Us[3 + c] + Ud[6 + r] * Us[6 + c]);
  for (int r = 0; r < 3; r++) {
    const double cs0 = ((s[0] + s[3]) + s[6]) / 3.0, cs1 = ((s[1] + s[4]) + s[7]) / 3.0, cs2 = ((s[2] + s[5]) + s[8]) / 3.0;
    const double cd = ((d[r] + d[3 + r]) + d[6 + r]) / 3.0;
    t[r] = cd - (R[3 * r] * cs0 + (R[3 * r + 1] * cs1 + R[3 * r + 2] * cs2));
  }
  for (int i = 0; i < 9; i++) if (!corr_finite(R[i])) return CORR_DEGENERATE;      // (a collinear triangle: 0 / 0)
  for (int i = 0; i < 3; i++) if (!corr_finite(t[i])) return CORR_DEGENERATE;
  // Shepperd: the largest of (trace, R00, R11, R22), the first on a tie
  const double tr = R[0] + (R[4] + R[8]);
  int br = 0;
  double best = tr;
  if (R[0] > best) { best = R[0]; br = 1; }
  if (R[4] > best) { best = R[4]; br = 2; }
  if (R[8] > best) { best = R[8]; br = 3; }
  double x, y, z, w;
  if (br == 0) {
    w = 0.5 * sqrt(1.0 + tr);
    const double f = 0.25 / w;
    x = (R[7] - R[5]) * f; y = (R[2] - R[6]) * f; z = (R[3] - R[1]) * f;
  } else if (br == 1) {
    x = 0.5 * sqrt(1.0 + ((R[0] - R[4]) - R[8]));
    const double f = 0.25 / x;
    w = (R[7] - R[5]) * f; y = (R[1] + R[3]) * f; z = (R[2] + R[6]) * f;
  } else if (br == 2) {
    y = 0.5 * sqrt(1.0 + ((R[4] - R[0]) - R[8]));
    const double f = 0.25 / y;
    w = (R[2] - R[6]) * f; x = (R[1] + R[3]) * f; z = (R[5] + R[7]) * f;
  } else {
    z = 0.5 * sqrt(1.0 + ((R[8] - R[0]) - R[4]));
    const double f = 0.25 / z;
    w = (R[3] - R[1]) * f; x = (R[2] + R[6]) * f; y = (R[5] + R[7]) * f;
  }
  pose7[0] = t[0]; pose7[1] = t[1]; pose7[2] = t[2];
  pose7[3] = x; pose7[4] = y; pose7[5] = z; pose7[6] = w;
  // the matrix flimo_scan_fitness would form from this pose placed into an x26 (pose_from_x26: float32 casts, quat_to_rot_f)
  const float q[4] = {(float)x, (float)y, (float)z, (float)w};
  float Rf[9];
  quat_to_rot_f(q, Rf);
  for (int r = 0; r < 3; r++) {
    rt12[4 * r] = Rf[3 * r]; rt12[4 * r + 1] = Rf[3 * r + 1]; rt12[4 * r + 2] = Rf[3 * r + 2];
    rt12[4 * r + 3] = (float)t[r];
  }
  return CORR_OK;
}

}  // namespace flimo
