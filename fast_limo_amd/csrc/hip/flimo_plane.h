// fast_limo_amd/csrc/hip/flimo_plane.h
// The plane through one minimal sample of three stored points (flimo_map_planes, include/flimo_c.h): the edge and collinearity
// tests, the unit normal with its sign rule, the axis constraint and the offset, float64 on the float32 points widened, only
// + - * / sqrt, in the association the header states.  Host AND device: the solve kernel (flimo_plane.hip) and
// flimo_plane_solve_host run this one function, compiled without FMA contraction.  plane_inlier_t is the float32 test every stored
// point goes through, anchored at the sample's first point; plane_side is the compare of the mask and the removal.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace flimo {

constexpr int PLANE_OK = 0, PLANE_DEGENERATE = 1, PLANE_REJECTED = 2;      // FLIMO_PLANE_* (flimo_c.h)
constexpr int PLANE_SLAB = 8192;      // FLIMO_PLANE_SLAB: the points of a slab of the sum
constexpr int PLANE_RED = 256;        // threads of a count workgroup: the sum's shape (fit_reduce_kernel's FIT_RED)
inline unsigned plane_slabs(unsigned n_map) { return (n_map + (unsigned)PLANE_SLAB - 1u) / (unsigned)PLANE_SLAB; }      // (n_map < 2^31)

__host__ __device__ inline double plane_sq(double x, double y, double z) { return x * x + (y * y + z * z); }
__host__ __device__ inline bool plane_finite(double v) { return v - v == 0.0; }      // (false for NaN and the infinities)

// p3: the three points a, b, c packed xyz; axis is read only when min_cos > 0.  Returns PLANE_*; for PLANE_OK plane4 = (n, d) and
// nf = (float)n; both NaN otherwise.  (Two equal INDICES are the caller's to reject: two equal points fail q > 0 here.)
__host__ __device__ inline int plane_solve(const float p3[9], float min_edge, float min_sin, const float axis[3], float min_cos,
                                           double plane4[4], float nf[3]) {
  for (int i = 0; i < 4; i++) plane4[i] = __builtin_nan("");
  for (int i = 0; i < 3; i++) nf[i] = __builtin_nanf("");
  double p[9];
  for (int i = 0; i < 9; i++) p[i] = (double)p3[i];
  const double e1[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]};
  const double e2[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
  const double e3[3] = {p[6] - p[3], p[7] - p[4], p[8] - p[5]};
  const double l1 = plane_sq(e1[0], e1[1], e1[2]), l2 = plane_sq(e2[0], e2[1], e2[2]), l3 = plane_sq(e3[0], e3[1], e3[2]);
  const double min2 = (double)min_edge * (double)min_edge;
  if (!(l1 >= min2) || !(l2 >= min2) || !(l3 >= min2)) return PLANE_DEGENERATE;      // (a NaN coordinate fails here)
  const double cr[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  const double q = plane_sq(cr[0], cr[1], cr[2]);
  const double s2 = (double)min_sin * (double)min_sin;
  if (!(q > 0.0) || !(q >= s2 * (l1 * l2))) return PLANE_DEGENERATE;
  const double len = sqrt(q);
  double n[3] = {cr[0] / len, cr[1] / len, cr[2] / len};
  for (int i = 0; i < 3; i++)
    if (!plane_finite(n[i])) return PLANE_DEGENERATE;      // (an infinite edge: inf / inf)
  // the component of largest magnitude positive, the lowest axis on equal magnitudes (flimo_map_normals' rule with no viewpoint)
  int k = 0;
  if (fabs(n[1]) > fabs(n[k])) k = 1;
  if (fabs(n[2]) > fabs(n[k])) k = 2;
  if (n[k] < 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
  if (min_cos > 0.f) {
    const double c = fabs(n[0] * (double)axis[0] + (n[1] * (double)axis[1] + n[2] * (double)axis[2]));
    if (!(c >= (double)min_cos)) return PLANE_REJECTED;
  }
  plane4[0] = n[0]; plane4[1] = n[1]; plane4[2] = n[2];
  plane4[3] = -(n[0] * p[0] + (n[1] * p[1] + n[2] * p[2]));
  nf[0] = (float)n[0]; nf[1] = (float)n[1]; nf[2] = (float)n[2];
  return PLANE_OK;
}

// the signed float32 distance of point (x, y, z) from the plane of normal (nx, ny, nz) through the anchor (ax, ay, az)
__host__ __device__ inline float plane_t(float nx, float ny, float nz, float ax, float ay, float az, float x, float y, float z) {
  const float vx = x - ax, vy = y - ay, vz = z - az;
  return nx * vx + (ny * vy + nz * vz);
}
// side 0: |t| < dist; -1: t < dist (the plane and everything beneath it); +1: t > -dist.  False for a NaN.
__host__ __device__ inline bool plane_side(float t, float dist, int side) {
  return side == 0 ? fabsf(t) < dist : side < 0 ? t < dist : t > -dist;
}

}  // namespace flimo
