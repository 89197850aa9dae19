// fast_limo_amd/csrc/hip/flimo_ndt.h
// One term of the normal distributions transform (flimo_scan_ndt, include/flimo_c.h): the world point w of a scan point p under a
// pose with rotation R, against one CELL of the resident model -- the voxel's centroid, its three principal axes v0 v1 v2 and the
// weights wk = 1 / max(lk, eig_ratio * l2).  A cell is three orthogonal planes with those weights, so the term's rows are
// flimo_scan_linearize's, one per axis.  Host AND device: the kernels (flimo_ndt.hip) and flimo_ndt_term_host run these functions;
// only exp differs (OCML's on the device, libm's on the host), and it is handed in.  Everything float64, nothing contracted.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "flimo_voxel.h"

#pragma clang fp contract(off)

namespace flimo {

constexpr int NDT_SLOTS = 4;       // FLIMO_NDT_SLOTS: resident models of a context
constexpr int NDT_NUM = 28;        // the sums of a pose: 21 of H, 6 of g, the score
constexpr int NDT_HOOD_MAX = 7;    // the own cell and its six face neighbours

// 128 B, so that a lane fetches a record with eight 16-byte loads
struct alignas(16) NdtCell {
  double mean[3];
  double v[3][3];      // v[k]: the unit vector of lk (x, y, z)
  double w[3];
  double pad;
};
static_assert(sizeof(NdtCell) == 128, "an NDT cell record is 128 bytes");

// the key of neighbour slot s of cell ijk: 0 the cell itself, 1..6 = -x +x -y +y -z +z; false where the coordinate leaves the lattice
__host__ __device__ inline bool ndt_slot_key(const int32_t ijk[3], int s, unsigned long long* key) {
  int32_t c[3] = {ijk[0], ijk[1], ijk[2]};
  if (s > 0) {
    const int a = (s - 1) >> 1;
    c[a] += (s & 1) ? -1 : 1;
    if (c[a] <= -(1 << 20) || c[a] >= (1 << 20)) return false;
  }
  const long long h = 1ll << 20;
  *key = ((unsigned long long)(c[2] + h) << 42) | ((unsigned long long)(c[1] + h) << 21) | (unsigned long long)(c[0] + h);
  return true;
}

// the position of key among the model's ascending keys, or -1
__host__ __device__ inline int32_t ndt_find(const unsigned long long* keys, uint32_t nc, unsigned long long key) {
  uint32_t lo = 0, hi = nc;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (keys[mid] < key) lo = mid + 1u; else hi = mid;
  }
  return (lo < nc && keys[lo] == key) ? (int32_t)lo : -1;
}

// r = (double)w - mean, dk = vk . r, m = w0*(d0*d0) + (w1*(d1*d1) + w2*(d2*d2))
__host__ __device__ inline double ndt_m(const float w[3], const NdtCell& c, double d[3]) {
  const double rx = (double)w[0] - c.mean[0], ry = (double)w[1] - c.mean[1], rz = (double)w[2] - c.mean[2];
#pragma unroll
  for (int k = 0; k < 3; k++) d[k] = c.v[k][0] * rx + (c.v[k][1] * ry + c.v[k][2] * rz);
  return c.w[0] * (d[0] * d[0]) + (c.w[1] * (d[1] * d[1]) + c.w[2] * (d[2] * d[2]));
}

// The whole term: m, e = ex(cc * m) with cc = -0.5 * d2 formed by the caller, and -- where the term is LIVE, e > 0.0 -- its 28
// contributions, each ONE add onto acc (k ascending): acc[0..20] the upper triangle of H row-major, acc[21..26] g, acc[27] the
// score.  R: the nine rotation entries, row-major.  Returns whether the term is live; acc is untouched when it is not.
template <class Exp>
__host__ __device__ inline bool ndt_term(const float w[3], const float p[3], const float R[9], const NdtCell& c, double cc, double d2, Exp ex,
                                         double* m_out, double* e_out, double acc[NDT_NUM]) {
  double d[3];
  const double m = ndt_m(w, c, d);
  const double e = ex(cc * m);
  *m_out = m;
  *e_out = e;
  if (!(e > 0.0)) return false;      // (underflow and NaN alike)
  const double px = (double)p[0], py = (double)p[1], pz = (double)p[2];
  const double ed = e * d2;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double nx = c.v[k][0], ny = c.v[k][1], nz = c.v[k][2];
    double J[6];
    J[0] = (double)R[0] * nx + ((double)R[3] * ny + (double)R[6] * nz);
    J[1] = (double)R[1] * nx + ((double)R[4] * ny + (double)R[7] * nz);
    J[2] = (double)R[2] * nx + ((double)R[5] * ny + (double)R[8] * nz);
    J[3] = py * J[2] - pz * J[1];
    J[4] = pz * J[0] - px * J[2];
    J[5] = px * J[1] - py * J[0];
    const double s = ed * c.w[k];
    int t = 0;
#pragma unroll
    for (int a = 0; a < 6; a++) {
      const double sa = s * J[a];
#pragma unroll
      for (int b = a; b < 6; b++) { acc[t] = acc[t] + sa * J[b]; t++; }
    }
    const double sd = s * d[k];
#pragma unroll
    for (int a = 0; a < 6; a++) acc[21 + a] = acc[21 + a] + sd * J[a];
  }
  acc[27] = acc[27] + e;
  return true;
}

}  // namespace flimo
