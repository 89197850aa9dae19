// fast_limo_amd/csrc/hip/flimo_sc.h
// Scan Context (Kim & Kim, IROS 2018) as flimo_scan_context / flimo_sc_match define it (include/flimo_c.h): the bin of one point, the
// normalised form of a descriptor's column, and the distance of two descriptors over every column shift.  float32 throughout, one
// rounding per written operation, nothing contracted; fmaf is written out.  Host AND device: the kernels of flimo_sc.hip and the
// host entries flimo_sc_bin_host / flimo_sc_dist_host run these functions.  tests/sc_common.py restates them in numpy.
//
// The shift: the sector index grows with the angle in the sensor frame, and at shift s query column (j + s) mod sectors meets
// candidate column j, so a query that finds a candidate at shift s is turned by psi_query = psi_candidate - s * 2 pi / sectors.
// The descriptor carries no translation.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "flimo_math.h"

#pragma clang fp contract(off)

namespace flimo {

constexpr int SC_MAX_RINGS = 32, SC_MAX_SECTORS = 64, SC_MAX_K = 8;      // FLIMO_SC_MAX_* (flimo_c.h)
constexpr int SC_SLOTS = 64;                                            // slots of the sum's tree; lanes of a wave

// flimo_sc_cfg with what the host derives from it once
struct ScBinCfg {
  int rings, sectors;
  float min_range, max_range, z_offset;
  float rscale, sscale;      // (float)((double)rings / (double)max_range), (float)((double)sectors / 6.283185307179586)
  int has_frame;
  float frame[12];           // row-major 3 x 4
};

__host__ __device__ inline bool sc_finite(float v) { return v - v == 0.f; }      // (false for NaN and the infinities)

__host__ __device__ inline void sc_scales(ScBinCfg& K) {
  K.rscale = (float)((double)K.rings / (double)K.max_range);
  K.sscale = (float)((double)K.sectors / 6.283185307179586);
}

// The bin of one point: false when it has none.
__host__ __device__ inline bool sc_bin(const ScBinCfg& K, float x, float y, float z, int* ring, int* sector, float* h) {
  float vx = x, vy = y, vz = z;
  if (K.has_frame) {
    const float* F = K.frame;
    vx = F[0] * x + (F[1] * y + (F[2] * z + F[3]));
    vy = F[4] * x + (F[5] * y + (F[6] * z + F[7]));
    vz = F[8] * x + (F[9] * y + (F[10] * z + F[11]));
  }
  if (!sc_finite(vx) || !sc_finite(vy) || !sc_finite(vz)) return false;
  const float r = fl_sqrt(vx * vx + vy * vy);
  if (!(r > 0.f) || !(r >= K.min_range) || !(r < K.max_range)) return false;
  const int ri = (int)(r * K.rscale);
  float a = libm_atan2f(vy, vx);
  if (a < 0.f) a = a + 0x1.921fb6p+2f;
  const int si = (int)(a * K.sscale);
  const float hh = vz + K.z_offset;
  if (!(hh > 0.f)) return false;
  *ring = ri < K.rings - 1 ? ri : K.rings - 1;
  *sector = si < K.sectors - 1 ? si : K.sectors - 1;
  *h = hh;
  return true;
}

// n_j = sqrt(c_R), c_0 = +0, c_{t+1} = fmaf(D[t][j], D[t][j], c_t), rings ascending
__host__ __device__ inline float sc_col_norm(const float* D, int rings, int sectors, int j) {
  float c = 0.f;
  for (int t = 0; t < rings; t++) c = fmaf(D[t * sectors + j], D[t * sectors + j], c);
  return fl_sqrt(c);
}
// one entry of the normalised form: D / n for a valid column, +0 otherwise
__host__ __device__ inline float sc_unit(float v, float n, bool valid) { return valid ? fl_div(v, n) : 0.f; }
// d(s) = 1 - sum / m, a negative result +0
__host__ __device__ inline float sc_shift_dist(float sum, int m) {
  const float d = 1.0f - fl_div(sum, (float)m);
  return d < 0.f ? 0.f : d;
}

// The normalised form of a whole descriptor on the host: u [rings][SC_SLOTS] (+0 beyond sectors), and the valid columns' bits.  A
// descriptor with a non-finite entry is excluded: no valid column, u all +0.
inline uint64_t sc_normalise(const float* D, int rings, int sectors, float* u) {
  bool ok = true;
  for (int e = 0; e < rings * sectors; e++) ok = ok && sc_finite(D[e]);
  uint64_t valid = 0;
  for (int j = 0; j < SC_SLOTS; j++) {
    const float n = (ok && j < sectors) ? sc_col_norm(D, rings, sectors, j) : 0.f;
    const bool v = n > 0.f;
    if (v) valid |= 1ull << j;
    for (int t = 0; t < rings; t++) u[t * SC_SLOTS + j] = j < sectors ? sc_unit(D[t * sectors + j], n, v) : 0.f;
  }
  return valid;
}
// The distance of two descriptors on the host: false when every shift is excluded.  profile [sectors] (may be null): d(s), NaN for
// an excluded shift.
inline bool sc_dist(const float* a, const float* b, int rings, int sectors, int min_cols, float* dist, int* shift, float* profile) {
  float ua[SC_MAX_RINGS * SC_SLOTS], ub[SC_MAX_RINGS * SC_SLOTS];
  const uint64_t va = sc_normalise(a, rings, sectors, ua), vb = sc_normalise(b, rings, sectors, ub);
  bool have = false;
  uint32_t best = 0;
  int best_s = -1;
  for (int s = 0; s < sectors; s++) {
    float term[SC_SLOTS];
    int m = 0;
    for (int j = 0; j < SC_SLOTS; j++) {
      term[j] = 0.f;
      if (j >= sectors) continue;
      const int jq = (j + s) % sectors;
      if (!((va >> jq) & 1) || !((vb >> j) & 1)) continue;
      float c = 0.f;
      for (int t = 0; t < rings; t++) c = fmaf(ua[t * SC_SLOTS + jq], ub[t * SC_SLOTS + j], c);
      term[j] = c;
      m++;
    }
    for (int w = 1; w < SC_SLOTS; w *= 2)
      for (int j = 0; j < SC_SLOTS; j += 2 * w) term[j] = term[j] + term[j + w];
    if (m < min_cols || m == 0) {
      if (profile) profile[s] = __builtin_nanf("");
      continue;
    }
    const float d = sc_shift_dist(term[0], m);
    if (profile) profile[s] = d;
    const uint32_t bits = __builtin_bit_cast(uint32_t, d);
    if (!have || bits < best) { have = true; best = bits; best_s = s; }
  }
  if (have) { *dist = __builtin_bit_cast(float, best); *shift = best_s; }
  return have;
}

}  // namespace flimo
