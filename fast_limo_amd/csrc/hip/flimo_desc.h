// fast_limo_amd/csrc/hip/flimo_desc.h
// The distance of two descriptor rows as flimo_desc_match defines it (include/flimo_c.h): float32 throughout, one rounding per
// written operation, the dot product a chain of correctly rounded fused multiply-adds in ascending index order.  Host AND device:
// the norm kernel (flimo_desc.hip) and flimo_desc_dist_host run these functions; the match kernel forms its dot products on
// v_mfma_f32_32x32x2_f32, whose result is this chain bit for bit, and finishes them with desc_dist.  fmaf is written out, so the
// build's -ffp-contract=off has nothing to say about it; the sum and the difference of desc_dist are never contracted.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#pragma clang fp contract(off)

namespace flimo {

constexpr int DESC_MAX_DIM = 64, DESC_MAX_K = 8;      // FLIMO_DESC_MAX_DIM / FLIMO_DESC_MAX_K (flimo_c.h)

// c_0 = +0, c_{t+1} = fmaf(a[t], b[t], c_t), t ascending
__host__ __device__ inline float desc_dot(const float* a, const float* b, int dim) {
  float c = 0.f;
  for (int t = 0; t < dim; t++) c = fmaf(a[t], b[t], c);
  return c;
}
__host__ __device__ inline bool desc_finite(float v) { return v - v == 0.f; }      // (false for NaN and the infinities)
// n(a) = dot(a, a); NaN for a row with a non-finite entry -- an excluded row: every distance to it comes out NaN (a row of finite
// entries has a norm >= 0 or +inf, never NaN)
__host__ __device__ inline float desc_norm(const float* a, int dim) {
  bool ok = true;
  for (int t = 0; t < dim; t++) ok = ok && desc_finite(a[t]);
  return ok ? desc_dot(a, a, dim) : __builtin_nanf("");
}
// d = (n(q) + n(r)) - 2 dot, a negative result +0; NaN stays NaN (the pair is excluded)
__host__ __device__ inline float desc_dist(float nq, float nr, float dot) {
  const float t = nq + nr;
  const float d = t - (dot + dot);
  return d < 0.f ? 0.f : d;
}

}  // namespace flimo
