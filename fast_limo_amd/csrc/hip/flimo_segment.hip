// fast_limo_amd/csrc/hip/flimo_segment.hip  -- gfx950 (MI355X) only.
//
// The move of flimo_map_correct / flimo_map_transform / flimo_map_corrected (include/flimo_c.h, "Map segments"): one pass over the
// stored points in insertion order that writes every point moved by its segment's matrix (flimo_segment.h: seg_find, seg_move)
// and leaves, for the host, how many points changed bits, how many moved components are not finite, and the moved points' box.
//
// A workgroup takes slabs of consecutive points; each of its four waves a quarter of the slab, 64 consecutive points (1 KiB, one
// 16-byte load and one 16-byte store a lane) per step.  A wave's quarter lies in one segment almost always: the wave looks up the
// segment of its first and of its last point (the same address in every lane: scalar loads), and when they agree the twelve
// matrix entries are wave-uniform and stay in scalar registers.  Where they differ each lane searches between the two.  Both ways
// run seg_move on the same numbers, so the result depends on neither the slab, the grid nor the table's length.
// Counts: one integer atomic per wave and launch each; box: integer min / max over the ordered bits of the floats, per wave.  No
// floating-point atomic, no LDS, no scratch.
#include <hip/hip_runtime.h>
#include <float.h>
#include <string.h>
#include <algorithm>
#include "../../../include/flimo_c.h"
#include "flimo_segment.h"

namespace flimo {

// order-preserving float -> uint mapping for atomic min / max (flimo_map.hip reads the words back)
__device__ __forceinline__ unsigned seg_f2o(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static inline float seg_o2f_host(unsigned o) {
  const unsigned u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

struct SegAcc {      // what a lane gathers over the launch
  float mn[3], mx[3];
  uint32_t changed, bad;      // wave-uniform: sums of ballots
};

// one point: load, move by m, store, account
__device__ __forceinline__ void seg_point(const float4* __restrict__ in, float4* __restrict__ out, uint32_t first, uint32_t i, const double* m,
                                          bool* chg, bool* bad, SegAcc& A) {
  const float4 p = in[i];
  float q[3];
  seg_move(m, p.x, p.y, p.z, q);
  if (out) out[i - first] = make_float4(q[0], q[1], q[2], __uint_as_float(i));
  *chg = (__float_as_uint(q[0]) != __float_as_uint(p.x)) | (__float_as_uint(q[1]) != __float_as_uint(p.y)) |
         (__float_as_uint(q[2]) != __float_as_uint(p.z));
  *bad = !(isfinite(q[0]) & isfinite(q[1]) & isfinite(q[2]));
#pragma unroll
  for (int a = 0; a < 3; a++) { A.mn[a] = fminf(A.mn[a], q[a]); A.mx[a] = fmaxf(A.mx[a], q[a]); }
}

__global__ __launch_bounds__(256) void seg_move_kernel(const float4* __restrict__ in, uint32_t first, uint32_t n,
                                                       const uint64_t* __restrict__ begin, const double* __restrict__ T, uint32_t S,
                                                       float4* __restrict__ out, uint32_t rows, uint32_t nslabs,
                                                       uint32_t* __restrict__ cnt, unsigned* __restrict__ box) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t per_wave = rows * 64u, slab = per_wave * 4u;
  const uint32_t end = first + n;                                   // (< 2^31: seg_move_launch)
  SegAcc A{{FLT_MAX, FLT_MAX, FLT_MAX}, {-FLT_MAX, -FLT_MAX, -FLT_MAX}, 0u, 0u};
  for (uint32_t sl = blockIdx.x; sl < nslabs; sl += gridDim.x) {
    const uint32_t w0 = first + sl * slab + wave * per_wave;        // the wave's first point ...
    if (w0 >= end) continue;
    const uint32_t w1 = min(w0 + per_wave, end) - 1u;               // ... and its last
    const uint32_t s0 = seg_find(begin, S, w0), s1 = seg_find(begin, S, w1);
    if (s0 == s1) {
      double m[12];
#pragma unroll
      for (int k = 0; k < 12; k++) m[k] = T[(size_t)s0 * 12u + k];
      for (uint32_t r = 0; r < rows; r++) {
        const uint32_t i = w0 + r * 64u + lane;
        bool chg = false, bad = false;
        if (i <= w1) seg_point(in, out, first, i, m, &chg, &bad, A);
        A.changed += (uint32_t)__popcll(__ballot(chg));
        A.bad += (uint32_t)__popcll(__ballot(bad));
      }
    } else {
      for (uint32_t r = 0; r < rows; r++) {
        const uint32_t i = w0 + r * 64u + lane;
        bool chg = false, bad = false;
        if (i <= w1) {
          const uint32_t s = s0 + seg_find(begin + s0, s1 - s0 + 1u, i);      // (begin[s0] <= w0 <= i <= w1 < begin[s1 + 1])
          double m[12];
#pragma unroll
          for (int k = 0; k < 12; k++) m[k] = T[(size_t)s * 12u + k];
          seg_point(in, out, first, i, m, &chg, &bad, A);
        }
        A.changed += (uint32_t)__popcll(__ballot(chg));
        A.bad += (uint32_t)__popcll(__ballot(bad));
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      A.mn[a] = fminf(A.mn[a], __shfl_xor(A.mn[a], off, 64));
      A.mx[a] = fmaxf(A.mx[a], __shfl_xor(A.mx[a], off, 64));
    }
  }
  if (lane == 0u) {
    if (A.changed) atomicAdd(&cnt[0], A.changed);
    if (A.bad) atomicAdd(&cnt[1], A.bad);
    if (A.mn[0] <= A.mx[0] || A.mn[1] <= A.mx[1] || A.mn[2] <= A.mx[2]) {      // (a wave without a point leaves the box alone)
#pragma unroll
      for (int a = 0; a < 3; a++) {
        atomicMin(&box[a], seg_f2o(A.mn[a]));
        atomicMax(&box[3 + a], seg_f2o(A.mx[a]));
      }
    }
  }
}

hipError_t seg_move_launch(hipStream_t st, const float4* in, size_t first, size_t n, const uint64_t* d_begin, const double* d_T, uint32_t S,
                           float4* out, size_t slab, int blocks, MapBuildScratch& scratch, size_t* changed, size_t* nonfinite, float bb[6]) {
  *changed = *nonfinite = 0;
  if (n == 0) return hipSuccess;
  if (first + n > 0x7fffffffull || S == 0u || slab < 256 || slab > SEG_SLAB_MAX || slab % 256 != 0) return hipErrorInvalidValue;
  hipError_t e = ensure_mail(scratch);
  if (e != hipSuccess) return e;
  if (!scratch.seg_cnt) {
    if ((e = hipMalloc(&scratch.seg_cnt, 2 * sizeof(uint32_t))) != hipSuccess) return e;
    if ((e = hipMemset(scratch.seg_cnt, 0, 2 * sizeof(uint32_t))) != hipSuccess) return e;
  }
  const size_t nslabs = (n + slab - 1) / slab;
  const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>(nslabs, (size_t)std::max(blocks, 1)));
  hipLaunchKernelGGL(seg_move_kernel, dim3(grid), dim3(256), 0, st, in, (uint32_t)first, (uint32_t)n, d_begin, d_T, S, out,
                     (uint32_t)(slab / 256), (uint32_t)nslabs, scratch.seg_cnt, (unsigned*)scratch.bbox);
  e = hipGetLastError();
  const MailPart parts[2] = {{scratch.seg_cnt, 2, MAIL_SEG}, {scratch.bbox, 6, MAIL_BBOX}};
  if (e == hipSuccess) e = mail_words(st, scratch, parts, 2, true, scratch.seg_cnt, 2);      // (box re-armed, counts zeroed behind the copy)
  if (e == hipSuccess) e = mail_wait(st, scratch);
  if (e != hipSuccess) {
    // the re-arming rode on the mail kernel that did not run: put the empty box and the zero counts back by hand
    const unsigned init[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
    (void)hipMemcpy(scratch.bbox, init, sizeof(init), hipMemcpyHostToDevice);
    (void)hipMemset(scratch.seg_cnt, 0, 2 * sizeof(uint32_t));
    return e;
  }
  *changed = (size_t)scratch.mail_host[MAIL_SEG];
  *nonfinite = (size_t)scratch.mail_host[MAIL_SEG + 1];
  for (int i = 0; i < 6; i++) bb[i] = seg_o2f_host(scratch.mail_host[MAIL_BBOX + i]);
  return hipSuccess;
}

}  // namespace flimo

extern "C" int flimo_seg_move_host(const double T[12], const float p[3], float out[3]) {
  if (!T || !p || !out) return FLIMO_ERR_INVALID;
  flimo::seg_move(T, p[0], p[1], p[2], out);
  return FLIMO_OK;
}
