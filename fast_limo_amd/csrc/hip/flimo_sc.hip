// fast_limo_amd/csrc/hip/flimo_sc.hip -- Scan Context place recognition (flimo_scan_context, flimo_sc_db_*, flimo_sc_match;
// include/flimo_c.h), every number as flimo_sc.h forms it.
//
//   sc_desc_kernel     the descriptor of the resident scan, behind a zeroing of desc and used.  A workgroup keeps a private image of
//                      rings x sectors ints in LDS (8 KB at most), takes its points with sc_bin and an LDS atomicMax over the bits of
//                      h (h > 0: bit order is value order), and at the end flushes its non-zero bins with a global integer atomicMax.
//                      used: one ballot per wave and step, one integer atomicAdd per wave.  No floating-point atomics.
//   sc_norm_kernel     one WAVE per descriptor, lane j = column j: the normalised form u [rings][64] (+0 beyond sectors, for an
//                      invalid column and for an excluded descriptor) and the bits of the valid columns.  Run at add time over the
//                      new entries and per chunk over the queries.
//   sc_match_kernel    the hot path, on the VALU.  A workgroup of four waves owns a tile of SC_QT queries, whose normalised rows sit
//                      in LDS [ring][column], the columns written twice in a row of 128 (so that column (j + s) mod sectors is
//                      element j + s) and the whole image a second time moved by one element (so that an odd lane's pair of
//                      elements is 8-byte aligned like an even lane's): ONE ds_read_b64 serves two shifts.  A wave takes SC_NC
//                      candidates at a time.  Lane j holds, per candidate, the 64 accumulators of its column's term at every
//                      shift; ring by ring it loads its candidate entries u[t][j] (one coalesced row, fetched one ring ahead) and
//                      issues 64 x SC_NC fmaf on 32 LDS reads -- every accumulator is the ascending chain of its (column, shift).
//                      The sums over the columns in the prescribed tree are a transposing butterfly: level l adds lanes j and
//                      j ^ 2^l, and each lane keeps the half of the shifts its bit l names, 63 exchanges for all 64 shifts (the first
//                      two levels by DPP); lane j ends with the sum of shift bitreverse6(j), counts m(s) from the two valid masks,
//                      forms d(s), and a wave minimum of (bits of d << 6 | s) is the pair's distance and shift.  Lane q of a wave
//                      keeps query q's list of the SC_KL smallest keys (bits of dist << 32 | id) with the shifts beside them; the
//                      four waves merge through LDS into (split, query)'s list.
//   sc_merge_kernel    one THREAD per query: the splits' lists into one, then idx / dist / shift / cnt.
//   sc_profile_kernel  one WAVE per returned pair: d(s) of every shift, NaN where excluded; NaN rows beyond cnt.
// The keys are unique and every step keeps the smallest by integer compare: the result is the same however the entries are split
// or taken in turn.
#include <algorithm>
#include "flimo_sc.h"
#include "flimo_kernels.h"

#pragma clang fp contract(off)

namespace flimo {

typedef unsigned long long sc_key;
constexpr sc_key SC_NONE = ~0ull;
constexpr int SC_QT = 2, SC_NC = 2, SC_KL = SC_MAX_K;

__global__ __launch_bounds__(256) void sc_desc_kernel(const float4* __restrict__ scan, unsigned n, ScBinCfg K, int* __restrict__ desc,
                                                      int* __restrict__ used) {
  __shared__ int s_img[SC_MAX_RINGS * SC_MAX_SECTORS];
  const int nb = K.rings * K.sectors;
  for (int i = threadIdx.x; i < nb; i += 256) s_img[i] = 0;
  __syncthreads();
  unsigned mine = 0;      // (lane 0 of each wave counts)
  for (size_t base = (size_t)blockIdx.x * 256; base < n; base += (size_t)gridDim.x * 256) {
    const size_t i = base + threadIdx.x;
    bool has = false;
    if (i < n) {
      const float4 p = scan[i];
      int ring, sector;
      float h;
      has = sc_bin(K, p.x, p.y, p.z, &ring, &sector, &h);
      if (has) atomicMax(&s_img[ring * K.sectors + sector], __float_as_int(h));
    }
    mine += (unsigned)__popcll(__ballot(has));
  }
  if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(used, (int)mine);
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += 256) {
    const int v = s_img[i];
    if (v) atomicMax(&desc[i], v);
  }
}

__global__ __launch_bounds__(256) void sc_norm_kernel(const float* __restrict__ raw, unsigned n, int rings, int sectors, float* __restrict__ un,
                                                      sc_key* __restrict__ valid) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned e = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (e >= n) return;
  const float* D = raw + (size_t)e * rings * sectors;
  bool fin = true;
  for (int i = (int)lane; i < rings * sectors; i += 64) fin = fin && sc_finite(D[i]);
  const bool ok = __ballot(!fin) == 0ull;
  const bool col = (int)lane < sectors;
  const float nj = (ok && col) ? sc_col_norm(D, rings, sectors, (int)lane) : 0.f;
  const bool v = nj > 0.f;
  const sc_key mask = __ballot(v);
  if (lane == 0) valid[e] = mask;
  float* u = un + (size_t)e * rings * SC_SLOTS + lane;
  for (int t = 0; t < rings; t++) u[t * SC_SLOTS] = col ? sc_unit(D[t * sectors + lane], nj, v) : 0.f;
}

__device__ __forceinline__ float sc_dpp_xor1(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));      // quad_perm [1, 0, 3, 2]
}
__device__ __forceinline__ float sc_dpp_xor2(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));      // quad_perm [2, 3, 0, 1]
}
__device__ __forceinline__ unsigned sc_brev6(unsigned lane) { return __brev(lane) >> 26; }

// The column sums of all 64 shifts at once: a [s] is this lane's term at shift s; returns the tree's sum of shift bitreverse6(lane).
// Level l pairs lanes j and j ^ 2^l -- the tree ((t0 + t1) + (t2 + t3)) + ... over the slots -- and leaves each lane the half of the
// remaining shifts that its bit l names.  An addition is commutative bit for bit, so both lanes of a pair form the same sum.
__device__ __forceinline__ float sc_butterfly(float (&a)[SC_SLOTS], unsigned lane) {
  {
    const bool up = lane & 1u;
#pragma unroll
    for (int i = 0; i < 32; i++) {
      const float x = a[i] + sc_dpp_xor1(a[i]), y = a[i + 32] + sc_dpp_xor1(a[i + 32]);
      a[i] = up ? y : x;
    }
  }
  {
    const bool up = lane & 2u;
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const float x = a[i] + sc_dpp_xor2(a[i]), y = a[i + 16] + sc_dpp_xor2(a[i + 16]);
      a[i] = up ? y : x;
    }
  }
#pragma unroll
  for (int l = 2; l < 6; l++) {
    const int nn = 32 >> l;
    const bool up = (lane >> l) & 1u;
#pragma unroll
    for (int i = 0; i < nn; i++) {      // (both sums, then the choice: a choice between two ELEMENTS would index the array by lane)
      const float x = a[i] + __shfl_xor(a[i], 1 << l), y = a[i + nn] + __shfl_xor(a[i + nn], 1 << l);
      a[i] = up ? y : x;
    }
  }
  return a[0];
}

// (bits of d(s) << 6 | s) of this lane's shift, SC_NONE when the shift is excluded.  cv / qv: the valid columns of the candidate and
// of the query; query column (j + s) mod sectors meets candidate column j.
__device__ __forceinline__ sc_key sc_shift_key(float sum, sc_key cv, sc_key qv, int s, int sectors, int min_cols) {
  if (s >= sectors) return SC_NONE;
  const sc_key qrot = s == 0 ? qv : ((qv >> s) | (qv << (sectors - s)));
  const int m = __popcll(cv & qrot);
  if (m < min_cols || m == 0) return SC_NONE;
  return ((sc_key)__float_as_uint(sc_shift_dist(sum, m)) << 6) | (sc_key)s;
}
__device__ __forceinline__ sc_key sc_shfl_xor_key(sc_key v, int mask) {
  const unsigned lo = __shfl_xor((unsigned)(v & 0xffffffffull), mask), hi = __shfl_xor((unsigned)(v >> 32), mask);
  return ((sc_key)hi << 32) | lo;
}
__device__ __forceinline__ sc_key sc_wave_min(sc_key v) {
#pragma unroll
  for (int mask = 32; mask > 0; mask >>= 1) {
    const sc_key o = sc_shfl_xor_key(v, mask);
    v = o < v ? o : v;
  }
  return v;
}

__device__ __forceinline__ void sc_insert(sc_key (&L)[SC_KL], int (&S)[SC_KL], sc_key key, int shift) {
  if (key < L[SC_KL - 1]) {
    L[SC_KL - 1] = key;
    S[SC_KL - 1] = shift;
#pragma unroll
    for (int j = SC_KL - 1; j > 0; j--)
      if (L[j] < L[j - 1]) {
        const sc_key t = L[j]; L[j] = L[j - 1]; L[j - 1] = t;
        const int u = S[j]; S[j] = S[j - 1]; S[j - 1] = u;
      }
  }
}
// the pair's (bits of d << 6 | s) into the list, when there is one and it is below the gate
__device__ __forceinline__ void sc_take(sc_key (&L)[SC_KL], int (&S)[SC_KL], sc_key pair, unsigned id, float max_dist) {
  if (pair == SC_NONE) return;
  const unsigned bits = (unsigned)(pair >> 6);
  if (!(__uint_as_float(bits) < max_dist)) return;
  sc_insert(L, S, ((sc_key)bits << 32) | id, (int)(pair & 63ull));
}

struct ScMatchArgs {
  const float* un;          // the database's normalised rows [size][rings][64]
  const sc_key* valid;      // [size]
  const float* qun;         // the chunk's queries, the same form
  const sc_key* qvalid;
  unsigned nq, e_first, e_end, per_split;
  int rings, sectors, min_cols;
  float max_dist;
  sc_key* part;             // [splits][nq][SC_KL]
  int* part_shift;
};

// floats of one query's image in LDS: rows of 128 for the image, 32 of room (the two copies then sit on different banks), the image
// moved by one element
__host__ __device__ inline int sc_query_floats(int rings) { return rings * 256 + 32; }

__global__ __launch_bounds__(256) void sc_match_kernel(ScMatchArgs A) {
  extern __shared__ float4 s_q4[];
  __shared__ sc_key s_keys[4][SC_QT][SC_KL];
  __shared__ int s_shift[4][SC_QT][SC_KL];
  float* s_q = reinterpret_cast<float*>(s_q4);
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const int rings = A.rings, sectors = A.sectors;
  const int qs = sc_query_floats(rings), moved = rings * 128 + 32;
  const unsigned qbase = blockIdx.x * (unsigned)SC_QT;
  for (int qi = 0; qi < SC_QT; qi++) {
    if (qbase + qi >= A.nq) break;
    const float* u = A.qun + (size_t)(qbase + qi) * rings * SC_SLOTS;
    float* img = s_q + qi * qs;
    for (int e = threadIdx.x; e < rings * 128; e += 256) {
      const int t = e >> 7, c = e & 127;
      img[e] = c < 2 * sectors ? u[t * SC_SLOTS + c % sectors] : 0.f;
      img[moved + e] = c + 1 < 2 * sectors ? u[t * SC_SLOTS + (c + 1) % sectors] : 0.f;
    }
  }
  __syncthreads();
  sc_key L[SC_KL];
  int S[SC_KL];
#pragma unroll
  for (int j = 0; j < SC_KL; j++) { L[j] = SC_NONE; S[j] = -1; }
  const unsigned e_lo = A.e_first + blockIdx.y * A.per_split;
  const unsigned e_hi = min(A.e_end, e_lo + A.per_split);
  const int s_mine = (int)sc_brev6(lane);
  const int lane_off = (lane & 1u) ? moved + (int)lane - 1 : (int)lane;
  for (unsigned e0 = e_lo + wave * SC_NC; e0 < e_hi; e0 += 4 * SC_NC) {
    const bool two = e0 + 1 < e_hi;
    const unsigned e1 = two ? e0 + 1 : e0;
    const sc_key cv0 = A.valid[e0], cv1 = A.valid[e1];
    const float* p0 = A.un + (size_t)e0 * rings * SC_SLOTS + lane;
    const float* p1 = A.un + (size_t)e1 * rings * SC_SLOTS + lane;
    for (int qi = 0; qi < SC_QT; qi++) {
      if (qbase + qi >= A.nq) break;
      float a0[SC_SLOTS], a1[SC_SLOTS];
#pragma unroll
      for (int s = 0; s < SC_SLOTS; s++) { a0[s] = 0.f; a1[s] = 0.f; }
      const float* row = s_q + qi * qs + lane_off;
      float c0 = p0[0], c1 = p1[0];
      for (int t = 0; t < rings; t++) {
        const int tn = t + 1 < rings ? t + 1 : t;
        const float n0 = p0[tn * SC_SLOTS], n1 = p1[tn * SC_SLOTS];
#pragma unroll
        for (int s = 0; s < SC_SLOTS; s += 2) {
          const float2 v = *reinterpret_cast<const float2*>(row + s);
          a0[s] = fmaf(v.x, c0, a0[s]);
          a0[s + 1] = fmaf(v.y, c0, a0[s + 1]);
          a1[s] = fmaf(v.x, c1, a1[s]);
          a1[s + 1] = fmaf(v.y, c1, a1[s + 1]);
        }
        row += 128;
        c0 = n0;
        c1 = n1;
      }
      const sc_key qv = A.qvalid[qbase + qi];
      const sc_key k0 = sc_wave_min(sc_shift_key(sc_butterfly(a0, lane), cv0, qv, s_mine, sectors, A.min_cols));
      const sc_key k1 = sc_wave_min(sc_shift_key(sc_butterfly(a1, lane), cv1, qv, s_mine, sectors, A.min_cols));
      if (lane == (unsigned)qi) {
        sc_take(L, S, k0, e0, A.max_dist);
        if (two) sc_take(L, S, k1, e1, A.max_dist);
      }
    }
  }
  if (lane < (unsigned)SC_QT) {
#pragma unroll
    for (int j = 0; j < SC_KL; j++) { s_keys[wave][lane][j] = L[j]; s_shift[wave][lane][j] = S[j]; }
  }
  __syncthreads();
  if (threadIdx.x < (unsigned)SC_QT && qbase + threadIdx.x < A.nq) {
    sc_key M[SC_KL];
    int MS[SC_KL];
#pragma unroll
    for (int j = 0; j < SC_KL; j++) { M[j] = s_keys[0][threadIdx.x][j]; MS[j] = s_shift[0][threadIdx.x][j]; }
#pragma unroll
    for (int w = 1; w < 4; w++)
#pragma unroll
      for (int j = 0; j < SC_KL; j++) sc_insert(M, MS, s_keys[w][threadIdx.x][j], s_shift[w][threadIdx.x][j]);
    const size_t o = ((size_t)blockIdx.y * A.nq + (qbase + threadIdx.x)) * SC_KL;
#pragma unroll
    for (int j = 0; j < SC_KL; j++) { A.part[o + j] = M[j]; A.part_shift[o + j] = MS[j]; }
  }
}

__global__ __launch_bounds__(256) void sc_merge_kernel(const sc_key* __restrict__ part, const int* __restrict__ part_shift, unsigned nsplit,
                                                       unsigned nq, int k, int32_t* __restrict__ idx, float* __restrict__ dist,
                                                       int32_t* __restrict__ shift, int32_t* __restrict__ cnt) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  sc_key M[SC_KL];
  int MS[SC_KL];
#pragma unroll
  for (int j = 0; j < SC_KL; j++) { M[j] = SC_NONE; MS[j] = -1; }
  for (unsigned sp = 0; sp < nsplit; sp++) {
    const size_t o = ((size_t)sp * nq + i) * SC_KL;
#pragma unroll
    for (int j = 0; j < SC_KL; j++) sc_insert(M, MS, part[o + j], part_shift[o + j]);
  }
  int n = 0;
#pragma unroll
  for (int j = 0; j < SC_KL; j++) {
    if (j < k) {
      const bool have = M[j] != SC_NONE;
      idx[(size_t)i * k + j] = have ? (int32_t)(M[j] & 0xffffffffull) : -1;
      dist[(size_t)i * k + j] = have ? __uint_as_float((unsigned)(M[j] >> 32)) : 0.f;
      shift[(size_t)i * k + j] = have ? MS[j] : -1;
      n += have ? 1 : 0;
    }
  }
  cnt[i] = n;
}

// one wave per (query, slot): lane j = candidate column j, the shifts one after another
__global__ __launch_bounds__(256) void sc_profile_kernel(const float* __restrict__ un, const sc_key* __restrict__ valid, const float* __restrict__ qun,
                                                         const sc_key* __restrict__ qvalid, const int32_t* __restrict__ idx, unsigned npairs, int k,
                                                         int rings, int sectors, int min_cols, float* __restrict__ profile) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned pair = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (pair >= npairs) return;
  float* out = profile + (size_t)pair * sectors;
  const int32_t e = idx[pair];
  if (e < 0) {
    if ((int)lane < sectors) out[lane] = __builtin_nanf("");
    return;
  }
  const unsigned q = pair / (unsigned)k;
  const float* uc = un + (size_t)e * rings * SC_SLOTS + lane;
  const float* uq = qun + (size_t)q * rings * SC_SLOTS;
  const sc_key cv = valid[e], qv = qvalid[q];
  for (int s = 0; s < sectors; s++) {
    const int jq = (int)((lane + (unsigned)s) % (unsigned)sectors);
    float c = 0.f;
    for (int t = 0; t < rings; t++) c = fmaf(uq[t * SC_SLOTS + jq], uc[t * SC_SLOTS], c);
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) c = c + __shfl_xor(c, mask);
    const sc_key key = sc_shift_key(c, cv, qv, s, sectors, min_cols);
    if (lane == 0) out[s] = key == SC_NONE ? __builtin_nanf("") : __uint_as_float((unsigned)(key >> 6));
  }
}

int sc_query_tile() { return SC_QT; }
int sc_list_len() { return SC_KL; }

hipError_t launch_sc_descriptor(hipStream_t st, const float4* scan, unsigned n, const ScBinCfg& K, float* desc, int* used) {
  hipError_t e = hipMemsetAsync(desc, 0, (size_t)K.rings * K.sectors * sizeof(float), st);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(used, 0, sizeof(int), st);
  if (e != hipSuccess || n == 0) return e;
  const unsigned blocks = std::min<unsigned>((n + 255u) / 256u, 1024u);
  hipLaunchKernelGGL(sc_desc_kernel, dim3(blocks), dim3(256), 0, st, scan, n, K, reinterpret_cast<int*>(desc), used);
  return hipGetLastError();
}

hipError_t launch_sc_norms(hipStream_t st, const float* raw, unsigned n, int rings, int sectors, float* un, unsigned long long* valid) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(sc_norm_kernel, dim3((n + 3u) / 4u), dim3(256), 0, st, raw, n, rings, sectors, un, valid);
  return hipGetLastError();
}

hipError_t launch_sc_match(hipStream_t st, const float* un, const unsigned long long* valid, unsigned e_first, unsigned e_end, unsigned per_split,
                           const float* qun, const unsigned long long* qvalid, unsigned nq, int rings, int sectors, int k, int min_cols,
                           float max_dist, unsigned long long* part, int* part_shift, int32_t* idx, float* dist, int32_t* shift, int32_t* cnt,
                           float* profile) {
  if (nq == 0 || e_end <= e_first) return hipSuccess;
  const unsigned nsplit = (e_end - e_first + per_split - 1u) / per_split;
  const size_t lds = (size_t)SC_QT * sc_query_floats(rings) * sizeof(float);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sc_match_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  const ScMatchArgs A{un, valid, qun, qvalid, nq, e_first, e_end, per_split, rings, sectors, min_cols, max_dist, part, part_shift};
  hipLaunchKernelGGL(sc_match_kernel, dim3((nq + SC_QT - 1u) / SC_QT, nsplit), dim3(256), lds, st, A);
  hipLaunchKernelGGL(sc_merge_kernel, dim3((nq + 255u) / 256u), dim3(256), 0, st, part, part_shift, nsplit, nq, k, idx, dist, shift, cnt);
  if (profile) {
    const unsigned npairs = nq * (unsigned)k;
    hipLaunchKernelGGL(sc_profile_kernel, dim3((npairs + 3u) / 4u), dim3(256), 0, st, un, valid, qun, qvalid, idx, npairs, k, rings, sectors, min_cols,
                       profile);
  }
  return hipGetLastError();
}

}  // namespace flimo
