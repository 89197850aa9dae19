// fast_limo_amd/csrc/hip/flimo_desc.hip -- nearest descriptors (flimo_desc_match, include/flimo_c.h): per query row the first k
// rows of the resident reference set in the order (float32 bits of d, reference index), d as flimo_desc.h forms it.
//
//   desc_norm_kernel   one THREAD per row: the VALU fmaf chain of its norm (desc_norm: NaN for a row with a non-finite entry), and
//                      NaN for the rows that only pad the last tile.  The reference set's run once, in flimo_desc_ref_set.
//   desc_pack_kernel   the reference set in the A-operand layout of v_mfma_f32_32x32x2_f32, once: tile g of 32 rows, K-step s,
//                      lane l holds row 32 g + (l & 31), entry 2 s + (l >> 5) -- zero beyond dim and beyond the last row -- so a
//                      wave's operand of one K-step is ONE coalesced 256-byte load.
//   desc_match_kernel  the hot path.  A workgroup of four waves owns NT tiles of 32 queries (the B operand: the columns, held in
//                      registers for the whole launch) and one split of the reference tiles, which its waves take in turn.  Per
//                      reference tile a wave issues the K-steps in ascending order into NT independent accumulators, zero at the
//                      start -- each element is then the fmaf chain of its pair --, and every lane finishes the 16 rows it holds of
//                      its own column: desc_dist, the key (d bits << 32 | reference index), one compare against the worst of its
//                      sorted list of KL keys, rarely an insertion.  Nothing crosses a lane while the tiles stream by.  At the end
//                      the two lanes of a column merge by a shuffle, the four waves through shared memory, and (split, query)
//                      gets its KL keys in scratch.
//   desc_merge_kernel  one THREAD per query: the splits' lists into one, then idx / dist / cnt.
// The keys are unique (the index is part of them) and every step keeps the smallest by integer compare: the result is the same
// however the references are tiled, split or taken in turn.  No atomics anywhere.
#include <algorithm>
#include "flimo_desc.h"
#include "flimo_kernels.h"

#pragma clang fp contract(off)

namespace flimo {

typedef float desc_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long desc_key;
constexpr desc_key DESC_NONE = ~0ull;      // an empty slot: above every key (a key's high word is at most +inf's bits)

__global__ __launch_bounds__(256) void desc_norm_kernel(const float* __restrict__ x, unsigned n, int dim, float* __restrict__ norm, unsigned npad) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npad) return;
  norm[i] = i < n ? desc_norm(x + (size_t)i * dim, dim) : __builtin_nanf("");
}

__global__ __launch_bounds__(256) void desc_pack_kernel(const float* __restrict__ x, unsigned n, int dim, int sp, float* __restrict__ rt, size_t total) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const unsigned lane = (unsigned)(e & 63);
    const size_t step = e >> 6;
    const int s = (int)(step % (size_t)sp);
    const size_t row = (step / (size_t)sp) * 32 + (lane & 31);
    const int k = 2 * s + (int)(lane >> 5);
    rt[e] = (row < n && k < dim) ? x[row * (size_t)dim + k] : 0.f;
  }
}

template <int KL>
__device__ inline void desc_insert(desc_key (&L)[KL], desc_key key) {
  if (key < L[KL - 1]) {
    L[KL - 1] = key;
#pragma unroll
    for (int j = KL - 1; j > 0; j--)
      if (L[j] < L[j - 1]) { const desc_key t = L[j]; L[j] = L[j - 1]; L[j - 1] = t; }
  }
}

// SP: K-steps of the packed layout (>= ceil(dim / 2); the steps beyond it multiply zeros: fmaf(0, 0, c) = c).  part: [splits][nq][KL].
template <int SP, int NT, int KL>
__global__ __launch_bounds__(256) void desc_match_kernel(const float* __restrict__ rt, const float* __restrict__ rnorm, unsigned ntiles,
                                                         unsigned tiles_per_split, const float* __restrict__ q, const float* __restrict__ qnorm,
                                                         unsigned nq, int dim, desc_key* __restrict__ part) {
  constexpr int QT = 32 * NT;      // queries of a workgroup
  __shared__ desc_key s_keys[4][KL][QT];
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, h = lane >> 5, col = lane & 31u;
  const unsigned qbase = blockIdx.x * (unsigned)QT;
  float bq[NT][SP], qn[NT];
  desc_key L[NT][KL];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const unsigned qi = qbase + 32u * t + col;
#pragma unroll
    for (int s = 0; s < SP; s++) {
      const int k = 2 * s + (int)h;
      bq[t][s] = (qi < nq && k < dim) ? q[(size_t)qi * dim + k] : 0.f;
    }
    qn[t] = qi < nq ? qnorm[qi] : __builtin_nanf("");
#pragma unroll
    for (int j = 0; j < KL; j++) L[t][j] = DESC_NONE;
  }
  const unsigned tile0 = blockIdx.y * tiles_per_split;
  const unsigned tile1 = min(ntiles, tile0 + tiles_per_split);
  for (unsigned tile = tile0 + wave; tile < tile1; tile += 4) {
    const float* p = rt + (size_t)tile * (SP * 64) + lane;
    float a[SP];
#pragma unroll
    for (int s = 0; s < SP; s++) a[s] = p[s * 64];
    desc_f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[t][r] = 0.f;
#pragma unroll
    for (int s = 0; s < SP; s++)
#pragma unroll
      for (int t = 0; t < NT; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bq[t][s], acc[t], 0, 0, 0);
    // register r of a lane is row (r & 3) + 8 (r >> 2) + 4 h of the tile: four runs of four consecutive rows
    const float4* np4 = reinterpret_cast<const float4*>(rnorm + (size_t)tile * 32 + 4 * h);
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const float4 rn4 = np4[2 * g];
      const float rn[4] = {rn4.x, rn4.y, rn4.z, rn4.w};
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const unsigned ref = tile * 32u + 8u * g + 4u * h + (unsigned)e;
#pragma unroll
        for (int t = 0; t < NT; t++) {
          const float d = desc_dist(qn[t], rn[e], acc[t][4 * g + e]);
          if (d == d) desc_insert<KL>(L[t], ((desc_key)__float_as_uint(d) << 32) | ref);
        }
      }
    }
  }
  // the two lanes of a column: the upper one's keys into the lower one's list
#pragma unroll
  for (int t = 0; t < NT; t++) {
    desc_key other[KL];
#pragma unroll
    for (int j = 0; j < KL; j++) {
      const unsigned lo = __shfl_xor((unsigned)(L[t][j] & 0xffffffffull), 32);
      const unsigned hi = __shfl_xor((unsigned)(L[t][j] >> 32), 32);
      other[j] = ((desc_key)hi << 32) | lo;
    }
#pragma unroll
    for (int j = 0; j < KL; j++) desc_insert<KL>(L[t], other[j]);
    if (h == 0) {
#pragma unroll
      for (int j = 0; j < KL; j++) s_keys[wave][j][32 * t + col] = L[t][j];
    }
  }
  __syncthreads();
  if (threadIdx.x < (unsigned)QT && qbase + threadIdx.x < nq) {
    desc_key M[KL];
#pragma unroll
    for (int j = 0; j < KL; j++) M[j] = s_keys[0][j][threadIdx.x];
#pragma unroll
    for (int w = 1; w < 4; w++)
#pragma unroll
      for (int j = 0; j < KL; j++) desc_insert<KL>(M, s_keys[w][j][threadIdx.x]);
    desc_key* out = part + ((size_t)blockIdx.y * nq + (qbase + threadIdx.x)) * KL;
#pragma unroll
    for (int j = 0; j < KL; j++) out[j] = M[j];
  }
}

template <int KL>
__global__ __launch_bounds__(256) void desc_merge_kernel(const desc_key* __restrict__ part, unsigned nsplit, unsigned nq, int k,
                                                         int32_t* __restrict__ idx, float* __restrict__ dist, int32_t* __restrict__ cnt) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  desc_key M[KL];
#pragma unroll
  for (int j = 0; j < KL; j++) M[j] = DESC_NONE;
  for (unsigned sp = 0; sp < nsplit; sp++) {
    const desc_key* in = part + ((size_t)sp * nq + i) * KL;
#pragma unroll
    for (int j = 0; j < KL; j++) desc_insert<KL>(M, in[j]);
  }
  int n = 0;
#pragma unroll
  for (int j = 0; j < KL; j++) {
    if (j < k) {
      const bool have = M[j] != DESC_NONE;
      idx[(size_t)i * k + j] = have ? (int32_t)(M[j] & 0xffffffffull) : -1;
      dist[(size_t)i * k + j] = have ? __uint_as_float((unsigned)(M[j] >> 32)) : 0.f;
      n += have ? 1 : 0;
    }
  }
  cnt[i] = n;
}

int desc_steps(int dim) {
  const int s = (dim + 1) / 2;
  return s <= 4 ? 4 : s <= 8 ? 8 : s <= 17 ? 17 : 32;
}
int desc_query_tile(int dim) { return desc_steps(dim) <= 17 ? 128 : 64; }
int desc_list_len(int k) { return k <= 2 ? 2 : 8; }

hipError_t launch_desc_norms(hipStream_t st, const float* x, unsigned n, int dim, float* norm, unsigned npad) {
  if (npad == 0) return hipSuccess;
  hipLaunchKernelGGL(desc_norm_kernel, dim3((npad + 255u) / 256u), dim3(256), 0, st, x, n, dim, norm, npad);
  return hipGetLastError();
}

hipError_t launch_desc_pack(hipStream_t st, const float* x, unsigned n, int dim, float* rt) {
  const size_t total = (size_t)((n + 31u) / 32u) * (size_t)desc_steps(dim) * 64;
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(desc_pack_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 65536)), dim3(256), 0, st, x, n, dim, desc_steps(dim), rt,
                     total);
  return hipGetLastError();
}

template <int SP, int NT>
static void desc_match_launch(hipStream_t st, const float* rt, const float* rnorm, unsigned ntiles, unsigned tiles_per_split, unsigned nsplit,
                              const float* q, const float* qnorm, unsigned nq, int dim, int k, desc_key* part, int32_t* idx, float* dist, int32_t* cnt) {
  const dim3 grid((nq + 32u * NT - 1u) / (32u * NT), nsplit);
  const dim3 mgrid((nq + 255u) / 256u);
  if (desc_list_len(k) == 2) {
    hipLaunchKernelGGL((desc_match_kernel<SP, NT, 2>), grid, dim3(256), 0, st, rt, rnorm, ntiles, tiles_per_split, q, qnorm, nq, dim, part);
    hipLaunchKernelGGL((desc_merge_kernel<2>), mgrid, dim3(256), 0, st, part, nsplit, nq, k, idx, dist, cnt);
  } else {
    hipLaunchKernelGGL((desc_match_kernel<SP, NT, 8>), grid, dim3(256), 0, st, rt, rnorm, ntiles, tiles_per_split, q, qnorm, nq, dim, part);
    hipLaunchKernelGGL((desc_merge_kernel<8>), mgrid, dim3(256), 0, st, part, nsplit, nq, k, idx, dist, cnt);
  }
}

hipError_t launch_desc_match(hipStream_t st, const float* rt, const float* rnorm, unsigned nr, unsigned tiles_per_split, const float* q,
                             float* qnorm, unsigned nq, int dim, int k, unsigned long long* part, int32_t* idx, float* dist, int32_t* cnt) {
  if (nq == 0 || nr == 0) return hipSuccess;
  const unsigned ntiles = (nr + 31u) / 32u;
  const unsigned nsplit = (ntiles + tiles_per_split - 1u) / tiles_per_split;
  hipError_t e = launch_desc_norms(st, q, nq, dim, qnorm, nq);
  if (e != hipSuccess) return e;
  switch (desc_steps(dim)) {
    case 4: desc_match_launch<4, 4>(st, rt, rnorm, ntiles, tiles_per_split, nsplit, q, qnorm, nq, dim, k, part, idx, dist, cnt); break;
    case 8: desc_match_launch<8, 4>(st, rt, rnorm, ntiles, tiles_per_split, nsplit, q, qnorm, nq, dim, k, part, idx, dist, cnt); break;
    case 17: desc_match_launch<17, 4>(st, rt, rnorm, ntiles, tiles_per_split, nsplit, q, qnorm, nq, dim, k, part, idx, dist, cnt); break;
    default: desc_match_launch<32, 2>(st, rt, rnorm, ntiles, tiles_per_split, nsplit, q, qnorm, nq, dim, k, part, idx, dist, cnt); break;
  }
  return hipGetLastError();
}

}  // namespace flimo
