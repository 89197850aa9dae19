// fast_limo_amd/csrc/hip/flimo_unionfind.h -- the lock-free union-find of the component kernels, shared by flimo_cluster.hip
// (Euclidean clusters) and flimo_region.hip (smooth-surface regions).  Device only; private to the two files.
//
// parent[x] <= x always, with equality exactly at a root: only two kinds of write exist,
//  * the hook: compare-and-swap of a ROOT's word from itself to a smaller index of the other tree.  It alone changes which points
//    belong together, and it succeeds only on a word that still is a root;
//  * path halving inside a find: an atomic minimum of parent[x] with an index that was an ancestor of x when it was read.  Trees
//    only merge, so it still is one; the word only decreases.
// Indices fall strictly along every path, so there is no cycle, and a tree's root is its smallest index.  Every access to `parent`
// in a link launch is a relaxed agent-scope atomic: the XCDs' L2s are not coherent and a CU's L1 is not refreshed by another CU's
// stores, so a plain load could return a line cached before the launch for ever.  A stale (older) value is still a valid ancestor:
// it costs a step, never a wrong label.  Nothing waits for another workgroup: a compare-and-swap fails only because another one
// succeeded, and the loop goes on from the value it returned.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace flimo {

typedef __attribute__((address_space(1))) uint32_t cl_gu32;
#define CL_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ uint32_t cl_load(cl_gu32* parent, uint32_t x) { return __hip_atomic_load(parent + x, CL_RLX_AGENT); }

// the root of x's tree as far as this lane can see (a root that is hooked a moment later is the caller's business: the CAS tells).
// Path halving: x's word is lowered to its grandparent where it has one -- no write where the path is already short.
__device__ __forceinline__ uint32_t cl_find(cl_gu32* parent, uint32_t x) {
  uint32_t p = cl_load(parent, x);
  while (p != x) {
    const uint32_t gp = cl_load(parent, p);
    if (gp == p) return p;
    __hip_atomic_fetch_min(parent + x, gp, CL_RLX_AGENT);
    x = gp;
    p = cl_load(parent, x);
  }
  return x;
}

// unites the trees of u and a; `a` stands for the group's own point t (any index of t's tree: the root found last time).  Returns
// the root both are under now as far as this lane saw it -- the next call's `a`.
__device__ __forceinline__ uint32_t cl_unite(cl_gu32* parent, uint32_t u, uint32_t a) {
  uint32_t ru = cl_find(parent, u), ra = cl_find(parent, a);
  while (ru != ra) {      // (equal roots -- almost every edge after a point's first few -- end here without a write)
    const uint32_t hi = max(ru, ra), lo = min(ru, ra);
    uint32_t seen = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, CL_RLX_AGENT)) return lo;
    // hi was hooked by somebody else in the meantime: go on from where it hangs now
    ru = cl_find(parent, seen);
    ra = cl_find(parent, lo);
  }
  return ra;
}

}  // namespace flimo
