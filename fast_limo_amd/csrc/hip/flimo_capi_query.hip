// fast_limo_amd/csrc/hip/flimo_capi_query.hip -- C ABI (include/flimo_c.h) over the gfx950 kernels: the analysis entries.
//
// The call-at-a-time entries over the stored map (k-NN, radius search, normals, outliers, FPFH, keypoints, clusters, planes, voxels,
// regions) and over the resident scan, correspondences and descriptors (scan fitness / linearize / NDT / GICP, flimo_corr_*, flimo_desc_*, Scan Context).  Each
// is glue of one shape: check the arguments, take a DevScratch, launch in chunks, copy back, wait once.  The registration path --
// context, map index, sweep front end, the passes and the chain -- is flimo_capi.hip, which also defines the three functions these
// entries call into it (ensure_index, flush_deskew, map_remove_masked); struct flimo_ctx and the shared helpers are flimo_ctx.h.
// This file reads no environment variable (the library's are listed in flimo_capi.hip).
#include <string.h>
#include <math.h>
#include <limits>
#include "flimo_ctx.h"
#include "flimo_math.h"
#include "flimo_pose.h"
#include "flimo_corr.h"
#include "flimo_plane.h"
#include "flimo_voxel.h"
#include "flimo_region.h"
#include "flimo_desc.h"
#include "flimo_sc.h"
#include "flimo_ndt.h"
#include "flimo_gicp.h"
#include "flimo_sums.h"

#pragma clang fp contract(off)

// ---- what the query entries share ----------------------------------------------------------------
// the distance gate of the k-NN entries; what: the caller's name in the message
static int check_gate(flimo_ctx* c, const char* what, float max_dist) {
  if (std::isnan(max_dist) || max_dist < 0.f) return fail(c, FLIMO_ERR_INVALID, "%s: max_dist must be >= 0 or INFINITY", what);
  return FLIMO_OK;
}
// the stored points [first, first + n) of the range entries (no first + n is formed: it could wrap)
static int check_range(flimo_ctx* c, const char* what, size_t first, size_t n) {
  if (first > c->map_n || n > c->map_n - first)
    return fail(c, FLIMO_ERR_INVALID, "%s: the range [%zu, %zu + %zu) ends beyond the map's %zu points", what, first, first, n, c->map_n);
  return FLIMO_OK;
}
// the entries whose kernels index the stored points with 32 bits
static int check_map_size(flimo_ctx* c, const char* what) {
  if (c->map_n >= 0x80000000ull) return fail(c, FLIMO_ERR_TOO_LARGE, "%s: the map must hold fewer than 2^31 points", what);
  return FLIMO_OK;
}
// the entries that search a map they know is not empty: its index, or a failure
static int need_index(flimo_ctx* c, const char* what) {
  { const int rc0 = ensure_index(c); if (rc0) return rc0; }
  if (!c->grid_valid) return fail(c, FLIMO_ERR_HIP, "%s: a map of %zu points has no index", what, c->map_n);
  return FLIMO_OK;
}
// the setters of the entries' chunk sizes: 0 puts the default back
static int set_chunk(flimo_ctx* c, size_t flimo_ctx::*chunk, size_t n, size_t dflt) {
  if (!c) return FLIMO_ERR_INVALID;
  c->*chunk = n ? n : dflt;
  return FLIMO_OK;
}

// ---- kNN --------------------------------------------------------------------------------------
extern "C" int flimo_knn(flimo_ctx* c, const float* q, size_t nq, int k, int32_t* idx, float* sqd, int32_t* cnt) {
  if (!c || !q || !idx || !sqd || !cnt) return FLIMO_ERR_INVALID;
  if (k < 1 || k > 5) return fail(c, FLIMO_ERR_UNSUPPORTED, "k must be in 1..5");
  if (nq == 0) return FLIMO_OK;
  { const int rc0 = ensure_index(c); if (rc0) return rc0; }
  if (!c->grid_valid) {                       // Octree::knn with root_ == nullptr returns nothing
    for (size_t i = 0; i < nq; i++) cnt[i] = 0;
    for (size_t i = 0; i < nq * (size_t)k; i++) { idx[i] = -1; sqd[i] = 0.f; }
    return FLIMO_OK;
  }
  ctx_enter(c);
  // scratch of this call, released on every exit path
  DevScratch d;
  float* d_q = d.get<float>(nq * 3);
  int32_t* d_idx = d.get<int32_t>(nq * k);
  float* d_sqd = d.get<float>(nq * k);
  int32_t* d_cnt = d.get<int32_t>(nq);
  { const int rc = d.ok(c); if (rc) return rc; }
  HIPCHK(c, hipMemcpyAsync(d_q, q, nq * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  // (no gate like a pass's MAX_DIST_PLANE: Octree::knn answers from anywhere.  A few rings of cells near the map, then -- round 6 --
  //  the best-first search over the tiles that exist (knn_far_kernel): a query hundreds of metres from every point of a sparse map
  //  of kilometres costs a look at the directory and at the nearest tiles, not (2r+1)^2 row lookups per ring)
  launch_knn(c->stream, c->grid, d_q, (int)nq, k, 1 << 29, d_idx, d_sqd, d_cnt);
  if (c->ties && c->gbook.active) {    // exactly tied distances: the reference's first-met choice (device copy of its octree)
    const BookView book{c->gbook.node_c, c->gbook.node_child, c->gbook.node_cnt, c->gbook.root, c->d_tie_settled};
    launch_knn_tie(c->stream, c->grid, book, d_q, (int)nq, k, d_idx, d_sqd, d_cnt);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(idx, d_idx, nq * k * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(sqd, d_sqd, nq * k * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(cnt, d_cnt, nq * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return FLIMO_OK;
}

// ---- radius search (Octree::radiusSearch, Objects/Octree.hpp:453-523) ---------------------------
// kernels and the meaning of the call: flimo_radius.hip.  count -> 64-bit exclusive sum -> offsets to the host (total, the cap
// decision) -> result scratch -> fill (the same walk) -> sorted: segmented sort of (distance bits, insertion index) keys -> copies
// back; one wait at the end of each half.
extern "C" int flimo_radius_search(flimo_ctx* c, const float* q, size_t nq, float radius, unsigned flags, uint64_t* offsets,
                                   int32_t* idx, float* sqd, float* xyz, size_t cap, uint64_t* total) {
  if (!c) return FLIMO_ERR_INVALID;
  if (!offsets || (nq > 0 && !q)) return fail(c, FLIMO_ERR_INVALID, "radius search: null queries / offsets");
  if (!(radius >= 0.f) || std::isinf(radius)) return fail(c, FLIMO_ERR_INVALID, "radius search: the radius must be finite and >= 0");
  if (flags & ~FLIMO_RADIUS_SORTED) return fail(c, FLIMO_ERR_INVALID, "radius search: unknown flag bits 0x%x", flags & ~FLIMO_RADIUS_SORTED);
  if (nq > 0x7fff0000ull) return fail(c, FLIMO_ERR_TOO_LARGE, "radius search: too many queries");
  if (total) *total = 0;
  offsets[0] = 0;
  if (nq == 0) return FLIMO_OK;
  { const int rc0 = ensure_index(c); if (rc0) return rc0; }
  if (!c->grid_valid) {                       // Octree::radiusSearch with root_ == nullptr returns nothing (Octree.hpp:459)
    for (size_t i = 0; i <= nq; i++) offsets[i] = 0;
    return FLIMO_OK;
  }
  ctx_enter(c);
  // scratch of this call, released on every exit path
  DevScratch d;
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "offsets are copied as they are");
  float* d_q = d.get<float>(nq * 3);
  uint32_t* d_cnt = d.get<uint32_t>(nq + 1);
  unsigned long long* d_off = d.get<unsigned long long>(nq + 1);
  { const int rc = d.ok(c); if (rc) return rc; }
  size_t scan_bytes = 0;
  HIPCHK(c, radius_offsets(c->stream, nullptr, scan_bytes, d_cnt, d_off, nq));
  unsigned char* d_tmp = d.get<unsigned char>(scan_bytes + 16);
  { const int rc = d.ok(c); if (rc) return rc; }
  HIPCHK(c, hipMemcpyAsync(d_q, q, nq * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(d_cnt + nq, 0, sizeof(uint32_t), c->stream));
  HIPCHK(c, launch_radius_count(c->stream, c->grid, d_q, (int)nq, radius, d_cnt, nullptr));
  HIPCHK(c, radius_offsets(c->stream, d_tmp, scan_bytes, d_cnt, d_off, nq));
  HIPCHK(c, hipMemcpyAsync(offsets, d_off, (nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint64_t n = offsets[nq];
  if (total) *total = n;
  if (!idx && !sqd && !xyz) return FLIMO_OK;      // count only
  if (n > 0x7fffffffull) return fail(c, FLIMO_ERR_TOO_LARGE, "radius search: %llu results (the limit is 2^31 - 1)", (unsigned long long)n);
  if (n > cap) return fail(c, FLIMO_ERR_TOO_LARGE, "radius search: %llu results, room for %zu", (unsigned long long)n, cap);
  if (n == 0) return FLIMO_OK;
  int32_t* d_idx = idx ? d.get<int32_t>(n) : nullptr;
  float* d_sqd = sqd ? d.get<float>(n) : nullptr;
  float* d_xyz = xyz ? d.get<float>(n * 3) : nullptr;
  { const int rc = d.ok(c); if (rc) return rc; }
  if (flags & FLIMO_RADIUS_SORTED) {
    unsigned long long* d_keys = d.get<unsigned long long>(n);
    unsigned long long* d_keys2 = d.get<unsigned long long>(n);
    { const int rc = d.ok(c); if (rc) return rc; }
    size_t sort_bytes = 0;
    HIPCHK(c, radius_sort_segments(c->stream, nullptr, sort_bytes, d_keys, d_keys2, (size_t)n, nq, d_off));
    d.drop(d_tmp);
    d_tmp = d.get<unsigned char>(sort_bytes + 16);
    { const int rc = d.ok(c); if (rc) return rc; }
    HIPCHK(c, launch_radius_fill(c->stream, c->grid, d_q, (int)nq, radius, d_off, nullptr, nullptr, nullptr, d_keys));
    HIPCHK(c, radius_sort_segments(c->stream, d_tmp, sort_bytes, d_keys, d_keys2, (size_t)n, nq, d_off));
    HIPCHK(c, launch_radius_unpack(c->stream, d_keys2, (size_t)n, c->d_map_raw, d_idx, d_sqd, d_xyz));
  } else {
    HIPCHK(c, launch_radius_fill(c->stream, c->grid, d_q, (int)nq, radius, d_off, d_idx, d_sqd, d_xyz, nullptr));
  }
  if (idx) HIPCHK(c, hipMemcpyAsync(idx, d_idx, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (sqd) HIPCHK(c, hipMemcpyAsync(sqd, d_sqd, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (xyz) HIPCHK(c, hipMemcpyAsync(xyz, d_xyz, n * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return FLIMO_OK;
}

extern "C" int flimo_radius_candidates(flimo_ctx* c, const float* q, size_t nq, float radius, uint64_t* cand) {
  if (!c) return FLIMO_ERR_INVALID;
  if (nq > 0 && (!q || !cand)) return fail(c, FLIMO_ERR_INVALID, "radius candidates: null queries / output");
  if (!(radius >= 0.f) || std::isinf(radius)) return fail(c, FLIMO_ERR_INVALID, "radius candidates: the radius must be finite and >= 0");
  if (nq > 0x7fff0000ull) return fail(c, FLIMO_ERR_TOO_LARGE, "radius candidates: too many queries");
  if (nq == 0) return FLIMO_OK;
  { const int rc0 = ensure_index(c); if (rc0) return rc0; }
  if (!c->grid_valid) { for (size_t i = 0; i < nq; i++) cand[i] = 0; return FLIMO_OK; }
  ctx_enter(c);
  DevScratch d;
  float* d_q = d.get<float>(nq * 3);
  uint32_t* d_cnt = d.get<uint32_t>(nq);
  unsigned long long* d_cand = d.get<unsigned long long>(nq);
  { const int rc = d.ok(c); if (rc) return rc; }
  HIPCHK(c, hipMemcpyAsync(d_q, q, nq * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, launch_radius_count(c->stream, c->grid, d_q, (int)nq, radius, d_cnt, d_cand));
  HIPCHK(c, hipMemcpyAsync(cand, d_cand, nq * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return FLIMO_OK;
}

// ---- k-NN for k up to FLIMO_KNN_MAX_K with a distance gate (Octree::knn, Objects/Octree.hpp:526-555) -------------
// kernels and the meaning of the call: flimo_knn_k.hip.  One block-search launch, one launch that finishes the worklist of what it
// could not prove over the directory's tiles, the copies back, one wait.  cand (developer counter, flimo_dev.h): the result arrays may then be NULL.
static int knn_k_run(flimo_ctx* c, const float* q, size_t nq, int k, float max_dist, int32_t* idx, float* sqd, float* xyz, int32_t* cnt,
                     uint64_t* cand) {
  static_assert(FLIMO_KNN_MAX_K == KNNK_MAX_K, "the header's limit is the kernels'");
  { const int rc = check_gate(c, "knn_k", max_dist); if (rc) return rc; }
  if (k < 1 || k > FLIMO_KNN_MAX_K) return fail(c, FLIMO_ERR_UNSUPPORTED, "knn_k: k must be in 1..%d", FLIMO_KNN_MAX_K);
  if ((unsigned long long)nq * (unsigned long long)k >= 0x80000000ull) return fail(c, FLIMO_ERR_TOO_LARGE, "knn_k: nq * k must be below 2^31");
  if (nq == 0) return FLIMO_OK;
  { const int rc0 = ensure_index(c); if (rc0) return rc0; }
  if (!c->grid_valid) {                       // Octree::knn with root_ == nullptr returns nothing
    for (size_t i = 0; i < nq; i++) { if (cnt) cnt[i] = 0; if (cand) cand[i] = 0; }
    for (size_t i = 0; i < nq * (size_t)k; i++) { if (idx) idx[i] = -1; if (sqd) sqd[i] = 0.f; }
    if (xyz) for (size_t i = 0; i < nq * (size_t)k * 3; i++) xyz[i] = 0.f;
    return FLIMO_OK;
  }
  ctx_enter(c);
  // scratch of this call, released on every exit path
  DevScratch d;
  float* d_q = d.get<float>(nq * 3);
  int32_t* d_idx = d.get<int32_t>(nq * k);
  float* d_sqd = d.get<float>(nq * k);
  float* d_xyz = xyz ? d.get<float>(nq * k * 3) : nullptr;
  int32_t* d_cnt = d.get<int32_t>(nq);
  unsigned long long* d_cand = cand ? d.get<unsigned long long>(nq) : nullptr;
  uint2* d_work = d.get<uint2>(nq + 1);      // the worklist and, behind it, its counter: one allocation, this call is short
  { const int rc = d.ok(c); if (rc) return rc; }
  unsigned* d_nwork = reinterpret_cast<unsigned*>(d_work + nq);
  HIPCHK(c, hipMemcpyAsync(d_q, q, nq * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, launch_knn_k(c->stream, c->grid, c->d_map_raw, d_q, (int)nq, k, max_dist, d_idx, d_sqd, d_xyz, d_cnt, d_cand, d_work, d_nwork));
  if (idx) HIPCHK(c, hipMemcpyAsync(idx, d_idx, nq * k * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (sqd) HIPCHK(c, hipMemcpyAsync(sqd, d_sqd, nq * k * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (xyz) HIPCHK(c, hipMemcpyAsync(xyz, d_xyz, nq * k * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (cnt) HIPCHK(c, hipMemcpyAsync(cnt, d_cnt, nq * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (cand) HIPCHK(c, hipMemcpyAsync(cand, d_cand, nq * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return FLIMO_OK;
}
extern "C" int flimo_knn_k(flimo_ctx* c, const float* q, size_t nq, int k, float max_dist, int32_t* idx, float* sqd, float* xyz, int32_t* cnt) {
  if (!c) return FLIMO_ERR_INVALID;
  if ((nq > 0 && !q) || !idx || !sqd || !cnt) return fail(c, FLIMO_ERR_INVALID, "knn_k: null queries / idx / sqd / cnt");
  return knn_k_run(c, q, nq, k, max_dist, idx, sqd, xyz, cnt, nullptr);
}
extern "C" int flimo_knn_k_candidates(flimo_ctx* c, const float* q, size_t nq, int k, float max_dist, uint64_t* cand) {
  if (!c) return FLIMO_ERR_INVALID;
  if (nq > 0 && (!q || !cand)) return fail(c, FLIMO_ERR_INVALID, "knn_k candidates: null queries / output");
  return knn_k_run(c, q, nq, k, max_dist, nullptr, nullptr, nullptr, nullptr, cand);
}

// ---- normals and covariances of k-NN neighbourhoods (PCL's NormalEstimation over the map) -------------------------
// kernels: flimo_knn_k.hip (flimo_knn_k's search, finished in registers).  Chunks of c->normals_chunk queries: per chunk the
// queries go up (q != NULL; the range form reads them from the map), three launches (block search, walk over the tiles, the
// eigen-decomposition), the results come back; device scratch is the chunk's, whatever nq, and nothing of nq * k entries exists.
static int normals_run(flimo_ctx* c, const float* q, size_t first, size_t nq, int k, float max_dist, int min_pts, const float* viewpoint,
                       float* normal, int32_t* cnt, double* centroid, double* cov, double* eig) {
  if (!normal || !cnt) return fail(c, FLIMO_ERR_INVALID, "map normals: null normal / cnt");
  { const int rc = check_gate(c, "map normals", max_dist); if (rc) return rc; }
  if (viewpoint && (std::isnan(viewpoint[0]) || std::isnan(viewpoint[1]) || std::isnan(viewpoint[2])))
    return fail(c, FLIMO_ERR_INVALID, "map normals: NaN viewpoint");
  if (k < 1 || k > FLIMO_KNN_MAX_K) return fail(c, FLIMO_ERR_UNSUPPORTED, "map normals: k must be in 1..%d", FLIMO_KNN_MAX_K);
  if (nq >= 0x80000000ull) return fail(c, FLIMO_ERR_TOO_LARGE, "map normals: the number of queries must be below 2^31");
  if (nq == 0) return FLIMO_OK;
  { const int rc0 = ensure_index(c); if (rc0) return rc0; }
  if (!c->grid_valid) {                       // an empty map: no neighbours anywhere
    const float fn = std::numeric_limits<float>::quiet_NaN();
    const double dn = std::numeric_limits<double>::quiet_NaN();
    for (size_t i = 0; i < nq; i++) cnt[i] = 0;
    for (size_t i = 0; i < nq * 4; i++) normal[i] = fn;
    if (centroid) for (size_t i = 0; i < nq * 3; i++) centroid[i] = dn;
    if (cov) for (size_t i = 0; i < nq * 6; i++) cov[i] = dn;
    if (eig) for (size_t i = 0; i < nq * 6; i++) eig[i] = dn;
    return FLIMO_OK;
  }
  ctx_enter(c);
  // scratch of this call, released on every exit path
  DevScratch d;
  const size_t m = std::min(nq, std::max<size_t>(c->normals_chunk, 1));
  float* d_q = q ? d.get<float>(m * 3) : nullptr;
  float4* d_normal = d.get<float4>(m);
  int32_t* d_cnt = d.get<int32_t>(m);
  double* d_centroid = centroid ? d.get<double>(m * 3) : nullptr;
  double* d_cov = cov ? d.get<double>(m * 6) : nullptr;
  double* d_eig = eig ? d.get<double>(m * 6) : nullptr;
  double* d_mom = d.get<double>(m * 9);
  uint2* d_work = d.get<uint2>(m);
  unsigned* d_nwork = d.get<unsigned>(1);
  { const int rc = d.ok(c); if (rc) return rc; }
  for (size_t a = 0; a < nq; a += m) {
    const size_t n = std::min(m, nq - a);
    if (q) HIPCHK(c, hipMemcpyAsync(d_q, q + 3 * a, n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_knn_k_normals(c->stream, c->grid, c->d_map_raw, d_q, (unsigned)(first + a), (int)n, k, max_dist, min_pts, viewpoint, d_normal,
                                   d_cnt, d_centroid, d_cov, d_eig, d_mom, d_work, d_nwork));
    HIPCHK(c, hipMemcpyAsync(normal + 4 * a, d_normal, n * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cnt + a, d_cnt, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (centroid) HIPCHK(c, hipMemcpyAsync(centroid + 3 * a, d_centroid, n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (cov) HIPCHK(c, hipMemcpyAsync(cov + 6 * a, d_cov, n * 6 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (eig) HIPCHK(c, hipMemcpyAsync(eig + 6 * a, d_eig, n * 6 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    // (the next chunk's upload overwrites d_q; the copies above read host memory the caller owns: one wait per chunk)
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return FLIMO_OK;
}
extern "C" int flimo_map_normals(flimo_ctx* c, const float* q, size_t nq, int k, float max_dist, int min_pts, const float viewpoint[3], float* normal,
                                 int32_t* cnt, double* centroid, double* cov, double* eig) {
  if (!c) return FLIMO_ERR_INVALID;
  if (nq > 0 && !q) return fail(c, FLIMO_ERR_INVALID, "map normals: null queries");
  return normals_run(c, nq ? q : nullptr, 0, nq, k, max_dist, min_pts, viewpoint, normal, cnt, centroid, cov, eig);
}
extern "C" int flimo_map_normals_range(flimo_ctx* c, size_t first, size_t n, int k, float max_dist, int min_pts, const float viewpoint[3],
                                       float* normal, int32_t* cnt, double* centroid, double* cov, double* eig) {
  if (!c) return FLIMO_ERR_INVALID;
  { const int rc = check_range(c, "map normals", first, n); if (rc) return rc; }
  return normals_run(c, nullptr, first, n, k, max_dist, min_pts, viewpoint, normal, cnt, centroid, cov, eig);
}
extern "C" int flimo_set_normals_chunk(flimo_ctx* c, size_t n) { return set_chunk(c, &flimo_ctx::normals_chunk, n, (size_t)1 << 20); }

// ---- outliers by neighbour statistics (PCL's StatisticalOutlierRemoval / RadiusOutlierRemoval over the map) --------------------
// kernels: flimo_knn_k.hip.  The search runs in chunks of c->outlier_chunk points into mean[] / cnt[] of the WHOLE range (12 B a
// point: the threshold needs all of them first); then the sum of the means and |T| (two launches, a wait), mu on the host, the sum
// of the squared deviations (two launches, a wait), sigma and the threshold on the host, the mask and its two counts (one launch).
// The removal hands the device mask to the crop's ordered compaction; from there on its host side is the crop's (map_keep_only).
static void outlier_stats_none(flimo_outlier_stats* s) {
  if (!s) return;
  const double dn = std::numeric_limits<double>::quiet_NaN();
  s->n = s->n_stat = 0; s->mu = s->sigma = s->threshold = dn; s->few = s->far = s->outliers = 0;
}
static int outlier_check(flimo_ctx* c, size_t first, size_t n, const flimo_outlier_cfg* cfg, const char* what) {
  static_assert(FLIMO_KNN_MAX_K == KNNK_MAX_K, "the header's limit is the kernels'");
  if (!cfg) return fail(c, FLIMO_ERR_INVALID, "%s: null cfg", what);
  { const int rc = check_range(c, what, first, n); if (rc) return rc; }
  { const int rc = check_gate(c, what, cfg->max_dist); if (rc) return rc; }
  if (std::isnan(cfg->std_mul) || cfg->std_mul < 0.f) return fail(c, FLIMO_ERR_INVALID, "%s: std_mul must be >= 0 or INFINITY", what);
  if (cfg->k < 1 || cfg->k > FLIMO_KNN_MAX_K - 1) return fail(c, FLIMO_ERR_UNSUPPORTED, "%s: k must be in 1..%d", what, FLIMO_KNN_MAX_K - 1);
  if (cfg->min_pts < 0 || cfg->min_pts > cfg->k) return fail(c, FLIMO_ERR_INVALID, "%s: min_pts must be in 0..k", what);
  return FLIMO_OK;
}
struct OutlierDev {      // what outliers_device leaves on the device for its caller, and the owner of all it allocated
  DevScratch mem;
  double* mean = nullptr; int32_t* cnt = nullptr; unsigned char* mask = nullptr;
};
// the predicate over [first, first + n), n > 0, arguments checked: d.mean, d.cnt, d.mask filled on the device, *st on the host; ends
// synchronised
static int outliers_device(flimo_ctx* c, size_t first, size_t n, const flimo_outlier_cfg& cfg, OutlierDev& d, flimo_outlier_stats* st) {
  { const int rc = need_index(c, "map outliers"); if (rc) return rc; }
  ctx_enter(c);
  const size_t m = std::min(std::min(n, std::max<size_t>(c->outlier_chunk, 1)), (size_t)1 << 24);
  const unsigned nseg = sum_segments(n);
  d.mean = d.mem.get<double>(n);
  d.cnt = d.mem.get<int32_t>(n);
  d.mask = d.mem.get<unsigned char>(n);
  uint2* d_work = d.mem.get<uint2>(m);
  unsigned* d_nwork = d.mem.get<unsigned>(1);
  double* d_part = d.mem.get<double>(nseg);
  int32_t* d_part_cnt = d.mem.get<int32_t>(nseg);
  unsigned long long* d_words = d.mem.get<unsigned long long>(3);      // {sum bits, |T|, few | far << 32}
  { const int rc = d.mem.ok(c); if (rc) return rc; }
  // (a chunk's worklist is read by its own second launch only: the stream orders the chunks, nothing waits in between)
  for (size_t a = 0; a < n; a += m)
    HIPCHK(c, launch_outlier_search(c->stream, c->grid, c->d_map_raw, (unsigned)(first + a), (int)std::min(m, n - a), cfg.k, cfg.max_dist, d.mean + a,
                                    d.cnt + a, d_work, d_nwork));
  const int need = std::max(1, cfg.min_pts);
  unsigned long long w[3] = {0, 0, 0};
  HIPCHK(c, launch_outlier_sum(c->stream, d.mean, d.cnt, (unsigned)n, need, 0, 0.0, d_part, d_part_cnt, d_words));
  HIPCHK(c, hipMemcpyAsync(w, d_words, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const double dn = std::numeric_limits<double>::quiet_NaN();
  const uint64_t N = w[1];
  if (N > n) return fail(c, FLIMO_ERR_HIP, "map outliers: counted %llu of %zu points", (unsigned long long)N, n);
  double sum_m, mu = dn, sigma = dn, threshold = dn;
  memcpy(&sum_m, &w[0], sizeof sum_m);
  if (N > 0) {
    mu = sum_m / (double)N;
    sigma = 0.0;
    if (N > 1) {
      HIPCHK(c, launch_outlier_sum(c->stream, d.mean, d.cnt, (unsigned)n, need, 1, mu, d_part, d_part_cnt, d_words));
      HIPCHK(c, hipMemcpyAsync(w, d_words, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      double sum_d;
      memcpy(&sum_d, &w[0], sizeof sum_d);
      sigma = std::sqrt(sum_d / (double)(N - 1));
    }
    threshold = mu + (double)cfg.std_mul * sigma;
  }
  unsigned* counts = reinterpret_cast<unsigned*>(d_words + 2);
  HIPCHK(c, launch_outlier_mask(c->stream, d.mean, d.cnt, (unsigned)n, cfg.min_pts, need, std::isfinite(cfg.std_mul), threshold, d.mask, counts));
  HIPCHK(c, hipMemcpyAsync(&w[2], d_words + 2, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  st->n = n; st->n_stat = N; st->mu = mu; st->sigma = sigma; st->threshold = threshold;
  st->few = w[2] & 0xffffffffull; st->far = w[2] >> 32; st->outliers = st->few + st->far;
  if (st->outliers > n) return fail(c, FLIMO_ERR_HIP, "map outliers: marked %llu of %zu points", (unsigned long long)st->outliers, n);
  return FLIMO_OK;
}
extern "C" int flimo_map_outliers(flimo_ctx* c, size_t first, size_t n, const flimo_outlier_cfg* cfg, unsigned char* mask, double* mean_dist,
                                  int32_t* cnt, flimo_outlier_stats* stats) {
  if (!c) return FLIMO_ERR_INVALID;
  { const int rc = outlier_check(c, first, n, cfg, "map outliers"); if (rc) return rc; }
  if (n == 0) { outlier_stats_none(stats); return FLIMO_OK; }
  if (n >= 0x80000000ull) return fail(c, FLIMO_ERR_TOO_LARGE, "map outliers: the range must hold fewer than 2^31 points");
  OutlierDev d;
  flimo_outlier_stats st;
  { const int rc = outliers_device(c, first, n, *cfg, d, &st); if (rc) return rc; }
  if (mask) HIPCHK(c, hipMemcpyAsync(mask, d.mask, n, hipMemcpyDeviceToHost, c->stream));
  if (mean_dist) HIPCHK(c, hipMemcpyAsync(mean_dist, d.mean, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (cnt) HIPCHK(c, hipMemcpyAsync(cnt, d.cnt, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (stats) *stats = st;
  return FLIMO_OK;
}
extern "C" int flimo_map_remove_outliers(flimo_ctx* c, size_t first, size_t n, const flimo_outlier_cfg* cfg, size_t* removed,
                                         flimo_outlier_stats* stats) {
  if (!c) return FLIMO_ERR_INVALID;
  { const int rc = outlier_check(c, first, n, cfg, "remove outliers"); if (rc) return rc; }
  if (n == 0) { if (removed) *removed = 0; outlier_stats_none(stats); return FLIMO_OK; }
  if (n >= 0x80000000ull) return fail(c, FLIMO_ERR_TOO_LARGE, "remove outliers: the range must hold fewer than 2^31 points");
  OutlierDev d;
  flimo_outlier_stats st;
  { const int rc = outliers_device(c, first, n, *cfg, d, &st); if (rc) return rc; }
  if (removed) *removed = 0;
  if (stats) *stats = st;
  if (st.outliers == 0) return FLIMO_OK;               // removing nothing changes nothing
  return map_remove_masked(c, d.mask, first, n, (size_t)st.outliers, &c->outlier_removals, &c->outlier_removed, removed, "remove outliers");
}
extern "C" int flimo_set_outlier_chunk(flimo_ctx* c, size_t n) { return set_chunk(c, &flimo_ctx::outlier_chunk, n, (size_t)1 << 20); }

// ---- FPFH descriptors of the stored points (pcl::FPFHEstimation over the map) ---------------------------------------------------
// kernels: flimo_knn_k.hip.  Three stages on the context's stream, the first two over the WHOLE map whatever the range (a neighbour
// can be anywhere), in chunks of c->fpfh_chunk points: the normals of flimo_map_normals_range left on the device (16 B a stored
// point; three launches a chunk), the SPFH rows and list lengths (34 B a stored point; two launches a chunk), then the FPFH rows of
// the range (two launches a chunk, 136 B a point of the chunk come back).  Per chunk the scratch is the normals' moments and count
// (76 B a point) and the worklist (8 B a point); nothing of points x k entries exists anywhere.
extern "C" int flimo_map_fpfh(flimo_ctx* c, size_t first, size_t n, const flimo_fpfh_cfg* cfg, float* fpfh, uint8_t* spfh, int32_t* cnt) {
  if (!c) return FLIMO_ERR_INVALID;
  if (!cfg) return fail(c, FLIMO_ERR_INVALID, "map fpfh: null cfg");
  { const int rc = check_range(c, "map fpfh", first, n); if (rc) return rc; }
  if (n > 0 && !fpfh) return fail(c, FLIMO_ERR_INVALID, "map fpfh: null fpfh");
  { const int rc = check_gate(c, "map fpfh", cfg->max_dist); if (rc) return rc; }
  { const int rc = check_gate(c, "map fpfh (normals)", cfg->normal_max_dist); if (rc) return rc; }
  if (cfg->has_viewpoint && (std::isnan(cfg->viewpoint[0]) || std::isnan(cfg->viewpoint[1]) || std::isnan(cfg->viewpoint[2])))
    return fail(c, FLIMO_ERR_INVALID, "map fpfh: NaN viewpoint");
  if (cfg->normal_min_pts < 0) return fail(c, FLIMO_ERR_INVALID, "map fpfh: normal_min_pts must be >= 0");
  if (cfg->k < 2 || cfg->k > FLIMO_KNN_MAX_K) return fail(c, FLIMO_ERR_UNSUPPORTED, "map fpfh: k must be in 2..%d", FLIMO_KNN_MAX_K);
  if (cfg->normal_k < 1 || cfg->normal_k > FLIMO_KNN_MAX_K) return fail(c, FLIMO_ERR_UNSUPPORTED, "map fpfh: normal_k must be in 1..%d", FLIMO_KNN_MAX_K);
  if (n == 0) return FLIMO_OK;
  const size_t N = c->map_n;
  { const int rc = check_map_size(c, "map fpfh"); if (rc) return rc; }
  { const int rc = need_index(c, "map fpfh"); if (rc) return rc; }
  ctx_enter(c);
  DevScratch d;
  const size_t m = std::min(N, std::max<size_t>(c->fpfh_chunk, 1));      // points of a chunk, of the map's stages and of the range's
  float4* d_normal = d.get<float4>(N);
  unsigned char* d_spfh = d.get<unsigned char>(N * 33);
  unsigned char* d_len = d.get<unsigned char>(N);
  int32_t* d_ncnt = d.get<int32_t>(m);
  double* d_mom = d.get<double>(m * 9);
  uint2* d_work = d.get<uint2>(m);
  unsigned* d_nwork = d.get<unsigned>(1);
  float* d_fpfh = d.get<float>(std::min(m, n) * 33);
  int32_t* d_cnt = d.get<int32_t>(std::min(m, n));
  { const int rc = d.ok(c); if (rc) return rc; }
  // (a chunk's worklist and moments are read by its own launches only: the stream orders the chunks, nothing waits in between)
  const float* vp = cfg->has_viewpoint ? cfg->viewpoint : nullptr;
  for (size_t a = 0; a < N; a += m)
    HIPCHK(c, launch_knn_k_normals(c->stream, c->grid, c->d_map_raw, nullptr, (unsigned)a, (int)std::min(m, N - a), cfg->normal_k, cfg->normal_max_dist,
                                   cfg->normal_min_pts, vp, d_normal + a, d_ncnt, nullptr, nullptr, nullptr, d_mom, d_work, d_nwork));
  for (size_t a = 0; a < N; a += m)
    HIPCHK(c, launch_fpfh_spfh(c->stream, c->grid, c->d_map_raw, d_normal, (unsigned)a, (int)std::min(m, N - a), cfg->k, cfg->max_dist, d_spfh, d_len,
                               d_work, d_nwork));
  if (spfh) HIPCHK(c, hipMemcpyAsync(spfh, d_spfh + first * 33, n * 33, hipMemcpyDeviceToHost, c->stream));
  for (size_t a = 0; a < n; a += m) {
    const size_t na = std::min(m, n - a);
    HIPCHK(c, launch_fpfh_sum(c->stream, c->grid, c->d_map_raw, d_spfh, d_len, (unsigned)(first + a), (int)na, cfg->k, cfg->max_dist, d_fpfh, d_cnt,
                              d_work, d_nwork));
    HIPCHK(c, hipMemcpyAsync(fpfh + 33 * a, d_fpfh, na * 33 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (cnt) HIPCHK(c, hipMemcpyAsync(cnt + a, d_cnt, na * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (the next chunk overwrites d_fpfh / d_cnt)
  }
  return FLIMO_OK;
}
extern "C" int flimo_set_fpfh_chunk(flimo_ctx* c, size_t n) { return set_chunk(c, &flimo_ctx::fpfh_chunk, n, (size_t)1 << 20); }

// ---- ISS keypoints of the stored points (pcl::ISSKeypoint3D over the map) -------------------------------------------------------
// kernels: flimo_knn_k.hip.  Two stages on the context's stream, in chunks of c->keypoints_chunk points: the saliency of the WHOLE
// map whatever the range (a neighbour can be anywhere; 8 B a stored point, three launches a chunk: flimo_map_normals_range's two
// searches and one thread per point in the place of its eigen-decomposition's outputs), then the suppression over the range (two
// launches a chunk, 1 B a point of the chunk comes back).  Per chunk the scratch is the moments and count (76 B a point), the
// worklist (8 B) and the mask (1 B); nothing of points x k entries exists anywhere.
extern "C" int flimo_map_keypoints(flimo_ctx* c, size_t first, size_t n, const flimo_keypoint_cfg* cfg, unsigned char* mask, double* saliency,
                                   int32_t* cnt, size_t* count) {
  if (!c) return FLIMO_ERR_INVALID;
  if (!cfg) return fail(c, FLIMO_ERR_INVALID, "map keypoints: null cfg");
  { const int rc = check_range(c, "map keypoints", first, n); if (rc) return rc; }
  { const int rc = check_gate(c, "map keypoints", cfg->max_dist); if (rc) return rc; }
  { const int rc = check_gate(c, "map keypoints (suppression)", cfg->nms_max_dist); if (rc) return rc; }
  if (!(cfg->gamma21 > 0.f && cfg->gamma21 <= 1.f) || !(cfg->gamma32 > 0.f && cfg->gamma32 <= 1.f))
    return fail(c, FLIMO_ERR_INVALID, "map keypoints: gamma21 and gamma32 must be in (0, 1]");
  if (cfg->min_pts < 0) return fail(c, FLIMO_ERR_INVALID, "map keypoints: min_pts must be >= 0");
  if (cfg->k < 3 || cfg->k > FLIMO_KNN_MAX_K) return fail(c, FLIMO_ERR_UNSUPPORTED, "map keypoints: k must be in 3..%d", FLIMO_KNN_MAX_K);
  if (cfg->nms_k < 2 || cfg->nms_k > FLIMO_KNN_MAX_K) return fail(c, FLIMO_ERR_UNSUPPORTED, "map keypoints: nms_k must be in 2..%d", FLIMO_KNN_MAX_K);
  const size_t N = c->map_n;
  { const int rc = check_map_size(c, "map keypoints"); if (rc) return rc; }
  if (n == 0) { if (count) *count = 0; return FLIMO_OK; }
  { const int rc = need_index(c, "map keypoints"); if (rc) return rc; }
  ctx_enter(c);
  DevScratch d;
  const size_t m = std::min(N, std::max<size_t>(c->keypoints_chunk, 1));      // points of a chunk, of the map's stage and of the range's
  double* d_sal = d.get<double>(N);
  int32_t* d_rcnt = cnt ? d.get<int32_t>(n) : nullptr;
  int32_t* d_ncnt = d.get<int32_t>(m);
  double* d_mom = d.get<double>(m * 9);
  uint2* d_work = d.get<uint2>(m);
  unsigned* d_nwork = d.get<unsigned>(1);
  unsigned* d_count = d.get<unsigned>(1);
  unsigned char* d_mask = d.get<unsigned char>(std::min(m, n));
  { const int rc = d.ok(c); if (rc) return rc; }
  // (a chunk's worklist and moments are read by its own launches only: the stream orders the chunks, nothing waits in between)
  for (size_t a = 0; a < N; a += m)
    HIPCHK(c, launch_iss_saliency(c->stream, c->grid, c->d_map_raw, (unsigned)a, (int)std::min(m, N - a), cfg->k, cfg->max_dist, cfg->min_pts,
                                  cfg->gamma21, cfg->gamma32, d_sal, (unsigned)first, (unsigned)n, d_rcnt, d_ncnt, d_mom, d_work, d_nwork));
  HIPCHK(c, hipMemsetAsync(d_count, 0, sizeof(unsigned), c->stream));
  if (saliency) HIPCHK(c, hipMemcpyAsync(saliency, d_sal + first, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (cnt) HIPCHK(c, hipMemcpyAsync(cnt, d_rcnt, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  for (size_t a = 0; a < n; a += m) {
    const size_t na = std::min(m, n - a);
    HIPCHK(c, launch_iss_suppress(c->stream, c->grid, c->d_map_raw, d_sal, (unsigned)(first + a), (int)na, cfg->nms_k, cfg->nms_max_dist, d_mask,
                                  d_count, d_work, d_nwork));
    if (mask) {
      HIPCHK(c, hipMemcpyAsync(mask + a, d_mask, na, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));      // (the next chunk overwrites d_mask)
    }
  }
  unsigned h_count = 0;
  HIPCHK(c, hipMemcpyAsync(&h_count, d_count, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((size_t)h_count > n) return fail(c, FLIMO_ERR_HIP, "map keypoints: counted %u of %zu points", h_count, n);
  if (count) *count = (size_t)h_count;
  return FLIMO_OK;
}
extern "C" int flimo_set_keypoints_chunk(flimo_ctx* c, size_t n) { return set_chunk(c, &flimo_ctx::keypoints_chunk, n, (size_t)1 << 20); }

// ---- Euclidean clusters of the stored points (pcl::EuclideanClusterExtraction over the map) -------------------------------------
// kernels: flimo_cluster.hip.  Four launches on the context's stream over the WHOLE map whatever the range (a component can reach
// anywhere): init, link in chunks of c->cluster_chunk stored points, flatten, finish; then the copies back, one wait.  Scratch: 8 B
// a stored point (parent, count), 1 B a point of the range (mask), 4 B each for label and size where they are asked for; nothing of
// points x neighbours exists anywhere.  The removal hands the device mask to the crop's ordered compaction (map_keep_only).
static void cluster_stats_none(flimo_cluster_stats* s) {
  if (s) s->n = s->clusters = s->largest = s->sel_clusters = s->sel_points = 0;
}
static int cluster_check(flimo_ctx* c, size_t first, size_t n, const flimo_cluster_cfg* cfg, const char* what) {
  if (!cfg) return fail(c, FLIMO_ERR_INVALID, "%s: null cfg", what);
  { const int rc = check_range(c, what, first, n); if (rc) return rc; }
  if (!(cfg->tol >= 0.f) || std::isinf(cfg->tol)) return fail(c, FLIMO_ERR_INVALID, "%s: tol must be finite and >= 0", what);
  if (cfg->min_size < 0 || cfg->max_size < 0) return fail(c, FLIMO_ERR_INVALID, "%s: min_size and max_size must be >= 0", what);
  if (cfg->max_size > 0 && cfg->max_size < cfg->min_size) return fail(c, FLIMO_ERR_INVALID, "%s: max_size must be 0 or >= min_size", what);
  return check_map_size(c, what);
}
struct ClusterDev {      // what clusters_device leaves on the device for its caller, and the owner of all it allocated
  DevScratch mem;
  int32_t* label = nullptr; int32_t* size = nullptr; unsigned char* mask = nullptr;
};
// the components of the whole map and the selection over [first, first + n), arguments checked, map not empty: d.mask (n > 0) and,
// where asked for, d.label / d.size filled on the device, *st on the host; ends synchronised
static int clusters_device(flimo_ctx* c, size_t first, size_t n, const flimo_cluster_cfg& cfg, bool want_label, bool want_size, ClusterDev& d,
                           flimo_cluster_stats* st) {
  { const int rc = need_index(c, "map clusters"); if (rc) return rc; }
  ctx_enter(c);
  const size_t N = c->map_n;
  const size_t m = std::min(std::min(N, std::max<size_t>(c->cluster_chunk, 1)), (size_t)1 << 24);      // (x 64 lanes: below 2^31 a launch)
  uint32_t* d_parent = d.mem.get<uint32_t>(N);
  uint32_t* d_count = d.mem.get<uint32_t>(N);
  uint32_t* d_words = d.mem.get<uint32_t>(4);      // {components, largest, selected components, ones of the mask}
  if (n > 0) d.mask = d.mem.get<unsigned char>(n);
  if (n > 0 && want_label) d.label = d.mem.get<int32_t>(n);
  if (n > 0 && want_size) d.size = d.mem.get<int32_t>(n);
  { const int rc = d.mem.ok(c); if (rc) return rc; }
  HIPCHK(c, hipMemsetAsync(d_words, 0, 4 * sizeof(uint32_t), c->stream));
  HIPCHK(c, launch_cluster_init(c->stream, d_parent, d_count, N));
  for (size_t a = 0; a < N; a += m)
    HIPCHK(c, launch_cluster_link(c->stream, c->grid, c->d_map_raw, (unsigned)a, (int)std::min(m, N - a), cfg.tol, d_parent));
  HIPCHK(c, launch_cluster_flatten(c->stream, d_parent, d_count, N));
  HIPCHK(c, launch_cluster_finish(c->stream, d_parent, d_count, N, first, n, cfg.min_size, cfg.max_size, d.label, d.size, d.mask, d_words));
  uint32_t w[4] = {0, 0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(w, d_words, sizeof w, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (w[0] < 1 || w[0] > N || w[1] < 1 || w[1] > N || w[2] > w[0] || w[3] > n)
    return fail(c, FLIMO_ERR_HIP, "map clusters: counted %u components (largest %u, %u selected, %u points) of %zu points", w[0], w[1], w[2], w[3], N);
  st->n = n; st->clusters = w[0]; st->largest = w[1]; st->sel_clusters = w[2]; st->sel_points = w[3];
  return FLIMO_OK;
}
extern "C" int flimo_map_clusters(flimo_ctx* c, size_t first, size_t n, const flimo_cluster_cfg* cfg, int32_t* label, int32_t* size,
                                  unsigned char* mask, flimo_cluster_stats* stats) {
  if (!c) return FLIMO_ERR_INVALID;
  { const int rc = cluster_check(c, first, n, cfg, "map clusters"); if (rc) return rc; }
  if (c->map_n == 0) { cluster_stats_none(stats); return FLIMO_OK; }
  if (n == 0 && !stats) return FLIMO_OK;
  ClusterDev d;
  flimo_cluster_stats st;
  { const int rc = clusters_device(c, first, n, *cfg, label != nullptr, size != nullptr, d, &st); if (rc) return rc; }
  if (n > 0) {
    if (label) HIPCHK(c, hipMemcpyAsync(label, d.label, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (size) HIPCHK(c, hipMemcpyAsync(size, d.size, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (mask) HIPCHK(c, hipMemcpyAsync(mask, d.mask, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (stats) *stats = st;
  return FLIMO_OK;
}
extern "C" int flimo_map_remove_clusters(flimo_ctx* c, size_t first, size_t n, const flimo_cluster_cfg* cfg, size_t* removed,
                                         flimo_cluster_stats* stats) {
  if (!c) return FLIMO_ERR_INVALID;
  { const int rc = cluster_check(c, first, n, cfg, "remove clusters"); if (rc) return rc; }
  if (c->map_n == 0) { if (removed) *removed = 0; cluster_stats_none(stats); return FLIMO_OK; }
  if (n == 0 && !stats) { if (removed) *removed = 0; return FLIMO_OK; }
  ClusterDev d;
  flimo_cluster_stats st;
  { const int rc = clusters_device(c, first, n, *cfg, false, false, d, &st); if (rc) return rc; }
  if (removed) *removed = 0;
  if (stats) *stats = st;
  if (st.sel_points == 0) return FLIMO_OK;             // removing nothing changes nothing
  return map_remove_masked(c, d.mask, first, n, (size_t)st.sel_points, &c->cluster_removals, &c->cluster_removed, removed, "remove clusters");
}
extern "C" int flimo_set_cluster_chunk(flimo_ctx* c, size_t n) { return set_chunk(c, &flimo_ctx::cluster_chunk, n, (size_t)1 << 20); }

// ---- RANSAC planes of the stored points (pcl::SACSegmentation's sample, model and count; ExtractIndices for the removal) ----------
// kernels: flimo_plane.hip.  The triplets go up once; the hypotheses run in chunks of c->plane_chunk: per chunk the solve, the count
// over every stored point and the finish are launched, into result arrays that hold all nh, and nothing waits between chunks (the
// chunk's scratch is re-used in stream order); the results come back behind the last chunk, one wait.  Device scratch: chunk x
// slabs x 12 B of partials and 36 B a hypothesis of the chunk (record, survivor entry), 60 B a hypothesis of the call (triplet,
// status, inliers, sum, plane).  Reads d_map_raw alone: no index is needed, but a map never goes without one (ensure_index).
static bool plane_cfg_ok(const flimo_plane_cfg* k) {
  if (std::isnan(k->dist) || k->dist < 0.f || std::isnan(k->min_edge) || k->min_edge < 0.f) return false;
  if (std::isnan(k->min_sin) || k->min_sin < 0.f || k->min_sin > 1.f || std::isnan(k->min_cos) || k->min_cos < 0.f || k->min_cos > 1.f) return false;
  if (k->min_cos > 0.f && !(std::isfinite(k->axis[0]) && std::isfinite(k->axis[1]) && std::isfinite(k->axis[2]))) return false;
  return true;
}
extern "C" int flimo_map_planes(flimo_ctx* c, const int32_t* tri, size_t nh, const flimo_plane_cfg* cfg, int32_t* status, int32_t* inliers,
                                double* sum_sq, double* plane) {
  if (!c) return FLIMO_ERR_INVALID;
  if (!cfg || !status || !inliers || !sum_sq || (nh > 0 && !tri))
    return fail(c, FLIMO_ERR_INVALID, "map planes: null tri / cfg / status / inliers / sum_sq");
  if (!plane_cfg_ok(cfg))
    return fail(c, FLIMO_ERR_INVALID, "map planes: dist and min_edge must be >= 0 (dist may be INFINITY), min_sin and min_cos in 0..1, the axis finite");
  const size_t N = c->map_n;
  if (N >= 0x80000000ull || nh >= 0x80000000ull) return fail(c, FLIMO_ERR_TOO_LARGE, "map planes: the map and nh must be below 2^31");
  if (nh == 0) return FLIMO_OK;
  for (size_t i = 0; i < 3 * nh; i++)
    if (tri[i] < 0 || (size_t)tri[i] >= N)
      return fail(c, FLIMO_ERR_INVALID, "map planes: index %d of hypothesis %zu is outside [0, %zu)", (int)tri[i], i / 3, N);
  { const int rc0 = ensure_index(c); if (rc0) return rc0; }
  ctx_enter(c);
  const size_t slabs = plane_slabs((unsigned)N);
  // hypotheses of a chunk: the grid's second dimension and 2^26 partials bound it
  size_t k = std::min(nh, std::max<size_t>(c->plane_chunk, 1));
  k = std::min(k, std::min<size_t>((size_t)1 << 16, std::max<size_t>(((size_t)1 << 26) / slabs, 1)));
  DevScratch d;
  int32_t* d_tri = d.get<int32_t>(3 * nh);
  int32_t* d_status = d.get<int32_t>(nh);
  int32_t* d_inliers = d.get<int32_t>(nh);
  double* d_sum = d.get<double>(nh);
  double* d_plane = d.get<double>(4 * nh);
  float4* d_rec = d.get<float4>(2 * k);
  int32_t* d_surv = d.get<int32_t>(k);
  unsigned* d_nsurv = d.get<unsigned>(1);
  int32_t* d_pcnt = d.get<int32_t>(k * slabs);
  double* d_psum = d.get<double>(k * slabs);
  { const int rc = d.ok(c); if (rc) return rc; }
  HIPCHK(c, hipMemcpyAsync(d_tri, tri, 3 * nh * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  for (size_t a = 0; a < nh; a += k) {
    const size_t ka = std::min(k, nh - a);
    HIPCHK(c, launch_plane_chunk(c->stream, c->d_map_raw, (unsigned)N, d_tri + 3 * a, (unsigned)ka, cfg->dist, cfg->min_edge, cfg->min_sin, cfg->axis,
                                 cfg->min_cos, d_status + a, d_plane + 4 * a, d_inliers + a, d_sum + a, d_rec, d_surv, d_nsurv, d_pcnt, d_psum));
  }
  // (into the stage first: the caller's arrays stay untouched if anything above or below fails)
  const size_t per = sizeof(int32_t) * 2 + sizeof(double) * (plane ? 5 : 1);
  { const int rc = ensure_stage(c, nh * per); if (rc) return rc; }
  double* h_sum = (double*)c->h_stage;
  double* h_plane = h_sum + nh;
  int32_t* h_status = (int32_t*)(h_sum + nh * (plane ? 5 : 1));
  int32_t* h_inliers = h_status + nh;
  HIPCHK(c, hipMemcpyAsync(h_sum, d_sum, nh * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (plane) HIPCHK(c, hipMemcpyAsync(h_plane, d_plane, 4 * nh * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(h_status, d_status, nh * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(h_inliers, d_inliers, nh * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(sum_sq, h_sum, nh * sizeof(double));
  if (plane) memcpy(plane, h_plane, 4 * nh * sizeof(double));
  memcpy(status, h_status, nh * sizeof(int32_t));
  memcpy(inliers, h_inliers, nh * sizeof(int32_t));
  return FLIMO_OK;
}
extern "C" int flimo_plane_solve_host(const float p3[9], const flimo_plane_cfg* cfg, double plane4[4], float nf[3]) {
  if (!p3 || !cfg || !plane4 || !nf || !plane_cfg_ok(cfg)) return FLIMO_ERR_INVALID;
  return plane_solve(p3, cfg->min_edge, cfg->min_sin, cfg->axis, cfg->min_cos, plane4, nf);
}
extern "C" int flimo_set_plane_chunk(flimo_ctx* c, size_t n) { return set_chunk(c, &flimo_ctx::plane_chunk, n, (size_t)1 << 10); }
static int plane_sel_check(flimo_ctx* c, size_t first, size_t n, const flimo_plane_sel* sel, const char* what) {
  if (!sel) return fail(c, FLIMO_ERR_INVALID, "%s: null sel", what);
  for (int a = 0; a < 3; a++)
    if (!std::isfinite(sel->normal[a]) || !std::isfinite(sel->anchor[a])) return fail(c, FLIMO_ERR_INVALID, "%s: normal and anchor must be finite", what);
  if (std::isnan(sel->dist) || sel->dist < 0.f) return fail(c, FLIMO_ERR_INVALID, "%s: dist must be >= 0 or INFINITY", what);
  if (sel->side < -1 || sel->side > 1) return fail(c, FLIMO_ERR_INVALID, "%s: side must be -1, 0 or 1", what);
  { const int rc = check_range(c, what, first, n); if (rc) return rc; }
  return check_map_size(c, what);
}
// the mask of the range on the device (d_mask [n], may be null) and its ones; arguments checked, n > 0; ends synchronised
static int plane_mask_device(flimo_ctx* c, size_t first, size_t n, const flimo_plane_sel& sel, unsigned char* d_mask, unsigned* d_count, size_t* count) {
  HIPCHK(c, hipMemsetAsync(d_count, 0, sizeof(unsigned), c->stream));
  HIPCHK(c, launch_plane_mask(c->stream, c->d_map_raw, (unsigned)first, (unsigned)n, sel.normal, sel.anchor, sel.dist, sel.side, d_mask, d_count));
  unsigned w = 0;
  HIPCHK(c, hipMemcpyAsync(&w, d_count, sizeof w, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (w > n) return fail(c, FLIMO_ERR_HIP, "plane mask: marked %u of %zu points", w, n);
  *count = w;
  return FLIMO_OK;
}
extern "C" int flimo_map_plane_mask(flimo_ctx* c, size_t first, size_t n, const flimo_plane_sel* sel, unsigned char* mask, size_t* count) {
  if (!c) return FLIMO_ERR_INVALID;
  { const int rc = plane_sel_check(c, first, n, sel, "plane mask"); if (rc) return rc; }
  if (n == 0) { if (count) *count = 0; return FLIMO_OK; }
  { const int rc0 = ensure_index(c); if (rc0) return rc0; }
  ctx_enter(c);
  DevScratch d;
  unsigned char* d_mask = mask ? d.get<unsigned char>(n) : nullptr;
  unsigned* d_count = d.get<unsigned>(1);
  { const int rc = d.ok(c); if (rc) return rc; }
  size_t ones = 0;
  { const int rc = plane_mask_device(c, first, n, *sel, d_mask, d_count, &ones); if (rc) return rc; }
  if (mask) {
    HIPCHK(c, hipMemcpyAsync(mask, d_mask, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (count) *count = ones;
  return FLIMO_OK;
}
extern "C" int flimo_map_remove_plane(flimo_ctx* c, size_t first, size_t n, const flimo_plane_sel* sel, size_t* removed) {
  if (!c) return FLIMO_ERR_INVALID;
  { const int rc = plane_sel_check(c, first, n, sel, "remove plane"); if (rc) return rc; }
  if (n == 0) { if (removed) *removed = 0; return FLIMO_OK; }
  { const int rc0 = ensure_index(c); if (rc0) return rc0; }
  ctx_enter(c);
  DevScratch d;
  unsigned char* d_mask = d.get<unsigned char>(n);
  unsigned* d_count = d.get<unsigned>(1);
  { const int rc = d.ok(c); if (rc) return rc; }
  size_t ones = 0;
  { const int rc = plane_mask_device(c, first, n, *sel, d_mask, d_count, &ones); if (rc) return rc; }
  if (removed) *removed = 0;
  if (ones == 0) return FLIMO_OK;                      // removing nothing changes nothing
  return map_remove_masked(c, d_mask, first, n, ones, &c->plane_removals, &c->plane_removed, removed, "remove plane");
}

// ---- voxel statistics and thinning of the stored points (pcl::VoxelGrid's leaves over the map, on a lattice that stays put) -------
// kernels: flimo_voxel.hip.  Keys, sort, heads and scan; the host reads the voxel count (one wait) and sizes the per-voxel arrays;
// segments, classes and -- where centroid, cov or the nearest member are wanted -- the run numbers; the host reads the classes' sizes
// (a second wait); moments; the per-point stage; the results come back through the pinned stage, so the caller's arrays stay
// untouched if anything fails.  Device scratch: 32 B a stored point (two key and two index arrays, head, scan; the 12 B of the
// sort's inputs are freed behind it) plus the sort's temporary storage, 16 B more a point under the sorted-copy plan; 24 B a voxel,
// 48 B more with the centroid and 52 B more with covariance and nearest; 84 B a run slot of the many-runs path (24 B without the
// second pass); 5 B a point of the range.
static void voxel_stats_none(flimo_voxel_stats* s) {
  if (s) s->n = s->voxels = s->largest = s->outside = s->sel_points = 0;
}
static bool voxel_cfg_ok(const flimo_voxel_cfg* k) {
  if (!(k->leaf > 0.f) || std::isinf(k->leaf) || !std::isfinite(1.0f / k->leaf)) return false;      // (a NaN fails the first test)
  if (k->keep < FLIMO_VOXEL_KEEP_FIRST || k->keep > FLIMO_VOXEL_KEEP_NEAREST || k->max_pts < 1) return false;
  return !(k->keep == FLIMO_VOXEL_KEEP_NEAREST && k->max_pts != 1);
}
static int voxel_check(flimo_ctx* c, size_t first, size_t n, const flimo_voxel_cfg* cfg, const char* what) {
  if (!cfg) return fail(c, FLIMO_ERR_INVALID, "%s: null cfg", what);
  if (!voxel_cfg_ok(cfg))
    return fail(c, FLIMO_ERR_INVALID, "%s: leaf must be finite and > 0 with a finite 1 / leaf, keep 0 or 1, max_pts >= 1 (1 with keep nearest)", what);
  { const int rc = check_range(c, what, first, n); if (rc) return rc; }
  return check_map_size(c, what);
}
struct VoxelDev {      // what voxels_device leaves on the device for its caller, and the owner of all it allocated
  DevScratch mem;
  size_t nv = 0;
  int32_t* ijk = nullptr; int32_t* count = nullptr; int32_t* first = nullptr; int32_t* rep = nullptr;
  double* centroid = nullptr; double* cov = nullptr;
  int32_t* voxel = nullptr; unsigned char* mask = nullptr;
};
// the voxels of the whole map and the selection over [first, first + n), arguments checked, map not empty.  moments: 0 none, 1 the
// centroid, 2 covariance and nearest as well.  cap: FLIMO_ERR_TOO_LARGE when the map has more voxels (d.nv is set first).  Ends
// synchronised; *st on the host.
static int voxels_device(flimo_ctx* c, size_t first, size_t n, const flimo_voxel_cfg& cfg, int moments, size_t cap, bool want_voxel, bool want_mask,
                         VoxelDev& d, flimo_voxel_stats* st) {
  { const int rc0 = ensure_index(c); if (rc0) return rc0; }
  ctx_enter(c);
  const size_t N = c->map_n;
  const int plan = c->voxel_plan;
  if (cfg.keep == FLIMO_VOXEL_KEEP_NEAREST) moments = 2;
  size_t tmp_bytes = 0;
  HIPCHK(c, voxel_tmp_bytes(N, &tmp_bytes));
  unsigned long long* d_keys_in = d.mem.get<unsigned long long>(N);
  unsigned long long* d_keys = d.mem.get<unsigned long long>(N);
  uint32_t* d_vals_in = d.mem.get<uint32_t>(N);
  uint32_t* d_perm = d.mem.get<uint32_t>(N);
  uint32_t* d_head = d.mem.get<uint32_t>(N);
  uint32_t* d_pos = d.mem.get<uint32_t>(N);
  uint32_t* d_words = d.mem.get<uint32_t>(VOXEL_WORDS);
  void* d_tmp = d.mem.get<unsigned char>(tmp_bytes);
  { const int rc = d.mem.ok(c); if (rc) return rc; }
  HIPCHK(c, hipMemsetAsync(d_words, 0, VOXEL_WORDS * sizeof(uint32_t), c->stream));
  HIPCHK(c, launch_voxel_sort(c->stream, c->d_map_raw, (unsigned)N, 1.0f / cfg.leaf, d_keys_in, d_keys, d_vals_in, d_perm, d_head, d_pos, d_tmp,
                              tmp_bytes, d_words));
  uint32_t h3[3] = {0, 0, 0};      // {scan of the last position, its head flag, the outside points}
  HIPCHK(c, hipMemcpyAsync(&h3[0], d_pos + (N - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&h3[1], d_head + (N - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&h3[2], d_words + VOXEL_W_OUTSIDE, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t nv = (size_t)h3[0] + h3[1], outside = h3[2];
  if (nv > N || outside > N || (nv == 0) != (outside == N))
    return fail(c, FLIMO_ERR_HIP, "map voxels: counted %zu voxels and %zu outside points of %zu points", nv, outside, N);
  d.nv = nv;
  if (nv > cap) return fail(c, FLIMO_ERR_TOO_LARGE, "map voxels: the map has %zu voxels, the arrays hold %zu", nv, cap);
  d.mem.drop(d_keys_in);
  d.mem.drop(d_vals_in);
  uint32_t* d_seg = d.mem.get<uint32_t>(nv + 1);
  d.ijk = d.mem.get<int32_t>(3 * nv + 1);
  d.first = d.mem.get<int32_t>(nv + 1);
  d.count = d.mem.get<int32_t>(nv + 1);
  uint32_t* d_runs = nullptr; uint32_t* d_roff = nullptr; uint32_t* d_lists = nullptr;
  if (moments) {
    d_runs = d.mem.get<uint32_t>(nv + 1);
    d_roff = d.mem.get<uint32_t>(nv + 1);
    d_lists = d.mem.get<uint32_t>(4 * nv + 1);
    d.centroid = d.mem.get<double>(3 * nv + 1);
    if (moments > 1) {
      d.cov = d.mem.get<double>(6 * nv + 1);
      d.rep = d.mem.get<int32_t>(nv + 1);
    }
  }
  { const int rc = d.mem.ok(c); if (rc) return rc; }
  HIPCHK(c, launch_voxel_classify(c->stream, d_keys, d_perm, d_head, d_pos, (unsigned)N, (unsigned)nv, (unsigned)(N - outside), plan, d_seg, d.ijk,
                                  d.first, d.count, d_runs, d_roff, d_lists, d_tmp, tmp_bytes, d_words));
  uint32_t w[VOXEL_WORDS] = {0};
  uint32_t R = 0;
  HIPCHK(c, hipMemcpyAsync(w, d_words, sizeof w, hipMemcpyDeviceToHost, c->stream));
  if (moments) HIPCHK(c, hipMemcpyAsync(&R, d_roff + nv, sizeof R, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const unsigned* nl = w + VOXEL_W_LIST;
  if (w[VOXEL_W_LARGEST] > N || (nv > 0 && w[VOXEL_W_LARGEST] < 1) ||
      (moments && ((size_t)nl[0] + nl[1] + nl[2] + nl[3] != nv || (size_t)R > N / 64 + nv)))
    return fail(c, FLIMO_ERR_HIP, "map voxels: the classes hold %u + %u + %u + %u of %zu voxels, %u run slots, largest %u", nl[0], nl[1], nl[2],
                nl[3], nv, R, w[VOXEL_W_LARGEST]);
  if (moments && nv > 0) {
    double* d_rs = nullptr; double* d_rc = nullptr; double* d_rq = nullptr; uint32_t* d_rp = nullptr;
    if (nl[3]) {
      d_rs = d.mem.get<double>(3 * (size_t)R);
      if (moments > 1) {
        d_rc = d.mem.get<double>(6 * (size_t)R);
        d_rq = d.mem.get<double>(R);
        d_rp = d.mem.get<uint32_t>(R);
      }
    }
    const float4* pts = c->d_map_raw;
    const uint32_t* gather = d_perm;
    if (plan & VOXEL_PLAN_SORTED) {
      float4* d_sorted = d.mem.get<float4>(N);
      { const int rc = d.mem.ok(c); if (rc) return rc; }
      HIPCHK(c, launch_voxel_sorted_copy(c->stream, c->d_map_raw, d_perm, (unsigned)N, d_sorted));
      pts = d_sorted;
      gather = nullptr;
    }
    { const int rc = d.mem.ok(c); if (rc) return rc; }
    HIPCHK(c, launch_voxel_moments(c->stream, pts, gather, d_perm, d_seg, (unsigned)nv, d_lists, nl, d_roff, R, moments > 1, d_rs, d_rc, d_rq, d_rp,
                                   d.centroid, d.cov, d.rep));
  }
  if (cfg.keep == FLIMO_VOXEL_KEEP_FIRST) d.rep = d.first;      // (the oldest member)
  uint32_t sel = 0;
  if (n > 0) {
    if (want_voxel) d.voxel = d.mem.get<int32_t>(n);
    if (want_mask) d.mask = d.mem.get<unsigned char>(n);
    { const int rc = d.mem.ok(c); if (rc) return rc; }
    HIPCHK(c, launch_voxel_points(c->stream, d_keys, d_perm, d_head, d_pos, d_seg, d.rep, (unsigned)N, (unsigned)first, (unsigned)n, cfg.keep,
                                  (unsigned)cfg.max_pts, d.voxel, d.mask, d_words));
    HIPCHK(c, hipMemcpyAsync(&sel, d_words + VOXEL_W_SEL, sizeof sel, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((size_t)sel > n) return fail(c, FLIMO_ERR_HIP, "map voxels: selected %u of %zu points", sel, n);
  st->n = n; st->voxels = nv; st->largest = w[VOXEL_W_LARGEST]; st->outside = outside; st->sel_points = sel;
  return FLIMO_OK;
}
extern "C" int flimo_map_voxels(flimo_ctx* c, const flimo_voxel_cfg* cfg, size_t cap, size_t* nv, int32_t* ijk, int32_t* count, int32_t* first,
                                int32_t* rep, double* centroid, double* cov, flimo_voxel_stats* stats) {
  if (!c) return FLIMO_ERR_INVALID;
  { const int rc = voxel_check(c, 0, 0, cfg, "map voxels"); if (rc) return rc; }
  const size_t N = c->map_n;
  if (N == 0) { if (nv) *nv = 0; voxel_stats_none(stats); return FLIMO_OK; }
  const bool arrays = ijk || count || first || rep || centroid || cov;
  VoxelDev d;
  flimo_voxel_stats st;
  const int moments = cov ? 2 : centroid ? 1 : 0;
  {
    // (the selection is counted over the whole map, and only where the stats are asked for)
    const int rc = voxels_device(c, 0, stats ? N : 0, *cfg, moments, arrays ? cap : (size_t)-1, false, false, d, &st);
    if (nv && (rc == FLIMO_OK || (rc == FLIMO_ERR_TOO_LARGE && d.nv > cap))) *nv = d.nv;
    if (rc) return rc;
  }
  const size_t m = d.nv;
  if (arrays && m > 0) {
    const size_t bytes = m * ((centroid ? 24 : 0) + (cov ? 48 : 0) + (ijk ? 12 : 0) + (count ? 4 : 0) + (first ? 4 : 0) + (rep ? 4 : 0));
    { const int rc = ensure_stage(c, bytes); if (rc) return rc; }
    char* h = (char*)c->h_stage;      // (the float64 arrays first: every part stays aligned)
    struct Part { void* dst; const void* src; size_t bytes; char* at; } parts[6] = {
        {centroid, d.centroid, 24 * m, nullptr}, {cov, d.cov, 48 * m, nullptr}, {ijk, d.ijk, 12 * m, nullptr},
        {count, d.count, 4 * m, nullptr},        {first, d.first, 4 * m, nullptr}, {rep, d.rep, 4 * m, nullptr}};
    for (Part& p : parts) {
      if (!p.dst) continue;
      p.at = h;
      h += p.bytes;
      HIPCHK(c, hipMemcpyAsync(p.at, p.src, p.bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (const Part& p : parts)
      if (p.dst) memcpy(p.dst, p.at, p.bytes);
  }
  if (stats) *stats = st;
  return FLIMO_OK;
}
extern "C" int flimo_map_voxel_mask(flimo_ctx* c, size_t first, size_t n, const flimo_voxel_cfg* cfg, int32_t* voxel, unsigned char* mask,
                                    flimo_voxel_stats* stats) {
  if (!c) return FLIMO_ERR_INVALID;
  { const int rc = voxel_check(c, first, n, cfg, "voxel mask"); if (rc) return rc; }
  if (c->map_n == 0) { voxel_stats_none(stats); return FLIMO_OK; }
  if (n == 0 && !stats) return FLIMO_OK;
  VoxelDev d;
  flimo_voxel_stats st;
  { const int rc = voxels_device(c, first, n, *cfg, 0, (size_t)-1, voxel != nullptr, mask != nullptr, d, &st); if (rc) return rc; }
  if (n > 0 && (voxel || mask)) {
    { const int rc = ensure_stage(c, n * 5); if (rc) return rc; }
    int32_t* h_voxel = (int32_t*)c->h_stage;
    unsigned char* h_mask = (unsigned char*)c->h_stage + 4 * n;
    if (voxel) HIPCHK(c, hipMemcpyAsync(h_voxel, d.voxel, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (mask) HIPCHK(c, hipMemcpyAsync(h_mask, d.mask, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (voxel) memcpy(voxel, h_voxel, n * sizeof(int32_t));
    if (mask) memcpy(mask, h_mask, n);
  }
  if (stats) *stats = st;
  return FLIMO_OK;
}
extern "C" int flimo_map_thin(flimo_ctx* c, size_t first, size_t n, const flimo_voxel_cfg* cfg, size_t* removed, flimo_voxel_stats* stats) {
  if (!c) return FLIMO_ERR_INVALID;
  { const int rc = voxel_check(c, first, n, cfg, "map thin"); if (rc) return rc; }
  if (c->map_n == 0) { if (removed) *removed = 0; voxel_stats_none(stats); return FLIMO_OK; }
  if (n == 0 && !stats) { if (removed) *removed = 0; return FLIMO_OK; }
  VoxelDev d;
  flimo_voxel_stats st;
  { const int rc = voxels_device(c, first, n, *cfg, 0, (size_t)-1, false, true, d, &st); if (rc) return rc; }
  if (removed) *removed = 0;
  if (stats) *stats = st;
  if (st.sel_points == 0) return FLIMO_OK;             // removing nothing changes nothing
  return map_remove_masked(c, d.mask, first, n, (size_t)st.sel_points, &c->thin_removals, &c->thin_removed, removed, "map thin");
}
extern "C" int flimo_voxel_key_host(const float p[3], float leaf, int32_t ijk[3], uint64_t* key) {
  const flimo_voxel_cfg k{leaf, FLIMO_VOXEL_KEEP_FIRST, 1};
  if (!p || !voxel_cfg_ok(&k)) return FLIMO_ERR_INVALID;
  int32_t cell[3];
  unsigned long long kk = 0;
  const bool inside = voxel_key(p[0], p[1], p[2], 1.0f / leaf, cell, &kk);
  if (ijk) { ijk[0] = cell[0]; ijk[1] = cell[1]; ijk[2] = cell[2]; }
  if (key) *key = kk;
  return inside ? 0 : 1;
}

// ---- smooth-surface regions of the stored points (pcl::RegionGrowing over the map, without its seed order) -----------------------
// kernels: flimo_region.hip.  On the context's stream over the WHOLE map whatever the range (a region can reach anywhere): the
// normals of flimo_map_normals_range left on the device, in chunks of c->normals_chunk points as flimo_map_fpfh forms them (three
// launches a chunk); init, link in chunks of c->region_chunk stored points, flatten, count, finish; then the copies back, one wait.
// Scratch: 28 B a stored point (normal, parent, count, attach), 84 B a point of a normals chunk (moments, count, worklist), 1 B a
// point of the range (mask), 4 B each for label and size where they are asked for; nothing of points x neighbours exists anywhere.
// The listing adds the voxels' sort (32 B a stored point plus the sort's own) and at most 116 B a listed region, 84 B a run of a
// region above 1024 points.  The removal hands the device mask to the crop's ordered compaction (map_remove_masked).
static void region_stats_none(flimo_region_stats* s) {
  if (s) s->n = s->smooth = s->regions = s->largest = s->sel_regions = s->unassigned = s->sel_points = 0;
}
static bool region_cfg_ok(const flimo_region_cfg* k) {      // (every test fails for a NaN)
  return k->tol >= 0.f && !std::isinf(k->tol) && k->min_cos >= 0.f && k->min_cos <= 1.f && k->max_curv >= 0.f;
}
static int region_check(flimo_ctx* c, size_t first, size_t n, const flimo_region_cfg* cfg, const char* what) {
  if (!cfg) return fail(c, FLIMO_ERR_INVALID, "%s: null cfg", what);
  { const int rc = check_range(c, what, first, n); if (rc) return rc; }
  if (!region_cfg_ok(cfg))
    return fail(c, FLIMO_ERR_INVALID, "%s: tol must be finite and >= 0, min_cos in 0..1, max_curv >= 0 or INFINITY", what);
  { const int rc = check_gate(c, what, cfg->normal_max_dist); if (rc) return rc; }
  if (cfg->normal_min_pts < 0) return fail(c, FLIMO_ERR_INVALID, "%s: normal_min_pts must be >= 0", what);
  if (cfg->min_size < 0 || cfg->max_size < 0) return fail(c, FLIMO_ERR_INVALID, "%s: min_size and max_size must be >= 0", what);
  if (cfg->max_size > 0 && cfg->max_size < cfg->min_size) return fail(c, FLIMO_ERR_INVALID, "%s: max_size must be 0 or >= min_size", what);
  if (cfg->normal_k < 1 || cfg->normal_k > FLIMO_KNN_MAX_K) return fail(c, FLIMO_ERR_UNSUPPORTED, "%s: normal_k must be in 1..%d", what, FLIMO_KNN_MAX_K);
  return check_map_size(c, what);
}
struct RegionDev {      // what regions_device leaves on the device for its caller, and the owner of all it allocated
  DevScratch mem;
  int32_t* label = nullptr; int32_t* size = nullptr; unsigned char* mask = nullptr;
  unsigned long long* keys = nullptr; uint32_t* vals = nullptr;      // the listing's key and index of every stored point
  size_t listed = 0;                                                 // stored points in selected regions
};
// the regions of the whole map and the selection over [first, first + n), arguments checked, map not empty: where asked for d.mask
// (n > 0), d.label / d.size and d.keys / d.vals filled on the device, *st on the host; ends synchronised
static int regions_device(flimo_ctx* c, size_t first, size_t n, const flimo_region_cfg& cfg, bool want_label, bool want_size, bool want_mask,
                          bool want_keys, RegionDev& d, flimo_region_stats* st) {
  { const int rc = need_index(c, "map regions"); if (rc) return rc; }
  ctx_enter(c);
  const size_t N = c->map_n;
  const size_t mn = std::min(N, std::max<size_t>(c->normals_chunk, 1));
  const size_t ml = std::min(std::min(N, std::max<size_t>(c->region_chunk, 1)), (size_t)1 << 24);      // (x 64 lanes: below 2^31 a launch)
  float4* d_normal = d.mem.get<float4>(N);
  uint32_t* d_parent = d.mem.get<uint32_t>(N);
  uint32_t* d_count = d.mem.get<uint32_t>(N);
  uint32_t* d_attach = d.mem.get<uint32_t>(N);
  uint32_t* d_words = d.mem.get<uint32_t>(REGION_WORDS);
  int32_t* d_ncnt = d.mem.get<int32_t>(mn);
  double* d_mom = d.mem.get<double>(mn * 9);
  uint2* d_work = d.mem.get<uint2>(mn);
  unsigned* d_nwork = d.mem.get<unsigned>(1);
  if (n > 0 && want_mask) d.mask = d.mem.get<unsigned char>(n);
  if (n > 0 && want_label) d.label = d.mem.get<int32_t>(n);
  if (n > 0 && want_size) d.size = d.mem.get<int32_t>(n);
  if (want_keys) { d.keys = d.mem.get<unsigned long long>(N); d.vals = d.mem.get<uint32_t>(N); }
  { const int rc = d.mem.ok(c); if (rc) return rc; }
  // (a chunk's worklist and moments are read by its own launches only: the stream orders the chunks, nothing waits in between)
  for (size_t a = 0; a < N; a += mn)
    HIPCHK(c, launch_knn_k_normals(c->stream, c->grid, c->d_map_raw, nullptr, (unsigned)a, (int)std::min(mn, N - a), cfg.normal_k, cfg.normal_max_dist,
                                   cfg.normal_min_pts, nullptr, d_normal + a, d_ncnt, nullptr, nullptr, nullptr, d_mom, d_work, d_nwork));
  HIPCHK(c, hipMemsetAsync(d_words, 0, REGION_WORDS * sizeof(uint32_t), c->stream));
  HIPCHK(c, launch_region_init(c->stream, d_parent, d_count, d_attach, N));
  for (size_t a = 0; a < N; a += ml)
    HIPCHK(c, launch_region_link(c->stream, c->grid, c->d_map_raw, d_normal, (unsigned)a, (int)std::min(ml, N - a), cfg.tol, cfg.min_cos, cfg.max_curv,
                                 cfg.border, d_parent, d_attach));
  HIPCHK(c, launch_region_labels(c->stream, d_parent, d_attach, d_normal, cfg.max_curv, d_count, d_words, N));
  HIPCHK(c, launch_region_finish(c->stream, d_parent, d_count, N, first, n, cfg.min_size, cfg.max_size, d.label, d.size, d.mask,
                                 d.keys, d.vals, d_words));
  uint32_t w[REGION_WORDS] = {0};
  HIPCHK(c, hipMemcpyAsync(w, d_words, sizeof w, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint32_t regions = w[REGION_W_REGIONS], smooth = w[REGION_W_SMOOTH], none = w[REGION_W_UNASSIGNED];
  if (smooth > N || none > N - smooth || regions > smooth || (regions == 0) != (smooth == 0) || w[REGION_W_LARGEST] > N - none ||
      (regions > 0 && w[REGION_W_LARGEST] < 1) || w[REGION_W_SEL] > regions || w[REGION_W_SEL_PTS] > n || w[REGION_W_LISTED] > N - none)
    return fail(c, FLIMO_ERR_HIP, "map regions: counted %u regions (largest %u, %u selected, %u points) of %u smooth and %u unassigned of %zu points",
                regions, w[REGION_W_LARGEST], w[REGION_W_SEL], w[REGION_W_SEL_PTS], smooth, none, N);
  d.listed = w[REGION_W_LISTED];
  st->n = n; st->smooth = smooth; st->regions = regions; st->largest = w[REGION_W_LARGEST]; st->sel_regions = w[REGION_W_SEL];
  st->unassigned = none; st->sel_points = w[REGION_W_SEL_PTS];
  return FLIMO_OK;
}
extern "C" int flimo_map_regions(flimo_ctx* c, size_t first, size_t n, const flimo_region_cfg* cfg, int32_t* label, int32_t* size,
                                 unsigned char* mask, flimo_region_stats* stats) {
  if (!c) return FLIMO_ERR_INVALID;
  { const int rc = region_check(c, first, n, cfg, "map regions"); if (rc) return rc; }
  if (c->map_n == 0) { region_stats_none(stats); return FLIMO_OK; }
  if (n == 0 && !stats) return FLIMO_OK;
  RegionDev d;
  flimo_region_stats st;
  { const int rc = regions_device(c, first, n, *cfg, label != nullptr, size != nullptr, mask != nullptr, false, d, &st); if (rc) return rc; }
  if (n > 0 && (label || size || mask)) {
    if (label) HIPCHK(c, hipMemcpyAsync(label, d.label, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (size) HIPCHK(c, hipMemcpyAsync(size, d.size, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (mask) HIPCHK(c, hipMemcpyAsync(mask, d.mask, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (stats) *stats = st;
  return FLIMO_OK;
}
extern "C" int flimo_map_region_list(flimo_ctx* c, const flimo_region_cfg* cfg, size_t cap, size_t* nr, int32_t* label, int32_t* count,
                                     int32_t* first, double* centroid, double* cov, flimo_region_stats* stats) {
  if (!c) return FLIMO_ERR_INVALID;
  { const int rc = region_check(c, 0, 0, cfg, "map region list"); if (rc) return rc; }
  const size_t N = c->map_n;
  if (N == 0) { if (nr) *nr = 0; region_stats_none(stats); return FLIMO_OK; }
  const bool arrays = label || count || first || centroid || cov;
  if (!arrays && !nr && !stats) return FLIMO_OK;      // nothing is asked for
  RegionDev d;
  flimo_region_stats st;
  { const int rc = regions_device(c, 0, N, *cfg, false, false, false, arrays, d, &st); if (rc) return rc; }
  const size_t m = (size_t)st.sel_regions;
  if (nr) *nr = m;
  if (arrays && m > cap) return fail(c, FLIMO_ERR_TOO_LARGE, "map region list: %zu regions are selected, the arrays hold %zu", m, cap);
  if (arrays && m > 0) {
    // the voxels' machinery behind ready keys: a stable sort (members in ascending insertion index), heads, classes, moments
    const int moments = cov ? 2 : centroid ? 1 : 0;
    size_t tmp_bytes = 0;
    HIPCHK(c, voxel_tmp_bytes(N, &tmp_bytes));
    unsigned long long* d_keys = d.mem.get<unsigned long long>(N);
    uint32_t* d_perm = d.mem.get<uint32_t>(N);
    uint32_t* d_head = d.mem.get<uint32_t>(N);
    uint32_t* d_pos = d.mem.get<uint32_t>(N);
    uint32_t* d_vwords = d.mem.get<uint32_t>(VOXEL_WORDS);
    void* d_tmp = d.mem.get<unsigned char>(tmp_bytes);
    uint32_t* d_seg = d.mem.get<uint32_t>(m + 1);
    int32_t* d_label = d.mem.get<int32_t>(m);
    int32_t* d_first = d.mem.get<int32_t>(m);
    int32_t* d_cnt = d.mem.get<int32_t>(m);
    uint32_t* d_runs = nullptr; uint32_t* d_roff = nullptr; uint32_t* d_lists = nullptr;
    double* d_centroid = nullptr; double* d_cov = nullptr; int32_t* d_rep = nullptr;
    if (moments) {
      d_runs = d.mem.get<uint32_t>(m + 1);
      d_roff = d.mem.get<uint32_t>(m + 1);
      d_lists = d.mem.get<uint32_t>(4 * m);
      d_centroid = d.mem.get<double>(3 * m);
      if (moments > 1) { d_cov = d.mem.get<double>(6 * m); d_rep = d.mem.get<int32_t>(m); }
    }
    { const int rc = d.mem.ok(c); if (rc) return rc; }
    HIPCHK(c, hipMemsetAsync(d_vwords, 0, VOXEL_WORDS * sizeof(uint32_t), c->stream));
    HIPCHK(c, launch_voxel_sort_keys(c->stream, (unsigned)N, d.keys, d_keys, d.vals, d_perm, d_head, d_pos, d_tmp, tmp_bytes));
    HIPCHK(c, launch_voxel_classify(c->stream, d_keys, d_perm, d_head, d_pos, (unsigned)N, (unsigned)m, (unsigned)d.listed, c->voxel_plan, d_seg, nullptr,
                                    d_first, d_cnt, d_runs, d_roff, d_lists, d_tmp, tmp_bytes, d_vwords));
    uint32_t h2[2] = {0, 0};      // {scan of the last position, its head flag}: the heads must number the selected regions
    uint32_t w[VOXEL_WORDS] = {0};
    uint32_t R = 0;
    HIPCHK(c, hipMemcpyAsync(&h2[0], d_pos + (N - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&h2[1], d_head + (N - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(w, d_vwords, sizeof w, hipMemcpyDeviceToHost, c->stream));
    if (moments) HIPCHK(c, hipMemcpyAsync(&R, d_roff + m, sizeof R, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const unsigned* nl = w + VOXEL_W_LIST;
    if ((size_t)h2[0] + h2[1] != m || w[VOXEL_W_LARGEST] > N || (moments && ((size_t)nl[0] + nl[1] + nl[2] + nl[3] != m || (size_t)R > N / 64 + m)))
      return fail(c, FLIMO_ERR_HIP, "map region list: %u heads for %zu regions, classes %u + %u + %u + %u, %u run slots", h2[0] + h2[1], m, nl[0], nl[1],
                  nl[2], nl[3], R);
    if (moments) {
      double* d_rs = nullptr; double* d_rc = nullptr; double* d_rq = nullptr; uint32_t* d_rp = nullptr;
      if (nl[3]) {
        d_rs = d.mem.get<double>(3 * (size_t)R);
        if (moments > 1) {
          d_rc = d.mem.get<double>(6 * (size_t)R);
          d_rq = d.mem.get<double>(R);
          d_rp = d.mem.get<uint32_t>(R);
        }
      }
      { const int rc = d.mem.ok(c); if (rc) return rc; }
      HIPCHK(c, launch_voxel_moments(c->stream, c->d_map_raw, d_perm, d_perm, d_seg, (unsigned)m, d_lists, nl, d_roff, R, moments > 1, d_rs, d_rc, d_rq,
                                     d_rp, d_centroid, d_cov, d_rep));
    }
    HIPCHK(c, launch_region_list_labels(c->stream, d_keys, d_seg, (unsigned)m, d_label));
    // the results come back through the pinned stage, so the caller's arrays stay untouched if anything fails
    const size_t bytes = m * ((centroid ? 24 : 0) + (cov ? 48 : 0) + (label ? 4 : 0) + (count ? 4 : 0) + (first ? 4 : 0));
    { const int rc = ensure_stage(c, bytes); if (rc) return rc; }
    char* h = (char*)c->h_stage;      // (the float64 arrays first: every part stays aligned)
    struct Part { void* dst; const void* src; size_t bytes; char* at; } parts[5] = {
        {centroid, d_centroid, 24 * m, nullptr}, {cov, d_cov, 48 * m, nullptr}, {label, d_label, 4 * m, nullptr},
        {count, d_cnt, 4 * m, nullptr},          {first, d_first, 4 * m, nullptr}};
    for (Part& p : parts) {
      if (!p.dst) continue;
      p.at = h;
      h += p.bytes;
      HIPCHK(c, hipMemcpyAsync(p.at, p.src, p.bytes, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (const Part& p : parts)
      if (p.dst) memcpy(p.dst, p.at, p.bytes);
  }
  if (stats) *stats = st;
  return FLIMO_OK;
}
extern "C" int flimo_map_remove_regions(flimo_ctx* c, size_t first, size_t n, const flimo_region_cfg* cfg, size_t* removed,
                                        flimo_region_stats* stats) {
  if (!c) return FLIMO_ERR_INVALID;
  { const int rc = region_check(c, first, n, cfg, "remove regions"); if (rc) return rc; }
  if (c->map_n == 0) { if (removed) *removed = 0; region_stats_none(stats); return FLIMO_OK; }
  if (n == 0 && !stats) { if (removed) *removed = 0; return FLIMO_OK; }
  RegionDev d;
  flimo_region_stats st;
  { const int rc = regions_device(c, first, n, *cfg, false, false, true, false, d, &st); if (rc) return rc; }
  if (removed) *removed = 0;
  if (stats) *stats = st;
  if (st.sel_points == 0) return FLIMO_OK;             // removing nothing changes nothing
  return map_remove_masked(c, d.mask, first, n, (size_t)st.sel_points, &c->region_removals, &c->region_removed, removed, "remove regions");
}
extern "C" int flimo_set_region_chunk(flimo_ctx* c, size_t n) { return set_chunk(c, &flimo_ctx::region_chunk, n, (size_t)1 << 20); }
extern "C" int flimo_region_joined_host(const float pi[3], const float ni[4], const float pj[3], const float nj[4], const flimo_region_cfg* cfg,
                                        int* smooth_i, int* smooth_j, int* joined) {
  if (!pi || !ni || !pj || !nj || !cfg || !region_cfg_ok(cfg)) return FLIMO_ERR_INVALID;
  const float r2 = cfg->tol * cfg->tol;      // one float32 product
  if (smooth_i) *smooth_i = region_smooth(ni[0], ni[1], ni[2], ni[3], cfg->max_curv) ? 1 : 0;
  if (smooth_j) *smooth_j = region_smooth(nj[0], nj[1], nj[2], nj[3], cfg->max_curv) ? 1 : 0;
  if (joined)
    *joined = region_has_normal(ni[0], ni[1], ni[2], ni[3]) && region_has_normal(nj[0], nj[1], nj[2], nj[3]) &&
                      region_joined(pi, ni, pj, nj, r2, cfg->min_cos) ? 1 : 0;
  return FLIMO_OK;
}
extern "C" int flimo_set_voxel_plan(flimo_ctx* c, int plan) {
  if (!c) return FLIMO_ERR_INVALID;
  if (plan < 0 || (plan & ~VOXEL_PLAN_SORTED) > VOXEL_PLAN_RUNS) return fail(c, FLIMO_ERR_INVALID, "voxel plan: %d is none of 0..4, + 8", plan);
  c->voxel_plan = plan;
  return FLIMO_OK;
}

// ---- fitness of the resident scan under pose hypotheses (pcl::Registration::getFitnessScore over the map) ----------
// kernels: flimo_knn_k.hip.  Chunks of whole poses, c->fitness_chunk (pose, point) pairs at most unless one pose alone has more:
// per chunk the poses' matrices go up (pose_from_x26 on the host, as flimo_scan_to_world forms them), three launches (block search,
// walk over the tiles, the reduction per pose), two numbers per pose -- and the slots, where asked for -- come back; device scratch
// is the chunk's, whatever np.  Reads d_scan only: d_scan_world and the pass's buffers are left alone.
// what the entries over pose hypotheses (this one, flimo_scan_linearize, flimo_scan_ndt, flimo_scan_gicp) share: the poses' check (what: the
// caller's name in the message) ...
static int check_poses(flimo_ctx* c, const char* what, const double* x26, size_t np) {
  if (np >= 0x80000000ull) return fail(c, FLIMO_ERR_TOO_LARGE, "%s: the number of poses must be below 2^31", what);
  for (size_t j = 0; j < np; j++)
    for (int t = 0; t < 7; t++)
      if (!std::isfinite(x26[26 * j + t])) return fail(c, FLIMO_ERR_INVALID, "%s: pose %zu has a non-finite position or rotation", what, j);
  return FLIMO_OK;
}
// ... the poses per chunk of at most chunk_pairs pairs, n > 0 points each: whole poses, at least one; the kernels' pair numbers are
// 32-bit and a search launch has the poses as its grid's y ...
static size_t pose_chunk(size_t chunk_pairs, size_t n, size_t np) {
  const size_t pairs_max = std::min<size_t>(std::max<size_t>(chunk_pairs, 1), (size_t)1 << 28);
  return std::min(np, std::min<size_t>(std::max<size_t>(pairs_max / n, 1), FIT_MAX_POSES));
}
// ... the entry into the stream: a pending deskew of the resident scan runs first ...
static int enter_flushed(flimo_ctx* c) { ctx_enter(c); return flush_deskew(c); }
// ... the loop over the chunks.  m: the poses of a chunk; d_poses is the first buffer of the entry's scratch d (the entry checks
// d.ok() after its own).  run, per chunk of k poses from pose a on: the RT rows are formed in rt and go up, launch(a, k) queues the
// entry's kernels, copy_back(a, k) its hipMemcpyAsyncs (each returns a FLIMO code), one wait, then after(a, k) on the host ...
struct PoseChunks {
  size_t m;
  float* d_poses;
  std::vector<float> rt;
  PoseChunks(DevScratch& d, size_t chunk_pairs, size_t n, size_t np) : m(pose_chunk(chunk_pairs, n, np)), d_poses(d.get<float>(m * 12)), rt(m * 12) {}
  template <class Launch, class CopyBack, class After>
  int run(flimo_ctx* c, const double* x26, size_t np, Launch launch, CopyBack copy_back, After after) {
    for (size_t a = 0; a < np; a += m) {
      const size_t k = std::min(m, np - a);
      for (size_t j = 0; j < k; j++) {
        PoseMats P;
        pose_from_x26(x26 + 26 * (a + j), P);
        memcpy(&rt[12 * j], P.RT, 12 * sizeof(float));
      }
      HIPCHK(c, hipMemcpyAsync(d_poses, rt.data(), k * 12 * sizeof(float), hipMemcpyHostToDevice, c->stream));
      { const int rc = launch(a, k); if (rc) return rc; }
      { const int rc = copy_back(a, k); if (rc) return rc; }
      // (the next chunk's poses overwrite rt and d_poses: one wait per chunk)
      HIPCHK(c, hipStreamSynchronize(c->stream));
      after(a, k);
    }
    return FLIMO_OK;
  }
};
// ... a chunk's sums [k][28] taken apart into H, g and the cost or score of the poses from a on, and H and g of np poses without a term
static void unpack_sums(const double* sums, size_t a, size_t k, double* H, double* g, double* last) {
  for (size_t j = 0; j < k; j++) {
    memcpy(H + 21 * (a + j), sums + 28 * j, 21 * sizeof(double));
    memcpy(g + 6 * (a + j), sums + 28 * j + 21, 6 * sizeof(double));
    last[a + j] = sums[28 * j + 27];
  }
}
static void zero_H_g(double* H, double* g, size_t np) { std::fill_n(H, np * 21, 0.0); std::fill_n(g, np * 6, 0.0); }
extern "C" int flimo_scan_fitness(flimo_ctx* c, const double* x26, size_t np, float max_dist, int32_t* inliers, double* sum_sqd, float* nn_sqd,
                                  int32_t* nn_idx) {
  if (!c) return FLIMO_ERR_INVALID;
  if ((np > 0 && !x26) || !inliers || !sum_sqd) return fail(c, FLIMO_ERR_INVALID, "scan fitness: null poses / inliers / sum_sqd");
  { const int rc = check_gate(c, "scan fitness", max_dist); if (rc) return rc; }
  { const int rc = check_poses(c, "scan fitness", x26, np); if (rc) return rc; }
  if (np == 0) return FLIMO_OK;
  const size_t n = c->scan_n;
  { const int rc0 = ensure_index(c); if (rc0) return rc0; }
  if (n == 0 || !c->grid_valid || max_dist == 0.f) {      // an empty scan or map, a gate that admits nothing: every query is empty
    for (size_t j = 0; j < np; j++) { inliers[j] = 0; sum_sqd[j] = 0.0; }
    if (nn_sqd) for (size_t i = 0; i < np * n; i++) nn_sqd[i] = -1.f;
    if (nn_idx) for (size_t i = 0; i < np * n; i++) nn_idx[i] = -1;
    return FLIMO_OK;
  }
  { const int rcf = enter_flushed(c); if (rcf) return rcf; }
  // scratch of this call, released on every exit path
  DevScratch d;
  PoseChunks P(d, c->fitness_chunk, n, np);
  const size_t m = P.m;
  float* d_poses = P.d_poses;
  float* d_sqd = d.get<float>(m * n);
  int32_t* d_idx = nn_idx ? d.get<int32_t>(m * n) : nullptr;
  uint2* d_work = d.get<uint2>(m * n);
  unsigned* d_nwork = d.get<unsigned>(1);
  int32_t* d_inliers = d.get<int32_t>(m);
  double* d_sum = d.get<double>(m);
  { const int rc = d.ok(c); if (rc) return rc; }
  return P.run(c, x26, np,
    [&](size_t, size_t k) -> int {
      HIPCHK(c, launch_scan_fitness(c->stream, c->grid, c->d_scan, (unsigned)n, d_poses, (unsigned)k, max_dist, d_sqd, d_idx, d_work, d_nwork,
                                    d_inliers, d_sum));
      return FLIMO_OK;
    },
    [&](size_t a, size_t k) -> int {
      HIPCHK(c, hipMemcpyAsync(inliers + a, d_inliers, k * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(sum_sqd + a, d_sum, k * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      if (nn_sqd) HIPCHK(c, hipMemcpyAsync(nn_sqd + a * n, d_sqd, k * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
      if (nn_idx) HIPCHK(c, hipMemcpyAsync(nn_idx + a * n, d_idx, k * n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
      return FLIMO_OK;
    },
    [](size_t, size_t) {});
}
extern "C" int flimo_set_fitness_chunk(flimo_ctx* c, size_t pairs) { return set_chunk(c, &flimo_ctx::fitness_chunk, pairs, (size_t)1 << 22); }

// ---- pose hypotheses from point correspondences (pcl::SampleConsensusPrerejective's sample, pre-rejection, pose and count) --------
// kernels: flimo_corr.hip.  Both clouds go up once; the hypotheses run in chunks of c->corr_chunk (fewer when pair_sqd is asked for:
// at most 2^26 slots a chunk): per chunk the triplets go up, the solve, the fill of pair_sqd where asked for and the count are
// launched, and the chunk's results come back; device scratch is the chunk's, whatever nh.  Reads neither the map nor the scan.
static bool corr_cfg_ok(const flimo_corr_cfg* k) {
  return !(std::isnan(k->edge_sim) || k->edge_sim < 0.f || k->edge_sim > 1.f || std::isnan(k->min_edge) || k->min_edge < 0.f ||
           std::isnan(k->max_dist) || k->max_dist < 0.f);
}
extern "C" int flimo_corr_poses(flimo_ctx* c, const float* src_xyz, const float* dst_xyz, size_t m, const int32_t* tri, size_t nh,
                                const flimo_corr_cfg* cfg, int32_t* status, int32_t* inliers, double* sum_sqd, double* pose, float* pair_sqd) {
  if (!c) return FLIMO_ERR_INVALID;
  if (!cfg || !status || !inliers || !sum_sqd || (m > 0 && (!src_xyz || !dst_xyz)) || (nh > 0 && !tri))
    return fail(c, FLIMO_ERR_INVALID, "corr poses: null src / dst / tri / cfg / status / inliers / sum_sqd");
  if (!corr_cfg_ok(cfg)) return fail(c, FLIMO_ERR_INVALID, "corr poses: edge_sim must be in 0..1, min_edge and max_dist >= 0 (max_dist may be INFINITY)");
  if (m >= 0x80000000ull || nh >= 0x80000000ull) return fail(c, FLIMO_ERR_TOO_LARGE, "corr poses: m and nh must be below 2^31");
  if (pair_sqd && (unsigned long long)nh * (unsigned long long)m >= 0x80000000ull)
    return fail(c, FLIMO_ERR_TOO_LARGE, "corr poses: nh * m must be below 2^31 when pair_sqd is asked for");
  if (nh == 0) return FLIMO_OK;
  for (size_t i = 0; i < 3 * nh; i++)
    if (tri[i] < 0 || (size_t)tri[i] >= m)
      return fail(c, FLIMO_ERR_INVALID, "corr poses: index %d of hypothesis %zu is outside [0, %zu)", (int)tri[i], i / 3, m);
  ctx_enter(c);
  DevScratch d;
  size_t k = std::min(nh, std::max<size_t>(c->corr_chunk, 1));      // hypotheses of a chunk
  if (pair_sqd) k = std::min(k, std::max<size_t>(((size_t)1 << 26) / m, 1));
  float* d_src = d.get<float>(3 * m);
  float* d_dst = d.get<float>(3 * m);
  int32_t* d_tri = d.get<int32_t>(3 * k);
  int32_t* d_status = d.get<int32_t>(k);
  double* d_pose = d.get<double>(7 * k);
  float* d_rt = d.get<float>(12 * k);
  int32_t* d_surv = d.get<int32_t>(k);
  unsigned* d_nsurv = d.get<unsigned>(1);
  int32_t* d_inliers = d.get<int32_t>(k);
  double* d_sum = d.get<double>(k);
  float* d_pair = pair_sqd ? d.get<float>(k * m) : nullptr;
  { const int rc = d.ok(c); if (rc) return rc; }
  HIPCHK(c, hipMemcpyAsync(d_src, src_xyz, 3 * m * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_dst, dst_xyz, 3 * m * sizeof(float), hipMemcpyHostToDevice, c->stream));
  for (size_t a = 0; a < nh; a += k) {
    const size_t ka = std::min(k, nh - a);
    HIPCHK(c, hipMemcpyAsync(d_tri, tri + 3 * a, 3 * ka * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_corr_poses(c->stream, d_src, d_dst, (unsigned)m, d_tri, (unsigned)ka, cfg->edge_sim, cfg->min_edge, cfg->max_dist, d_status,
                                d_pose, d_rt, d_surv, d_nsurv, d_inliers, d_sum, d_pair));
    HIPCHK(c, hipMemcpyAsync(status + a, d_status, ka * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(inliers + a, d_inliers, ka * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(sum_sqd + a, d_sum, ka * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (pose) HIPCHK(c, hipMemcpyAsync(pose + 7 * a, d_pose, 7 * ka * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (pair_sqd) HIPCHK(c, hipMemcpyAsync(pair_sqd + a * m, d_pair, ka * m * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (the next chunk overwrites the chunk's buffers)
  }
  return FLIMO_OK;
}
extern "C" int flimo_corr_pose_host(const float src3[9], const float dst3[9], const flimo_corr_cfg* cfg, double pose7[7], float rt12[12]) {
  if (!src3 || !dst3 || !cfg || !pose7 || !rt12 || !corr_cfg_ok(cfg)) return FLIMO_ERR_INVALID;
  return corr_solve(src3, dst3, cfg->edge_sim, cfg->min_edge, pose7, rt12);
}
extern "C" int flimo_set_corr_chunk(flimo_ctx* c, size_t n) { return set_chunk(c, &flimo_ctx::corr_chunk, n, (size_t)1 << 16); }

// ---- the consistency graph of the correspondences and its core numbers (the step between the putative pairs and the samples) ------
// kernels: flimo_corr.hip.  Both clouds go up, the bit matrix and the degrees are two launches, then the rounds of the h-index
// iteration are enqueued CORR_GRAPH_ROUNDS at a time and the last one's flag is read: the iteration has ended when a round changed
// nothing, however many that takes.  Everything comes back at the end; the scratch (the matrix, at most 128 MB) is the call's.
static constexpr int CORR_GRAPH_ROUNDS = 8;      // rounds per read of the flags: one wait of the host per batch
static bool corr_graph_cfg_ok(const flimo_corr_graph_cfg* k) {
  return std::isfinite(k->tol) && k->tol >= 0.f && std::isfinite(k->min_edge) && k->min_edge >= 0.f && !std::isnan(k->edge_sim) &&
         k->edge_sim >= 0.f && k->edge_sim <= 1.f;
}
extern "C" int flimo_corr_graph(flimo_ctx* c, const float* src_xyz, const float* dst_xyz, size_t m, const flimo_corr_graph_cfg* cfg, int32_t* degree,
                                int32_t* core, int32_t* max_core, uint64_t* adj) {
  if (!c) return FLIMO_ERR_INVALID;
  if (!cfg || !degree || !core || (m > 0 && (!src_xyz || !dst_xyz))) return fail(c, FLIMO_ERR_INVALID, "corr graph: null src / dst / cfg / degree / core");
  if (!corr_graph_cfg_ok(cfg)) return fail(c, FLIMO_ERR_INVALID, "corr graph: tol and min_edge must be finite and >= 0, edge_sim in 0..1");
  if (m > (size_t)FLIMO_CORR_GRAPH_MAX_M) return fail(c, FLIMO_ERR_TOO_LARGE, "corr graph: m must be at most %d", FLIMO_CORR_GRAPH_MAX_M);
  if (m == 0) return FLIMO_OK;
  ctx_enter(c);
  const size_t W = (m + 63) / 64;
  DevScratch d;
  float* d_src = d.get<float>(3 * m);
  float* d_dst = d.get<float>(3 * m);
  uint64_t* d_adj = d.get<uint64_t>(m * W);
  int32_t* d_degree = d.get<int32_t>(m);
  int32_t* d_c[2] = {d.get<int32_t>(m), d.get<int32_t>(m)};
  unsigned* d_flags = d.get<unsigned>(CORR_GRAPH_ROUNDS);
  { const int rc = d.ok(c); if (rc) return rc; }
  HIPCHK(c, hipMemcpyAsync(d_src, src_xyz, 3 * m * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_dst, dst_xyz, 3 * m * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, launch_corr_adjacency(c->stream, d_src, d_dst, (unsigned)m, cfg->tol, cfg->min_edge, cfg->edge_sim, d_adj, d_degree, d_c[0]));
  int cur = 0;
  for (;;) {
    unsigned flags[CORR_GRAPH_ROUNDS];
    HIPCHK(c, launch_corr_core_rounds(c->stream, d_adj, (unsigned)m, d_c, &cur, d_flags, CORR_GRAPH_ROUNDS));
    HIPCHK(c, hipMemcpyAsync(flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (flags[CORR_GRAPH_ROUNDS - 1] == 0u) break;      // (a round that changed nothing: so did every round behind it)
  }
  std::vector<int32_t> h_core(m);      // (the outputs stay untouched until nothing can fail any more)
  HIPCHK(c, hipMemcpyAsync(h_core.data(), d_c[cur], m * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpyAsync(degree, d_degree, m * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (adj) HIPCHK(c, hipMemcpyAsync(adj, d_adj, m * W * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::copy(h_core.begin(), h_core.end(), core);
  if (max_core) *max_core = *std::max_element(h_core.begin(), h_core.end());
  return FLIMO_OK;
}
extern "C" int flimo_corr_compatible_host(const float si[3], const float sj[3], const float di[3], const float dj[3], const flimo_corr_graph_cfg* cfg) {
  if (!si || !sj || !di || !dj || !cfg || !corr_graph_cfg_ok(cfg)) return FLIMO_ERR_INVALID;
  const double a[3] = {(double)si[0], (double)si[1], (double)si[2]}, b[3] = {(double)sj[0], (double)sj[1], (double)sj[2]};
  const double p[3] = {(double)di[0], (double)di[1], (double)di[2]}, q[3] = {(double)dj[0], (double)dj[1], (double)dj[2]};
  return corr_compatible(a, b, p, q, (double)cfg->min_edge * (double)cfg->min_edge, (double)cfg->tol, (double)cfg->edge_sim * (double)cfg->edge_sim) ? 1 : 0;
}

// ---- nearest descriptors: the resident reference set and the match (the step between flimo_map_fpfh and flimo_corr_poses) ---------
// kernels: flimo_desc.hip.  flimo_desc_ref_set uploads the rows once, and two launches leave their norms and their MFMA operand
// layout on the device.  flimo_desc_match runs the queries in chunks of c->desc_chunk: per chunk the rows go up, three launches
// (the queries' norms, the match over (query tiles) x (splits of the reference set), the merge of the splits), idx / dist / cnt
// come back; device scratch is the chunk's, whatever nq.  Reads neither the map nor the scan.
static void desc_ref_free(flimo_ctx* c) {
  (void)hipFree(c->d_desc_rt); (void)hipFree(c->d_desc_norm);
  c->d_desc_rt = c->d_desc_norm = nullptr;
  c->desc_nr = 0;
  c->desc_dim = 0;
}
extern "C" int flimo_desc_ref_set(flimo_ctx* c, const float* desc, size_t nr, int dim) {
  if (!c) return FLIMO_ERR_INVALID;
  if (nr > 0 && !desc) return fail(c, FLIMO_ERR_INVALID, "desc ref set: null desc");
  if (nr > 0 && (dim < 1 || dim > FLIMO_DESC_MAX_DIM)) return fail(c, FLIMO_ERR_UNSUPPORTED, "desc ref set: dim must be in 1..%d", FLIMO_DESC_MAX_DIM);
  if (nr >= 0x80000000ull) return fail(c, FLIMO_ERR_TOO_LARGE, "desc ref set: nr must be below 2^31");
  ctx_enter(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  desc_ref_free(c);
  if (nr == 0) return FLIMO_OK;
  const size_t ntiles = (nr + 31) / 32;
  DevScratch d;
  float* d_rows = d.get<float>(nr * (size_t)dim);
  { const int rc = d.ok(c); if (rc) return rc; }
  HIPCHK(c, hipMalloc(&c->d_desc_rt, ntiles * (size_t)desc_steps(dim) * 64 * sizeof(float)));
  HIPCHK(c, hipMalloc(&c->d_desc_norm, ntiles * 32 * sizeof(float)));
  HIPCHK(c, hipMemcpyAsync(d_rows, desc, nr * (size_t)dim * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, launch_desc_norms(c->stream, d_rows, (unsigned)nr, dim, c->d_desc_norm, (unsigned)(ntiles * 32)));
  HIPCHK(c, launch_desc_pack(c->stream, d_rows, (unsigned)nr, dim, c->d_desc_rt));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->desc_nr = nr;
  c->desc_dim = dim;
  return FLIMO_OK;
}
extern "C" size_t flimo_desc_ref_size(const flimo_ctx* c) { return c ? c->desc_nr : 0; }
extern "C" int flimo_desc_ref_dim(const flimo_ctx* c) { return c ? c->desc_dim : 0; }
extern "C" int flimo_desc_match(flimo_ctx* c, const float* q, size_t nq, int dim, int k, int32_t* idx, float* dist, int32_t* cnt) {
  if (!c) return FLIMO_ERR_INVALID;
  if ((nq > 0 && !q) || !idx || !dist || !cnt) return fail(c, FLIMO_ERR_INVALID, "desc match: null q / idx / dist / cnt");
  if (dim < 1 || dim > FLIMO_DESC_MAX_DIM) return fail(c, FLIMO_ERR_UNSUPPORTED, "desc match: dim must be in 1..%d", FLIMO_DESC_MAX_DIM);
  if (k < 1 || k > FLIMO_DESC_MAX_K) return fail(c, FLIMO_ERR_UNSUPPORTED, "desc match: k must be in 1..%d", FLIMO_DESC_MAX_K);
  if (nq >= 0x80000000ull || (unsigned long long)nq * (unsigned long long)k >= 0x80000000ull)
    return fail(c, FLIMO_ERR_TOO_LARGE, "desc match: nq and nq * k must be below 2^31");
  if (c->desc_nr > 0 && dim != c->desc_dim)
    return fail(c, FLIMO_ERR_INVALID, "desc match: the queries have dim %d, the resident set %d", dim, c->desc_dim);
  if (nq == 0) return FLIMO_OK;
  c->desc_last_ms = 0.f;
  if (c->desc_nr == 0) {      // nothing to be nearest to
    for (size_t i = 0; i < nq; i++) cnt[i] = 0;
    for (size_t i = 0; i < nq * (size_t)k; i++) { idx[i] = -1; dist[i] = 0.f; }
    return FLIMO_OK;
  }
  ctx_enter(c);
  const size_t m = std::min(nq, std::max<size_t>(c->desc_chunk, 1));      // queries of a chunk
  const size_t ntiles = (c->desc_nr + 31) / 32;
  // reference tiles per split: the caller's, or as many splits as bring the grid to about four workgroups a compute unit, none
  // below 32 tiles; never more than 32768 splits
  size_t tps;
  if (c->desc_split) tps = (c->desc_split + 31) / 32;
  else {
    const size_t groups = (m + (size_t)desc_query_tile(dim) - 1) / (size_t)desc_query_tile(dim);
    const size_t want = std::max<size_t>(1024 / groups, 1);
    tps = std::max<size_t>((ntiles + want - 1) / want, 32);
  }
  tps = std::max(tps, (ntiles + 32767) / 32768);
  const size_t nsplit = (ntiles + tps - 1) / tps;
  const int kl = desc_list_len(k);
  DevScratch d;
  float* d_q = d.get<float>(m * (size_t)dim);
  float* d_qnorm = d.get<float>(m);
  unsigned long long* d_part = d.get<unsigned long long>(nsplit * m * (size_t)kl);
  int32_t* d_idx = d.get<int32_t>(m * (size_t)k);
  float* d_dist = d.get<float>(m * (size_t)k);
  int32_t* d_cnt = d.get<int32_t>(m);
  { const int rc = d.ok(c); if (rc) return rc; }
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (c->timing) { HIPCHK(c, hipEventCreate(&ev[0])); HIPCHK(c, hipEventCreate(&ev[1])); }
  for (size_t a = 0; a < nq; a += m) {
    const size_t na = std::min(m, nq - a);
    HIPCHK(c, hipMemcpyAsync(d_q, q + a * (size_t)dim, na * (size_t)dim * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (ev[0]) HIPCHK(c, hipEventRecord(ev[0], c->stream));
    HIPCHK(c, launch_desc_match(c->stream, c->d_desc_rt, c->d_desc_norm, (unsigned)c->desc_nr, (unsigned)tps, d_q, d_qnorm, (unsigned)na, dim, k,
                                d_part, d_idx, d_dist, d_cnt));
    if (ev[1]) HIPCHK(c, hipEventRecord(ev[1], c->stream));
    HIPCHK(c, hipMemcpyAsync(idx + a * (size_t)k, d_idx, na * (size_t)k * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(dist + a * (size_t)k, d_dist, na * (size_t)k * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cnt + a, d_cnt, na * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (the next chunk overwrites the chunk's buffers)
    if (ev[0]) { float ms = 0.f; if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) c->desc_last_ms += ms; }
  }
  if (ev[0]) { (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]); }
  return FLIMO_OK;
}
extern "C" int flimo_desc_dist_host(const float* a, const float* b, int dim, float* d) {
  if (!a || !b || !d) return FLIMO_ERR_INVALID;
  if (dim < 1 || dim > FLIMO_DESC_MAX_DIM) return FLIMO_ERR_UNSUPPORTED;
  *d = desc_dist(desc_norm(a, dim), desc_norm(b, dim), desc_dot(a, b, dim));
  return FLIMO_OK;
}
extern "C" int flimo_set_desc_chunk(flimo_ctx* c, size_t queries_per_chunk, size_t refs_per_split) {
  if (!c) return FLIMO_ERR_INVALID;
  c->desc_chunk = queries_per_chunk ? queries_per_chunk : (size_t)1 << 16;
  c->desc_split = refs_per_split;
  return FLIMO_OK;
}
extern "C" float flimo_desc_last_ms(const flimo_ctx* c) { return c ? c->desc_last_ms : 0.f; }

// ---- Scan Context: the descriptor of the resident scan, the resident database of descriptors and the match over every shift -------
// kernels: flimo_sc.hip; the definition: flimo_sc.h.  flimo_scan_context is a zeroing and one launch over the scan.  The database
// is three arrays that grow geometrically by device-to-device copy (raw rows, normalised rows, valid-column bits); an add uploads
// (or, flimo_sc_db_add_scan, forms in place) the raw rows and one launch normalises them.  flimo_sc_match runs the queries in chunks
// of c->sc_chunk: per chunk the rows go up, the launches (the queries' normalised form, the match over (query tiles) x (splits of
// the range), the merge of the splits, the profiles of the returned pairs), the results come back.  Reads neither the map nor --
// the two scan entries apart -- the scan.
static int sc_check_shape(flimo_ctx* c, const char* what, int rings, int sectors) {
  if (rings < 1 || rings > FLIMO_SC_MAX_RINGS) return fail(c, FLIMO_ERR_INVALID, "%s: rings must be in 1..%d", what, FLIMO_SC_MAX_RINGS);
  if (sectors < 2 || sectors > FLIMO_SC_MAX_SECTORS) return fail(c, FLIMO_ERR_INVALID, "%s: sectors must be in 2..%d", what, FLIMO_SC_MAX_SECTORS);
  return FLIMO_OK;
}
static int sc_check_cfg(flimo_ctx* c, const char* what, const flimo_sc_cfg* cfg, const float* frame12, ScBinCfg* K) {
  if (!cfg) return fail(c, FLIMO_ERR_INVALID, "%s: null cfg", what);
  { const int rc = sc_check_shape(c, what, cfg->rings, cfg->sectors); if (rc) return rc; }
  if (!(cfg->min_range >= 0.f) || !std::isfinite(cfg->max_range) || !(cfg->max_range > cfg->min_range))
    return fail(c, FLIMO_ERR_INVALID, "%s: 0 <= min_range < max_range, max_range finite, must hold", what);
  if (!std::isfinite(cfg->z_offset)) return fail(c, FLIMO_ERR_INVALID, "%s: non-finite z_offset", what);
  K->rings = cfg->rings; K->sectors = cfg->sectors;
  K->min_range = cfg->min_range; K->max_range = cfg->max_range; K->z_offset = cfg->z_offset;
  sc_scales(*K);
  K->has_frame = frame12 ? 1 : 0;
  for (int a = 0; a < 12; a++) {
    if (frame12 && !std::isfinite(frame12[a])) return fail(c, FLIMO_ERR_INVALID, "%s: non-finite frame12 entry", what);
    K->frame[a] = frame12 ? frame12[a] : 0.f;
  }
  return FLIMO_OK;
}
extern "C" int flimo_sc_bin_host(const float p[3], const flimo_sc_cfg* cfg, const float frame12[12], int* ring, int* sector, float* h) {
  if (!p || !ring || !sector || !h) return FLIMO_ERR_INVALID;
  ScBinCfg K;
  { const int rc = sc_check_cfg(nullptr, "sc bin", cfg, frame12, &K); if (rc) return rc; }
  return sc_bin(K, p[0], p[1], p[2], ring, sector, h) ? 1 : 0;
}
extern "C" int flimo_scan_context(flimo_ctx* c, const flimo_sc_cfg* cfg, const float frame12[12], float* desc, int32_t* used) {
  if (!c) return FLIMO_ERR_INVALID;
  if (!desc) return fail(c, FLIMO_ERR_INVALID, "scan context: null desc");
  ScBinCfg K;
  { const int rc = sc_check_cfg(c, "scan context", cfg, frame12, &K); if (rc) return rc; }
  if (c->scan_n >= 0x80000000ull) return fail(c, FLIMO_ERR_TOO_LARGE, "scan context: the scan must hold fewer than 2^31 points");
  const size_t nb = (size_t)K.rings * K.sectors;
  if (c->scan_n == 0) {
    memset(desc, 0, nb * sizeof(float));
    if (used) *used = 0;
    return FLIMO_OK;
  }
  { const int rc = enter_flushed(c); if (rc) return rc; }
  DevScratch d;
  float* d_desc = d.get<float>(nb);
  int* d_used = d.get<int>(1);
  { const int rc = d.ok(c); if (rc) return rc; }
  float h_desc[FLIMO_SC_MAX_RINGS * FLIMO_SC_MAX_SECTORS];
  int h_used = 0;
  HIPCHK(c, launch_sc_descriptor(c->stream, c->d_scan, (unsigned)c->scan_n, K, d_desc, d_used));
  HIPCHK(c, hipMemcpyAsync(h_desc, d_desc, nb * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&h_used, d_used, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(desc, h_desc, nb * sizeof(float));
  if (used) *used = h_used;
  return FLIMO_OK;
}
static void sc_db_free(flimo_ctx* c) {
  (void)hipFree(c->d_sc_raw); (void)hipFree(c->d_sc_un); (void)hipFree(c->d_sc_valid);
  c->d_sc_raw = c->d_sc_un = nullptr;
  c->d_sc_valid = nullptr;
  c->sc_n = c->sc_cap = 0;
  c->sc_rings = c->sc_sectors = 0;
}
// room for `more` entries of this shape behind the sc_n there are: the shape must be the database's, the three arrays grow to at
// least twice their capacity, the entries move by device-to-device copy.  Nothing changes when it fails.
static int sc_db_reserve(flimo_ctx* c, const char* what, size_t more, int rings, int sectors) {
  if (c->sc_n > 0 && (rings != c->sc_rings || sectors != c->sc_sectors))
    return fail(c, FLIMO_ERR_INVALID, "%s: a %d x %d descriptor for a database of %d x %d", what, rings, sectors, c->sc_rings, c->sc_sectors);
  if (c->sc_n + more >= 0x80000000ull) return fail(c, FLIMO_ERR_TOO_LARGE, "%s: the database must hold fewer than 2^31 entries", what);
  if (c->sc_n == 0 && c->sc_cap > 0 && (rings != c->sc_rings || sectors != c->sc_sectors)) sc_db_free(c);      // (an empty one of another shape)
  const size_t need = c->sc_n + more;
  if (need > c->sc_cap) {
    const size_t ncap = std::max<size_t>(std::max(need, 2 * c->sc_cap), 64);
    const size_t nb = (size_t)rings * sectors, nu = (size_t)rings * 64;
    struct New { float *raw = nullptr, *un = nullptr; unsigned long long* valid = nullptr;
                 ~New() { (void)hipFree(raw); (void)hipFree(un); (void)hipFree(valid); } } nw;
    HIPCHK(c, hipMalloc(&nw.raw, ncap * nb * sizeof(float)));
    HIPCHK(c, hipMalloc(&nw.un, ncap * nu * sizeof(float)));
    HIPCHK(c, hipMalloc(&nw.valid, ncap * sizeof(unsigned long long)));
    if (c->sc_n) {
      HIPCHK(c, hipMemcpyAsync(nw.raw, c->d_sc_raw, c->sc_n * nb * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(nw.un, c->d_sc_un, c->sc_n * nu * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(nw.valid, c->d_sc_valid, c->sc_n * sizeof(unsigned long long), hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::swap(nw.raw, c->d_sc_raw); std::swap(nw.un, c->d_sc_un); std::swap(nw.valid, c->d_sc_valid);
    c->sc_cap = ncap;
  }
  c->sc_rings = rings; c->sc_sectors = sectors;
  return FLIMO_OK;
}
// the normalised form of the `more` raw rows behind the sc_n entries; they then count
static int sc_db_commit(flimo_ctx* c, size_t more) {
  const size_t nb = (size_t)c->sc_rings * c->sc_sectors, nu = (size_t)c->sc_rings * 64;
  HIPCHK(c, launch_sc_norms(c->stream, c->d_sc_raw + c->sc_n * nb, (unsigned)more, c->sc_rings, c->sc_sectors, c->d_sc_un + c->sc_n * nu,
                            c->d_sc_valid + c->sc_n));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->sc_n += more;
  return FLIMO_OK;
}
extern "C" int flimo_sc_db_add(flimo_ctx* c, const float* desc, size_t n, int rings, int sectors, size_t* first_id) {
  if (!c) return FLIMO_ERR_INVALID;
  if (n > 0 && !desc) return fail(c, FLIMO_ERR_INVALID, "sc db add: null desc");
  { const int rc = sc_check_shape(c, "sc db add", rings, sectors); if (rc) return rc; }
  if (n >= 0x80000000ull) return fail(c, FLIMO_ERR_TOO_LARGE, "sc db add: the database must hold fewer than 2^31 entries");
  if (n == 0) {
    if (c->sc_n > 0 && (rings != c->sc_rings || sectors != c->sc_sectors)) return fail(c, FLIMO_ERR_INVALID, "sc db add: not the database's shape");
    if (first_id) *first_id = c->sc_n;
    return FLIMO_OK;
  }
  ctx_enter(c);
  { const int rc = sc_db_reserve(c, "sc db add", n, rings, sectors); if (rc) return rc; }
  const size_t nb = (size_t)rings * sectors, id = c->sc_n;
  HIPCHK(c, hipMemcpyAsync(c->d_sc_raw + id * nb, desc, n * nb * sizeof(float), hipMemcpyHostToDevice, c->stream));
  { const int rc = sc_db_commit(c, n); if (rc) return rc; }
  if (first_id) *first_id = id;
  return FLIMO_OK;
}
extern "C" int flimo_sc_db_add_scan(flimo_ctx* c, const flimo_sc_cfg* cfg, const float frame12[12], size_t* id) {
  if (!c) return FLIMO_ERR_INVALID;
  ScBinCfg K;
  { const int rc = sc_check_cfg(c, "sc db add scan", cfg, frame12, &K); if (rc) return rc; }
  if (c->scan_n >= 0x80000000ull) return fail(c, FLIMO_ERR_TOO_LARGE, "sc db add scan: the scan must hold fewer than 2^31 points");
  { const int rc = enter_flushed(c); if (rc) return rc; }
  { const int rc = sc_db_reserve(c, "sc db add scan", 1, K.rings, K.sectors); if (rc) return rc; }
  DevScratch d;
  int* d_used = d.get<int>(1);
  { const int rc = d.ok(c); if (rc) return rc; }
  const size_t at = c->sc_n;
  HIPCHK(c, launch_sc_descriptor(c->stream, c->d_scan, (unsigned)c->scan_n, K, c->d_sc_raw + at * K.rings * K.sectors, d_used));
  { const int rc = sc_db_commit(c, 1); if (rc) return rc; }
  if (id) *id = at;
  return FLIMO_OK;
}
extern "C" size_t flimo_sc_db_size(const flimo_ctx* c) { return c ? c->sc_n : 0; }
extern "C" int flimo_sc_db_shape(const flimo_ctx* c, int* rings, int* sectors) {
  if (!c) return FLIMO_ERR_INVALID;
  if (rings) *rings = c->sc_n ? c->sc_rings : 0;
  if (sectors) *sectors = c->sc_n ? c->sc_sectors : 0;
  return FLIMO_OK;
}
extern "C" int flimo_sc_db_get(flimo_ctx* c, size_t first, size_t n, float* desc) {
  if (!c) return FLIMO_ERR_INVALID;
  if (first > c->sc_n || n > c->sc_n - first) return fail(c, FLIMO_ERR_INVALID, "sc db get: [%zu, %zu + %zu) ends beyond the %zu entries", first, first, n, c->sc_n);
  if (n == 0) return FLIMO_OK;
  if (!desc) return fail(c, FLIMO_ERR_INVALID, "sc db get: null desc");
  ctx_enter(c);
  const size_t nb = (size_t)c->sc_rings * c->sc_sectors;
  HIPCHK(c, hipMemcpyAsync(desc, c->d_sc_raw + first * nb, n * nb * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return FLIMO_OK;
}
extern "C" int flimo_sc_db_clear(flimo_ctx* c) {
  if (!c) return FLIMO_ERR_INVALID;
  ctx_enter(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  sc_db_free(c);
  return FLIMO_OK;
}
extern "C" int flimo_sc_match(flimo_ctx* c, const float* q, size_t nq, int rings, int sectors, size_t first, size_t n, const flimo_sc_match_cfg* cfg,
                              int32_t* idx, float* dist, int32_t* shift, int32_t* cnt, float* profile) {
  if (!c) return FLIMO_ERR_INVALID;
  if ((nq > 0 && !q) || !cfg || !idx || !dist || !shift || !cnt) return fail(c, FLIMO_ERR_INVALID, "sc match: null q / cfg / idx / dist / shift / cnt");
  { const int rc = sc_check_shape(c, "sc match", rings, sectors); if (rc) return rc; }
  if (cfg->k < 1 || cfg->k > FLIMO_SC_MAX_K) return fail(c, FLIMO_ERR_INVALID, "sc match: k must be in 1..%d", FLIMO_SC_MAX_K);
  if (cfg->min_cols < 1 || cfg->min_cols > sectors) return fail(c, FLIMO_ERR_INVALID, "sc match: min_cols must be in 1..sectors");
  if (!(cfg->max_dist > 0.f)) return fail(c, FLIMO_ERR_INVALID, "sc match: max_dist must be > 0 or INFINITY");
  const int k = cfg->k;
  if (nq >= 0x80000000ull || (unsigned long long)nq * (unsigned long long)k >= 0x80000000ull)
    return fail(c, FLIMO_ERR_TOO_LARGE, "sc match: nq * k must be below 2^31");
  if (c->sc_n > 0 && (rings != c->sc_rings || sectors != c->sc_sectors))
    return fail(c, FLIMO_ERR_INVALID, "sc match: %d x %d queries for a database of %d x %d", rings, sectors, c->sc_rings, c->sc_sectors);
  if (nq == 0) return FLIMO_OK;
  c->sc_last_ms = 0.f;
  if (first >= c->sc_n || n == 0) {      // nobody to be near
    for (size_t i = 0; i < nq; i++) cnt[i] = 0;
    for (size_t i = 0; i < nq * (size_t)k; i++) { idx[i] = -1; dist[i] = 0.f; shift[i] = -1; }
    if (profile) for (size_t i = 0; i < nq * (size_t)k * sectors; i++) profile[i] = std::numeric_limits<float>::quiet_NaN();
    return FLIMO_OK;
  }
  n = std::min(n, c->sc_n - first);
  ctx_enter(c);
  const size_t m = std::min(nq, std::max<size_t>(c->sc_chunk, 1));      // queries of a chunk
  // entries per split: the caller's, or as many splits as bring the grid to about four workgroups a compute unit, none below eight
  // entries (a workgroup's waves take two at a time); never more than 32768 splits
  size_t eps;
  if (c->sc_split) eps = std::min(c->sc_split, n);
  else {
    const size_t groups = (m + (size_t)sc_query_tile() - 1) / (size_t)sc_query_tile();
    const size_t want = std::max<size_t>(1024 / groups, 1);
    eps = std::max<size_t>((n + want - 1) / want, 8);
  }
  eps = std::max(eps, (n + 32767) / 32768);
  const size_t nsplit = (n + eps - 1) / eps;
  const size_t nb = (size_t)rings * sectors, nu = (size_t)rings * 64, kl = (size_t)sc_list_len();
  DevScratch d;
  float* d_q = d.get<float>(m * nb);
  float* d_qun = d.get<float>(m * nu);
  unsigned long long* d_qvalid = d.get<unsigned long long>(m);
  unsigned long long* d_part = d.get<unsigned long long>(nsplit * m * kl);
  int* d_part_shift = d.get<int>(nsplit * m * kl);
  int32_t* d_idx = d.get<int32_t>(m * (size_t)k);
  float* d_dist = d.get<float>(m * (size_t)k);
  int32_t* d_shift = d.get<int32_t>(m * (size_t)k);
  int32_t* d_cnt = d.get<int32_t>(m);
  float* d_profile = profile ? d.get<float>(m * (size_t)k * sectors) : nullptr;
  { const int rc = d.ok(c); if (rc) return rc; }
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (c->timing) { HIPCHK(c, hipEventCreate(&ev[0])); HIPCHK(c, hipEventCreate(&ev[1])); }
  for (size_t a = 0; a < nq; a += m) {
    const size_t na = std::min(m, nq - a), nk = na * (size_t)k;
    HIPCHK(c, hipMemcpyAsync(d_q, q + a * nb, na * nb * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (ev[0]) HIPCHK(c, hipEventRecord(ev[0], c->stream));
    HIPCHK(c, launch_sc_norms(c->stream, d_q, (unsigned)na, rings, sectors, d_qun, d_qvalid));
    HIPCHK(c, launch_sc_match(c->stream, c->d_sc_un, c->d_sc_valid, (unsigned)first, (unsigned)(first + n), (unsigned)eps, d_qun, d_qvalid,
                              (unsigned)na, rings, sectors, k, cfg->min_cols, cfg->max_dist, d_part, d_part_shift, d_idx, d_dist, d_shift, d_cnt,
                              d_profile));
    if (ev[1]) HIPCHK(c, hipEventRecord(ev[1], c->stream));
    HIPCHK(c, hipMemcpyAsync(idx + a * (size_t)k, d_idx, nk * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(dist + a * (size_t)k, d_dist, nk * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(shift + a * (size_t)k, d_shift, nk * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cnt + a, d_cnt, na * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (profile) HIPCHK(c, hipMemcpyAsync(profile + a * (size_t)k * sectors, d_profile, nk * sectors * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (the next chunk overwrites the chunk's buffers)
    if (ev[0]) { float ms = 0.f; if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) c->sc_last_ms += ms; }
  }
  if (ev[0]) { (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]); }
  return FLIMO_OK;
}
extern "C" int flimo_sc_dist_host(const float* a, const float* b, int rings, int sectors, int min_cols, float* dist, int* shift, float* profile) {
  if (!a || !b || !dist || !shift) return FLIMO_ERR_INVALID;
  if (rings < 1 || rings > FLIMO_SC_MAX_RINGS || sectors < 2 || sectors > FLIMO_SC_MAX_SECTORS || min_cols < 1 || min_cols > sectors)
    return FLIMO_ERR_INVALID;
  float d = 0.f;
  int s = -1;
  const bool have = sc_dist(a, b, rings, sectors, min_cols, &d, &s, profile);
  *dist = d;
  *shift = s;
  return have ? 1 : 0;
}
extern "C" int flimo_set_sc_chunk(flimo_ctx* c, size_t queries_per_chunk, size_t entries_per_split) {
  if (!c) return FLIMO_ERR_INVALID;
  c->sc_chunk = queries_per_chunk ? queries_per_chunk : (size_t)1 << 12;
  c->sc_split = entries_per_split;
  return FLIMO_OK;
}
extern "C" float flimo_sc_last_ms(const flimo_ctx* c) { return c ? c->sc_last_ms : 0.f; }

// ---- point-to-plane normal equations of the resident scan under pose hypotheses: one linearisation of a registration ----------
// kernels: flimo_knn_k.hip.  Chunks of whole poses as flimo_scan_fitness, c->linearize_chunk pairs at most unless one pose alone
// has more: per chunk the poses' matrices go up, five launches (block search, walk over the tiles, the plane and the row per
// pair, the sums' two levels), 29 numbers per pose -- and the rows and counts, where asked for -- come back.  Reads d_scan only.
extern "C" int flimo_scan_linearize(flimo_ctx* c, const double* x26, size_t np, int k, float max_dist, int min_pts, float max_curv, int32_t* valid,
                                    double* H, double* g, double* cost, double* rows, int32_t* pair_cnt) {
  if (!c) return FLIMO_ERR_INVALID;
  if ((np > 0 && !x26) || !valid || !H || !g || !cost) return fail(c, FLIMO_ERR_INVALID, "scan linearize: null poses / valid / H / g / cost");
  { const int rc = check_gate(c, "scan linearize", max_dist); if (rc) return rc; }
  if (std::isnan(max_curv) || max_curv < 0.f) return fail(c, FLIMO_ERR_INVALID, "scan linearize: max_curv must be >= 0 or INFINITY");
  if (k < 3 || k > FLIMO_KNN_MAX_K) return fail(c, FLIMO_ERR_UNSUPPORTED, "scan linearize: k must be in 3..%d", FLIMO_KNN_MAX_K);
  { const int rc = check_poses(c, "scan linearize", x26, np); if (rc) return rc; }
  if (np == 0) return FLIMO_OK;
  const size_t n = c->scan_n;
  { const int rc0 = ensure_index(c); if (rc0) return rc0; }
  if (n > ((size_t)1 << 28)) return fail(c, FLIMO_ERR_TOO_LARGE, "scan linearize: a scan of more than 2^28 points");
  if (n == 0 || !c->grid_valid || max_dist == 0.f) {      // an empty scan or map, a gate that admits nothing: no pair has a plane
    for (size_t j = 0; j < np; j++) { valid[j] = 0; cost[j] = 0.0; }
    zero_H_g(H, g, np);
    if (rows) for (size_t i = 0; i < np * n * 7; i++) rows[i] = std::numeric_limits<double>::quiet_NaN();
    if (pair_cnt) for (size_t i = 0; i < np * n; i++) pair_cnt[i] = 0;
    return FLIMO_OK;
  }
  { const int rcf = enter_flushed(c); if (rcf) return rcf; }
  // scratch of this call, released on every exit path
  DevScratch d;
  PoseChunks P(d, c->linearize_chunk, n, np);
  const size_t m = P.m, nseg = sum_segments(n);
  float* d_poses = P.d_poses;
  int32_t* d_cnt = d.get<int32_t>(m * n);
  double* d_mom = d.get<double>(m * n * 9);
  uint2* d_work = d.get<uint2>(m * n);
  unsigned* d_nwork = d.get<unsigned>(1);
  double* d_rows = d.get<double>(m * n * 7);
  unsigned char* d_ok = d.get<unsigned char>(m * n);
  double* d_part = d.get<double>(m * nseg * 28);
  int32_t* d_part_cnt = d.get<int32_t>(m * nseg);
  double* d_sums = d.get<double>(m * 28);
  long long* d_valid = d.get<long long>(m);
  { const int rc = d.ok(c); if (rc) return rc; }
  std::vector<double> sums(m * 28);
  std::vector<long long> counts(m);
  return P.run(c, x26, np,
    [&](size_t, size_t kk) -> int {
      HIPCHK(c, launch_scan_linearize(c->stream, c->grid, c->d_map_raw, c->d_scan, (unsigned)n, d_poses, (unsigned)kk, k, max_dist, min_pts, max_curv,
                                      d_cnt, d_mom, d_work, d_nwork, d_rows, d_ok, d_part, d_part_cnt, d_sums, d_valid));
      return FLIMO_OK;
    },
    [&](size_t a, size_t kk) -> int {
      HIPCHK(c, hipMemcpyAsync(counts.data(), d_valid, kk * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(sums.data(), d_sums, kk * 28 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      if (rows) HIPCHK(c, hipMemcpyAsync(rows + a * n * 7, d_rows, kk * n * 7 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      if (pair_cnt) HIPCHK(c, hipMemcpyAsync(pair_cnt + a * n, d_cnt, kk * n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
      return FLIMO_OK;
    },
    [&](size_t a, size_t kk) {
      unpack_sums(sums.data(), a, kk, H, g, cost);
      for (size_t j = 0; j < kk; j++) valid[a + j] = (int32_t)counts[j];
    });
}
extern "C" int flimo_set_linearize_chunk(flimo_ctx* c, size_t pairs) { return set_chunk(c, &flimo_ctx::linearize_chunk, pairs, (size_t)1 << 20); }

// ---- NDT: the resident cell model and the per-pose score and normal equations against it (pcl::NormalDistributionsTransform) ------
// kernels: flimo_ndt.hip.  The build is voxels_device's launches (flimo_map_voxels with cov: the same keys, sort and moments, so the
// same bits), then the eigen-solve per voxel, a scan of the cell flags and the pack into the slot's own buffers -- 8 + 4 + 24 + 128 B
// a cell, kept until the slot is rebuilt or cleared; the new model replaces the old one only when everything has succeeded.  A pass
// runs in chunks of whole poses as flimo_scan_linearize, three launches a chunk (lookup, reduce, final); reads d_scan only.
static int ndt_slot_check(flimo_ctx* c, const char* what, int slot) {
  if (slot < 0 || slot >= FLIMO_NDT_SLOTS) return fail(c, FLIMO_ERR_INVALID, "%s: slot must be in 0..%d", what, FLIMO_NDT_SLOTS - 1);
  return FLIMO_OK;
}
extern "C" int flimo_ndt_build(flimo_ctx* c, int slot, const flimo_ndt_cfg* cfg, size_t* nc) {
  if (!c) return FLIMO_ERR_INVALID;
  if (!cfg) return fail(c, FLIMO_ERR_INVALID, "ndt build: null cfg");
  { const int rc = ndt_slot_check(c, "ndt build", slot); if (rc) return rc; }
  const flimo_voxel_cfg vk{cfg->leaf, FLIMO_VOXEL_KEEP_FIRST, 1};
  { const int rc = voxel_check(c, 0, 0, &vk, "ndt build"); if (rc) return rc; }
  if (cfg->min_pts < 3 || !(cfg->eig_ratio > 0.0 && cfg->eig_ratio <= 1.0))      // (a NaN fails the test)
    return fail(c, FLIMO_ERR_INVALID, "ndt build: min_pts must be >= 3 and eig_ratio in (0, 1]");
  struct Fresh {      // the model under construction: released unless it is handed to the slot
    flimo_ctx::NdtModel m;
    bool keep = false;
    ~Fresh() { if (!keep) m.release(); }
  } f;
  f.m.built = true; f.m.leaf = cfg->leaf; f.m.min_pts = cfg->min_pts; f.m.eig_ratio = cfg->eig_ratio;
  f.m.map_n = c->map_n; f.m.epoch = c->map_epoch;
  if (c->map_n > 0) {
    VoxelDev d;
    flimo_voxel_stats st;
    { const int rc = voxels_device(c, 0, 0, vk, 2, (size_t)-1, false, false, d, &st); if (rc) return rc; }
    const size_t nv = d.nv;
    if (nv > 0) {
      size_t tmp_bytes = 0;
      HIPCHK(c, ndt_tmp_bytes(nv, &tmp_bytes));
      double* d_eig = d.mem.get<double>(12 * nv);
      uint32_t* d_flag = d.mem.get<uint32_t>(nv + 1);
      uint32_t* d_pos = d.mem.get<uint32_t>(nv + 1);
      void* d_tmp = d.mem.get<unsigned char>(tmp_bytes);
      { const int rc = d.mem.ok(c); if (rc) return rc; }
      HIPCHK(c, launch_ndt_cells(c->stream, d.count, d.cov, (unsigned)nv, cfg->min_pts, d_eig, d_flag, d_pos, d_tmp, tmp_bytes));
      uint32_t cells = 0;
      HIPCHK(c, hipMemcpyAsync(&cells, d_pos + nv, sizeof cells, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      if ((size_t)cells > nv) return fail(c, FLIMO_ERR_HIP, "ndt build: counted %u cells of %zu voxels", cells, nv);
      if (cells > 0) {
        HIPCHK(c, hipMalloc(&f.m.d_keys, (size_t)cells * sizeof(unsigned long long)));
        HIPCHK(c, hipMalloc(&f.m.d_count, (size_t)cells * sizeof(int32_t)));
        HIPCHK(c, hipMalloc(&f.m.d_eval, (size_t)cells * 3 * sizeof(double)));
        HIPCHK(c, hipMalloc(&f.m.d_cells, (size_t)cells * sizeof(NdtCell)));
        HIPCHK(c, launch_ndt_pack(c->stream, d_flag, d_pos, d.ijk, d.count, d.centroid, d_eig, (unsigned)nv, cfg->eig_ratio, f.m.d_keys, f.m.d_count,
                                  f.m.d_eval, f.m.d_cells));
        HIPCHK(c, hipStreamSynchronize(c->stream));
      }
      f.m.nc = cells;
    }
  }
  c->ndt[slot].release();
  c->ndt[slot] = f.m;
  f.keep = true;
  if (nc) *nc = f.m.nc;
  return FLIMO_OK;
}
static int ndt_model_of(flimo_ctx* c, const char* what, int slot, const flimo_ctx::NdtModel** m) {
  { const int rc = ndt_slot_check(c, what, slot); if (rc) return rc; }
  if (!c->ndt[slot].built) return fail(c, FLIMO_ERR_NOMAP, "%s: slot %d holds no model (flimo_ndt_build)", what, slot);
  *m = &c->ndt[slot];
  return FLIMO_OK;
}
extern "C" int flimo_ndt_cells(flimo_ctx* c, int slot, size_t cap, size_t* nc, int32_t* ijk, int32_t* count, double* mean, double* evec, double* wgt,
                               double* eval) {
  if (!c) return FLIMO_ERR_INVALID;
  const flimo_ctx::NdtModel* m = nullptr;
  { const int rc = ndt_model_of(c, "ndt cells", slot, &m); if (rc) return rc; }
  const size_t n = m->nc;
  const bool arrays = ijk || count || mean || evec || wgt || eval;
  if (nc) *nc = n;
  if (arrays && n > cap) return fail(c, FLIMO_ERR_TOO_LARGE, "ndt cells: the model has %zu cells, the arrays hold %zu", n, cap);
  if (!arrays || n == 0) return FLIMO_OK;
  ctx_enter(c);
  // (through vectors of the call: the caller's arrays stay untouched if a copy fails)
  std::vector<unsigned long long> keys(ijk ? n : 0);
  std::vector<int32_t> cnt(count ? n : 0);
  std::vector<double> ev(eval ? 3 * n : 0);
  std::vector<NdtCell> rec((mean || evec || wgt) ? n : 0);
  if (ijk) HIPCHK(c, hipMemcpyAsync(keys.data(), m->d_keys, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  if (count) HIPCHK(c, hipMemcpyAsync(cnt.data(), m->d_count, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (eval) HIPCHK(c, hipMemcpyAsync(ev.data(), m->d_eval, 3 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (!rec.empty()) HIPCHK(c, hipMemcpyAsync(rec.data(), m->d_cells, n * sizeof(NdtCell), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (ijk) for (size_t v = 0; v < n; v++) voxel_cell_of_key(keys[v], ijk + 3 * v);
  if (count) memcpy(count, cnt.data(), n * sizeof(int32_t));
  if (eval) memcpy(eval, ev.data(), 3 * n * sizeof(double));
  for (size_t v = 0; v < rec.size(); v++) {
    if (mean) memcpy(mean + 3 * v, rec[v].mean, 3 * sizeof(double));
    if (evec) memcpy(evec + 9 * v, rec[v].v, 9 * sizeof(double));
    if (wgt) memcpy(wgt + 3 * v, rec[v].w, 3 * sizeof(double));
  }
  return FLIMO_OK;
}
extern "C" int flimo_ndt_info(flimo_ctx* c, int slot, flimo_ndt_model_info* info) {
  if (!c) return FLIMO_ERR_INVALID;
  if (!info) return fail(c, FLIMO_ERR_INVALID, "ndt info: null info");
  const flimo_ctx::NdtModel* m = nullptr;
  { const int rc = ndt_model_of(c, "ndt info", slot, &m); if (rc) return rc; }
  info->cells = m->nc; info->map_size_at_build = m->map_n; info->eig_ratio = m->eig_ratio; info->leaf = m->leaf; info->min_pts = m->min_pts;
  info->stale = m->epoch != c->map_epoch ? 1 : 0;
  return FLIMO_OK;
}
extern "C" int flimo_ndt_clear(flimo_ctx* c, int slot) {
  if (!c) return FLIMO_ERR_INVALID;
  if (slot != -1) { const int rc = ndt_slot_check(c, "ndt clear", slot); if (rc) return rc; }
  ctx_enter(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int s = 0; s < FLIMO_NDT_SLOTS; s++)
    if (slot == -1 || slot == s) c->ndt[s].release();
  return FLIMO_OK;
}
extern "C" int flimo_scan_ndt(flimo_ctx* c, int slot, const double* x26, size_t np, int hood, double d2, int32_t* valid, int64_t* cells, double* H,
                              double* g, double* score, double* terms, int32_t* term_cell) {
  if (!c) return FLIMO_ERR_INVALID;
  if ((np > 0 && !x26) || !valid || !cells || !H || !g || !score)
    return fail(c, FLIMO_ERR_INVALID, "scan ndt: null poses / valid / cells / H / g / score");
  if (hood != 1 && hood != NDT_HOOD_MAX) return fail(c, FLIMO_ERR_INVALID, "scan ndt: hood must be 1 or 7");
  if (!(d2 > 0.0) || std::isinf(d2)) return fail(c, FLIMO_ERR_INVALID, "scan ndt: d2 must be finite and > 0");
  const flimo_ctx::NdtModel* m = nullptr;
  { const int rc = ndt_model_of(c, "scan ndt", slot, &m); if (rc) return rc; }
  { const int rc = check_poses(c, "scan ndt", x26, np); if (rc) return rc; }
  if (np == 0) return FLIMO_OK;
  const size_t n = c->scan_n;
  if (n > ((size_t)1 << 28)) return fail(c, FLIMO_ERR_TOO_LARGE, "scan ndt: a scan of more than 2^28 points");
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (terms) for (size_t i = 0; i < np * n * 14; i++) terms[i] = nan;      // (the slots a pass has no cell for stay so)
  if (term_cell) for (size_t i = 0; i < np * n * 7; i++) term_cell[i] = -1;
  if (n == 0 || m->nc == 0) {      // an empty scan or model: no pair has a term
    for (size_t j = 0; j < np; j++) { valid[j] = 0; cells[j] = 0; score[j] = 0.0; }
    zero_H_g(H, g, np);
    return FLIMO_OK;
  }
  { const int rcf = enter_flushed(c); if (rcf) return rcf; }
  // scratch of this call, released on every exit path
  DevScratch d;
  PoseChunks P(d, c->ndt_chunk, n, np);
  const size_t k = P.m, nseg = sum_segments(n), slots = k * n * (size_t)hood;
  float* d_poses = P.d_poses;
  int32_t* d_cell = d.get<int32_t>(slots);
  double* d_e = d.get<double>(slots);
  double* d_m = terms ? d.get<double>(slots) : nullptr;
  double* d_part = d.get<double>(k * nseg * NDT_NUM);
  int32_t* d_part_cnt = d.get<int32_t>(k * nseg * 2);
  double* d_sums = d.get<double>(k * NDT_NUM);
  long long* d_counts = d.get<long long>(k * 2);
  { const int rc = d.ok(c); if (rc) return rc; }
  static_assert(NDT_NUM == 28, "unpack_sums takes 28 numbers a pose");
  std::vector<double> sums(k * NDT_NUM), he, hm;
  std::vector<long long> counts(k * 2);
  std::vector<int32_t> hc;
  if (terms) { he.resize(slots); hm.resize(slots); }
  if (terms || term_cell) hc.resize(slots);
  return P.run(c, x26, np,
    [&](size_t, size_t kk) -> int {
      HIPCHK(c, launch_scan_ndt(c->stream, c->d_scan, (unsigned)n, d_poses, (unsigned)kk, hood, 1.0f / m->leaf, d2, m->d_keys, m->d_cells,
                                (unsigned)m->nc, d_cell, d_e, d_m, d_part, d_part_cnt, d_sums, d_counts));
      return FLIMO_OK;
    },
    [&](size_t, size_t kk) -> int {
      const size_t used = kk * n * (size_t)hood;
      HIPCHK(c, hipMemcpyAsync(sums.data(), d_sums, kk * NDT_NUM * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(counts.data(), d_counts, kk * 2 * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
      if (terms) {
        HIPCHK(c, hipMemcpyAsync(he.data(), d_e, used * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(hm.data(), d_m, used * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      }
      if (!hc.empty()) HIPCHK(c, hipMemcpyAsync(hc.data(), d_cell, used * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
      return FLIMO_OK;
    },
    [&](size_t a, size_t kk) {
      unpack_sums(sums.data(), a, kk, H, g, score);
      for (size_t j = 0; j < kk; j++) {
        valid[a + j] = (int32_t)counts[2 * j];
        cells[a + j] = (int64_t)counts[2 * j + 1];
      }
      if (!hc.empty())
        for (size_t pr = 0; pr < kk * n; pr++)
          for (int s = 0; s < hood; s++) {
            const size_t from = pr * (size_t)hood + (size_t)s, to = (a * n + pr) * 7 + (size_t)s;
            const bool present = hc[from] >= 0;
            if (term_cell) term_cell[to] = hc[from];
            if (terms && present) { terms[2 * to] = hm[from]; terms[2 * to + 1] = he[from]; }
          }
    });
}
extern "C" int flimo_set_ndt_chunk(flimo_ctx* c, size_t pairs) { return set_chunk(c, &flimo_ctx::ndt_chunk, pairs, (size_t)1 << 20); }
extern "C" int flimo_ndt_term_host(const float w3[3], const float p3[3], const float R9[9], const double mean3[3], const double evec9[9],
                                   const double wgt3[3], double d2, double out30[30]) {
  if (!w3 || !p3 || !R9 || !mean3 || !evec9 || !wgt3 || !out30) return FLIMO_ERR_INVALID;
  NdtCell r;
  memcpy(r.mean, mean3, sizeof r.mean);
  memcpy(r.v, evec9, sizeof r.v);
  memcpy(r.w, wgt3, sizeof r.w);
  r.pad = 0.0;
  double acc[NDT_NUM] = {0.0};
  const bool live = ndt_term(w3, p3, R9, r, -0.5 * d2, d2, [](double x) { return ::exp(x); }, &out30[0], &out30[1], acc);
  memcpy(out30 + 2, acc, sizeof acc);
  return live ? 1 : 0;
}

// ---- GICP: the resident covariance model and the per-pose normal equations against it (pcl::GeneralizedIterativeClosestPoint) -----
// kernels: flimo_gicp.hip.  The build is flimo_map_fpfh's first loop -- flimo_map_normals_range's launches over the WHOLE map in
// chunks of c->normals_chunk points, the covariances left on the device (so the same bits) -- and per chunk the pack into the
// model's own buffer, 48 B a stored point, kept until the model is rebuilt or cleared; the new model replaces the old one only when
// everything has succeeded.  Per chunk the scratch is the normals' (normal, count, cov, moments: 140 B a point) and the worklist
// (8 B); nothing of points x k entries exists and nothing is downloaded.  A pass runs in chunks of whole poses as
// flimo_scan_linearize, four launches a chunk (flimo_scan_fitness' two searches, reduce, final); reads d_scan only.
static bool gicp_cfg_ok(const flimo_gicp_cfg* k) {      // (a NaN eps fails the test)
  return k->min_pts >= 0 && (k->rule == FLIMO_GICP_PLANE || k->rule == FLIMO_GICP_CLAMP) && k->eps > 0.0 && k->eps <= 1.0;
}
extern "C" int flimo_gicp_build(flimo_ctx* c, const flimo_gicp_cfg* cfg, size_t* n_cov) {
  static_assert(FLIMO_GICP_PLANE == GICP_PLANE && FLIMO_GICP_CLAMP == GICP_CLAMP, "the header's rules are the kernels'");
  if (!c) return FLIMO_ERR_INVALID;
  if (!cfg) return fail(c, FLIMO_ERR_INVALID, "gicp build: null cfg");
  { const int rc = check_gate(c, "gicp build", cfg->max_dist); if (rc) return rc; }
  if (!gicp_cfg_ok(cfg)) return fail(c, FLIMO_ERR_INVALID, "gicp build: min_pts must be >= 0, rule FLIMO_GICP_PLANE or _CLAMP and eps in (0, 1]");
  if (cfg->k < 3 || cfg->k > FLIMO_KNN_MAX_K) return fail(c, FLIMO_ERR_UNSUPPORTED, "gicp build: k must be in 3..%d", FLIMO_KNN_MAX_K);
  { const int rc = check_map_size(c, "gicp build"); if (rc) return rc; }
  struct Fresh {      // the model under construction: released unless it is handed to the context
    flimo_ctx::GicpModel m;
    bool keep = false;
    ~Fresh() { if (!keep) m.release(); }
  } f;
  const size_t N = c->map_n;
  f.m.built = true; f.m.n = N; f.m.cfg = *cfg; f.m.epoch = c->map_epoch;
  if (N > 0) {
    { const int rc = need_index(c, "gicp build"); if (rc) return rc; }
    ctx_enter(c);
    DevScratch d;
    const size_t m = std::min(N, std::max<size_t>(c->normals_chunk, 1));
    float4* d_normal = d.get<float4>(m);
    int32_t* d_cnt = d.get<int32_t>(m);
    double* d_cov = d.get<double>(m * 6);
    double* d_mom = d.get<double>(m * 9);
    uint2* d_work = d.get<uint2>(m);
    unsigned* d_nwork = d.get<unsigned>(1);
    unsigned* d_count = d.get<unsigned>(1);
    { const int rc = d.ok(c); if (rc) return rc; }
    HIPCHK(c, hipMalloc(&f.m.d_cov, N * 6 * sizeof(double)));
    HIPCHK(c, hipMemsetAsync(d_count, 0, sizeof(unsigned), c->stream));
    // (a chunk's scratch is read by its own launches only: the stream orders the chunks, nothing waits in between)
    for (size_t a = 0; a < N; a += m) {
      const size_t na = std::min(m, N - a);
      HIPCHK(c, launch_knn_k_normals(c->stream, c->grid, c->d_map_raw, nullptr, (unsigned)a, (int)na, cfg->k, cfg->max_dist, cfg->min_pts, nullptr,
                                     d_normal, d_cnt, nullptr, d_cov, nullptr, d_mom, d_work, d_nwork));
      HIPCHK(c, launch_gicp_pack(c->stream, d_cov, (unsigned)na, cfg->rule, cfg->eps, f.m.d_cov + 6 * a, d_count));
    }
    unsigned h_count = 0;
    HIPCHK(c, hipMemcpyAsync(&h_count, d_count, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((size_t)h_count > N) return fail(c, FLIMO_ERR_HIP, "gicp build: counted %u covariances of %zu points", h_count, N);
    f.m.n_cov = h_count;
  }
  c->gicp.release();
  c->gicp = f.m;
  f.keep = true;
  if (n_cov) *n_cov = f.m.n_cov;
  return FLIMO_OK;
}
static int gicp_model_of(flimo_ctx* c, const char* what) {
  if (!c->gicp.built) return fail(c, FLIMO_ERR_NOMAP, "%s: the context holds no model (flimo_gicp_build)", what);
  return FLIMO_OK;
}
extern "C" int flimo_gicp_model(flimo_ctx* c, size_t first, size_t n, double* cov) {
  if (!c) return FLIMO_ERR_INVALID;
  { const int rc = gicp_model_of(c, "gicp model"); if (rc) return rc; }
  const flimo_ctx::GicpModel& m = c->gicp;
  if (first > m.n || n > m.n - first)
    return fail(c, FLIMO_ERR_INVALID, "gicp model: the range [%zu, %zu + %zu) ends beyond the model's %zu points", first, first, n, m.n);
  if (n == 0) return FLIMO_OK;
  if (!cov) return fail(c, FLIMO_ERR_INVALID, "gicp model: null cov");
  ctx_enter(c);
  HIPCHK(c, hipMemcpyAsync(cov, m.d_cov + 6 * first, n * 6 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return FLIMO_OK;
}
extern "C" int flimo_gicp_info(flimo_ctx* c, flimo_gicp_model_info* info) {
  if (!c) return FLIMO_ERR_INVALID;
  if (!info) return fail(c, FLIMO_ERR_INVALID, "gicp info: null info");
  { const int rc = gicp_model_of(c, "gicp info"); if (rc) return rc; }
  const flimo_ctx::GicpModel& m = c->gicp;
  info->points = m.n; info->n_cov = m.n_cov; info->eps = m.cfg.eps; info->k = m.cfg.k; info->max_dist = m.cfg.max_dist;
  info->min_pts = m.cfg.min_pts; info->rule = m.cfg.rule;
  info->stale = m.epoch != c->map_epoch ? 1 : 0;
  return FLIMO_OK;
}
extern "C" int flimo_gicp_clear(flimo_ctx* c) {
  if (!c) return FLIMO_ERR_INVALID;
  ctx_enter(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->gicp.release();
  return FLIMO_OK;
}
extern "C" int flimo_scan_cov_set(flimo_ctx* c, const double* cov6, size_t n) {
  if (!c) return FLIMO_ERR_INVALID;
  if (!cov6 || n == 0) { c->scan_cov_n = 0; return FLIMO_OK; }
  if (n != c->scan_n) return fail(c, FLIMO_ERR_INVALID, "scan cov set: %zu covariances for a resident scan of %zu points", n, c->scan_n);
  ctx_enter(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));      // (a pass still reading the old rows ends first)
  c->scan_cov_n = 0;
  { const int rc = ensure_dev(c, c->d_scan_cov, c->scan_cov_cap, n * 6, false, 0); if (rc) return rc; }
  HIPCHK(c, hipMemcpyAsync(c->d_scan_cov, cov6, n * 6 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->scan_cov_n = n;
  return FLIMO_OK;
}
extern "C" size_t flimo_scan_cov_size(const flimo_ctx* c) { return c ? c->scan_cov_n : 0; }
extern "C" int flimo_scan_gicp(flimo_ctx* c, const double* x26, size_t np, float max_dist, int32_t* valid, double* H, double* g, double* cost,
                               int32_t* pair_idx, double* pair_m) {
  if (!c) return FLIMO_ERR_INVALID;
  if ((np > 0 && !x26) || !valid || !H || !g || !cost) return fail(c, FLIMO_ERR_INVALID, "scan gicp: null poses / valid / H / g / cost");
  { const int rc = check_gate(c, "scan gicp", max_dist); if (rc) return rc; }
  { const int rc = check_poses(c, "scan gicp", x26, np); if (rc) return rc; }
  { const int rc = gicp_model_of(c, "scan gicp"); if (rc) return rc; }
  if (c->gicp.epoch != c->map_epoch || c->gicp.n != c->map_n)
    return fail(c, FLIMO_ERR_NOMAP, "scan gicp: the model is stale: the stored points have changed since flimo_gicp_build");
  const size_t n = c->scan_n;
  if (c->scan_cov_n != n || (n > 0 && !c->d_scan_cov))
    return fail(c, FLIMO_ERR_NOMAP, "scan gicp: the resident scan of %zu points has no covariances (flimo_scan_cov_set)", n);
  if (np == 0) return FLIMO_OK;
  { const int rc0 = ensure_index(c); if (rc0) return rc0; }
  if (n > ((size_t)1 << 28)) return fail(c, FLIMO_ERR_TOO_LARGE, "scan gicp: a scan of more than 2^28 points");
  if (n == 0 || !c->grid_valid || max_dist == 0.f) {      // an empty scan or map, a gate that admits nothing: no pair has a neighbour
    for (size_t j = 0; j < np; j++) { valid[j] = 0; cost[j] = 0.0; }
    zero_H_g(H, g, np);
    if (pair_idx) for (size_t i = 0; i < np * n; i++) pair_idx[i] = -1;
    if (pair_m) for (size_t i = 0; i < np * n; i++) pair_m[i] = std::numeric_limits<double>::quiet_NaN();
    return FLIMO_OK;
  }
  { const int rcf = enter_flushed(c); if (rcf) return rcf; }
  // scratch of this call, released on every exit path
  DevScratch d;
  PoseChunks P(d, c->gicp_chunk, n, np);
  const size_t m = P.m, nseg = sum_segments(n);
  float* d_poses = P.d_poses;
  float* d_sqd = d.get<float>(m * n);
  int32_t* d_idx = d.get<int32_t>(m * n);
  uint2* d_work = d.get<uint2>(m * n);
  unsigned* d_nwork = d.get<unsigned>(1);
  double* d_m = pair_m ? d.get<double>(m * n) : nullptr;
  double* d_part = d.get<double>(m * nseg * GICP_NUM);
  int32_t* d_part_cnt = d.get<int32_t>(m * nseg);
  double* d_sums = d.get<double>(m * GICP_NUM);
  long long* d_valid = d.get<long long>(m);
  { const int rc = d.ok(c); if (rc) return rc; }
  static_assert(GICP_NUM == 28, "unpack_sums takes 28 numbers a pose");
  // (the results of every chunk are gathered on the host first: the caller's arrays stay untouched if a later chunk fails)
  std::vector<double> sums(m * GICP_NUM), all_sums(np * GICP_NUM), hm(pair_m ? np * n : 0);
  std::vector<long long> counts(m), all_counts(np);
  std::vector<int32_t> hi(pair_idx ? np * n : 0);
  const int rc = P.run(c, x26, np,
    [&](size_t, size_t kk) -> int {
      HIPCHK(c, launch_scan_gicp(c->stream, c->grid, c->d_map_raw, c->d_scan, (unsigned)n, d_poses, (unsigned)kk, max_dist, c->gicp.d_cov, c->d_scan_cov,
                                 d_sqd, d_idx, d_work, d_nwork, d_m, d_part, d_part_cnt, d_sums, d_valid));
      return FLIMO_OK;
    },
    [&](size_t a, size_t kk) -> int {
      HIPCHK(c, hipMemcpyAsync(counts.data(), d_valid, kk * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(sums.data(), d_sums, kk * GICP_NUM * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      if (pair_idx) HIPCHK(c, hipMemcpyAsync(hi.data() + a * n, d_idx, kk * n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
      if (pair_m) HIPCHK(c, hipMemcpyAsync(hm.data() + a * n, d_m, kk * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      return FLIMO_OK;
    },
    [&](size_t a, size_t kk) {
      memcpy(all_sums.data() + a * GICP_NUM, sums.data(), kk * GICP_NUM * sizeof(double));
      memcpy(all_counts.data() + a, counts.data(), kk * sizeof(long long));
    });
  if (rc) return rc;
  unpack_sums(all_sums.data(), 0, np, H, g, cost);
  for (size_t j = 0; j < np; j++) valid[j] = (int32_t)all_counts[j];
  if (pair_idx) memcpy(pair_idx, hi.data(), hi.size() * sizeof(int32_t));
  if (pair_m) memcpy(pair_m, hm.data(), hm.size() * sizeof(double));
  return FLIMO_OK;
}
extern "C" int flimo_set_gicp_chunk(flimo_ctx* c, size_t pairs) { return set_chunk(c, &flimo_ctx::gicp_chunk, pairs, (size_t)1 << 20); }
extern "C" int flimo_gicp_eigen_host(const double cov6[6], double eig12[12]) {
  if (!cov6 || !eig12) return FLIMO_ERR_INVALID;
  double l[3], v[3][3];
  gicp_eigen(cov6, l, v);
  memcpy(eig12, l, sizeof l);
  memcpy(eig12 + 3, v, sizeof v);
  return FLIMO_OK;
}
extern "C" int flimo_gicp_regularize_host(const double cov6[6], int rule, double eps, double out6[6]) {
  if (!cov6 || !out6) return FLIMO_ERR_INVALID;
  if ((rule != FLIMO_GICP_PLANE && rule != FLIMO_GICP_CLAMP) || !(eps > 0.0 && eps <= 1.0)) return FLIMO_ERR_INVALID;
  return gicp_regularize(cov6, rule, eps, out6) ? 1 : 0;
}
extern "C" int flimo_gicp_term_host(const float w3[3], const float b3[3], const float p3[3], const float R9[9], const double CA6[6], const double CB6[6],
                                    double out30[30]) {
  if (!w3 || !b3 || !p3 || !R9 || !CA6 || !CB6 || !out30) return FLIMO_ERR_INVALID;
  return gicp_term(w3, b3, p3, R9, CA6, CB6, out30) ? 1 : 0;
}
