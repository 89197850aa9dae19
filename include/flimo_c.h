/* include/flimo_c.h -- C ABI of the MI355X-native fast_LIMO registration hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  Each entry point
 * names the reference interface it replaces (paths relative to the fast_LIMO tree,
 * include/fast_limo/... unless stated).  INTEGRATION.md shows how the reference's
 * Mapper / Localizer / h_share_model call these.
 *
 * Conventions
 *   - every function returns FLIMO_OK (0) or a negative error code; flimo_last_error() gives text.
 *     Nothing throws or exits across this boundary (the reference prints and returns,
 *     Modules/Localizer.cpp:249-260,379-380).
 *   - one flimo_ctx owns one GPU's map, scan scratch and HIP stream; it is not re-entrant (the
 *     reference serialises the update under mtx_ikfom, Modules/Localizer.cpp:326-353).
 *   - the library fails loudly (FLIMO_ERR_NO_DEVICE) when no gfx950 device is present: there is
 *     no CPU fallback.
 *   - x26 = flat state_ikfom (IKFoM/use-ikfom.hpp:12-21):
 *       pos[3] rot(x,y,z,w) offset_R_L_I(x,y,z,w) offset_T_L_I[3] vel[3] bg[3] ba[3] grav[3]
 */
#ifndef FLIMO_C_H
#define FLIMO_C_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define FLIMO_OK 0
#define FLIMO_ERR_NO_DEVICE (-1)
#define FLIMO_ERR_INVALID (-2)
#define FLIMO_ERR_HIP (-3)
#define FLIMO_ERR_NOMAP (-4)
#define FLIMO_ERR_TOO_LARGE (-5)
#define FLIMO_ERR_UNSUPPORTED (-6)
#define FLIMO_ERR_TIMEOUT (-7)      /* a pass did not publish its result within the wait bound (flimo_set_wait_timeout_ms) */

typedef struct flimo_ctx flimo_ctx;

/* Config::iKFoM::Mapping::Octree (Utils/Config.hpp:64-68) + the GPU grid knob. */
typedef struct flimo_map_cfg {
  float min_extent;  /* Octree/min_extent (default 0.2) */
  int bucket_size;   /* accepted and ignored: the reference setter is a no-op, effective 32
                        (Objects/Octree.hpp:155,178-180) */
  int downsample;    /* Octree/downsampling */
  float cell_size;   /* GPU hash-grid cell edge [m]; <= 0 selects the default (0.5 m) */
} flimo_map_cfg;

/* Config::iKFoM::Mapping (Utils/Config.hpp:58-63) + ikfom.estimate_extrinsics */
typedef struct flimo_match_cfg {
  int NUM_MATCH_POINTS;    /* k in 3..8; 5 (every shipped configuration) runs the specialised kernels, other values a general pass */
  int MAX_NUM_MATCHES;     /* Modules/Localizer.cpp:539 */
  int MAX_NUM_PC2MATCH;    /* Modules/Mapper.cpp:63 */
  double MAX_DIST_PLANE;   /* Objects/Plane.cpp:47 (compared with a SQUARED distance) */
  double PLANE_THRESHOLD;  /* Objects/Plane.cpp:73,110 */
  int estimate_extrinsics; /* Modules/Localizer.cpp:569 */
} flimo_match_cfg;

/* One per scan point: what Mapper::match_plane produced (debug / parity surface; replaces
 * Localizer::get_matches(), Modules/Localizer.cpp:139-141,575-576). */
typedef struct flimo_match_rec {
  float H[12];       /* calculate_H row [n, A, B, C] (B, C zero unless estimate_extrinsics) */
  float h;           /* -dist */
  float valid;       /* 1.0f if the plane passed all gates (Match::lisanAlGaib) else 0.0f */
  float n[4];        /* plane n_ABCD */
  float p_global[3]; /* scan point in the world frame */
  float sqd[5];      /* ascending squared distances of the 5 neighbours */
  int32_t nbr[5];    /* indices into the map's insertion order (see flimo_map_points) or -1 */
  int32_t n_nbr;
} flimo_match_rec;

/* IMU frame handed to the deskew kernel: fast_limo::State (Objects/State.hpp:22-48) */
typedef struct flimo_frame {
  float p[3], q[4] /* x,y,z,w */, v[3], g[3], w[3], a[3], bg[3], ba[3];
  double time;
} flimo_frame;

/* ---- context ---- */
int flimo_ctx_create(int device, flimo_ctx** out);
void flimo_ctx_destroy(flimo_ctx* ctx);
const char* flimo_last_error(const flimo_ctx* ctx);
const char* flimo_version(void);

/* ---- map: replaces fast_limo::Mapper::{set_config,add,exists,size} (Modules/Mapper.cpp:38-57,88-96)
 *      and octree::Octree::{initialize,update} (Objects/Octree.hpp:282-432) ---- */
int flimo_map_config(flimo_ctx* ctx, const flimo_map_cfg* cfg);
/* xyz: n points, stride_bytes between consecutive points (>= 12), host memory.  NaN points are
 * dropped (Octree::processPoints, Objects/Octree.hpp:243-244); a batch without a finite point changes nothing.
 * Where the reference has no answer: a map whose stored points all lie at one location (octree root of size zero) takes a batch
 * that leaves that location as initialize(stored points followed by the batch), everything stored, in order.
 * FLIMO_ERR_UNSUPPORTED, map untouched: the octree root the batch needs lies more than 48 halvings above 2 * min_extent
 * ("octree too deep").  Both hold for every call that adds to the map. */
int flimo_map_add(flimo_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes, double stamp);
int flimo_map_clear(flimo_ctx* ctx);
/* A local map (no counterpart in the reference, whose octree has no erase): keeps the stored points inside [lo, hi] (inclusive,
 * per axis, float32 compares), in insertion order; afterwards the map is the reference octree's clear() + initialize(kept)
 * (Objects/Octree.hpp:186-189, 282-298): insertion indices are renumbered (a kept point's new index is its rank among the kept
 * ones), the down-sampling memory of the kept region starts afresh, the k-NN index is laid out over the kept points' box.
 * *removed (may be NULL) receives how many points went.  A crop that removes nothing changes nothing; one that removes everything
 * leaves the map as flimo_map_clear does, except flimo_map_last_time, which a crop never touches.  FLIMO_ERR_INVALID for a NULL /
 * NaN / lo > hi box.  Same calling rules as flimo_map_add: no pass of this context in flight. */
int flimo_map_crop_box(flimo_ctx* ctx, const float lo[3], const float hi[3], size_t* removed);
/* Forgetting by sight: the stored points that the scan resident in the context (flimo_scan_set / flimo_deskew...) measurably looks
 * THROUGH from the sensor origin -- a car that drove off, a person who walked by, a door now open.  The standard visibility
 * (range-image) cleaning of a LiDAR map; the counterpart of flimo_scan_fitness, which finds scan points without map support.
 *
 * Definition (every operation float32, IEEE, nothing contracted; tests/carve_common.py restates it in numpy, bit for bit):
 *  - pixel of a point x (a scan point moved to the world frame, or a stored point): v = x - sensor_xyz.  No pixel when a component of
 *    v is not finite or the depth m below is 0.  Face axis: x if |vx| >= |vy| and |vx| >= |vz|, else y if |vy| >= |vz|, else z;
 *    m = |v_axis| (the depth a z-buffer on a cube face stores), face = 2 * axis + (v_axis < 0).  (a, b) = the other two components
 *    in cyclic order (x: y,z  y: z,x  z: x,y); u = a / m, t = b / m; hr = (float)(0.5 * res); column iu = min(res - 1,
 *    (int)((u + 1.0f) * hr)), row it likewise from t.  A cube map needs only '/' and compares, no atan2 / asin.
 *  - range image D[6][res][res]: the minimum of m over the scan's world points that have a pixel -- point i of
 *    flimo_scan_to_world(ctx, x26, ..), the same matrix, the same c0*x + (c1*y + (c2*z + c3)); a pending deskew runs first --,
 *    +inf where there is none.  A minimum over the floats' bits: the order of the scan and the launch shape do not matter.
 *  - a stored point q with pixel (f, it, iu) and depth m is seen through iff m <= max_depth (INFINITY: no bound), the window
 *    [it - win, it + win] x [iu - win, iu + win] lies wholly on the face, D[f][it][iu] is finite (an empty pixel is no evidence),
 *    and with thr = m + (margin + rel_margin * m), thr < D (strict) at every pixel of the window that holds a return.
 *  The window never wraps over a cube edge: a stored point whose pixel is closer than `win` pixels to its face's border is KEPT,
 *  whatever the scan says (a strip of win / res of each face along the cube's edges; another sweep, from another place, sees it
 *  elsewhere on a face).  With margin, rel_margin >= 0 the scan's own points are never seen through, inserted or not.  win >= 1 is
 *  the recommended setting: at win 0 a grazing surface is carved by its own neighbouring returns.
 * x26: pos and rot are read.  sensor_xyz: the sensor origin in the WORLD frame (the caller's: t + R * lidar-to-body translation). */
typedef struct flimo_carve_cfg {
  int res;            /* pixels along a cube face's side, 8..1024 (the image is 24 * res * res bytes of device scratch) */
  int win;            /* half-width of the window of pixels a point is tested against, 0..3 */
  float margin;       /* metres a return must lie behind the point, >= 0 */
  float rel_margin;   /* ... plus this share of the point's depth, >= 0 */
  float max_depth;    /* points deeper than this are kept; > 0 or INFINITY */
} flimo_carve_cfg;
/* The predicate alone: mask[i] (may be NULL; cap >= flimo_map_size elements otherwise) = 1 where stored point i (insertion order) is
 * seen through, 0 elsewhere; *count (may be NULL) = how many are.  Changes nothing: not the map, not the scan, not the bits of a
 * later pass.  An empty map or an empty scan: FLIMO_OK, count 0. */
int flimo_map_seen_through(flimo_ctx* ctx, const double x26[26], const float sensor_xyz[3], const flimo_carve_cfg* cfg,
                           unsigned char* mask, size_t cap, size_t* count);
/* Keeps the stored points that are NOT seen through and -- when a box is given (lo, hi both non-NULL; both NULL: no box) -- lie
 * inside [lo, hi] (inclusive, as flimo_map_crop_box), in insertion order, in one pass over the map; a sweep that is due a crop and a
 * carve pays for one relayout.  Afterwards everything is as flimo_map_crop_box documents: the map is clear() + initialize(kept),
 * insertion indices are renumbered, flimo_map_last_time is untouched.  *removed (may be NULL) receives how many points went.
 * Removing nothing changes nothing; removing everything leaves the map as a crop that removes everything does.  An empty map or an
 * empty scan: FLIMO_OK, *removed = 0, nothing changes -- also with a box (the box alone is flimo_map_crop_box's business).
 * Both calls: FLIMO_ERR_INVALID -- outputs and map untouched -- for a NULL ctx / x26 / sensor_xyz / cfg, a non-finite position,
 * rotation or sensor value, res outside 8..1024, win outside 0..3, a NaN or negative margin / rel_margin, max_depth NaN or <= 0, a
 * NaN / lo > hi box or only one of lo / hi, cap < flimo_map_size with a non-NULL mask.  Same calling rules as flimo_map_crop_box:
 * no pass of this context in flight. */
int flimo_map_carve(flimo_ctx* ctx, const double x26[26], const float sensor_xyz[3], const flimo_carve_cfg* cfg,
                    const float lo[3], const float hi[3], size_t* removed);
/* Forgetting by neighbour statistics: the stored points that belong to no surface -- returns from rain, dust and multipath, the
 * thin residue a carve leaves behind a departed car.  PCL's StatisticalOutlierRemoval and RadiusOutlierRemoval over the map, one
 * call, the neighbour lists never leaving the GPU.
 *
 * Definition (tests/outliers_common.py restates it in numpy).  Point i of the range is stored point first + i, insertion order:
 *  - neighbour list L_i = flimo_knn_k(p_i, k + 1, max_dist): the same predicate (strict float32 sqd < max_dist * max_dist, one
 *    float32 product; INFINITY: no gate), the same unique order (float32 squared-distance bits, then insertion index), over the WHOLE
 *    map whatever the range.
 *  - the point itself: the slot whose index is first + i is dropped.  When no slot holds it and the list is full -- more than k exact
 *    duplicates with lower indices precede the point --, the last slot is dropped.  (A gate that admits not even the point itself:
 *    the list is empty, nothing is dropped.)  cnt[i] = c_i = the slots left, <= k.
 *  - distances d_j = (double)sqrtf(sqd_j), the correctly rounded float32 square root, widened.
 *  - S_i = the pairwise tree ((s0 + s1) + (s2 + s3)) + ... over the 64 slots of L_i in their original positions, the dropped slot
 *    and the empty slots holding +0.0; mean_dist[i] = m_i = S_i / c_i, NaN for c_i = 0.  The bits depend on the list alone.
 *  - statistics set T = { i : c_i >= max(1, min_pts) }, N = |T| = n_stat; mu = (sum over T of m_i) / N; sigma = sqrt((sum over T of
 *    (m_i - mu)^2) / (N - 1)), two passes, 0 for N = 1; threshold = mu + (double)std_mul * sigma.  The two sums are float64, taken
 *    on the device in one fixed shape over the range's n slots (a slot outside T adds +0.0; flimo_sums.h), no floating-point
 *    atomics: their bits depend on the stored points, first, n and the cfg only -- not on the chunking, the cell size or the path
 *    of the search.  The divisions, the square root and the threshold are the host's.  N = 0: mu, sigma and threshold are NaN and
 *    the statistical rule selects nothing.
 *  - point i is an outlier iff c_i < min_pts (the count rule: `few`), or std_mul is finite and i is in T and m_i > threshold (the
 *    statistical rule: `far`).  T makes the two disjoint: outliers = few + far.
 * min_pts = 0, max_dist = INFINITY is StatisticalOutlierRemoval (mean k, std_mul); std_mul = INFINITY, max_dist = r, min_pts = m
 * is RadiusOutlierRemoval (radius r, at least m neighbours) for m <= k. */
typedef struct flimo_outlier_cfg {
  int   k;         /* neighbours per point, the point itself excluded: 1 .. FLIMO_KNN_MAX_K - 1 (63) */
  float max_dist;  /* gate as flimo_knn_k (strict sqd < max_dist*max_dist, one float32 product); INFINITY: none */
  int   min_pts;   /* count rule: a point with fewer neighbours inside the gate is an outlier; 0 .. k; 0: off */
  float std_mul;   /* statistical rule: mean distance > mu + std_mul * sigma; >= 0; INFINITY: off */
} flimo_outlier_cfg;
typedef struct flimo_outlier_stats {
  uint64_t n, n_stat;          /* points of the range; those that enter mu / sigma */
  double   mu, sigma, threshold;
  uint64_t few, far, outliers; /* by the count rule, by the statistical rule, together */
} flimo_outlier_stats;
/* The predicate alone over the stored points first .. first + n - 1: mask[i] = 1 where point i is an outlier, 0 elsewhere;
 * mean_dist[i] = m_i; cnt[i] = c_i; *stats.  Each output may be NULL.  Changes nothing: not the map, not the scan, not the bits of
 * a later pass.  n = 0 (also on an empty map, first = 0): FLIMO_OK, the counts of *stats 0, mu / sigma / threshold NaN. */
int flimo_map_outliers(flimo_ctx* ctx, size_t first, size_t n, const flimo_outlier_cfg* cfg, unsigned char* mask, double* mean_dist,
                       int32_t* cnt, flimo_outlier_stats* stats);
/* Keeps every stored point that is outside the range or is not an outlier, in insertion order, in one ordered compaction pass (the
 * range form cleans what was added since the last cleaning; the neighbours are the whole map's all the same).  Afterwards
 * everything is as flimo_map_crop_box documents: the map is clear() + initialize(kept), insertion indices are renumbered,
 * flimo_map_last_time is untouched.  *removed (may be NULL) receives how many points went, *stats (may be NULL) the predicate's.
 * Removing nothing changes nothing; removing everything leaves the map as a crop that removes everything does.
 * Both calls: FLIMO_ERR_INVALID -- outputs and map untouched -- for a NULL ctx or cfg, first + n beyond flimo_map_size, max_dist
 * or std_mul NaN or negative, min_pts outside 0..k; FLIMO_ERR_UNSUPPORTED for k outside 1..63.  Same calling rules as
 * flimo_map_crop_box: no pass of this context in flight. */
int flimo_map_remove_outliers(flimo_ctx* ctx, size_t first, size_t n, const flimo_outlier_cfg* cfg, size_t* removed,
                              flimo_outlier_stats* stats);
size_t flimo_map_size(const flimo_ctx* ctx);
double flimo_map_last_time(const flimo_ctx* ctx);
/* copies the stored points (insertion order: what neighbour indices refer to) as packed xyz; *n receives the total count
 * (Octree::getData, Objects/Octree.hpp:198-215) */
int flimo_map_points(flimo_ctx* ctx, float* xyz_out, size_t cap, size_t* n);

/* ---- exact k-NN: replaces octree::Octree::knn (Objects/Octree.hpp:526-555) for a batch ----
 * q_xyz packed [nq][3] host; outputs host: idx [nq][k] (the map's insertion order, -1 padded),
 * sqd [nq][k] ascending squared distances (0 padded), cnt [nq].  k <= 5.  No gate: like Octree::knn the call answers from
 * anywhere -- rings of cells near the map, then a best-first search over the index's tiles (nearest tile first, until the next
 * one is farther than the k-th best): a query kilometres from every point costs a look at the tile directory, not at the
 * empty space in between. */
int flimo_knn(flimo_ctx* ctx, const float* q_xyz, size_t nq, int k, int32_t* idx, float* sqd, int32_t* cnt);

/* ---- exact radius search: replaces octree::Octree::radiusSearch (Objects/Octree.hpp:453-523) for a batch ----
 * For every query q the call returns exactly the stored points p with
 *     sqdist3(q, p) < radius * radius     (strict; all float32: dx*dx + (dy*dy + dz*dz) uncontracted, the reference's
 *                                          (p - query).squaredNorm(); radius * radius one float32 product, Octree.hpp:467)
 * each with its insertion index (what flimo_knn returns, what flimo_map_points is ordered by), that squared distance and,
 * optionally, its xyz.
 *  - The reference takes every point of an octant whose farthest corner lies inside the ball without testing the point
 *    (Octree.hpp:485-503).  In exact arithmetic that is the same set; in float32 it could differ by a rounding.  A restatement of
 *    that traversal (tests/radius_ref) agrees with the plain predicate on every query checked; the contract here is the predicate.
 *  - The reference's order within a query is its tree's traversal order; it is not reproduced.  Default: unspecified, but the same
 *    for two calls on an unchanged map.  FLIMO_RADIUS_SORTED: ascending by (squared-distance bits, insertion index) -- unique.
 * Output in CSR form, host memory: the results of query i are [offsets[i], offsets[i + 1]) of idx / sqd / xyz ([..][3]);
 * *total = offsets[nq].  offsets ([nq + 1]) is required; idx, sqd, xyz and total may each be NULL.  All three of idx, sqd, xyz
 * NULL: count only (no fill launch, no result scratch).  cap = results the non-NULL arrays can hold: total > cap returns
 * FLIMO_ERR_TOO_LARGE with offsets and *total valid and the arrays untouched (call again with room); so does a total above
 * 2^31 - 1, whatever cap (a count-only call has no such limit).  FLIMO_ERR_INVALID: NULL ctx / q_xyz (nq > 0) / offsets, a
 * radius that is NaN, infinite or negative, unknown flag bits.  radius == 0: every query is empty (nothing is < 0); a query with
 * a NaN coordinate is empty; an empty map (Octree.hpp:459) gives all offsets 0; nq == 0 gives offsets[0] = 0.  The cost follows
 * the points and the index tiles the ball meets, not its volume: a ball of kilometres over a sparse map skips the tiles that do
 * not exist.  Calling rules as flimo_knn. */
#define FLIMO_RADIUS_SORTED 1u
int flimo_radius_search(flimo_ctx* ctx, const float* q_xyz, size_t nq, float radius, unsigned flags, uint64_t* offsets /* [nq + 1] */,
                        int32_t* idx, float* sqd, float* xyz /* [..][3] */, size_t cap, uint64_t* total);

/* ---- exact k-NN for any k up to FLIMO_KNN_MAX_K, with a distance gate: octree::Octree::knn (Objects/Octree.hpp:526-555), which
 *      takes any k, and -- with a finite gate -- the max_nn form of a radius search (PCL's radiusSearch(p, r, idx, d, max_nn)) ----
 * Order the stored points of a query by the key (float32 squared-distance bits, insertion index), ascending.  The distance is
 * sqdist3: dx*dx + (dy*dy + dz*dz), uncontracted, float32 (distances are non-negative floats, so bit order is value order); the
 * index is what flimo_knn, flimo_radius_search and flimo_map_points use.  That is a total order, unique, and independent of where a
 * point lies in the map's internal arrays.
 *  - max_dist == INFINITY: no gate.  The result is the first min(k, map size) points of that order.
 *  - a finite max_dist >= 0 admits only points with sqd < max_dist * max_dist (strict; the square one float32 product: exactly
 *    flimo_radius_search's predicate).  The result is then, entry for entry, the first k results of
 *    flimo_radius_search(.., max_dist, FLIMO_RADIUS_SORTED).  max_dist == 0: every query is empty.
 * Outputs, host memory: cnt[q] = number of results of query q; idx [nq][k], sqd [nq][k] and (optional, may be NULL) xyz [nq][k][3]
 * hold them in that order; the slots beyond cnt[q] are idx = -1, sqd = 0, xyz = 0.  idx, sqd and cnt are required.
 * Difference from flimo_knn: for k <= 5 sqd is bit-equal to flimo_knn's; idx may differ only where candidates tie exactly in
 * distance -- flimo_knn keeps the reference's first-met choice among them (the registration depends on it), this call its own
 * unique order.
 * A query with a NaN coordinate gives cnt 0; an empty map gives all cnt 0 (Octree::knn with root_ == nullptr); nq == 0 returns
 * FLIMO_OK.  FLIMO_ERR_INVALID: NULL ctx / q_xyz (nq > 0) / idx / sqd / cnt, max_dist NaN or negative.  FLIMO_ERR_UNSUPPORTED: k
 * outside 1 .. FLIMO_KNN_MAX_K.  FLIMO_ERR_TOO_LARGE: nq * k >= 2^31.
 * Calling rules as flimo_knn, and like it the call answers from anywhere at bounded cost: a few rings of cells near the map, then
 * a best-first walk over the index's existing tiles (nearest first, until the next one is farther than the k-th best or the
 * gate); a query kilometres from every point, or in the empty middle of a sparse map, costs a look at the tile directory and the
 * nearest tiles.  With a finite gate the search also stops at the gate. */
#define FLIMO_KNN_MAX_K 64
int flimo_knn_k(flimo_ctx* ctx, const float* q_xyz, size_t nq, int k, float max_dist, int32_t* idx /* [nq][k] */,
                float* sqd /* [nq][k] */, float* xyz /* [nq][k][3], may be NULL */, int32_t* cnt /* [nq] */);

/* ---- plane normals and covariances of the map's k-NN neighbourhoods: what pcl::NormalEstimation computes (the reference's ROS
 *      side links PCL), over the resident map and without the neighbour lists ever leaving the GPU ----
 * The neighbourhood of query i is exactly flimo_knn_k(q_i, k, max_dist): same predicate, same unique order, same cnt.  With its
 * n = cnt[i] points p_j, all in float64:
 *     r_j = (double)p_j - (double)q          (exact: the precision does not depend on how far the map lies from the origin)
 *     m   = sum r_j / n                      centroid = (double)q + m
 *     C   = sum (r_j - m)(r_j - m)^T / n     (divided by n, as pcl::computeMeanAndCovarianceMatrix)
 *     l0 <= l1 <= l2 the eigenvalues of C; the normal is the unit eigenvector of l0 (equal eigenvalues: the lower axis of the
 *     decomposition first); curvature = l0 / (l0 + l1 + l2), 0 when that sum is 0 (PCL's rule).
 * Orientation: with a viewpoint the normal is flipped so that n . (viewpoint - q) >= 0 (pcl::flipNormalTowardsViewpoint); with
 * viewpoint == NULL its component of largest magnitude is made positive (equal magnitudes: the lowest axis decides).
 * Outputs, host memory: normal [nq][4] = nx ny nz curvature, the float32 roundings of the float64 values; cnt [nq]; optional
 * (each may be NULL) centroid [nq][3], cov [nq][6] = xx xy xz yy yz zz, eig [nq][6] = l0 l1 l2 and the float64 normal.
 * cnt[i] < max(3, min_pts): normal, centroid, cov and eig of query i are NaN; cnt[i] is still reported.  A query with a NaN
 * coordinate gives cnt 0; an empty map gives cnt 0 everywhere and FLIMO_OK; nq == 0 returns FLIMO_OK.
 * A query's results depend on its neighbour list alone: every sum is taken in one fixed shape over the list's slots, so the same
 * bits come out whatever path of the search finished the query, whatever the map's cell size, however the call is cut into
 * chunks, and in the range form below.
 * FLIMO_ERR_INVALID: NULL ctx / q_xyz (nq > 0) / normal / cnt, max_dist NaN or negative, a NaN viewpoint.  FLIMO_ERR_UNSUPPORTED:
 * k outside 1 .. FLIMO_KNN_MAX_K.  flimo_knn_k's nq * k < 2^31 does not apply (nothing of that size exists): the only bound is
 * nq < 2^31 (FLIMO_ERR_TOO_LARGE).  The outputs are untouched on an error.  Calling rules and cost as flimo_knn_k; device memory
 * is taken per chunk of 2^20 queries, not per call. */
int flimo_map_normals(flimo_ctx* ctx, const float* q_xyz, size_t nq, int k, float max_dist, int min_pts,
                      const float viewpoint[3] /* may be NULL */, float* normal /* [nq][4]: nx ny nz curvature */, int32_t* cnt /* [nq] */,
                      double* centroid /* [nq][3], may be NULL */, double* cov /* [nq][6] xx xy xz yy yz zz, may be NULL */,
                      double* eig /* [nq][6]: l0 <= l1 <= l2, then the float64 unit normal; may be NULL */);
/* The same with query i = stored point first + i (insertion index: flimo_map_points' order): nothing is uploaded, and the point is
 * its own first neighbour (distance 0), as in PCL when the search surface is the input.  Bit for bit flimo_map_normals on those
 * points.  FLIMO_ERR_INVALID also for first + n beyond flimo_map_size. */
int flimo_map_normals_range(flimo_ctx* ctx, size_t first, size_t n, int k, float max_dist, int min_pts, const float viewpoint[3],
                            float* normal, int32_t* cnt, double* centroid, double* cov, double* eig);

/* ---- FPFH descriptors of the stored points: pcl::FPFHEstimation over the map (the reference's relocation/KISS-matcher branch starts
 * its global registration from them) ----
 * 11 + 11 + 11 bins, weight 1 / squared distance, no separate own-SPFH term.  The neighbour lists and the normals never leave the
 * GPU.  The scan's descriptors come from the same call on a second context whose map is the scan.
 *
 * Definition (tests/fpfh_common.py restates it in numpy).  All arithmetic is float64 on the float32 inputs widened, nothing
 * contracted, in exactly the written association.  Point i of the range is stored point j = first + i, insertion order:
 *  - normals: N[j] = the float32 normal[j][0..2] of flimo_map_normals_range(0, flimo_map_size, normal_k, normal_max_dist,
 *    normal_min_pts, viewpoint or NULL), bit for bit: NaN below max(3, normal_min_pts) neighbours.  Of EVERY stored point.
 *  - list L_j = flimo_knn_k(p_j, k, max_dist) over the whole map, c_j entries: the same predicate, the same unique order; slot s
 *    holds the index j_s and the float32 sqd_s.
 *  - pair features of source s = j and target t = j_s, for every slot with sqd_s != 0 (this drops the point itself and its exact
 *    duplicates); no pair if a component of N[s] or N[t] is NaN.  d = p_t - p_s; f4 = sqrt(d.x*d.x + (d.y*d.y + d.z*d.z));
 *    a1 = (N[s].x*d.x + (N[s].y*d.y + N[s].z*d.z)) / f4, a2 the same with N[t].  If fabs(a1) < fabs(a2): u = N[t], m = N[s],
 *    d = -d, f3 = -a2; otherwise u = N[s], m = N[t], f3 = a1 (PCL's acos(|a1|) > acos(|a2|) without the acos).  v = d x u, each
 *    component a*b - c*d as two products and one subtraction; vn = sqrt(v.x*v.x + (v.y*v.y + v.z*v.z)); no pair if vn == 0;
 *    v = v / vn (three divisions).  w = u x v; f2 = v.x*m.x + (v.y*m.y + v.z*m.z); f1 = atan2(w.m, u.m), the dot products in the
 *    same association, the device's float64 atan2.  Bins, each clamped to 0..10: h1 = floor(11.0 * ((f1 + M_PI) * (1.0 / (2.0 *
 *    M_PI)))), h2 = floor(11.0 * ((f2 + 1.0) * 0.5)), h3 = floor(11.0 * ((f3 + 1.0) * 0.5)).
 *  - spfh[j][0..32]: the integer counts per bin (h1 in 0..10, h2 in 11..21, h3 in 22..32) over the pairs of j; the increment is
 *    inc_j = c_j >= 2 ? 100.0 / (double)(c_j - 1) : 0.0 (PCL's 100 / (indices.size() - 1)).  A point with a NaN normal has an
 *    all-zero row; its FPFH is still formed from its neighbours.
 *  - fpfh: for slot s of L_j, w_s = sqd_s != 0 ? 1.0 / (double)sqd_s : +0.0 and t_s[b] = w_s * ((double)spfh[j_s][b] * inc_{j_s});
 *    F[b] = the pairwise tree ((t_0 + t_1) + (t_2 + t_3)) + ... over the 64 slots, empty ones holding +0.0 (flimo_map_outliers'
 *    tree).  Per group g of 11 bins S_g = F[11g] + F[11g+1] + ... in ascending order; fpfh[i][b] = S_g != 0 ? (float)(F[b] *
 *    (100.0 / S_g)) : 0.0f.  cnt[i] = c_j.
 * The integer rows depend on nothing but the lists and the normals and the sums have one fixed shape: the bits of a row do not
 * depend on the chunking, the cell size or the path of the search.
 * Cost: the normals and the SPFH rows are formed for the WHOLE map whatever the range (a neighbour can be anywhere), nothing is kept
 * between calls; device scratch is 50 B a stored point plus 220 B a point of a chunk of 2^20.
 * n = 0 (also on an empty map, first = 0): FLIMO_OK, nothing touched.  FLIMO_ERR_INVALID -- outputs untouched -- for a NULL ctx or
 * cfg, a NULL fpfh with n > 0, first + n beyond flimo_map_size, max_dist or normal_max_dist NaN or negative, a NaN viewpoint with
 * has_viewpoint, normal_min_pts < 0; FLIMO_ERR_UNSUPPORTED for k outside 2..FLIMO_KNN_MAX_K or normal_k outside
 * 1..FLIMO_KNN_MAX_K.  Calling rules as flimo_map_outliers: no pass of this context in flight; changes nothing: not the map, not the
 * scan, not the bits of a later pass. */
typedef struct flimo_fpfh_cfg {
  int   k;               /* feature neighbourhood, the point itself included: 2 .. FLIMO_KNN_MAX_K */
  float max_dist;        /* gate of that neighbourhood, as flimo_knn_k; INFINITY: none */
  int   normal_k;        /* the normals: those of flimo_map_normals_range with normal_k, normal_max_dist, normal_min_pts, viewpoint */
  float normal_max_dist;
  int   normal_min_pts;
  int   has_viewpoint;   /* 0: the normals' own orientation rule */
  float viewpoint[3];
} flimo_fpfh_cfg;
int flimo_map_fpfh(flimo_ctx* ctx, size_t first, size_t n, const flimo_fpfh_cfg* cfg, float* fpfh /* [n][33], required */,
                   uint8_t* spfh /* [n][33], may be NULL */, int32_t* cnt /* [n], may be NULL */);

/* ---- ISS keypoints of the stored points: pcl::ISSKeypoint3D (Zhong 2009) over the map -- the detector that goes in front of the
 * descriptors, so that flimo_map_fpfh's rows of plane interiors need not be matched ----
 * The neighbour lists and the eigenvalues never leave the GPU; the non-maximum suppression is a gather over the list.
 *
 * Definition (tests/keypoints_common.py restates it in numpy).  Point i of the range is stored point j = first + i, insertion order.
 *  - saliency of EVERY stored point t: (c_t, l0, l1, l2) = cnt and eig[0..2] of flimo_map_normals_range(t, 1, k, max_dist, min_pts,
 *    NULL), bit for bit (the orientation does not enter).  t is SALIENT iff c_t >= max(3, min_pts), l0 > 0.0,
 *    l1 < (double)gamma21 * l2 and l0 < (double)gamma32 * l1: each test one float64 product and a strict compare, no division; a
 *    NaN fails.  s_t = l0 then.  saliency[i] = s_j, a quiet NaN when j is not salient; cnt[i] = c_j.
 *  - suppression: N_j = flimo_knn_k(p_j, nms_k, nms_max_dist) over the whole map, the same predicate, the same unique order.  j is a
 *    KEYPOINT iff it is salient and no entry t != j of N_j is salient with s_t > s_j, or with s_t == s_j and t < j: among exact ties
 *    the lower insertion index wins, so of a point and its exact duplicates at most one survives.  mask[i] = 1 / 0; *count = the
 *    number of ones, exact.
 * Differences from PCL: the scatter is taken about the neighbourhood's centroid and divided by n, as flimo_map_normals forms it
 * (PCL: about the point); the neighbourhoods are the max_nn form of a radius search -- the first k inside the gate --, not every
 * point in the radius; ties are broken instead of both points kept; there is no border estimation.
 * Every output is an integer, a bit, or a float64 that flimo_map_normals_range already defines: the bits do not depend on the
 * chunking, the cell size, the range form or the path of the search.
 * Cost: the saliency is formed for the WHOLE map whatever the range (a neighbour can be anywhere), nothing is kept between calls;
 * device scratch is 8 B a stored point plus 85 B a point of a chunk of 2^20.
 * n = 0 (also on an empty map, first = 0): FLIMO_OK, *count = 0, nothing else touched.  FLIMO_ERR_INVALID -- outputs untouched --
 * for a NULL ctx or cfg, first + n beyond flimo_map_size, max_dist or nms_max_dist NaN or negative, gamma21 or gamma32 NaN or outside
 * (0, 1], min_pts < 0; FLIMO_ERR_UNSUPPORTED for k outside 3..FLIMO_KNN_MAX_K or nms_k outside 2..FLIMO_KNN_MAX_K;
 * FLIMO_ERR_TOO_LARGE for a map of 2^31 points or more.  Calling rules as flimo_map_fpfh: no pass of this context in flight;
 * changes nothing: not the map, not the scan, not the bits of a later pass. */
typedef struct flimo_keypoint_cfg {
  int   k;             /* salient neighbourhood, the point itself included: 3 .. FLIMO_KNN_MAX_K */
  float max_dist;      /* its gate, as flimo_knn_k (the salient radius); INFINITY: none */
  int   min_pts;       /* fewer neighbours than max(3, min_pts): not salient; >= 0 */
  float gamma21;       /* l1 < gamma21 * l2 required; in (0, 1] */
  float gamma32;       /* l0 < gamma32 * l1 required; in (0, 1] */
  int   nms_k;         /* suppression neighbourhood, the point itself included: 2 .. FLIMO_KNN_MAX_K */
  float nms_max_dist;  /* its gate (the non-max radius); INFINITY: none */
} flimo_keypoint_cfg;
int flimo_map_keypoints(flimo_ctx* ctx, size_t first, size_t n, const flimo_keypoint_cfg* cfg,
                        unsigned char* mask /* [n], may be NULL */, double* saliency /* [n], may be NULL */,
                        int32_t* cnt /* [n], may be NULL */, size_t* count /* may be NULL */);

/* ---- Euclidean clusters of the stored points: pcl::EuclideanClusterExtraction over the map -- which stored points belong
 * together.  Cleaning (forget every component of fewer than m points: the tight blob flimo_map_outliers cannot see), objects (the
 * index lists a tracker starts from), segments for relocalisation ----
 * The neighbour lists never leave the GPU: one walk of each point's ball ends in a lock-free union-find on the device.
 *
 * Definition (tests/clusters_common.py restates it in numpy):
 *  - the vertices are the N stored points in insertion order: the order flimo_map_points returns and flimo_knn_k indexes.
 *  - {i, j}, i != j, is an edge iff sqdist3(p_i, p_j) < tol * tol: strict, all float32; sqdist3 = dx*dx + (dy*dy + dz*dz),
 *    uncontracted; tol * tol one float32 product.  flimo_radius_search's predicate with a stored point as the query; symmetric bit for
 *    bit (a - b and b - a differ by sign only).
 *  - tol == 0: no edges; every point, exact duplicates included, is its own cluster.  With tol > 0 exact duplicates share a cluster.
 *  - a cluster is a connected component of that graph over the WHOLE map, whatever the range.
 *  - label[i] = the smallest insertion index in the component of stored point first + i: unique, so the way it is computed cannot
 *    show.  size[i] = that component's number of stored points.
 *  - selection: a component is SELECTED iff min_size <= size and (max_size == 0 or size <= max_size); max_size == 0 means no upper
 *    bound.  mask[i] = 1 iff the component of point first + i is selected, 0 otherwise.
 *  - stats: n = points of the range; clusters, largest, sel_clusters = components, points of the largest one and selected components
 *    of the WHOLE map; sel_points = ones of the mask (range only).
 * Every output is an integer with one correct value: nothing depends on the chunking, the cell size, the range form, the order in
 * which edges are met or the path of the walk.  PCL's "report clusters within [min, max]" is the same two fields; dropping debris
 * is flimo_map_remove_clusters with min_size = 1, max_size = m - 1.
 * Cost: the components are formed for the whole map whatever the range, nothing is kept between calls; device scratch is 8 B a
 * stored point, 1 B a point of the range and 4 B each for label and size where they are asked for. */
typedef struct flimo_cluster_cfg {
  float tol;       /* two points closer than this (strict, float32) are joined; finite, >= 0 */
  int   min_size;  /* selected: min_size <= size ...; >= 0 */
  int   max_size;  /* ... <= max_size; 0: no upper bound; otherwise >= min_size */
} flimo_cluster_cfg;
typedef struct flimo_cluster_stats {
  uint64_t n;            /* points of the range */
  uint64_t clusters;     /* components of the whole map */
  uint64_t largest;      /* points of the largest component */
  uint64_t sel_clusters; /* selected components of the whole map */
  uint64_t sel_points;   /* ones of the mask (range only) */
} flimo_cluster_stats;
/* label / size / mask [n] and *stats over the stored points first .. first + n - 1; every output may be NULL.  Changes nothing: not
 * the map, not the scan, not the bits of a later pass.  n = 0 (also on an empty map, first = 0): FLIMO_OK, stats.n and
 * stats.sel_points 0, the three whole-map fields still filled. */
int flimo_map_clusters(flimo_ctx* ctx, size_t first, size_t n, const flimo_cluster_cfg* cfg, int32_t* label, int32_t* size,
                       unsigned char* mask, flimo_cluster_stats* stats);
/* Forgets the points OF THE RANGE whose mask is 1 (a range that cuts a component removes only the members inside it) and keeps the
 * rest in insertion order, in the one ordered compaction pass flimo_map_remove_outliers uses.  Afterwards everything is as
 * flimo_map_crop_box documents: the map is clear() + initialize(kept), insertion indices are renumbered, flimo_map_last_time is
 * untouched.  *removed (may be NULL) receives how many points went (= stats.sel_points), *stats (may be NULL) the predicate's,
 * taken before the removal.  Removing nothing changes nothing; removing everything leaves the map as a crop that removes
 * everything does.
 * Both calls: FLIMO_ERR_INVALID -- outputs and map untouched -- for a NULL ctx or cfg, first + n beyond flimo_map_size, tol NaN,
 * negative or infinite, min_size < 0 or max_size < 0, 0 < max_size < min_size; FLIMO_ERR_TOO_LARGE for a map of 2^31 points or
 * more.  Same calling rules as flimo_map_crop_box: no pass of this context in flight. */
int flimo_map_remove_clusters(flimo_ctx* ctx, size_t first, size_t n, const flimo_cluster_cfg* cfg, size_t* removed,
                              flimo_cluster_stats* stats);

/* ---- RANSAC planes of the stored points: what pcl::SACSegmentation(SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE, SAC_RANSAC)
 * does per sample, for all of the caller's samples at once against EVERY stored point -- the ground that holds the clusters of an
 * outdoor map together (find it, flimo_map_remove_plane, then flimo_map_clusters), walls, a table top ----
 * Nothing of size nh x N exists anywhere and the map never leaves the GPU.
 *
 * Definition (tests/planes_common.py restates it in numpy).  Hypothesis j is the triplet (a, b, c) = tri[j] of insertion indices
 * into the N stored points (the order flimo_map_points returns).  The samples are the caller's, so the call is deterministic.
 * Steps 1-5 are float64 on the float32 points widened, nothing contracted, exactly the written association;
 * sq(v) = v.x*v.x + (v.y*v.y + v.z*v.z).
 *  1. e1 = p_b - p_a, e2 = p_c - p_a, e3 = p_c - p_b.  DEGENERATE if two indices are equal, or if any of sq(e1), sq(e2), sq(e3)
 *     fails ">= (double)min_edge * (double)min_edge".
 *  2. cr = e1 x e2, each component y z' - z y' as two products and one subtraction; q = sq(cr).  DEGENERATE unless q > 0.0 and
 *     q >= s2 * (sq(e1) * sq(e2)), s2 = (double)min_sin * (double)min_sin: the squared sine of the angle at a.  No division.
 *  3. n = cr / sqrt(q), three divisions.  DEGENERATE if an entry is not finite.
 *  4. sign: the component of largest magnitude is made positive (equal magnitudes: the lowest axis decides) -- flimo_map_normals'
 *     rule with no viewpoint.  Negation is exact: (a, b, c) and (a, c, b) give the same bits.
 *  5. REJECTED if min_cos > 0 and not fabs(n.x*ax + (n.y*ay + n.z*az)) >= (double)min_cos; the axis is used as given, NOT normalised.
 *  6. otherwise d = -(n.x*a.x + (n.y*a.y + n.z*a.z)), plane[j] = (n, d), nf = (float)n.
 *  7. the inlier test is float32 and anchored at the sample's first point, so that its precision does not depend on how far the map
 *     lies from the origin: for stored point i, v = p_i - p_a (three float32 subtractions), t = nf.x*v.x + (nf.y*v.y + nf.z*v.z)
 *     uncontracted, and i is an inlier iff fabsf(t) < dist.  The three sample points count like any other.
 *  8. inliers[j] = the exact count over ALL N stored points.
 *  9. sum_sq[j] = the float64 sum of (double)t * (double)t (exact products) over the inliers, in ONE fixed shape: slab s is the
 *     points [s * FLIMO_PLANE_SLAB, min(N, (s + 1) * FLIMO_PLANE_SLAB)); within a slab thread T of 256 adds the slab's slots T,
 *     T + 256, ... in ascending order into a partial that starts at +0.0 (a non-inlier adds nothing); then
 *     partial[T] += partial[T + o] for o = 128, 64 .. 1; then S = ((0.0 + P_0) + P_1) + ... over the slabs in ascending order.
 * A hypothesis that is not OK has inliers 0, sum_sq +0.0 and plane NaN.  No floating-point atomics: the bits of a hypothesis's
 * outputs depend on the stored points, its triplet and the cfg alone -- not on nh, the other hypotheses, the order of tri, the
 * chunking (flimo_set_plane_chunk), the cell size or which hypotheses share a workgroup.
 * Cost: nh x N float32 tests; device scratch is chunk x ceil(N / FLIMO_PLANE_SLAB) x 12 B plus 36 B a hypothesis of the chunk and
 * 60 B a hypothesis of the call. */
#define FLIMO_PLANE_OK 0
#define FLIMO_PLANE_DEGENERATE 1
#define FLIMO_PLANE_REJECTED 2
#define FLIMO_PLANE_SLAB 8192        /* part of the contract: the sum's shape */
typedef struct flimo_plane_cfg {
  float dist;      /* inlier gate [m]: |t| < dist, strict float32; >= 0, INFINITY allowed */
  float min_edge;  /* >= 0 [m]: a sample triangle with a shorter edge is degenerate */
  float min_sin;   /* 0..1: sine of the angle at vertex a below this: degenerate (near-collinear samples) */
  float axis[3];   /* read only when min_cos > 0; used as given, NOT normalised */
  float min_cos;   /* 0..1; > 0: |n . axis| >= min_cos required (SACMODEL_PERPENDICULAR_PLANE's eps_angle); 0: none */
} flimo_plane_cfg;
/* status / inliers / sum_sq [nh] and, where given, plane [nh][4].  Changes nothing: not the map, not the scan, not the bits of a
 * later pass.  nh == 0: FLIMO_OK.  FLIMO_ERR_INVALID -- outputs untouched -- for a NULL ctx / cfg / status / inliers / sum_sq, a
 * NULL tri with nh > 0, a cfg field that is NaN or negative, min_sin or min_cos above 1, a non-finite axis with min_cos > 0, a
 * triplet index outside [0, N) (all are checked before any launch: nh > 0 on an empty map is invalid); FLIMO_ERR_TOO_LARGE for N
 * or nh >= 2^31.  Same calling rules as flimo_map_clusters: no pass of this context in flight. */
int flimo_map_planes(flimo_ctx* ctx, const int32_t* tri /* [nh][3] insertion indices */, size_t nh, const flimo_plane_cfg* cfg,
                     int32_t* status /* [nh] */, int32_t* inliers /* [nh] */, double* sum_sq /* [nh] */,
                     double* plane /* [nh][4] nx ny nz d, may be NULL */);
/* Steps 1-6 for one triplet on the host (p3 = the points a, b, c, packed xyz), through the same function the kernel calls: the
 * status, or FLIMO_ERR_INVALID for a NULL argument or a cfg flimo_map_planes rejects.  plane4 and nf are NaN unless the status is
 * FLIMO_PLANE_OK.  Needs no context and no device. */
int flimo_plane_solve_host(const float p3[9], const flimo_plane_cfg* cfg, double plane4[4], float nf[3]);

/* The mask of ONE plane and the removal: step 7's arithmetic with nf = sel->normal and p_a = sel->anchor over the stored points
 * first .. first + n - 1, the compare chosen by side.  With normal = (float)plane[j][0..2], anchor = stored point tri[j][0], the
 * same dist, side 0 and the whole map, count == inliers[j].  side -1 with the ground's normal is "the ground and everything
 * beneath it" (multipath ghosts under the road). */
typedef struct flimo_plane_sel {
  float normal[3]; float anchor[3]; float dist; int side;   /* side 0: |t| < dist;  -1: t < dist;  +1: t > -dist */
} flimo_plane_sel;
/* mask [n] (1 = inside) and *count (the ones); changes nothing.  n == 0 (also on an empty map): FLIMO_OK, *count = 0. */
int flimo_map_plane_mask(flimo_ctx* ctx, size_t first, size_t n, const flimo_plane_sel* sel,
                         unsigned char* mask /* [n], may be NULL */, size_t* count /* may be NULL */);
/* Forgets the points of the range whose mask is 1 and keeps the rest in insertion order, in the one ordered compaction pass
 * flimo_map_remove_clusters uses.  Afterwards everything is as flimo_map_crop_box documents: the map is clear() +
 * initialize(kept), insertion indices are renumbered, flimo_map_last_time is untouched.  *removed (may be NULL) receives how many
 * points went.  Removing nothing changes nothing; removing everything leaves the map as a crop that removes everything does.
 * Both calls: FLIMO_ERR_INVALID -- outputs and map untouched -- for a NULL ctx or sel, a non-finite normal or anchor, dist NaN or
 * negative, side outside -1..1, first + n beyond flimo_map_size; FLIMO_ERR_TOO_LARGE for a map of 2^31 points or more. */
int flimo_map_remove_plane(flimo_ctx* ctx, size_t first, size_t n, const flimo_plane_sel* sel, size_t* removed);

/* ---- voxel statistics and thinning of the stored points: what pcl::VoxelGrid computes per leaf -- count, centroid -- and the
 * covariance an NDT or voxel-map matcher keeps per cell, over the map; and the way to forget by DENSITY: a place visited fifty
 * times keeps no more points than a registration needs, without the map leaving the GPU ----
 *
 * Definition (tests/voxels_common.py restates it in numpy).  Stored point i (insertion order, the order flimo_map_points returns)
 * is p_i; stored points are always finite.
 * Lattice: anchored at the world origin, so a voxel is the same set of space whatever the map's extent.  inv = 1.0f / leaf (one
 *   float32 division); c_a = floorf(p_a * inv) for a = x, y, z (one float32 product, then floorf): the cells of pcl::VoxelGrid and
 *   of the scan's voxel filter, shifted by whole cells.  A point is OUTSIDE when any fabsf(c_a) >= FLIMO_VOXEL_HALF (2^20): it
 *   belongs to no voxel, is never selected and never removed, and is counted in stats.outside.  Otherwise
 *   key = ((cz + 2^20) << 42) | ((cy + 2^20) << 21) | (cx + 2^20).
 * Voxels: the occupied keys of the WHOLE map whatever the range (as flimo_map_clusters treats components), listed in ascending
 *   key, which is ascending (cz, cy, cx): PCL's output order.  Voxel v has the members m_0 < m_1 < ... < m_{c-1} (insertion
 *   indices).  ijk[v] = (cx, cy, cz), count[v] = c, first[v] = m_0.
 * SHAPE of a float64 sum over values u_0 .. u_{c-1} taken in member order: run j holds the slots 64 j .. 64 j + 63
 *   (FLIMO_VOXEL_RUN), an absent slot holds +0.0; a run's sum is the pairwise tree ((u0 + u1) + (u2 + u3)) + ... over its 64 slots
 *   (flimo_map_outliers' tree; equivalently the butterfly t[s] += t[s ^ o] for o = 1, 2, 4, 8, 16, 32); then
 *   S = ((+0.0 + R_0) + R_1) + ... over the runs in ascending order.  The leading +0.0 fixes the sign of a zero sum.
 * centroid[v][a] = S_a / (double)c, S_a the SHAPE over (double)p[m_r][a].
 * cov[v] = (xx, xy, xz, yy, yz, zz): each entry the SHAPE over d_a * d_b with d = (double)p - centroid (three float64
 *   subtractions, one product), divided by (double)c -- the / n convention of flimo_map_normals; two passes, never E[xx] - E[x]^2.
 * rep[v]: with keep == FLIMO_VOXEL_KEEP_FIRST m_0; with FLIMO_VOXEL_KEEP_NEAREST the member with the smallest
 *   q = d.x*d.x + (d.y*d.y + d.z*d.z), float64 and uncontracted, ties to the smallest insertion index.
 * Selection (the thinning rule; mask[i] = 1: stored point first + i goes).  KEEP_FIRST with max_pts = m >= 1: a point goes iff at
 *   least m members of its voxel have a smaller insertion index -- a voxel of at most m points is untouched, the oldest m stay;
 *   over a range of newly added points this is "drop what arrives where the voxel is already full", the octree's batch-drop rule
 *   made exact and independent of batch boundaries.  KEEP_NEAREST (max_pts must be 1): a point goes iff it is not rep of its
 *   voxel.  Both rules are idempotent: a second thinning with the same cfg removes nothing.
 * voxel[i]: the position of the point's voxel in the listing, -1 for an outside point.
 * stats: n (the range; flimo_map_voxels: the whole map), voxels, largest, outside (whole map), sel_points (ones of the mask over
 *   the range).  With n == 0 the whole-map fields are still formed where stats is given.
 * Nothing depends on the chunking, the map index's cell size, the number of insert batches, the lane plan (flimo_set_voxel_plan)
 * or what else the context did before.  No floating-point atomics.
 * Cost: one 64-bit radix sort of the stored points and two passes over them; device scratch is 32 B a stored point plus the
 * sort's own, at most 124 B a voxel and 84 B a run of a voxel above 1024 points. */
#define FLIMO_VOXEL_KEEP_FIRST 0
#define FLIMO_VOXEL_KEEP_NEAREST 1
#define FLIMO_VOXEL_RUN 64              /* part of the contract: the sum's shape */
#define FLIMO_VOXEL_HALF 1048576        /* 2^20 cells either side of the origin on every axis */
typedef struct flimo_voxel_cfg {
  float leaf;      /* edge of a voxel [m]: finite, > 0, 1.0f / leaf finite */
  int keep;        /* FLIMO_VOXEL_KEEP_FIRST / FLIMO_VOXEL_KEEP_NEAREST */
  int max_pts;     /* >= 1: the members a voxel keeps; 1 with KEEP_NEAREST */
} flimo_voxel_cfg;
typedef struct flimo_voxel_stats { uint64_t n, voxels, largest, outside, sel_points; } flimo_voxel_stats;
/* The voxels of the whole map.  Every output may be NULL.  *nv (the number of voxels, <= flimo_map_size) is written whenever the
 * call gets that far: a non-NULL per-voxel array with cap < nv returns FLIMO_ERR_TOO_LARGE, *nv set, the arrays untouched; a
 * caller passes cap = flimo_map_size and makes one call.  Changes nothing: not the map, not the scan, not the bits of a later
 * pass.  An empty map: FLIMO_OK, *nv = 0, stats 0. */
int flimo_map_voxels(flimo_ctx* ctx, const flimo_voxel_cfg* cfg, size_t cap, size_t* nv, int32_t* ijk /* [nv][3] */, int32_t* count /* [nv] */,
                     int32_t* first /* [nv] */, int32_t* rep /* [nv] */, double* centroid /* [nv][3] */, double* cov /* [nv][6] */,
                     flimo_voxel_stats* stats);
/* voxel [n] and mask [n] of the stored points first .. first + n - 1 (either may be NULL), the voxels being those of the whole map.
 * Changes nothing. */
int flimo_map_voxel_mask(flimo_ctx* ctx, size_t first, size_t n, const flimo_voxel_cfg* cfg, int32_t* voxel /* [n] */,
                         unsigned char* mask /* [n] */, flimo_voxel_stats* stats);
/* Forgets the points of the range whose mask is 1 and keeps the rest in insertion order, in the one ordered compaction pass
 * flimo_map_remove_plane uses.  Afterwards everything is as flimo_map_crop_box documents: the map is clear() + initialize(kept),
 * insertion indices are renumbered, flimo_map_last_time is untouched.  *removed (may be NULL) receives how many points went
 * (== stats->sel_points).  Removing nothing changes nothing.
 * All three calls: FLIMO_ERR_INVALID -- outputs and map untouched -- for a NULL ctx or cfg, leaf NaN, <= 0 or infinite or with
 * 1.0f / leaf not finite, keep outside 0..1, max_pts < 1, KEEP_NEAREST with max_pts != 1, first + n beyond flimo_map_size;
 * FLIMO_ERR_TOO_LARGE for a map of 2^31 points or more.  Same calling rules as flimo_map_clusters: no pass of this context in flight. */
int flimo_map_thin(flimo_ctx* ctx, size_t first, size_t n, const flimo_voxel_cfg* cfg, size_t* removed, flimo_voxel_stats* stats);
/* The lattice for one point on the host, through the same function the key kernel calls: 0 inside (ijk = (cx, cy, cz) and key
 * written), 1 outside (ijk = 0, key all ones), FLIMO_ERR_INVALID for a NULL p or a leaf flimo_map_voxels rejects.  ijk and key may
 * be NULL.  Needs no context and no device. */
int flimo_voxel_key_host(const float p[3], float leaf, int32_t ijk[3], uint64_t* key);

/* ---- smooth-surface regions of the stored points: what pcl::RegionGrowing finds -- neighbours whose normals agree grow one
 * region --, stated so that the seed order cannot show.  Walls, floor and ceiling as separate segments where flimo_map_clusters
 * reports one component of everything that touches; the objects left over when the large smooth regions are forgotten
 * (flimo_map_remove_regions, then flimo_map_clusters); one plane per region as a landmark or for map compression ----
 * Normals and neighbour lists never leave the GPU.
 *
 * Definition (tests/regions_common.py restates it in numpy).  The vertices are the N stored points in insertion order: the order
 * flimo_map_points returns and flimo_knn_k indexes.
 *  1. normals: (n_i, curv_i) is the float32 row normal[i] = nx ny nz curvature of flimo_map_normals_range(first = 0, n = N, normal_k,
 *     normal_max_dist, normal_min_pts, viewpoint = NULL), bit for bit.  A point HAS A NORMAL iff all four floats are finite.
 *  2. smooth: point i is SMOOTH iff it has a normal and curv_i <= max_curv (a float32 compare; max_curv may be INFINITY).
 *  3. edge: {i, j}, i != j, both smooth, is an edge iff sqdist3(p_i, p_j) < tol * tol -- exactly flimo_map_clusters' predicate -- and
 *     fabsf(n_i.x*n_j.x + (n_i.y*n_j.y + n_i.z*n_j.z)) >= min_cos: float32, uncontracted, in this association, so the predicate is
 *     symmetric bit for bit.  min_cos is a cosine, not an angle: no cosf enters the contract.
 *  4. region: a connected component of that graph over the smooth points of the WHOLE map, whatever the range.  Its label is the
 *     smallest insertion index among its smooth points.
 *  5. border (border != 0): a point b that has a normal but is not smooth joins the region of the smooth point j that passes both
 *     tests of 3. against b; among such j the one with the smallest key (bits of the float32 sqdist3(p_b, p_j), insertion index j):
 *     flimo_knn_k's order.  Such a point never carries a region further, counts towards the region's size, and leaves the region's
 *     label as 4. defines it, even where b's own index is smaller.
 *  6. unassigned: a point with no region has label -1 and size 0; it is never selected and never removed.
 *  7. selection and mask as flimo_map_clusters' (min_size, max_size; 0: no upper bound).  stats: n = points of the range; smooth,
 *     regions, largest, sel_regions, unassigned over the WHOLE map; sel_points = ones of the mask (range only).
 *  8. listing (flimo_map_region_list): the selected regions in ascending label; region r has the members m_0 < m_1 < ... in
 *     insertion order, border members included: label[r], count[r], first[r] = m_0, centroid[r][3] and cov[r][6] float64 exactly as
 *     flimo_map_voxels defines them for a voxel -- the same SHAPE of every sum (runs of FLIMO_VOXEL_RUN, the pairwise tree, the runs
 *     chained from +0.0), two passes, divided by count.  No floating-point atomics.
 *  9. tol == 0: no edges and no border attachment; every smooth point is its own region.  min_cos == 0 with max_curv == INFINITY:
 *     the regions are the Euclidean clusters of the points that have a normal.
 * Every integer output has one correct value given the normals, and no bit of the listing depends on the lane plan, the chunks, the
 * cell size, the order in which edges are met or earlier calls.
 * Cost: normals and regions are formed for the whole map whatever the range, nothing is kept between calls; device scratch is 28 B a
 * stored point, 84 B a point of a normals chunk, 1 B a point of the range and 4 B each for label and size where they are asked for;
 * the listing adds one 64-bit radix sort of the stored points. */
typedef struct flimo_region_cfg {
  float tol;             /* two points closer than this (strict, float32) can be joined; finite, >= 0 */
  int   normal_k;        /* neighbourhood of the normals: 1 .. FLIMO_KNN_MAX_K */
  float normal_max_dist; /* ... its distance gate; >= 0 or INFINITY */
  int   normal_min_pts;  /* ... and the neighbours a normal needs (at least 3 are always needed); >= 0 */
  float min_cos;         /* normals agree iff |n_i . n_j| >= min_cos; in 0 .. 1 */
  float max_curv;        /* smooth iff curvature <= max_curv; >= 0 or INFINITY */
  int   border;          /* != 0: points with a normal that are not smooth attach to a neighbouring region */
  int   min_size;        /* selected: min_size <= size ...; >= 0 */
  int   max_size;        /* ... <= max_size; 0: no upper bound; otherwise >= min_size */
} flimo_region_cfg;
typedef struct flimo_region_stats {
  uint64_t n;            /* points of the range */
  uint64_t smooth;       /* smooth points of the whole map */
  uint64_t regions;      /* regions of the whole map */
  uint64_t largest;      /* points of the largest region */
  uint64_t sel_regions;  /* selected regions of the whole map */
  uint64_t unassigned;   /* points of the whole map with no region */
  uint64_t sel_points;   /* ones of the mask (range only) */
} flimo_region_stats;
/* label / size / mask [n] and *stats over the stored points first .. first + n - 1; every output may be NULL.  Changes nothing: not
 * the map, not the scan, not the bits of a later pass.  n = 0 (also on an empty map, first = 0): FLIMO_OK, stats.n and
 * stats.sel_points 0, the whole-map fields still filled. */
int flimo_map_regions(flimo_ctx* ctx, size_t first, size_t n, const flimo_region_cfg* cfg, int32_t* label, int32_t* size,
                      unsigned char* mask, flimo_region_stats* stats);
/* The selected regions of the whole map (stats.n = flimo_map_size).  Every output may be NULL.  *nr (the number of selected regions)
 * is written whenever the call gets that far: a non-NULL per-region array with cap < nr returns FLIMO_ERR_TOO_LARGE, *nr set, the
 * arrays untouched; a caller passes cap = flimo_map_size and makes one call, or asks for *nr first.  Changes nothing.  An empty
 * map: FLIMO_OK, *nr = 0, stats 0. */
int flimo_map_region_list(flimo_ctx* ctx, const flimo_region_cfg* cfg, size_t cap, size_t* nr, int32_t* label /* [nr] */,
                          int32_t* count /* [nr] */, int32_t* first /* [nr] */, double* centroid /* [nr][3] */, double* cov /* [nr][6] */,
                          flimo_region_stats* stats);
/* Forgets the points OF THE RANGE whose mask is 1 and keeps the rest in insertion order; afterwards everything is exactly as
 * flimo_map_remove_clusters documents it.  *removed (may be NULL) receives how many points went (= stats.sel_points), *stats (may
 * be NULL) the predicate's, taken before the removal.  Removing nothing changes nothing.
 * All three calls: FLIMO_ERR_INVALID -- outputs and map untouched -- for a NULL ctx or cfg, first + n beyond flimo_map_size, tol NaN,
 * negative or infinite, min_cos NaN or outside 0 .. 1, max_curv NaN or negative, normal_max_dist NaN or negative, normal_min_pts < 0,
 * min_size < 0 or max_size < 0, 0 < max_size < min_size; FLIMO_ERR_UNSUPPORTED for normal_k outside 1 .. FLIMO_KNN_MAX_K;
 * FLIMO_ERR_TOO_LARGE for a map of 2^31 points or more.  Same calling rules as flimo_map_clusters: no pass of this context in flight. */
int flimo_map_remove_regions(flimo_ctx* ctx, size_t first, size_t n, const flimo_region_cfg* cfg, size_t* removed,
                             flimo_region_stats* stats);
/* The predicates for one pair on the host, through the same functions the link kernel calls (normals as rows nx ny nz curvature):
 * *smooth_i / *smooth_j = 2. for either point; *joined = 1 iff both points have a normal and both tests of 3. pass -- so {i, j} is
 * an edge iff all three are 1, and a border point b attaches to a smooth j only if joined.  Each output may be NULL.
 * FLIMO_ERR_INVALID for a NULL input or a cfg whose tol, min_cos or max_curv flimo_map_regions rejects (the other fields are not
 * read).  Needs no context and no device. */
int flimo_region_joined_host(const float pi[3], const float ni[4], const float pj[3], const float nj[4], const flimo_region_cfg* cfg,
                             int* smooth_i, int* smooth_j, int* joined);

/* ---- scan: pc2match of the reference (Modules/Localizer.hpp:36) ---- */
int flimo_scan_set(flimo_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes);
size_t flimo_scan_size(const flimo_ctx* ctx);
/* copy the resident scan back (packed xyz) */
int flimo_scan_get(flimo_ctx* ctx, float* xyz_out, size_t cap, size_t* n);

/* ---- voxel-grid filter on the resident scan: replaces pcl::VoxelGrid in Localizer::updatePointCloud
 *      (Modules/Localizer.cpp:313-321): centroid per occupied voxel, ascending voxel index.  Non-finite points are skipped; a scan
 *      with no finite point becomes empty.  The lattice is formed in 64-bit, as PCL forms it: floor(min / leaf) and floor(max / leaf)
 *      per axis, their difference + 1 and the product of the three counts as int64.  A product above INT_MAX -- one axis alone may
 *      exceed it -- leaves the scan as it is, non-finite points included (PCL warns "leaf size is too small" and returns its input).
 *      So does a floor that does not fit an int, |x / leaf| >= 2^31: PCL casts it to int, which is undefined there. ---- */
int flimo_scan_voxel_filter(flimo_ctx* ctx, float leaf_size, size_t* n_out);

/* ---- deskew: replaces the OpenMP loop of Localizer::deskewPointCloud
 *      (Modules/Localizer.cpp:820-843) incl. State::update (Objects/State.cpp:76-119) and
 *      binary_search_tailored (Utils/Algorithms.hpp:25-38).  Input: time-sorted LiDAR-frame points
 *      (xyz, stride) with per-point absolute times t[i] (= extract_point_time + offset, double);
 *      frames sorted by time; lidar2baselink_T row-major 4x4; last_x26 = _iKFoM.get_x().
 *      The result (body frame at scan end) becomes the resident scan (pc2match). ---- */
int flimo_deskew(flimo_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes, const double* t,
                 const flimo_frame* frames, size_t n_frames, const float lidar2baselink_T[16],
                 const double last_x26[26]);
/* the same in two steps, so that the raw scan can be made resident in HBM ahead of time */
int flimo_raw_scan_set(flimo_ctx* ctx, const float* xyz, size_t n, size_t stride_bytes, const double* t);
int flimo_deskew_resident(flimo_ctx* ctx, const flimo_frame* frames, size_t n_frames,
                          const float lidar2baselink_T[16], const double last_x26[26]);

/* ---- input filters + stamps of a raw sweep on the GPU: replaces removeNaNFromPointCloud, the negative CropBox and the rate /
 *      min-distance filters of Localizer::updatePointCloud (Modules/Localizer.cpp:262-302) and the per-point stamp of
 *      deskewPointCloud (:741-805) for sweeps that may reach the GPU in arrival order.  points32: n records in the reference's
 *      32-byte PointType layout (Common.hpp:100-113), host memory.  The kept points (order preserved) become the resident raw
 *      scan; *n_kept their number; *last_stamp = stamp (without the sweep offset) of the point the reference's time sort puts
 *      last; *nan_stamp = 1 when a kept stamp is NaN (the caller then takes the host path).  The FoV filter (:873-876) runs here
 *      too (fov_active): atan2 of two floats as glibc's fdlibm routine evaluates it, checked once per context against THIS host's
 *      libm on a set of argument pairs (a host whose atan2f rounds differently declines the filter: the call then reports
 *      FLIMO_ERR_UNSUPPORTED and the caller filters on the host).  Follow with flimo_deskew_resident_offset. ---- */
typedef struct flimo_filter_cfg {
  int crop_active;  float crop_min[3], crop_max[3];
  int dist_active;  float min_dist;
  int rate_active;  int rate_value;
  int time_kind;    /* 0 OUSTER (uint32 t, ns), 1 VELODYNE (float time, s), 2 HESAI (double timestamp, s), 3 LIVOX (double, ns) */
  int end_of_sweep;
  double sweep_ref_time;
  int fov_active;   float fov_angle;   /* FoV filter (Localizer.cpp:873-876): fabs(atan2(y, x)) < fov_angle, atan2 as the host's libm rounds it */
} flimo_filter_cfg;
int flimo_raw_scan_filter_set(flimo_ctx* ctx, const void* points32, size_t n, const flimo_filter_cfg* cfg, size_t* n_kept,
                              double* last_stamp, int* nan_stamp);
/* Optional: the context's pinned upload buffer (>= bytes).  A caller that copies the sweep's records into it -- from several threads
 * if it likes -- and passes THAT pointer as points32 to the next flimo_raw_scan_filter_set / _order_set saves the call's own
 * single-threaded staging copy (pcl clouds live in pageable memory).  Valid until the next call on the context that stages data. */
int flimo_upload_stage(flimo_ctx* ctx, size_t bytes, void** host_ptr);
/* The same, and with time_order != 0 the kept points are put into the order of the reference's time sort (std::partial_sort_copy by
 * stamp, Localizer.cpp:789-790) on the device: the order MAX_NUM_PC2MATCH / MAX_NUM_MATCHES ("the first N of pc2match") and the
 * voxel grid's float sums are defined in.  That order is unique -- a stable radix sort gives it -- when no two kept stamps are
 * equal; with equal stamps it is the library's heap moves', *tied = 1 is returned, nothing is made resident, and the caller takes
 * the host routine.  flimo_raw_scan_order: time rank -> position among the kept points (for the clouds handed back to callers).
 * time_order bit 1 (value 2): the sweep is NOT put into the spatial order the per-pass kernels like -- for a caller that runs
 * flimo_scan_voxel_filter right after the deskew, which re-orders the scan anyway.
 * time_order bit 2 (value 4): points32 holds 16-byte records {float x, y, z; 32-bit time word (PointType offset 24: OUSTER's uint32 t,
 * VELODYNE's float time)} instead of PointType records: time_kind 0 or 1 only.  A caller that stages the upload itself
 * (flimo_upload_stage) packs the sweep while it copies it and halves the bytes over PCIe.
 * time_order bit 3 (value 8): equal stamps keep their ARRIVAL order (the radix sort is stable) and the sweep is made resident all
 * the same; *tied = 1 still says that there were some.  Among equal stamps the reference's order is whatever its heap sort leaves
 * -- observable only as ulp-level voxel centroids and as which of several equally stamped points a cap cuts off. */
int flimo_raw_scan_filter_order_set(flimo_ctx* ctx, const void* points32, size_t n, const flimo_filter_cfg* cfg, int time_order,
                                    size_t* n_kept, double* last_stamp, int* nan_stamp, int* tied);
int flimo_raw_scan_order(flimo_ctx* ctx, uint32_t* order_out, size_t cap, size_t* n);
/* The resident raw sweep of `src` (what flimo_raw_scan_filter_set / _order_set left there) becomes `dst`'s: the two contexts exchange
 * the buffers of the Morton-ordered points and stamps (no copy) and dst's stream is ordered behind src's queued work.  Both contexts
 * on one GPU.  The input stage of a sweep -- upload, filters, stamps, time order (Localizer.cpp:262-302,741-805) -- does not read
 * the map: a caller runs it on a context of its own while dst's stream still carries the previous sweep's Mapper::add, then hands
 * the sweep over.  src keeps the time order (flimo_raw_scan_order) and no sweep. */
int flimo_scan_adopt(flimo_ctx* dst, flimo_ctx* src);
/* flimo_deskew_resident with the sweep's time offset added to every resident stamp (Localizer.cpp:795-800) */
int flimo_deskew_resident_offset(flimo_ctx* ctx, const flimo_frame* frames, size_t n_frames, const float lidar2baselink_T[16],
                                 const double last_x26[26], double t_offset);

/* ---- one measurement pass: replaces IKFoM::h_share_model (IKFoM/use-ikfom.cpp:10-31) =
 *      Mapper::match (Modules/Mapper.cpp:59-86) + Localizer::calculate_H
 *      (Modules/Localizer.cpp:537-577) + the h_x^T h_x / h_x^T h products of
 *      esekf::update_iterated_dyn_share_modified (esekfom.hpp:1723,1727).
 *      HTH row-major 12x12, HTh 12, *M = number of matches used (after both caps). ---- */
int flimo_match_reduce(flimo_ctx* ctx, const double x26[26], const flimo_match_cfg* cfg, double HTH[144],
                       double HTh[12], int* M);
/* The same pass, with host work of the caller to do WHILE the GPU runs it: `while_in_flight(arg)` is called at most once, after
 * the pass's launches are queued and before the call waits for their result.  In esekf::update_iterated_dyn_share_modified the
 * part of an iteration that does not depend on the measurement (x boxminus x_propagated, the re-projection of P through the
 * manifold Jacobians, esekfom.hpp:1652-1697) is such work.  On paths that do not wait (errors, an empty map) the function is not
 * called: the caller checks and runs it itself. */
int flimo_match_reduce_overlap(flimo_ctx* ctx, const double x26[26], const flimo_match_cfg* cfg, double HTH[144], double HTh[12], int* M,
                               void (*while_in_flight)(void*), void* arg);
/* ---- the iterated update of the resident scan, enqueued at once: replaces the loop of esekf::update_iterated_dyn_share_modified
 *      (IKFoM_toolkit/esekfom/esekfom.hpp:1620-1823) up to the iteration whose covariance update is due.  Every outer iteration =
 *      the pass above (h_share_model) + the 23-dof algebra of :1652-1760, run INSIDE the pass's reducing launch: one extra workgroup
 *      does the half that does not depend on the measurement beside the pass, the workgroup that completes the launch goes on from
 *      the sums to the gain, the step, boxplus and the convergence test and leaves the next pass's pose in device memory; passes
 *      queued behind the end of the chain leave at once.  No host round trip and no launch between the passes.
 *      The loop always comes back to the caller (status FLIMO_CHAIN_HANDED_BACK) at iteration it_next with counter t, state x26_out:
 *        reason FLIMO_CHAIN_FINAL       that iteration ends the loop (:1764: converged twice, or the last one): its pass has run,
 *                                       meas_* hold its sums -- the caller runs :1652-1820 for it without another pass;
 *        reason FLIMO_CHAIN_DEGENERATE  H^T H needs the eigen-decomposition of :1736-1744 (or the solve met a zero pivot): meas_* valid;
 *        reason FLIMO_CHAIN_FEW         M < 23 (:1701-1709 needs the dense rows): the caller runs the iteration through
 *                                       flimo_match_reduce / flimo_match_fetch_H;
 *        reason FLIMO_CHAIN_TIES        exact float32 distance ties to settle the reference's way: likewise;
 *      or not at all: FLIMO_CHAIN_DECLINED, nothing was run (records / caps / debug / timing level 2 / NUM_MATCH_POINTS != 5 / gates
 *      wider than 3 rings / more than FLIMO_CHAIN_MAX_PASSES iterations / FLIMO_HOST_UPDATE=1): the caller runs its loop.
 *      The gain is the matrix-inversion-lemma form of :1722-1729 (one 12x12 solve), as in csrc/host/flimo_ikfom.cpp. ---- */
#define FLIMO_CHAIN_MAX_PASSES 12
#define FLIMO_CHAIN_DECLINED 0
#define FLIMO_CHAIN_HANDED_BACK 2
#define FLIMO_CHAIN_FEW 1
#define FLIMO_CHAIN_TIES 2
#define FLIMO_CHAIN_DEGENERATE 3
#define FLIMO_CHAIN_FINAL 5
typedef struct flimo_chain_pass {
  int M, stragglers, ties;       /* matches of the pass, queries that needed more than their 3x3x3 block, queries on an exact tie */
  double HTH[144], HTh[12];      /* want_log only: the pass's sums, */
  double dx[23], x_after[26];    /* the un-projected step dx_ (:1733) and the state after boxplus (:1747) */
} flimo_chain_pass;
typedef struct flimo_chain_io {
  /* in */
  double x26[26];                /* x_ at entry (= x_propagated) */
  double P[529];                 /* P_ at entry, 23 x 23 row-major */
  double limits[23];             /* esekf::limit (:1757-1763) */
  double R, D;                   /* measurement noise, degeneracy threshold (Localizer.cpp:333: 0.001, 5.0) */
  int max_iter;                  /* maximum_iter (MAX_NUM_ITERS): iterations -1 .. max_iter - 1 */
  int want_log;                  /* also fill log[].HTH / HTh / dx / x_after */
  /* out */
  int status, reason;
  int passes;                    /* outer iterations completed on the device */
  int it_next, t;                /* loop variables to resume with (it_next = -1 + passes) */
  double x26_out[26];            /* x_ at that iteration */
  int meas_valid, meas_M;        /* that iteration's pass: usable sums (reasons FINAL, DEGENERATE) */
  double meas_HTH[144], meas_HTh[12];
  flimo_chain_pass log[FLIMO_CHAIN_MAX_PASSES];   /* entries 0 .. passes - 1 (+ the handed-back iteration's M / stragglers / ties) */
} flimo_chain_io;
int flimo_update_chain(flimo_ctx* ctx, const flimo_match_cfg* cfg, flimo_chain_io* io);
/* Which way a caller's update runs: 0 (default) and 1 = flimo_update_chain declines and the caller's host loop runs the update pass
 * by pass; 2 = the chain runs.  The choice is the caller's, never a measurement's: the two layouts agree to 1e-15 per pass but not
 * bit for bit, so a choice made from timing (round 4 chose by the launch round trip measured at context creation) made the
 * filter's bits depend on the host.  A host whose launch -> result round trip (reported below) is beyond ~16 us gains from mode 2.
 * FLIMO_HOST_UPDATE=1 / 0 preset 1 / 2.
 * flimo_update_mode: *chained = 1 when flimo_update_chain will run, *launch_rtt_us = the measured round trip. */
/* Host loop, pipelined.  With the switch on, a flimo_match_reduce that ran a one-launch pass queues the NEXT pass of the same update
 * right behind it: a kernel whose workgroups are placed on the GPU when the current pass ends and wait there for their pose.  The next
 * flimo_match_reduce (same scan, same settings) stores the pose into device memory instead of launching: the doorbell -> dispatch ->
 * kernel start of a launch leave the iteration's critical path (4-5 us per pass).  What it asks of the caller: say when the update is
 * over (flimo_pass_pipeline_end, right after the loop of esekfom.hpp:1652-1820) -- a pass nobody asks for is also told to leave by the
 * next call on the context and gives up by itself after 50 ms, but until then a device-wide synchronisation anywhere in the process
 * waits for it.  Off by default for that reason; fast_limo::Localizer switches it on and makes the call.  FLIMO_PIPELINE=0/1 presets it.
 */
int flimo_set_pass_pipeline(flimo_ctx* ctx, int on);
int flimo_pass_pipeline_end(flimo_ctx* ctx);
/* Optional hint of the same loop: the NEXT flimo_match_reduce is the last pass its update can run (the loop's i == maximum_iter - 1,
 * esekfom.hpp:1634) -- nothing is queued behind it.  Without the hint one launch per update is queued for nothing and told to leave. */
int flimo_pass_pipeline_last(flimo_ctx* ctx);
int flimo_set_update_mode(flimo_ctx* ctx, int mode);
int flimo_update_mode(const flimo_ctx* ctx, int* chained, double* launch_rtt_us);
/* per-point records of the last flimo_match_reduce (first min(N, MAX_NUM_PC2MATCH) points) */
/* also write the per-point debug part of flimo_match_rec (plane, neighbours, candidate counts) */
int flimo_set_debug_records(flimo_ctx* ctx, int on);
int flimo_match_fetch(flimo_ctx* ctx, flimo_match_rec* out, size_t cap, size_t* n);
/* dense H (M x 12 row-major, compacted in scan order, capped) and h of the last pass: needed by the
 * M < 23 branch of the update (esekfom.hpp:1701-1709) */
int flimo_match_fetch_H(flimo_ctx* ctx, double* H, double* h, size_t cap_rows, size_t* M);

/* ---- path exit: pcl::transformPointCloud(pc2match, state.get_RT()) + Mapper::add
 *      (Modules/Localizer.cpp:361-377).  world_xyz_out may be NULL. ---- */
int flimo_scan_to_world(flimo_ctx* ctx, const double x26[26], float* world_xyz_out, size_t cap);
/* ---- how well the resident scan fits the map at each of np pose hypotheses: what pcl::Registration::getFitnessScore computes
 *      for one pose (nearest stored point of every transformed scan point, gated), for a batch of poses and without the world
 *      points or the neighbours ever leaving the GPU ----
 * x26 [np][26]: the poses; only pos (x26[j][0..2]) and rot (x26[j][3..6]) of a pose are read.  n = flimo_scan_size(ctx).
 * w(j, i), the world point of resident scan point i under pose j, is the reference's s.get_RT() * bl4_point (Modules/Mapper.cpp:72)
 * in float32: exactly point i of flimo_scan_to_world(ctx, x26[j], ..) -- the matrix of that call, the same
 * c0*x + (c1*y + (c2*z + c3)), uncontracted --, i in the order of flimo_scan_get / flimo_scan_to_world.
 * The neighbour of w(j, i) is exactly flimo_knn_k(w, k = 1, max_dist): same predicate (strict sqd < max_dist * max_dist, the
 * square one float32 product; INFINITY: no gate), same unique order (float32 squared-distance bits, insertion index).
 * Outputs, host memory:
 *  - nn_sqd [np][n] (may be NULL): that squared distance, -1.0f when the query is empty (gated out, a NaN coordinate in w, an empty
 *    map); nn_idx [np][n] (may be NULL): the insertion index, or -1.  Both bit-equal to flimo_knn_k.
 *  - inliers [np]: the number of non-empty queries of pose j, exact.
 *  - sum_sqd [np]: the float64 sum of their float32 sqd, taken in ONE fixed shape over the scan's slots (no floating-point
 *    atomics): its bits depend on the scan, the map's points and pose j alone -- not on np, the other poses, how the call is cut
 *    into chunks, the map's cell size or which path of the search finished a query -- and do not differ between two calls.
 * The mean squared distance (sum_sqd / inliers: getFitnessScore's number) and any robust cost are the caller's arithmetic.
 * FLIMO_OK with all inliers / sum_sqd 0 and all nn_sqd / nn_idx -1 for an empty map, an empty scan and max_dist == 0; np == 0
 * returns FLIMO_OK and touches nothing.  FLIMO_ERR_INVALID: NULL ctx / x26 (np > 0) / inliers / sum_sqd, max_dist NaN or negative, a
 * non-finite value among x26[j][0..6] of any pose.  FLIMO_ERR_TOO_LARGE: np >= 2^31; there is no limit on np * n.  The outputs are
 * untouched on an error.
 * A scan whose deskew still rides on the next launch is deskewed first (as flimo_scan_to_world does).  The call changes neither the
 * resident scan nor the map nor the bits of a later pass.  Calling rules and cost as flimo_knn_k (no pass in flight; a pose that
 * throws the scan kilometres from the map costs a look at the tile directory per point); device memory is taken per chunk of 2^22
 * (pose, point) pairs -- whole poses --, not per call. */
int flimo_scan_fitness(flimo_ctx* ctx, const double* x26 /* [np][26] */, size_t np, float max_dist, int32_t* inliers /* [np] */,
                       double* sum_sqd /* [np] */, float* nn_sqd /* [np][n], may be NULL */, int32_t* nn_idx /* [np][n], may be NULL */);
/* ---- one linearisation of a point-to-plane registration of the resident scan, for each of np pose hypotheses: the 6 x 6 normal
 *      equations per pose, without the world points, the neighbourhoods or the planes ever leaving the GPU.  The caller solves and
 *      iterates (fast_limo_amd.api.scan_align does); flimo_scan_fitness ranks the guesses, this refines the best ones. ----
 * x26 [np][26]: the poses; only pos and rot are read.  n = flimo_scan_size(ctx).  Every step is a quantity an existing call defines:
 *  - w(j, i): the float32 world point of resident scan point i under pose j, exactly as in flimo_scan_fitness (pose_from_x26's
 *    matrix, c0*x + (c1*y + (c2*z + c3)), uncontracted).
 *  - the plane of pair (j, i): exactly what flimo_map_normals(q = w(j, i), k, max_dist, min_pts, viewpoint = NULL) returns -- cnt, the
 *    float64 centroid c, the eigenvalues l0 <= l1 <= l2 and the float64 unit normal nrm in its NULL-viewpoint orientation, bit for
 *    bit; curvature = l0 / (l0 + l1 + l2), 0 for a zero trace, as that call forms it.
 *  - the pair is VALID iff cnt >= max(3, min_pts) and curvature <= (double)max_curv (a float64 compare; max_curv == INFINITY: no
 *    curvature gate).
 *  - the terms of a valid pair, all float64, nothing contracted, in exactly this association (p: the float32 scan point widened; R:
 *    the nine float32 rotation entries of the pose's matrix widened; w widened):
 *      d  = nrm.x*(w.x - c.x) + (nrm.y*(w.y - c.y) + nrm.z*(w.z - c.z))
 *      a  = R^T nrm:  a0 = R00*nrm.x + (R10*nrm.y + R20*nrm.z), a1 and a2 likewise with R's columns 1 and 2
 *      b  = p x a:    b0 = p.y*a2 - p.z*a1, b1 = p.z*a0 - p.x*a2, b2 = p.x*a1 - p.y*a0
 *      J  = (a0, a1, a2, b0, b1, b2)
 *    J is the derivative of d under the body-frame perturbation t <- t + R*drho, R <- R*Exp(dphi) with the plane held fixed; it is
 *    built from scan coordinates, not world coordinates, so the system stays well conditioned kilometres from the origin.
 * Outputs, host memory, per pose over its valid pairs:
 *  - H [np][21]: the upper-triangle sums of J_a*J_b, row-major 00, 01 .. 05, 11 .. 55;  g [np][6]: the sums of J_a*d;
 *    cost [np]: the sum of d*d;  valid [np]: the exact count.  The Gauss-Newton step solves H xi = -g, xi = (drho, dphi).
 *    Every sum is taken in ONE fixed shape over the scan's n slots, an invalid slot adding +0.0, without floating-point atomics
 *    (flimo_sums.h and DESIGN.md section 8 state the shape; it is a function of n alone): the bits of a pose's 28 numbers depend on the scan, the
 *    map's stored points, the pose and the four parameters -- not on np, the other poses, how the call is cut into chunks, the map's
 *    cell size or which path of the search finished a pair.
 *  - rows [np][n][7] (may be NULL): J0..J5, d per pair, NaN for an invalid pair.
 *  - pair_cnt [np][n] (may be NULL): the neighbour count of the pair, for invalid pairs as well.
 * FLIMO_OK with all sums and valid 0 (rows NaN, pair_cnt 0) for an empty map, an empty scan and max_dist == 0; np == 0 returns
 * FLIMO_OK and touches nothing; a NaN scan point gives an invalid pair.  FLIMO_ERR_INVALID: NULL ctx / x26 (np > 0) / valid / H / g /
 * cost, max_dist or max_curv NaN or negative, a non-finite value among x26[j][0..6] of any pose.  FLIMO_ERR_UNSUPPORTED: k outside
 * 3 .. FLIMO_KNN_MAX_K.  FLIMO_ERR_TOO_LARGE: np >= 2^31; there is no limit on np * n.  The outputs are untouched on an error.
 * A pending deskew is run first; the call changes neither the resident scan nor the map nor the bits of a later pass.  Calling rules
 * and cost as flimo_scan_fitness; device memory is taken per chunk of 2^20 (pose, point) pairs -- whole poses --, 141 B a pair. */
int flimo_scan_linearize(flimo_ctx* ctx, const double* x26 /* [np][26] */, size_t np, int k, float max_dist, int min_pts, float max_curv,
                         int32_t* valid /* [np] */, double* H /* [np][21] */, double* g /* [np][6] */, double* cost /* [np] */,
                         double* rows /* [np][n][7], may be NULL */, int32_t* pair_cnt /* [np][n], may be NULL */);
/* ---- NDT, the normal distributions transform (what pcl::NormalDistributionsTransform computes; the reference has no counterpart):
 *      the consumer of flimo_map_voxels' covariances.  A resident CELL MODEL is built from the map's voxels once; flimo_scan_ndt then
 *      gives, for each of np pose hypotheses, the score and the 6 x 6 Gauss-Newton normal equations of the resident scan against it.
 *      A pair costs a cell lookup instead of a neighbour search, and the basin grows with the leaf: a context holds FLIMO_NDT_SLOTS
 *      models, one per leaf of a coarse-to-fine schedule (fast_limo_amd.api.ndt_align runs one). ----
 * flimo_ndt_build(ctx, slot, cfg, &nc): the model of slot `slot` from the voxels of the WHOLE map at cfg->leaf.
 *  - key, count, centroid and cov of a voxel are exactly flimo_map_voxels' (leaf), bit for bit: its key, sort and moments launches run
 *    on the device and nothing is downloaded.
 *  - the eigen-solve of cov is the cyclic Jacobi of flimo_map_normals' plane (the same rotations; ascending eigenvalues
 *    l0 <= l1 <= l2, on a tie the lower column first); all three unit vectors v0 v1 v2 are kept with whatever sign the rotations leave.
 *  - a voxel is a CELL iff count >= min_pts and l2 > 0.0.  Its record: floor = eig_ratio * l2 (one float64 product),
 *    lk' = lk < floor ? floor : lk, wk = 1.0 / lk'; mean[3] (the centroid), v[3][3], w[3], padded to 128 bytes.  Cells are listed in
 *    ascending key, that is ascending (cz, cy, cx).
 *  - the model is a SNAPSHOT: inserts, crops, removals and flimo_map_clear do not touch it (a saved map's model survives a local-map
 *    crop); flimo_ndt_info's `stale` is 1 once the stored points have changed since the build.  A build on an empty map gives an
 *    empty model: FLIMO_OK, *nc = 0.  A build into a slot that holds a model replaces it.
 *  FLIMO_ERR_INVALID: NULL ctx / cfg, a leaf flimo_map_voxels rejects, min_pts < 3, eig_ratio NaN or outside (0, 1], slot outside
 *  0 .. FLIMO_NDT_SLOTS - 1; FLIMO_ERR_TOO_LARGE as flimo_map_voxels.  On an error *nc and the slot's old model are untouched.
 *  Calling rules of flimo_map_voxels (no pass in flight); the map, the scan and the bits of a later pass are unchanged.  nc may be NULL.
 * flimo_ndt_cells(ctx, slot, cap, &nc, ...): downloads the model, any subset of the arrays (NULL skips one): ijk [nc][3] = (cx, cy, cz),
 *  count [nc], mean [nc][3], evec [nc][9] = v0 v1 v2, wgt [nc][3], eval [nc][3] = l0 l1 l2 before the clamp.  The cap rule is
 *  flimo_map_voxels': cap < nc with an array asked for gives FLIMO_ERR_TOO_LARGE, *nc is set and the arrays are untouched.
 *  FLIMO_ERR_NOMAP: no model in the slot.
 * flimo_ndt_info(ctx, slot, &info): FLIMO_ERR_NOMAP for an empty slot.  flimo_ndt_clear(ctx, slot): frees a slot, slot = -1 all. */
#define FLIMO_NDT_SLOTS 4
typedef struct flimo_ndt_cfg {
  float leaf;
  int min_pts;       /* >= 3 */
  double eig_ratio;  /* in (0, 1]: no eigenvalue of a cell counts as smaller than eig_ratio * l2 (PCL: 0.01) */
} flimo_ndt_cfg;
typedef struct flimo_ndt_model_info {
  uint64_t cells;              /* nc */
  uint64_t map_size_at_build;  /* stored points the build saw */
  double eig_ratio;
  float leaf;
  int min_pts;
  int stale;                   /* 1: the stored points have changed since the build */
} flimo_ndt_model_info;
int flimo_ndt_build(flimo_ctx* ctx, int slot, const flimo_ndt_cfg* cfg, size_t* nc);
int flimo_ndt_cells(flimo_ctx* ctx, int slot, size_t cap, size_t* nc, int32_t* ijk /* [nc][3] */, int32_t* count /* [nc] */,
                    double* mean /* [nc][3] */, double* evec /* [nc][9] */, double* wgt /* [nc][3] */, double* eval /* [nc][3] */);
int flimo_ndt_info(flimo_ctx* ctx, int slot, flimo_ndt_model_info* info);
int flimo_ndt_clear(flimo_ctx* ctx, int slot);
/* ---- the NDT score and normal equations of the resident scan against the model of `slot`, for each of np pose hypotheses ----
 * x26 [np][26]: the poses; only pos and rot are read.  n = flimo_scan_size(ctx).  Every quantity is float64 and uncontracted unless
 * stated otherwise.
 *  - w(j, i): the float32 world point of resident scan point i under pose j, exactly as in flimo_scan_fitness.
 *  - its cell is voxel_key(w, 1.0f / leaf) -- flimo_voxel_key_host's function; an outside point or a NaN coordinate gives no cell.
 *    Neighbour slots: s = 0 is the own cell (cx, cy, cz); with hood == 7, s = 1..6 are -x, +x, -y, +y, -z, +z (PCL's DIRECT1 and
 *    DIRECT7).  A neighbour whose coordinate leaves the lattice is absent, and so is a key that is no CELL of the model.
 *  - the term of a present cell (p: the float32 scan point widened; R: the nine float32 rotation entries of the pose's matrix widened;
 *    k = 0, 1, 2):
 *      r   = (double)w - mean                               (three subtractions)
 *      d_k = v_k.x*r.x + (v_k.y*r.y + v_k.z*r.z)
 *      m   = w0*(d_0*d_0) + (w1*(d_1*d_1) + w2*(d_2*d_2))
 *      x   = c * m,  c = -0.5 * d2 formed once, on the host;   e = exp(x), the device's float64 exp
 *    The term is LIVE iff e > 0.0 (underflow and NaN alike are excluded: no 0 * inf ever enters a sum).  For a live term
 *      a_k = R^T v_k, b_k = p x a_k, J_k = (a_k, b_k) in the associations flimo_scan_linearize states for a, b and J
 *      s_k = (e * d2) * w_k
 *    and, for k ascending: H_ab += (s_k * J_k[a]) * J_k[b] for the 21 upper-triangle entries, g_a += (s_k * d_k) * J_k[a];
 *    score += e once per term.
 *  g is the gradient of F = -sum e under flimo_scan_linearize's body-frame perturbation, H its positive-semidefinite Gauss-Newton
 *  part sum e*d2*B^T Sigma'^-1 B: H xi = -g is the step fast_limo_amd.api.scan_align already solves.  The overall factor d1 of PCL's
 *  score is the caller's (fast_limo_amd.api.ndt_params gives PCL's (d1, d2) for an outlier ratio and a leaf).
 * Outputs, host memory, per pose:
 *  - H [np][21], g [np][6], score [np]; valid [np]: the pairs with at least one live term; cells [np]: the live terms.
 *    The 28 sums are taken in the one shape of flimo_scan_linearize's and flimo_map_outliers' sums, stated in
 *    fast_limo_amd/csrc/hip/flimo_sums.h (and DESIGN.md section 8), a slot being a scan point: inside a slot the neighbour slots
 *    s ascend, inside a term k ascends, every contribution ONE add onto the thread's accumulator, which starts at +0.0.
 *    No floating-point atomics: the bits depend on the scan, the
 *    model, the pose, hood and d2 alone -- not on np, the other poses, the chunking or the lookup method.
 *  - terms [np][n][7][2] (may be NULL): (m, e) per neighbour slot, NaN for an absent cell (with hood == 1 the slots 1..6 are absent);
 *    term_cell [np][n][7] (may be NULL): the cell's position in flimo_ndt_cells' listing, or -1.
 * FLIMO_ERR_NOMAP: no model in `slot`.  FLIMO_ERR_INVALID: NULL ctx / x26 (np > 0) / valid / cells / H / g / score, hood not 1 or
 * 7, d2 NaN, <= 0 or infinite, a non-finite value among x26[j][0..6], a slot outside 0 .. FLIMO_NDT_SLOTS - 1.  FLIMO_ERR_TOO_LARGE:
 * np >= 2^31.  The outputs are untouched on any error.  FLIMO_OK with all sums and counts 0 (terms NaN, term_cell -1) for an empty
 * model and an empty scan; np == 0 returns FLIMO_OK and touches nothing.  A pending deskew runs first; the scan, the map, the model
 * and the bits of a later pass are unchanged.  Device memory is taken per chunk of 2^20 (pose, point) pairs -- whole poses --, 12 B a
 * neighbour slot (84 B a pair at hood 7; 20 B a slot when terms are asked for). */
int flimo_scan_ndt(flimo_ctx* ctx, int slot, const double* x26 /* [np][26] */, size_t np, int hood /* 1 or 7 */, double d2,
                   int32_t* valid /* [np] */, int64_t* cells /* [np] */, double* H /* [np][21] */, double* g /* [np][6] */,
                   double* score /* [np] */, double* terms /* [np][n][7][2], may be NULL */, int32_t* term_cell /* [np][n][7], may be NULL */);
/* One term on the host: the function the kernels call (flimo_ndt.h), with libm's exp.  w3: the float32 world point, p3: the float32
 * scan point, R9: the rotation, row-major; mean3 / evec9 / wgt3: a cell as flimo_ndt_cells lists it.  out30 = m, e, then the 28
 * contributions (H's 21, g's 6, the score) summed over k from +0.0 -- all 0 when the term is not live.  Returns 1 for a live term,
 * 0 otherwise, FLIMO_ERR_INVALID for a NULL pointer.  Needs no device. */
int flimo_ndt_term_host(const float w3[3], const float p3[3], const float R9[9], const double mean3[3], const double evec9[9],
                        const double wgt3[3], double d2, double out30[30]);
/* ---- GICP, generalized ICP or plane-to-plane (what pcl::GeneralizedIterativeClosestPoint and fast_gicp linearise; the reference
 *      has no counterpart): the consumer of flimo_map_normals' covariances.  Every residual -- the scan point at the pose minus its
 *      nearest stored point -- is weighed by the shape of BOTH surfaces, M = (CB + R CA R^T)^-1.  The map's covariances are a
 *      resident MODEL built once (flimo_gicp_build); the scan's are the caller's, uploaded once per scan (flimo_scan_cov_set: the
 *      library does not index the scan; a second context whose map is the scan computes them, fast_limo_amd.api.gicp_covs);
 *      flimo_scan_gicp then gives, for each of np pose hypotheses, the 6 x 6 Gauss-Newton normal equations.  Every quantity below is
 *      float64 on float32 inputs widened, uncontracted, in exactly the written association; a covariance is its six numbers
 *      xx xy xz yy yz zz; a three-term sum is written x0 + (x1 + x2). ----
 * The regularised covariance C' of a neighbourhood covariance C (gicp_regularize, fast_limo_amd/csrc/hip/flimo_gicp.h):
 *  - the eigen-solve of C is the cyclic Jacobi of flimo_map_normals' plane and of the NDT cells (ascending l0 <= l1 <= l2, on a tie the
 *    lower column first; unit vectors v0 v1 v2 with whatever sign the rotations leave).
 *  - NO covariance: any of the six numbers non-finite, or not l2 > 0.0.  C' is then six NaN.
 *  - FLIMO_GICP_PLANE (PCL's rule; eps in (0, 1], PCL: 1e-3): l0' = eps, l1' = l2' = 1.0.
 *    FLIMO_GICP_CLAMP (the NDT model's rule; eps plays eig_ratio): floor = eps * l2 (one product), lk' = lk < floor ? floor : lk.
 *  - C'_ab = ((0.0 + (l0' * v0[a]) * v0[b]) + (l1' * v1[a]) * v1[b]) + (l2' * v2[a]) * v2[b] for the six ab.
 * flimo_gicp_build(ctx, cfg, &n_cov): ONE model per context, a row of six numbers per stored point in insertion order.
 *  - C of stored point i is exactly flimo_map_normals_range(0, map size, k, max_dist, min_pts)'s cov[i], bit for bit (six NaN below
 *    max(3, min_pts) neighbours): its launches run over the whole map in chunks of flimo_set_normals_chunk points, the covariances
 *    stay on the device, nothing of points x k entries exists and nothing is downloaded.  Row i is C' of that; *n_cov counts the rows
 *    that got one.
 *  - the model is a SNAPSHOT indexed by insertion index, and a removal renumbers the stored points: it is usable only for the map
 *    it was built from.  flimo_gicp_info's `stale` is 1, and flimo_scan_gicp refuses the model, once the stored points have changed
 *    (an insert, a crop or another removal, flimo_map_clear).  A build on an empty map gives an empty model: FLIMO_OK, *n_cov = 0.
 *    A build replaces the context's model -- only when everything has succeeded.
 *  FLIMO_ERR_UNSUPPORTED: k outside 3 .. FLIMO_KNN_MAX_K.  FLIMO_ERR_INVALID: NULL ctx / cfg, max_dist NaN or < 0 (INFINITY: no
 *  gate), min_pts < 0, an unknown rule, eps NaN or outside (0, 1].  FLIMO_ERR_TOO_LARGE: a map of 2^31 points or more.  On an error
 *  *n_cov and the old model are untouched.  Calling rules of flimo_map_normals (no pass in flight); the map, the scan and the bits of
 *  a later pass are unchanged.  n_cov may be NULL.
 * flimo_gicp_model(ctx, first, n, cov): downloads rows first .. first + n - 1, cov [n][6].  FLIMO_ERR_INVALID for a range beyond the
 *  model's points or a NULL cov with n > 0.  flimo_gicp_info(ctx, &info).  Both: FLIMO_ERR_NOMAP without a model.
 *  flimo_gicp_clear(ctx): frees the model. */
#define FLIMO_GICP_PLANE 0
#define FLIMO_GICP_CLAMP 1
typedef struct flimo_gicp_cfg {
  int k;            /* neighbours of a stored point's covariance, 3 .. FLIMO_KNN_MAX_K (PCL: 20) */
  float max_dist;   /* their gate [m]; INFINITY: none */
  int min_pts;      /* a point with fewer than max(3, min_pts) neighbours has no covariance */
  int rule;         /* FLIMO_GICP_PLANE or FLIMO_GICP_CLAMP */
  double eps;       /* in (0, 1] */
} flimo_gicp_cfg;
typedef struct flimo_gicp_model_info {
  uint64_t points;  /* stored points the build saw: the model's rows */
  uint64_t n_cov;   /* rows that hold a covariance */
  double eps;       /* the cfg of the build: eps, k, max_dist, min_pts, rule */
  int k;
  float max_dist;
  int min_pts;
  int rule;
  int stale;        /* 1: the stored points have changed since the build; flimo_scan_gicp refuses the model */
} flimo_gicp_model_info;
int flimo_gicp_build(flimo_ctx* ctx, const flimo_gicp_cfg* cfg, size_t* n_cov);
int flimo_gicp_model(flimo_ctx* ctx, size_t first, size_t n, double* cov /* [n][6] */);
int flimo_gicp_info(flimo_ctx* ctx, flimo_gicp_model_info* info);
int flimo_gicp_clear(flimo_ctx* ctx);
/* The covariances of the resident scan's points: cov6 [n][6], one REGULARISED covariance per point, in the body frame, in
 * flimo_scan_to_world's order; a row with a NaN means "this point has none".  n must be flimo_scan_size(ctx) (FLIMO_ERR_INVALID
 * otherwise); n == 0 or a NULL cov6 drops the covariances.  Every call that replaces the resident scan drops them too
 * (flimo_scan_set, flimo_scan_voxel_filter, the raw-scan and deskew entries); a deskew still pending does not: it is the same
 * points in the same order.  flimo_scan_cov_size: n, or 0 when there are none. */
int    flimo_scan_cov_set(flimo_ctx* ctx, const double* cov6 /* [n][6] */, size_t n);
size_t flimo_scan_cov_size(const flimo_ctx* ctx);
/* ---- the GICP normal equations of the resident scan against the stored points, for each of np pose hypotheses ----
 * x26 [np][26]: the poses; only pos and rot are read.  n = flimo_scan_size(ctx).  Per (pose j, scan point i):
 *  - w: the float32 world point and b: its nearest stored point are exactly flimo_scan_fitness(max_dist)'s -- nn_idx under the same
 *    gate and the same order (distance bits, insertion index); b's coordinates are the stored point's float32.
 *  - CB = the model's row of b, CA = the scan's row i; p: the float32 scan point, R: the nine float32 rotation entries of the pose's
 *    matrix, row-major.  The term (gicp_term, flimo_gicp.h):
 *      r      = (double)w - (double)b                                  (three subtractions)
 *      T_ij   = R_i0*CA_0j + (R_i1*CA_1j + R_i2*CA_2j)                 (T = R CA)
 *      S_ij   = CB_ij + (T_i0*R_j0 + (T_i1*R_j1 + T_i2*R_j2))          for the six i <= j (S = CB + R CA R^T)
 *      c00 = S11*S22 - S12*S12, c01 = S02*S12 - S01*S22, c02 = S01*S12 - S02*S11,
 *      c11 = S00*S22 - S02*S02, c12 = S01*S02 - S00*S12, c22 = S00*S11 - S01*S01   (the cofactors)
 *      det    = S00*c00 + (S01*c01 + S02*c02);   M_ij = c_ij / det     (six divisions; M symmetric)
 *    The pair is LIVE iff all twelve covariance numbers are finite and det > 0.0 and 1.0 / det is finite.  For a live pair
 *      y_i    = M_i0*r_0 + (M_i1*r_1 + M_i2*r_2);   m = r_0*y_0 + (r_1*y_1 + r_2*y_2)
 *      J_c    = column c of R for c = 0, 1, 2;  J_3 = p.y*J_2 - p.z*J_1,  J_4 = p.z*J_0 - p.x*J_2,  J_5 = p.x*J_1 - p.y*J_0
 *               (componentwise: the columns of [R | -R [p]x], the derivative of r under flimo_scan_linearize's body-frame
 *               perturbation t <- t + R drho, R <- R Exp(dphi), with M held fixed)
 *      U_c[i] = M_i0*J_c[0] + (M_i1*J_c[1] + M_i2*J_c[2])
 *      H_ab   = J_a[0]*U_b[0] + (J_a[1]*U_b[1] + J_a[2]*U_b[2])  for the 21 upper-triangle entries, row-major 00, 01 .. 55
 *      g_a    = J_a[0]*y_0 + (J_a[1]*y_1 + J_a[2]*y_2);   cost = m
 *    J is built from R and scan coordinates and r is a difference: a map kilometres from the origin costs no conditioning.  g is the
 *    gradient of (1/2) sum m at fixed M, H is positive semidefinite whenever S is positive definite: H xi = -g is the step
 *    fast_limo_amd.api.scan_align already solves (api.gicp_align iterates it).
 *  - the pair is VALID iff it has a neighbour inside the gate and its term is live.
 * Outputs, host memory, per pose: H [np][21], g [np][6], cost [np] (the sum of m); valid [np].  The 28 sums are taken in the one
 * shape of fast_limo_amd/csrc/hip/flimo_sums.h, a slot being a scan point: every contribution ONE add onto
 * the thread's accumulator, which starts at +0.0; an invalid slot adds +0.0.  No floating-point atomics: the bits depend on the
 * scan, its covariances, the stored points, the model, the pose and max_dist alone -- not on np, the other poses, the chunking, the
 * cell size or the search path.  pair_idx [np][n] (may be NULL): the neighbour's insertion index or -1, for an invalid pair with a
 * neighbour as well; pair_m [np][n] (may be NULL): m, NaN for an invalid pair.
 * FLIMO_ERR_NOMAP: no model, a stale model (the message says so), or no covariances of the resident scan.  FLIMO_ERR_INVALID: NULL
 * ctx / x26 (np > 0) / valid / H / g / cost, max_dist NaN or < 0, a non-finite value among x26[j][0..6].  FLIMO_ERR_TOO_LARGE:
 * np >= 2^31.  The outputs are untouched on any error.  FLIMO_OK with all sums 0, pair_idx -1 and pair_m NaN for an empty scan, an
 * empty map and max_dist == 0; np == 0 returns FLIMO_OK and touches nothing.  A pending deskew runs first; the scan, the map, the
 * model and the bits of a later pass are unchanged.  Device memory is taken per chunk of 2^20 (pose, point) pairs -- whole poses
 * (flimo_set_gicp_chunk, flimo_dev.h) --, 16 B a pair (24 B with pair_m). */
int flimo_scan_gicp(flimo_ctx* ctx, const double* x26 /* [np][26] */, size_t np, float max_dist, int32_t* valid /* [np] */,
                    double* H /* [np][21] */, double* g /* [np][6] */, double* cost /* [np] */, int32_t* pair_idx /* [np][n], may be NULL */,
                    double* pair_m /* [np][n], may be NULL */);
/* The functions the kernels call (flimo_gicp.h), on the host; none needs a device.  flimo_gicp_eigen_host: eig12 = l0 l1 l2, v0, v1,
 * v2 of cov6 by the Jacobi above.  flimo_gicp_regularize_host: out6 = C'; returns 1, or 0 (six NaN) where there is no covariance;
 * FLIMO_ERR_INVALID for a NULL pointer, an unknown rule, eps NaN or outside (0, 1].  flimo_gicp_term_host: w3 the float32 world point,
 * b3 the float32 stored point, p3 the float32 scan point, R9 the rotation, row-major; out30 = m, det, then the 28 contributions (H's
 * 21, g's 6, the cost) -- all 0 when the term is not live.  Returns 1 for a live term, 0 otherwise, FLIMO_ERR_INVALID for a NULL
 * pointer. */
int flimo_gicp_eigen_host(const double cov6[6], double eig12[12]);
int flimo_gicp_regularize_host(const double cov6[6], int rule, double eps, double out6[6]);
int flimo_gicp_term_host(const float w3[3], const float b3[3], const float p3[3], const float R9[9], const double CA6[6], const double CB6[6],
                         double out30[30]);
/* ---- pose hypotheses from point correspondences: what pcl::SampleConsensusPrerejective does per sample (the reference's
 *      relocation branch gets the same from KISS-Matcher's pruning and solver) -- minimal samples of three correspondences, a cheap
 *      polygon test, a closed-form rigid pose for each of the rest, and the count of the correspondences each pose explains, for
 *      all of the caller's samples at once.  The poses are the pos / rot entries of x26 rows for flimo_scan_fitness and
 *      flimo_scan_linearize. ----
 * Correspondence i says that body-frame point src[i] is map point dst[i] (both packed xyz, [m][3]).  Hypothesis j is the triplet
 * (a, b, c) = tri[j]; the samples are the caller's, so the call is deterministic.  Everything below is float64 on the float32 inputs
 * widened, nothing contracted, in exactly the written association, unless it says float32; sq(v) = v.x*v.x + (v.y*v.y + v.z*v.z).
 *  1. Edges, for both clouds: e_ab = sq(p_b - p_a), e_bc = sq(p_c - p_b), e_ca = sq(p_a - p_c).
 *  2. The hypothesis is FLIMO_CORR_DEGENERATE if two of its indices are equal, or if any of the six edges fails
 *     e >= (double)min_edge * (double)min_edge (a NaN coordinate fails it).
 *  3. Otherwise it is FLIMO_CORR_REJECTED if any of the pairs (e_s, e_d) = the same edge in src and dst fails
 *     fmin(e_s, e_d) >= s2 * fmax(e_s, e_d), s2 = (double)edge_sim * (double)edge_sim (no division; edge_sim == 0 rejects nothing).
 *  4. Otherwise the pose is TRIAD's (only + - * / sqrt).  Per cloud: e1 = p_b - p_a, e2 = p_c - p_a, u1 = e1 / sqrt(sq(e1)) (three
 *     divisions), cr = u1 x e2 = (y z' - z y', z x' - x z', x y' - y x'), u3 = cr / sqrt(sq(cr)), u2 = u3 x u1.  Then
 *       R[r][c] = u1d[r]*u1s[c] + (u2d[r]*u2s[c] + u3d[r]*u3s[c])
 *       cs = ((s_a + s_b) + s_c) / 3.0 per coordinate, cd likewise
 *       t[r] = cd[r] - (R[r][0]*cs[0] + (R[r][1]*cs[1] + R[r][2]*cs[2]))
 *     A non-finite entry of R or t (a collinear triangle) makes the hypothesis FLIMO_CORR_DEGENERATE.  The quaternion is Shepperd's:
 *     the largest of (trace, R00, R11, R22) with trace = R00 + (R11 + R22), the first on a tie, selects the branch --
 *       trace: w = 0.5*sqrt(1 + trace),               f = 0.25 / w, x = (R21 - R12)*f, y = (R02 - R20)*f, z = (R10 - R01)*f
 *       R00:   x = 0.5*sqrt(1 + ((R00 - R11) - R22)), f = 0.25 / x, w = (R21 - R12)*f, y = (R01 + R10)*f, z = (R02 + R20)*f
 *       R11:   y = 0.5*sqrt(1 + ((R11 - R00) - R22)), f = 0.25 / y, w = (R02 - R20)*f, x = (R01 + R10)*f, z = (R12 + R21)*f
 *       R22:   z = 0.5*sqrt(1 + ((R22 - R00) - R11)), f = 0.25 / z, w = (R10 - R01)*f, x = (R02 + R20)*f, y = (R12 + R21)*f
 *     -- without sign normalisation or renormalisation.  pose7 = (t, x, y, z, w).
 *  5. The inlier test is float32, so that it is what flimo_scan_fitness would see: RT is the 3 x 4 matrix pose_from_x26 forms from
 *     pose7 placed into an x26 (float32 casts, Eigen's toRotationMatrix); w_i = c0*x + (c1*y + (c2*z + c3)) of src[i] per row, the
 *     arithmetic of flimo_scan_to_world; sqd_i = (w_i - dst[i]).squaredNorm() as the searches form it (dx*dx + (dy*dy + dz*dz));
 *     pair i is an inlier iff sqd_i < max_dist * max_dist (one float32 product, a strict compare; INFINITY: no gate).
 * Outputs, host memory:
 *  - status [nh]: FLIMO_CORR_OK / _DEGENERATE / _REJECTED.
 *  - pose [nh][7] (may be NULL): pose7.
 *  - pair_sqd [nh][m] (may be NULL): sqd_i for an inlier, -1.0f for a non-inlier.
 *  - inliers [nh]: the exact count.  sum_sqd [nh]: the float64 sum of the inliers' float32 sqd in the shape of flimo_scan_fitness'
 *    sum with n = m: thread t of 256 adds slots t, t + 256, ... in ascending order (a non-inlier adds nothing), then
 *    partial[t] += partial[t + o] for o = 128, 64 .. 1.  No floating-point atomics: the bits of a hypothesis's outputs depend on the
 *    two clouds, its triplet and the cfg alone -- not on nh, the other hypotheses, the chunking or which survivors share a workgroup.
 * A hypothesis that is not OK has inliers 0, sum_sqd +0.0, pose NaN, pair_sqd -1.
 * nh == 0 returns FLIMO_OK and touches nothing.  FLIMO_ERR_INVALID: a NULL ctx / cfg / status / inliers / sum_sqd, NULL src or dst
 * (m > 0) or tri (nh > 0), a cfg field that is NaN or negative, edge_sim > 1, a triplet index outside [0, m) (the host checks all of
 * them before anything is launched).  FLIMO_ERR_TOO_LARGE: m or nh >= 2^31, or nh * m >= 2^31 when pair_sqd is asked for.  The
 * outputs are untouched on an error.  The map and the resident scan are neither read nor changed; an empty context will do.  Calling
 * rules as flimo_knn_k (no pass in flight).  Device memory: both clouds, and scratch per chunk of 2^16 hypotheses (at most 2^26
 * slots of pair_sqd), not per call.
 * flimo_corr_pose_host: steps 1 - 4 and the matrix of step 5 for ONE triplet on the host, by the same host / device function the
 * kernel calls: src3 / dst3 = the points a, b, c.  Returns the status (>= 0; pose7 and rt12 -- the upper three rows of RT,
 * row-major -- are NaN unless it is FLIMO_CORR_OK), or FLIMO_ERR_INVALID for a NULL pointer or a cfg the call above rejects. */
typedef struct flimo_corr_cfg {
  float edge_sim;   /* 0 .. 1: polygon pre-rejection, 0 = none */
  float min_edge;   /* >= 0 [m]: shorter triangle edges are degenerate */
  float max_dist;   /* >= 0 [m], INFINITY allowed: the inlier gate */
} flimo_corr_cfg;
#define FLIMO_CORR_OK 0
#define FLIMO_CORR_DEGENERATE 1
#define FLIMO_CORR_REJECTED 2
int flimo_corr_poses(flimo_ctx* ctx, const float* src_xyz /* [m][3] */, const float* dst_xyz /* [m][3] */, size_t m,
                     const int32_t* tri /* [nh][3] */, size_t nh, const flimo_corr_cfg* cfg,
                     int32_t* status /* [nh] */, int32_t* inliers /* [nh] */, double* sum_sqd /* [nh] */,
                     double* pose /* [nh][7], may be NULL */, float* pair_sqd /* [nh][m], may be NULL */);
int flimo_corr_pose_host(const float src3[9], const float dst3[9], const flimo_corr_cfg* cfg, double pose7[7], float rt12[12]);
/* ---- the consistency graph of the correspondences and its core numbers: the step between the putative pairs and the samples of
 *      flimo_corr_poses (what the reference's relocation branch gets from ROBIN's pruning of the compatibility graph).  A rigid
 *      motion preserves distances: correspondences i and j can both be true only if the edge from i to j is as long in src as in
 *      dst.  True pairs are therefore compatible with each other -- a clique --, a false pair is compatible with few others, and the
 *      core numbers of the graph tell the two apart.  tests/corr_graph_common.py restates everything below in numpy; every output
 *      is an integer or a bit and is compared exactly. ----
 * Vertices are the correspondences (src[i], dst[i]), both clouds packed xyz, [m][3].  Everything is float64 on the float32 inputs
 * widened, nothing contracted, in exactly the written association; sq(v) as for flimo_corr_poses.  For i != j, with
 * e_s = sq(s_j - s_i) and e_d = sq(d_j - d_i), {i, j} is an EDGE iff all three hold:
 *  1. e_s >= min2 and e_d >= min2, min2 = (double)min_edge * (double)min_edge;
 *  2. fabs(sqrt(e_s) - sqrt(e_d)) <= (double)tol;
 *  3. fmin(e_s, e_d) >= s2 * fmax(e_s, e_d), s2 = (double)edge_sim * (double)edge_sim (the polygon test of flimo_corr_poses on this
 *     edge; edge_sim == 0 rejects nothing).
 * Consequences: a NaN coordinate fails test 1, so its vertex is isolated (an infinite one fails test 1 or 2).  i == j is never an
 * edge.  The predicate is symmetric bit for bit: (a - b)^2 and (b - a)^2 are the same double.  Several scan points paired with ONE
 * map point have e_d = 0: with min_edge > 0 they are never compatible with each other -- the many-to-one case a ratio test leaves
 * behind.
 * Outputs, host memory:
 *  - adj [m][(m + 63) / 64] (may be NULL): bit j & 63 of word j >> 6 of row i is 1 iff {i, j} is an edge; the padding bits beyond m
 *    are 0.
 *  - degree [m]: the number of edges at i.
 *  - core [m]: the core number of i -- the largest c such that i lies in a set of vertices each of which has at least c neighbours
 *    inside the set.  It is unique: how it is computed cannot show in the result.
 *  - max_core (may be NULL): the largest core.
 * m == 0 returns FLIMO_OK and touches nothing (a max_core of 0 is the caller's to assume).  FLIMO_ERR_INVALID: a NULL ctx / cfg /
 * degree / core, NULL src or dst (m > 0), a cfg field that is NaN or negative, edge_sim > 1, an infinite tol or min_edge.
 * FLIMO_ERR_TOO_LARGE: m > FLIMO_CORR_GRAPH_MAX_M (the bit matrix is m * ((m + 63) / 64) * 8 B of device memory: 128 MB at the
 * limit; it is the call's, freed when it returns).  The outputs are untouched on an error.  The map and the resident scan are neither
 * read nor changed; an empty context will do.  Calling rules as flimo_corr_poses.  The core numbers are iterated on the device until
 * a round changes nothing: the number of rounds depends on the graph (about m / 2 for a chain, tens for a clique among noise) and is
 * not capped.
 * flimo_corr_compatible_host: the three tests for ONE pair of correspondences on the host, by the same host / device function the
 * adjacency kernel calls: 1 / 0, or FLIMO_ERR_INVALID for a NULL pointer or a cfg the call above rejects.  It sees points, not
 * indices: that i == j is no edge is the call's rule, not this function's. */
typedef struct flimo_corr_graph_cfg {
  float tol;        /* >= 0 [m]: two pairs are compatible when their two edge lengths differ by at most this */
  float min_edge;   /* >= 0 [m]: shorter edges (in either cloud) are never compatible */
  float edge_sim;   /* 0 .. 1: the polygon test of flimo_corr_poses on this edge, 0 = none */
} flimo_corr_graph_cfg;
#define FLIMO_CORR_GRAPH_MAX_M 32768
int flimo_corr_graph(flimo_ctx* ctx, const float* src_xyz /* [m][3] */, const float* dst_xyz /* [m][3] */, size_t m,
                     const flimo_corr_graph_cfg* cfg, int32_t* degree /* [m] */, int32_t* core /* [m] */,
                     int32_t* max_core /* may be NULL */, uint64_t* adj /* [m][(m + 63) / 64], may be NULL */);
int flimo_corr_compatible_host(const float si[3], const float sj[3], const float di[3], const float dj[3],
                               const flimo_corr_graph_cfg* cfg);
/* ---- nearest descriptors: which row of one descriptor array belongs to which row of another -- the step between flimo_map_fpfh
 *      (33-float rows) and flimo_corr_poses (matched pairs); pcl::search over FPFH space, brute force and exact, for all query
 *      rows at once.  tests/desc_common.py restates everything below in numpy; the tests compare every bit. ----
 * flimo_desc_ref_set makes a REFERENCE SET resident on the device (the map's descriptors: computed once, matched against many
 * times): desc [nr][dim] row-major, host memory.  It replaces the previous set; nr == 0 clears it.  It touches neither the map nor
 * the scan nor the bits of any later pass, and is freed with the context.  flimo_desc_ref_size / flimo_desc_ref_dim: the resident
 * set's rows and dim (0, 0: none).
 * flimo_desc_match answers, per query row q[i], with the first k reference rows in the order below.  Everything is float32 with
 * ONE rounding per written operation; fmaf is the correctly rounded fused multiply-add.
 *  - dot(a, b) = c_dim, where c_0 = +0.0f and c_{t+1} = fmaf(a[t], b[t], c_t) for t = 0 .. dim - 1 ascending.
 *  - n(a) = dot(a, a), the same chain.
 *  - d(q, r) = (n(q) + n(r)) - 2 dot(q, r): one float32 addition, then one rounding of the difference (2 dot is exact, so
 *    fmaf(-2, dot, n(q) + n(r)) and t - (dot + dot) are the same number); a negative result becomes +0.0f: d < 0 ? 0 : d.
 *  Consequences: two bit-identical rows are at distance exactly 0.  d is the squared L2 distance within
 *  (2 dim + 4) * 2^-24 * (n(q) + n(r)) of the exact value -- the standard bound of the three chains plus the two final roundings;
 *  about 0.25 for two FPFH rows at their largest possible norms (three histograms of sum 100: n <= 30 000), far less typically.
 *  That is the expanded form's accuracy, NOT the difference form's (sum of (q[t] - r[t])^2), which is relative to d itself: for
 *  two nearly equal long rows d may be all rounding error.  The order below is exact all the same.
 *  - Exclusion: a row with a non-finite entry is EXCLUDED -- as a query it has cnt 0, as a reference row it is never returned.  A
 *    pair whose d comes out NaN (huge finite entries that overflow a chain: inf - inf) is not returned either.  d = +inf is a
 *    distance like any other.
 *  - Order: (float32 bits of d, reference index), ascending.  d is non-negative, so bit order is value order; the order is total
 *    and unique, and does not depend on how the work is tiled, split or chunked.
 * Outputs, host memory: idx [nq][k] the reference rows, dist [nq][k] their d, cnt [nq] = min(k, admissible reference rows of the
 * query); the slots beyond cnt hold idx = -1, dist = 0.
 * No resident set: FLIMO_OK, every cnt 0.  nq == 0: FLIMO_OK, nothing touched.  FLIMO_ERR_INVALID: NULL ctx / q (nq > 0) / idx /
 * dist / cnt, dim not equal to the resident set's, NULL desc with nr > 0.  FLIMO_ERR_UNSUPPORTED: dim outside 1 ..
 * FLIMO_DESC_MAX_DIM, k outside 1 .. FLIMO_DESC_MAX_K.  FLIMO_ERR_TOO_LARGE: nr or nq >= 2^31, nq * k >= 2^31.  The outputs are
 * untouched on an error.  Calling rules as flimo_corr_poses (no pass in flight); neither the map nor the scan is read.  Device
 * memory: the resident set (its rows padded to an even dim and to whole tiles of 32, and 4 B a row), and per chunk of 2^16 queries
 * their rows, results and the partial lists of the grid's reference splits -- not per call.
 * flimo_desc_dist_host: d for ONE pair on the host, by the same host / device functions the device code uses for the norms and the
 * final step (NaN for a pair that the match excludes).  FLIMO_ERR_INVALID for a NULL pointer, FLIMO_ERR_UNSUPPORTED for a dim
 * outside 1 .. FLIMO_DESC_MAX_DIM. */
#define FLIMO_DESC_MAX_DIM 64
#define FLIMO_DESC_MAX_K 8
int flimo_desc_ref_set(flimo_ctx* ctx, const float* desc /* [nr][dim] */, size_t nr, int dim);
size_t flimo_desc_ref_size(const flimo_ctx* ctx);
int flimo_desc_ref_dim(const flimo_ctx* ctx);
int flimo_desc_match(flimo_ctx* ctx, const float* q /* [nq][dim] */, size_t nq, int dim, int k, int32_t* idx /* [nq][k] */,
                     float* dist /* [nq][k] */, int32_t* cnt /* [nq] */);
int flimo_desc_dist_host(const float* a, const float* b, int dim, float* d);
/* ---- Scan Context place recognition (Kim & Kim, IROS 2018): which earlier sweep was taken where this sweep was taken, and how is
 *      it turned relative to it -- a global descriptor per keyframe, a resident database of them, and the exact match of a batch of
 *      queries against every entry at every column shift.  The definition is ONE host / device header (csrc/hip/flimo_sc.h);
 *      tests/sc_common.py restates everything below in numpy; the tests compare every bit.  Everything is float32 with ONE rounding
 *      per written operation, nothing contracted; fmaf is the correctly rounded fused multiply-add. ----
 * 1. The descriptor of the resident scan: flimo_scan_context fills desc [rings][sectors] (host memory) and, unless NULL, *used.
 *  Per point (sc_bin):
 *  - Frame: with frame12 NULL, v is the point; otherwise v is the row-major 3 x 4 transform, c0*x + (c1*y + (c2*z + c3)) per row
 *    (a lidar-to-base or gravity alignment).  A point with a non-finite component of v has no bin.
 *  - Ring: r = sqrt(vx*vx + vy*vy), correctly rounded.  No bin unless r > 0, r >= min_range and r < max_range.
 *    ring = min(rings - 1, (int)(r * rscale)), rscale = (float)((double)rings / (double)max_range).
 *  - Sector: a = atan2f(vy, vx) as csrc/hip/flimo_math.h restates glibc's; if a < 0 then a = a + 0x1.921fb6p+2f.
 *    sector = min(sectors - 1, (int)(a * sscale)), sscale = (float)((double)sectors / 6.283185307179586).
 *  - Height: h = vz + z_offset.  No bin unless h > 0.
 *  desc[ring][sector] is the maximum h over the points that have that bin, +0.0f where none has; used is how many points have a
 *  bin.  h > 0, so the maximum is an integer maximum over the floats' bits: the scan's order and the launch shape move no bit.
 *  A pending deskew runs first, as for flimo_map_seen_through.  An empty scan: FLIMO_OK, an all-zero descriptor, used = 0.
 *  FLIMO_ERR_INVALID, outputs untouched: a NULL ctx, cfg or desc, a cfg value outside its range, a non-finite frame12 entry.  The
 *  map, the scan and the bits of a later pass are not touched.  The descriptor assumes a roughly level sensor (frame12 is where a
 *  gravity alignment goes) and carries no translation: two places that look alike from above are alike to it.
 *  flimo_sc_bin_host: sc_bin for ONE point on the host; returns 1 when the point has a bin (ring, sector, h are then set), 0 when
 *  it has none, FLIMO_ERR_INVALID as above.
 * 2. The resident database: entries get ids 0, 1, 2, .. in the order added; its shape is that of the first entry after a clear,
 *  any other shape is FLIMO_ERR_INVALID.  flimo_sc_db_add appends n descriptors from host memory (*first_id, unless NULL: the id of
 *  the first); flimo_sc_db_add_scan appends flimo_scan_context's result without a round trip -- its entry is bit-equal to
 *  flimo_sc_db_add of the downloaded descriptor.  At add time a launch forms each entry's normalised form (3.), kept on the device
 *  beside the raw rows; flimo_sc_db_get returns the raw rows of the entries [first, first + n) (FLIMO_ERR_INVALID when the range
 *  ends beyond the size).  flimo_sc_db_size / flimo_sc_db_shape: entries and shape (0 x 0: none).  flimo_sc_db_clear frees it.
 *  The capacity grows geometrically by device-to-device copy.  The database is independent of the map and of the scan -- inserts,
 *  crops and clears of the map leave it alone -- and is freed with the context.  FLIMO_ERR_TOO_LARGE at 2^31 entries; a failed
 *  add leaves the database as it was.  Device memory: 4 B * rings * (sectors + 64) + 8 B an entry.
 * 3. The match: flimo_sc_match answers, per query descriptor q[i], with the first k of the entries [first, first + n).
 *  Columns: for column j of a descriptor D, n_j = sqrt(c_R) with c_0 = +0, c_{t+1} = fmaf(D[t][j], D[t][j], c_t), rings ascending.
 *  The column is VALID iff n_j > 0; its normalised form is u[t][j] = D[t][j] / n_j (one correctly rounded division per entry),
 *  +0 for an invalid column.  A descriptor with a non-finite entry is EXCLUDED: as a query it has cnt 0, as an entry it is never
 *  returned.
 *  Per shift s in 0 .. sectors - 1, query column (j + s) mod sectors meets candidate column j: term_j is the ascending fmaf chain
 *  over the rings of uq[t][(j + s) % sectors] * uc[t][j] from +0 when both columns are valid, +0 otherwise; m(s) is the number of
 *  valid pairs; sum(s) is the pairwise tree ((t0 + t1) + (t2 + t3)) + .. over 64 slots indexed by j (+0 at and beyond sectors);
 *  d(s) = 1.0f - sum(s) / (float)m(s), a negative result +0.0f.  A shift with m(s) < min_cols is excluded (profile: NaN).
 *  The pair's distance is the first d(s) in the order (bits of d, s), shift is that s; a pair with every shift excluded is not
 *  returned.  Per query the answer is the first k candidates in the order (bits of dist, id) among those with dist < max_dist
 *  (strict); cnt is how many; the slots beyond cnt hold idx = -1, dist = 0, shift = -1 and a NaN profile.  The order is total: it
 *  does not depend on tiling, splits, chunks or the other queries.
 *  The meaning of the shift: the sector index grows with the angle in the sensor frame, so
 *  psi_query = psi_candidate - shift * 2 pi / sectors.  The descriptor carries no translation.
 *  Outputs, host memory: idx / dist / shift [nq][k], cnt [nq], profile [nq][k][sectors] (may be NULL: d(s) of each returned pair).
 *  FLIMO_OK with every cnt 0: no database, n == 0, a range wholly beyond the size (a range reaching past the size is cut to it).
 *  FLIMO_OK with nothing touched: nq == 0.  FLIMO_ERR_INVALID: a NULL pointer, a shape outside its range or other than the
 *  database's, a cfg value outside its range.  FLIMO_ERR_TOO_LARGE: nq * k >= 2^31.  Outputs are untouched on an error.  Calling
 *  rules as flimo_desc_match; neither the map nor the scan is read.  Brute force, exact: sectors^2 * rings multiply-adds a pair.
 *  flimo_sc_dist_host: ONE pair on the host by the same functions; returns 1 and sets dist and shift (profile [sectors] unless
 *  NULL), 0 when every shift is excluded (dist 0, shift -1), FLIMO_ERR_INVALID for a NULL pointer or a value out of range. */
#define FLIMO_SC_MAX_RINGS 32
#define FLIMO_SC_MAX_SECTORS 64
#define FLIMO_SC_MAX_K 8
typedef struct flimo_sc_cfg {
  int rings;        /* 1..32 */
  int sectors;      /* 2..64 */
  float min_range;  /* >= 0 */
  float max_range;  /* finite, > min_range */
  float z_offset;   /* finite; sensor height */
} flimo_sc_cfg;
typedef struct flimo_sc_match_cfg {
  int k;           /* 1..8 */
  int min_cols;    /* 1..sectors */
  float max_dist;  /* > 0 or INFINITY */
} flimo_sc_match_cfg;
int flimo_scan_context(flimo_ctx* ctx, const flimo_sc_cfg* cfg, const float frame12[12] /* may be NULL */,
                       float* desc /* [rings][sectors] */, int32_t* used /* may be NULL */);
int flimo_sc_bin_host(const float p[3], const flimo_sc_cfg* cfg, const float frame12[12], int* ring, int* sector, float* h);
int flimo_sc_db_add(flimo_ctx* ctx, const float* desc /* [n][rings][sectors] */, size_t n, int rings, int sectors, size_t* first_id);
int flimo_sc_db_add_scan(flimo_ctx* ctx, const flimo_sc_cfg* cfg, const float frame12[12], size_t* id);
size_t flimo_sc_db_size(const flimo_ctx* ctx);
int flimo_sc_db_shape(const flimo_ctx* ctx, int* rings, int* sectors);
int flimo_sc_db_get(flimo_ctx* ctx, size_t first, size_t n, float* desc);
int flimo_sc_db_clear(flimo_ctx* ctx);
int flimo_sc_match(flimo_ctx* ctx, const float* q /* [nq][rings][sectors] */, size_t nq, int rings, int sectors, size_t first, size_t n,
                   const flimo_sc_match_cfg* cfg, int32_t* idx /* [nq][k] */, float* dist /* [nq][k] */, int32_t* shift /* [nq][k] */,
                   int32_t* cnt /* [nq] */, float* profile /* [nq][k][sectors], may be NULL */);
int flimo_sc_dist_host(const float* a, const float* b, int rings, int sectors, int min_cols, float* dist, int* shift,
                       float* profile /* [sectors], may be NULL */);
/* Both clouds the caller of Localizer::updatePointCloud may ask for (pc2match: body frame; final_scan: world frame of pose x26,
 * Localizer.cpp:361-371) in ONE round trip: packed float4 records (x, y, z, unused) in pinned memory owned by the context, valid
 * until the next flimo_scan_clouds on it.  *n = points in each. */
int flimo_scan_clouds(flimo_ctx* ctx, const double x26[26], const float** body_xyzw, const float** world_xyzw, size_t* n);
/* The two clouds Localizer::updatePointCloud keeps under config.debug, for the last deskew of the resident raw sweep:
 * deskewed_scan (each point deskewed into the world frame with its own IMU pose, Localizer.cpp:848-850) and final_raw_scan (the
 * un-voxelised deskewed sweep moved by pose x26, Localizer.cpp:373-374).  Packed float4 records (x, y, z, w: the 4th component the
 * reference's arithmetic leaves, 1 for rigid matrices), both in the order of flimo_scan_clouds' arrays before the voxel grid and
 * any MAX_NUM_PC2MATCH cut (all points of the deskew), in pinned memory owned by the context, valid until the next call; one round
 * trip.  *n = 0 (no launch) when the resident scan did not come from a deskew (flimo_scan_set, a new raw sweep, a hand-over). */
int flimo_scan_debug_clouds(flimo_ctx* ctx, const double x26_final[26], const float** deskewed_world_xyzw,
                            const float** final_raw_xyzw, size_t* n);
int flimo_map_add_scan(flimo_ctx* ctx, const double x26[26], double stamp);

/* ---- Map segments: moving the map after a loop closure, forgetting by age (no counterpart in the reference) ----
 * Stored points lie in insertion order, and that order survives both an append and a rebuild of the map from its own points.  So a
 * run of insertion indices is a stretch of the drive, at zero bytes per point.  A context keeps a table begin[0 .. S], S >= 1,
 * begin[0] = 0: segment s is the stored points with insertion index in [begin[s], begin[s + 1]); begin[S] is flimo_map_size, so
 * the last segment is open and grows with every add.  A fresh context and one after flimo_map_clear have S = 1.  The table is host
 * bookkeeping; no device memory, no change to the insert.
 *
 * The table stays valid through every call that adds (also a batch that meets the zero-size root, which stores all points again in
 * order), through flimo_map_correct / flimo_map_transform (same points, same indices) and through flimo_map_remove_range (which
 * shifts the boundaries exactly).  It goes STALE with every other removal that removed at least one point -- crop, carve,
 * remove_outliers / _clusters / _plane / _regions, thin: they renumber the points and report no count per boundary.  With a stale
 * table flimo_map_segment_mark, flimo_map_correct and flimo_map_corrected answer FLIMO_ERR_NOMAP ("... stale ...") until
 * flimo_map_segments_reset or flimo_map_clear.
 *
 * flimo_map_segment_mark: closes the open segment at the current size and opens a new one; *id (may be NULL) = its number.  Empty
 *   segments are allowed.  FLIMO_ERR_TOO_LARGE at FLIMO_SEG_MAX segments.
 * flimo_map_segments: *n_seg = S, *stale = 0 / 1, begin[0 .. S] (all three may be NULL: ask with begin = NULL for the count);
 *   FLIMO_ERR_INVALID for cap < S + 1 with a non-NULL begin.
 * flimo_map_segments_reset: one segment over everything, not stale.
 *
 * The move.  T is a row-major 3 x 4 float64 matrix, new world <- old world, applied as given (rigidity is the caller's business).
 * With X = (double)x and so on, r_k = T[4k] * X + (T[4k+1] * Y + (T[4k+2] * Z + T[4k+3])), every operation float64 with one
 * rounding and nothing contracted; the moved component is (float)r_k.  flimo_seg_move_host runs the device's function on the host;
 * tests/segments_common.py restates it in numpy, bit for bit.  The result depends on nothing else: not the launch shape, not the
 * table's length.
 *
 * flimo_map_corrected: the predicate alone.  xyz [n][3] (may be NULL) = where the stored points [first, first + n) would go, each
 *   by its segment's matrix T[s]; *changed (may be NULL) = how many of them have different bits afterwards.  n_seg must equal S.
 *   Changes nothing: not the map, not the scan, not the bits of a later pass.
 * flimo_map_correct: every stored point moves by its segment's matrix; n_seg must equal S.  If no point's bits change, nothing
 *   happens at all (index and epoch stay, as after a crop that removes nothing).  Otherwise the map is clear() + initialize(moved
 *   points, insertion order, one batch): same size, same insertion indices (the table stays valid), flimo_map_last_time untouched
 *   (a correction is no insert), the second level stays around the sensor; everything that names old positions goes as after a
 *   crop (the last pass's records, the pruning bound, a queued pass), a GICP model is stale afterwards (flimo_scan_gicp refuses it)
 *   and flimo_ndt_info reports stale.  The Scan Context database and the resident scan are untouched.  The FILTER'S POSE IS THE
 *   CALLER'S TO SET after a correction (flimo_loc_set_x): the map moved under it.
 *   A failed call leaves the map exactly as it was: FLIMO_ERR_UNSUPPORTED when a moved component is not finite in float32, or when
 *   a fresh octree would refuse the moved points' box ("octree too deep", flimo_map_add) -- both known before anything is forgotten.
 *   FLIMO_ERR_INVALID for a NULL T, a non-finite entry of T, n_seg != S.  An empty map: FLIMO_OK, *changed = 0.
 * flimo_map_transform: the same with ONE matrix for every point (a second session registered into this one's frame).  It does not
 *   read the table: it works on a stale one and leaves table and flag alone.
 * flimo_map_remove_range: forgetting by age.  The stored points [first, first + n) go (the range is cut to the size); afterwards
 *   everything is as flimo_map_crop_box documents.  The table follows exactly -- begin'[s] = begin[s] - |[first, first + n) with
 *   [0, begin[s])| -- and is not marked stale.
 * Calling rules of the four: those of flimo_map_crop_box, no pass of this context in flight. */
#define FLIMO_SEG_MAX ((size_t)1 << 20)
int flimo_map_segment_mark(flimo_ctx* ctx, size_t* id);
int flimo_map_segments(const flimo_ctx* ctx, uint64_t* begin, size_t cap, size_t* n_seg, int* stale);
int flimo_map_segments_reset(flimo_ctx* ctx);
int flimo_seg_move_host(const double T[12], const float p[3], float out[3]);
int flimo_map_corrected(flimo_ctx* ctx, const double* T /* [n_seg][12] */, size_t n_seg, size_t first, size_t n, float* xyz /* [n][3] */,
                        size_t* changed);
int flimo_map_correct(flimo_ctx* ctx, const double* T /* [n_seg][12] */, size_t n_seg, size_t* changed);
int flimo_map_transform(flimo_ctx* ctx, const double T[12], size_t* changed);
int flimo_map_remove_range(flimo_ctx* ctx, size_t first, size_t n, size_t* removed);

/* Wall-clock bound (milliseconds, default 2000) of the wait for a pass's result inside flimo_match_reduce: the reference's
 * Mapper::match (Modules/Mapper.cpp:59-86) cannot hang, a GPU launch can -- when the bound expires the call returns
 * FLIMO_ERR_TIMEOUT (kernel still running) or FLIMO_ERR_HIP (stream idle, nothing published) instead of blocking its caller,
 * which holds the filter's mutex (Localizer.cpp:326-353). */
int flimo_set_wait_timeout_ms(flimo_ctx* ctx, int ms);

#ifdef __cplusplus
}
#endif
#endif /* FLIMO_C_H */
