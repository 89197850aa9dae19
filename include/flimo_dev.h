/* include/flimo_dev.h -- developer instrumentation of libflimo_hip.so: timing, statistics and the A/B switches bench.py and the
 * tests use.  Nothing here is part of the drop-in boundary (include/flimo_c.h): no entry replaces a reference interface, none
 * changes a result.  Same library, same context handle. */
#ifndef FLIMO_DEV_H
#define FLIMO_DEV_H
#include "flimo_c.h"
#ifdef __cplusplus
extern "C" {
#endif

/* GPU time [ms] of the stages of the last flimo_match_reduce, from HIP events on the ctx stream:
 * k-NN fast path, ring widening of the worklist, fit + reductions.  flimo_set_timing level:
 * 0 off, 1 on: every dispatch of a pass carries its own begin / end events (no extra packets on the stream). */
int flimo_set_timing(flimo_ctx* ctx, int level);
/* level 1 only: time every `every`-th pass (default 1 = all); the totals count the timed passes only. */
int flimo_set_timing_stride(flimo_ctx* ctx, int every);
/* on != 0: the events of flimo_match_reduce's timed passes are read when the totals are asked for (flimo_timing_totals /
 * flimo_timing_split; at the latest after 64 timed passes) instead of right behind each pass.  Reading costs the host tens of
 * microseconds per pass; a series in which every pass is timed then leaves the GPU idle half of the time, and on some boxes its
 * clocks follow (the same kernels read 10-15 % long).  flimo_last_kernel_ms reports the last pass READ, not the last run. */
int flimo_set_timing_deferred(flimo_ctx* ctx, int on);
/* number of flimo_match_reduce passes launched on this context so far */
unsigned long long flimo_pass_count(const flimo_ctx* ctx);
/* ... of which ran as ONE launch (k-NN + in-kernel widening + fit + reduction); the others used separate dispatches (first pass
 * of a scan with a poor prior, records / caps / debug, non-default lanes per query, gates wider than 3 rings) */
unsigned long long flimo_fused_pass_count(const flimo_ctx* ctx);
/* exact float32 distance ties (Objects/Octree.hpp:72-87,558-599: the reference keeps the candidate its recursion meets first):
 * out[0] = passes whose rows were rebuilt after settling ties in a launch of their own (records / caps / debug path), out[1] =
 * queries settled so far -- there and inside the reducing launches of the per-pass fast paths, which settle a tied query where
 * they build its row */
int flimo_tie_stats(flimo_ctx* ctx, unsigned long long out[2]);   /* (enters the context and drains its stream: owner's thread only) */
/* second level over crowded regions (cells holding > 64 points get a grid with a quarter of the cell edge and a pre-pass):
 * out[0] = active now, out[1] = map points copied into it, out[2] = times it was (re)built, out[3] = passes that ran the pre-pass */
int flimo_fine_stats(const flimo_ctx* ctx, unsigned long long out[4]);
int flimo_last_kernel_ms(const flimo_ctx* ctx, float* knn_ms, float* widen_ms, float* fit_ms);
/* sums over every pass since the last reset (timing must be on): per-stage GPU ms, passes, k-NN queries */
int flimo_timing_totals(flimo_ctx* ctx, double* knn_ms, double* widen_ms, double* fit_ms, long long* passes,
                        long long* queries, int reset);
/* level-1 totals by kind of timed pass since the last reset: out[0] ms of the one-launch passes (k-NN + in-kernel widening + fit +
 * reduction), out[1] their count; out[2..4] ms of the k-NN, widening and fit dispatches of the passes that ran them separately,
 * out[5] their count */
int flimo_timing_split(flimo_ctx* ctx, double out[6], int reset);
/* A/B switches of the pass layout (each: 1 on, 0 off, negative = leave): `tail` finishes pending queries inside the k-NN launch,
 * `fuse` runs the whole pass as one launch.  Both on by default; the benchmark switches `fuse` off for a short series to time the
 * k-NN stage (fast path + widening) on its own. */
int flimo_set_path_switches(flimo_ctx* ctx, int tail, int fuse);
/* number of scan points of the last pass that needed more than the 3x3x3 cell block */
int flimo_last_widen_count(const flimo_ctx* ctx);
/* the same count as published by the pass itself with its result (fast path), -1 when the last pass took a path that does
 * not report it (records / caps / timing level 2) */
int flimo_last_stragglers(const flimo_ctx* ctx);
/* ... by the pass's position within its scan, as last reported: out[0] first pass .. out[3] fourth and later (what decides the
 * layout of the pass at the same position of the next scan) */
int flimo_stragglers_by_pass(const flimo_ctx* ctx, int out[4]);
/* mean number of candidate map points examined per query in the last pass */
double flimo_last_candidates_per_query(const flimo_ctx* ctx);

/* The cell-sorted copy of the map is maintained incrementally: points appended by an insert go into their rows in place, a map
 * that outgrows its grid has the grid grown around it; the whole map is sorted only at the first layout and when a tile shape,
 * the point array or the tile pool no longer does.  Debug check: sorts the whole map again with the current geometry and counts
 * where the maintained index differs (by meaning: a row's points in order, a row's position at every column) -- 0 by construction.
 * stats = {inserts in place, full layouts} so far. */
int flimo_map_grid_selfcheck(flimo_ctx* ctx, uint64_t* mismatches, uint64_t stats[2]);
/* flimo_map_crop_box so far: out[0] = calls that removed points (each one full layout), out[1] = points removed */
int flimo_map_crop_stats(const flimo_ctx* ctx, uint64_t out[2]);
/* flimo_map_carve so far: out[0] = calls that removed points (each one full layout), out[1] = points removed.  (flimo_map_crop_stats
 * counts crops only: a carve with a box is a carve.) */
int flimo_map_carve_stats(const flimo_ctx* ctx, uint64_t out[2]);
/* The launch of flimo_map_correct / flimo_map_transform / flimo_map_corrected: slab = stored points a workgroup takes per step (a
 * multiple of 256 up to 16384; 0: the default, 2048), blocks = workgroups (0: two a compute unit).  Neither changes a result
 * (tests, A/B). */
int flimo_set_segment_plan(flimo_ctx* ctx, size_t slab, int blocks);
/* flimo_radius_search's walk, counted: cand[i] = stored points query i's walk loads and tests at this radius (what the count and
 * the fill launch each read, 16 bytes apiece); cand: host, [nq].  Arguments as flimo_radius_search. */
int flimo_radius_candidates(flimo_ctx* ctx, const float* q_xyz, size_t nq, float radius, uint64_t* cand);
/* flimo_knn_k's walk, counted: cand[i] = stored points query i's search loads and tests (16 bytes apiece), the block search and --
 * where it ran -- the walk over the tiles together; cand: host, [nq].  Arguments as flimo_knn_k. */
int flimo_knn_k_candidates(flimo_ctx* ctx, const float* q_xyz, size_t nq, int k, float max_dist, uint64_t* cand);
/* flimo_map_normals / flimo_map_normals_range work in chunks of n queries (default 2^20; 0 restores it): the chunk bounds the call's
 * device scratch.  The results do not depend on it (tests, A/B). */
int flimo_set_normals_chunk(flimo_ctx* ctx, size_t n);
/* flimo_map_outliers / flimo_map_remove_outliers search in chunks of n points (default 2^20; 0 restores it): the chunk bounds the
 * search's worklist, 8 B a point; equal results whatever the chunk. */
int flimo_set_outlier_chunk(flimo_ctx* ctx, size_t n);
/* flimo_map_fpfh works in chunks of n points (default 2^20; 0 restores it), in its two stages over the whole map and in the one
 * over the range: the chunk bounds the normals' moments, the worklist and the rows on their way back, 220 B a point; equal results
 * whatever the chunk. */
int flimo_set_fpfh_chunk(flimo_ctx* ctx, size_t n);
/* flimo_map_keypoints works in chunks of n points (default 2^20; 0 restores it), in its stage over the whole map and in the one over
 * the range: the chunk bounds the moments, the worklist and the mask on its way back, 85 B a point; equal results whatever the
 * chunk. */
int flimo_set_keypoints_chunk(flimo_ctx* ctx, size_t n);
/* flimo_map_clusters / flimo_map_remove_clusters walk the stored points' balls in launches of n points (default 2^20; 0 restores
 * it; at most 2^24 are used): the chunk bounds a launch's lanes, not the scratch; equal results whatever the chunk. */
int flimo_set_cluster_chunk(flimo_ctx* ctx, size_t n);
/* flimo_map_planes works in chunks of n hypotheses (default 2^10; 0 restores it; at most 2^16 and 2^26 partials are used): the
 * chunk bounds the partials, ceil(N / FLIMO_PLANE_SLAB) x 12 B a hypothesis, and the records; equal results whatever the chunk. */
int flimo_set_plane_chunk(flimo_ctx* ctx, size_t n);
/* The lane plan of flimo_map_voxels' moments stage: 0 chooses by the voxel's count (at most 8 points: a group of 8 lanes; at most
 * 16: 16 lanes; at most 1024: a wave; more: the many-runs path, one wave per run of 64 and a chain over the runs); 1, 2, 3 force
 * the groups of 8, 16, 64 lanes for every voxel, 4 the many-runs path.  + 8: the points are first written in sorted order, so the
 * moments read them without a gather.  Equal results whatever the plan; FLIMO_ERR_INVALID for any other value. */
int flimo_set_voxel_plan(flimo_ctx* ctx, int plan);
/* The link launches of flimo_map_regions / flimo_map_region_list / flimo_map_remove_regions work in chunks of n stored points
 * (default 2^20; 0 restores it; at most 2^24 are used): a launch's lanes stay far below 2^31 whatever the map's size.  The normals
 * in front of them go by flimo_set_normals_chunk, the listing's moments by flimo_set_voxel_plan (its + 8 is not used: they
 * gather).  Equal results whatever the chunks and the plan. */
int flimo_set_region_chunk(flimo_ctx* ctx, size_t n);
/* flimo_corr_poses works in chunks of n hypotheses (default 2^16; 0 restores it): the chunk bounds the call's device scratch, 136 B
 * a hypothesis (and m floats each where pair_sqd is asked for: then at most 2^26 slots a chunk); equal results whatever the chunk. */
int flimo_set_corr_chunk(flimo_ctx* ctx, size_t n);
/* flimo_desc_match works in chunks of queries_per_chunk queries (default 2^16; 0 restores it), and its grid splits the resident set
 * into runs of refs_per_split rows, rounded up to whole tiles of 32 (0, the default: chosen per call so that the grid fills the
 * device); the two bound the call's device scratch: per query of a chunk its row, its results and 16 or 64 B a split.  Equal
 * results whatever the two (tests: one tile of queries, one tile of references a split). */
int flimo_set_desc_chunk(flimo_ctx* ctx, size_t queries_per_chunk, size_t refs_per_split);
/* GPU milliseconds of the launches of the last flimo_desc_match on the context, all chunks together (0 unless flimo_set_timing is on) */
float flimo_desc_last_ms(const flimo_ctx* ctx);
/* flimo_sc_match works in chunks of queries_per_chunk queries (default 2^12; 0 restores it), and its grid splits the candidate
 * range into runs of entries_per_split entries (0, the default: chosen per call so that the grid fills the device); the two bound
 * the call's device scratch: per query of a chunk its rows, its results and 96 B a split.  Equal results whatever the two. */
int flimo_set_sc_chunk(flimo_ctx* ctx, size_t queries_per_chunk, size_t entries_per_split);
/* GPU milliseconds of the launches of the last flimo_sc_match on the context, all chunks together (0 unless flimo_set_timing is on) */
float flimo_sc_last_ms(const flimo_ctx* ctx);
/* flimo_scan_fitness works in chunks of whole poses, at most `pairs` (pose, point) pairs each (default 2^22; 0 restores it); a
 * single pose with more points than that runs alone.  The chunk bounds the call's device scratch.  The results do not depend on it
 * (tests, A/B). */
int flimo_set_fitness_chunk(flimo_ctx* ctx, size_t pairs);
/* flimo_scan_linearize works in chunks of whole poses, at most `pairs` (pose, point) pairs each (default 2^20; 0 restores it); a
 * single pose with more points than that runs alone.  The chunk bounds the call's device scratch (141 B a pair).  The results do
 * not depend on it (tests, A/B). */
int flimo_set_linearize_chunk(flimo_ctx* ctx, size_t pairs);
/* flimo_scan_ndt works in chunks of whole poses, at most `pairs` (pose, point) pairs each (default 2^20; 0 restores it); a single
 * pose with more points than that runs alone.  The chunk bounds the call's device scratch (84 B a pair at hood 7).  The results do
 * not depend on it (tests, A/B). */
int flimo_set_ndt_chunk(flimo_ctx* ctx, size_t pairs);
/* flimo_scan_gicp works in chunks of whole poses, at most `pairs` (pose, point) pairs each (default 2^20; 0 restores it); a single
 * pose with more points than that runs alone.  The chunk bounds the call's device scratch (16 B a pair, 24 B with pair_m).  The
 * results do not depend on it (tests, A/B). */
int flimo_set_gicp_chunk(flimo_ctx* ctx, size_t pairs);

/* out[0] = GPU ms of the algebra launches timed so far (timing level 1), out[1] = their number,
 * out[2] = chains run, out[3] = chains that came back before the final iteration, out[4] = chains declined */
int flimo_chain_stats(flimo_ctx* ctx, double out[5], int reset);
/* bytes held by the map: out[0] = the stored points (16 B each), out[1] = its index (the tiles that exist, directory, row
 * starts, the rows' room and first positions, escape pool as allocated), out[2] = the second level over crowded regions (points +
 * index), 0 when none is active; out[3] = tiles of the index that exist (with the shared empty one), out[4] = inserts that found
 * the tile pool too small and had the index laid out afresh, out[5] = the cell-sorted array AS ALLOCATED (three times the raw
 * buffer's capacity: its rows keep room behind their last point, so that an insert touches only the rows it adds to) */
int flimo_map_index_bytes(const flimo_ctx* ctx, uint64_t out[6]);
/* The layout of the map's index as it was actually made (tests place points by it instead of deriving it again): level 0 = the
 * main grid, 1 = the second level over crowded regions.  out[0..2] = ox oy oz (origin of the cells), [3] = cell edge, [4] = xs (fine x
 * columns per cell); [5..7] = six siy siz (the grid's corner in cells of the origin's lattice), [8..10] = nx ny nz; [11..13] = ts ty
 * tz (log2 of a tile's extent in segments of 8 columns / rows / layers), [14..16] = ntx nty ntz (directory extent); [17] = capacity
 * of the escape pool in slots (a slot: the eight cumulative counts of a segment with a column of more than 15 points), [18] = slots
 * taken since the last full layout; [19] = 1 when that level's index is valid (everything else is 0 when it is not), [20] = points
 * it holds; level 1 only: [21..23] / [24..26] = lowest / highest fine cell per axis of a query the second level may settle.
 * A point p lies in column floor(((p.x - ox) * (1 / cell)) * xs) - six * xs of row (floor((p.y - oy) * (1 / cell)) - siy,
 * floor((p.z - oz) * (1 / cell)) - siz), all in float32.  [18] is read from the device behind a wait for the context's stream:
 * the owner's thread only. */
int flimo_map_index_layout(flimo_ctx* ctx, int level, double out[28]);
/* pipelined host loop (flimo_set_pass_pipeline): {passes that found their launch waiting, queued passes nobody asked for, passes
 * whose waiting launch was found too old to publish to (told to leave, launched the usual way), passes whose launch had left as a
 * whole before the publish reached it (launched again)} */
int flimo_pass_pipeline_stats(const flimo_ctx* ctx, unsigned long long out[4]);
/* the hardware's side of the pipelined host loop: *large_bar = 1 when the device maps the whole of its memory for the host
 * (hipDeviceAttributeIsLargeBar), whatever a context then made of it -- a context on such a device queues passes ahead */
int flimo_device_large_bar(int device, int* large_bar);

/* ---- the filter's device algebra on its own (csrc/hip/flimo_ieskf.h; tests/test_gpu_ieskf.py, tests/test_ieskf_host.py) ----
 * Batch evaluation of its helpers: item i reads in[i * n_in ..] and writes out[i * n_out ..], all doubles, quaternions as x y z w.
 *   op                       in (n_in)                                  out (n_out)
 *   FLIMO_IK_SO3_LOG         q[4]                                (4)    log[3]                                    (3)
 *   FLIMO_IK_A_T             v[3]                                (3)    A_matrix(v)^T, row-major                  (9)
 *   FLIMO_IK_EXP_QUAT        v[3], scale                         (4)    q[4]                                      (4)
 *   FLIMO_IK_COS_SINC_SQRT   x2                                  (1)    cos, sinc                                 (2)
 *   FLIMO_IK_S2_BX           g[3]                                (3)    Bx 3 x 2                                  (6)
 *   FLIMO_IK_S2_BOXMINUS     g[3], other[3]                      (6)    g boxminus other                          (2)
 *   FLIMO_IK_S2_J            now[3], prop[3], delta[2]           (8)    Nx_yy(now) Mx(prop, delta), 2 x 2         (4)
 *   FLIMO_IK_GJ12_INVERSE    T[144]                              (144)  T^-1 [144], ok                            (145)
 *   FLIMO_IK_GJ12_SOLVE      T[144], v[12]                       (156)  u[12] with T u = v, ok                    (13)
 *   FLIMO_IK_PRE             x[26], x_prop[26], P_prop[529], R   (582)  dx_new[23], A11^-1[144], G2[132]          (299)
 * On the device the scalar helpers run one lane per item, the two Gauss-Jordan routines one wave per system, FLIMO_IK_PRE
 * (ik_pre_block) one 256-thread workgroup per item.  ok = 0: a zero pivot; the other outputs of that item mean nothing. */
enum {
  FLIMO_IK_SO3_LOG = 0, FLIMO_IK_A_T = 1, FLIMO_IK_EXP_QUAT = 2, FLIMO_IK_COS_SINC_SQRT = 3, FLIMO_IK_S2_BX = 4,
  FLIMO_IK_S2_BOXMINUS = 5, FLIMO_IK_S2_J = 6, FLIMO_IK_GJ12_INVERSE = 7, FLIMO_IK_GJ12_SOLVE = 8, FLIMO_IK_PRE = 9
};
int flimo_ieskf_op_shape(int op, int* n_in, int* n_out);
int flimo_ieskf_eval(flimo_ctx* ctx, int op, const double* in, size_t n, double* out);
/* The same source compiled for the host (GJ12_INVERSE: ik_inverse_gj12_serial, PRE: ik_pre_serial; GJ12_SOLVE has no twin in this
 * library: see flimo_localizer_c.h).  branch (optional, [n]): which way item i went --
 *   SO3_LOG, A_T: 1 = the norm is below MTK's tolerance;  EXP_QUAT, COS_SINC_SQRT: 1 = the Taylor series;  S2_BX: 1 = the chart at -L e_x;
 *   S2_BOXMINUS: 0 general, 1 equal, 2 antipodal, + 4 when `other` is on the chart at -L e_x;
 *   S2_J: bit 0 = |delta| below the tolerance, bit 1 / bit 2 = now / prop on the chart at -L e_x;  the others: 0. */
int flimo_ieskf_eval_host(int op, const double* in, size_t n, double* out, int* branch);
/* The whole device algebra on caller-given sums, on the context's stream: per iteration the launch of the measurement-independent
 * half and the launch from the sums to the next state (the two one-workgroup launches tools/ieskf_bench.hip queues), the stream
 * drained after each.  max_iter + 1 <= 12.  Iteration i reads set min(i, n_sets - 1):
 *   partials [n_sets][8][91]  the 91 sums (upper triangle of H^T H row by row, H^T h, M) as eight groups' partial sums;
 *   extras   [n_sets][2]      stragglers, ties;   tag_ok [n_sets] or NULL: 0 = the set's granules carry another pass's number.
 * iter_out [max_iter + 1][FLIMO_IK_ITER_N], *n_iter = iterations run (the one that handed back included); record of an iteration:
 *   [0] pre_dxn[23]  [23] pre_AG[276] as its first launch left them;  [299] the log entry HTH[144] HTh[12] dx[23] x_after[26] (zeros
 *   when the iteration handed back);  [504] the head's PoseMats (66 floats)  [570] prev_RT[16]  [586] status  [587] it  [588] t
 *   [589] passes  [590] 1 = the chain went on.
 * final_out [FLIMO_IK_FINAL_N]: [0] status [1] reason [2] passes [3] it [4] t [5] x[26] [31] per pass M, stragglers, ties [67] the
 * handed-back 91 sums. */
#define FLIMO_IK_ITER_N 591
#define FLIMO_IK_FINAL_N 158
int flimo_ieskf_run_fixed(flimo_ctx* ctx, const double x26[26], const double P[529], const double limits[23], double R, double D,
                          int max_iter, int n_sets, const double* partials, const double* extras, const int* tag_ok,
                          double* iter_out, double* final_out, int* n_iter);
/* (host twins, libfast_limo.so: flimo_ieskf_gj12_host and flimo_ieskf_run_fixed_host, include/flimo_localizer_c.h) */

/* ---- host-side evaluation, no GPU (round 6: out of the boundary header): what the host C++ mirror's Plane / calculate_H objects and
 * the CPU tests call ----
 * Replays the map's insert rule (Octree::initialize / update, Objects/Octree.hpp:282-432) over a
 * sequence of batches of packed NaN-free points: keep[i] = 1 if point i is stored.  Host only. */
/* Host-side evaluation of the plane routines of the fit kernel (same source, compiled for the host): Plane::estimate_plane
 * (Objects/Plane.cpp:80-105) for exactly 5 points (xyz packed) and Plane::plane_eval (:107-114).  They back the
 * fast_limo::Plane object of the host C++ mirror; the registration path never calls them. */
void flimo_plane_fit5_host(const float xyz[15], float n_out[4]);
int  flimo_plane_eval5_host(const float n[4], const float xyz[15], float threshold);

/* Localizer::calculate_H (Localizer.cpp:537-577) for M given matches on the host, with the fit kernel's own row routine:
 * p_global [M][3], n [M][4] (plane.get_normal()), dist [M] (Match::dist); H [M][12] row-major, h [M] = -dist.  Backs the
 * Localizer::calculate_H method of the host C++ mirror; the registration path computes the same rows on the GPU. */
int flimo_calculate_H_host(const double x26[26], const float* p_global, const float* n, const float* dist, size_t M,
                           int estimate_extrinsics, double* H, double* h);

int flimo_insert_rule_replay(float min_extent, int downsample, const float* xyz, const size_t* batch_sizes,
                             size_t n_batches, unsigned char* keep, size_t* stored);

#ifdef __cplusplus
}
#endif
#endif /* FLIMO_DEV_H */
