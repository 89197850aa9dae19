// fast_limo_amd/csrc/hip/flimo_ctx.h -- the context behind the C ABI and what its two translation units share.
//
// Private to csrc/hip and no API: flimo_capi.hip (the registration path: context, map index, sweep front end, passes, chain) and
// flimo_capi_query.hip (the map and scan analysis entries) include it, nothing else does.  struct flimo_ctx, the error and
// buffer helpers every entry uses, the entry gate (ctx_enter), and the three functions flimo_capi.hip defines for both.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string>
#include <array>
#include <vector>
#include <algorithm>
#include <immintrin.h>
#include "../../../include/flimo_c.h"
#include "flimo_types.h"
#include "flimo_kernels.h"
#include "flimo_chain.h"
#include "flimo_insert.h"
#include "flimo_gbook.h"

using namespace flimo;

struct flimo_ctx {
  int device = -1;
  hipStream_t stream = nullptr;
  std::string err;
  // config
  flimo_map_cfg map_cfg{0.2f, 2, 1, 0.5f};
  int timing = 0;                  // 0 off, 1 k-NN kernel only (events ride on its dispatch), 2 every stage
  int tail_max_env = 0;            // developer: FLIMO_TAIL_MAX overrides the straggler count up to which a launch finishes its own
  int timing_stride = 1;           // level 1: time every n-th pass only (sampling keeps the perturbation small)
  bool debug_recs = false;
  // map
  float4* d_map_raw = nullptr;     // insertion order
  float4* d_map_sorted = nullptr;  // cell order
  float gbox[6] = {0, 0, 0, 0, 0, 0};   // box the grid geometry was laid out for (the map box plus slack on the sides that grew)
  bool have_gbox = false;
  bool force_full = false;         // the next index update lays the grid out afresh (cell size changed)
  bool full_rebuild = false;       // FLIMO_FULL_REBUILD=1: sort the whole map on every insert (A/B of the merge)
  uint64_t grid_merges = 0, grid_builds = 0, grid_regrids = 0, index_overflows = 0, pool_grows = 0;
  uint64_t crops = 0, crop_removed = 0;   // flimo_map_crop_box: calls that removed points, points removed so far
  uint64_t carves = 0, carve_removed = 0; // flimo_map_carve: the same
  uint64_t outlier_removals = 0, outlier_removed = 0;   // flimo_map_remove_outliers: the same
  uint64_t cluster_removals = 0, cluster_removed = 0;   // flimo_map_remove_clusters: the same
  uint64_t plane_removals = 0, plane_removed = 0;       // flimo_map_remove_plane: the same
  uint64_t thin_removals = 0, thin_removed = 0;         // flimo_map_thin: the same
  uint64_t region_removals = 0, region_removed = 0;     // flimo_map_remove_regions: the same
  uint64_t range_removals = 0, range_removed = 0;       // flimo_map_remove_range: the same
  // map segments (include/flimo_c.h): segment s is the insertion indices [seg_begin[s], seg_begin[s + 1]), the last one open up to
  // map_n; host bookkeeping only.  seg_stale: a removal renumbered the points and the table no longer says where a stretch lies
  std::vector<uint64_t> seg_begin{0};
  bool seg_stale = false;
  size_t seg_slab = 0;             // flimo_set_segment_plan: points per workgroup and step of the move (0: SEG_SLAB_DEFAULT) ...
  int seg_blocks = 0;              // ... and its grid (0: two workgroups a compute unit); neither changes a result
  bool have_origin = false;        // the origin of the map's cells is set (GridView: it stays; a grid that grows moves its corner by whole cells)
  size_t map_n = 0, map_cap = 0, sorted_cap = 0;
  size_t normals_chunk = (size_t)1 << 20;   // queries per launch of flimo_map_normals (flimo_set_normals_chunk): bounds its device scratch
  size_t outlier_chunk = (size_t)1 << 20;   // points per search launch of flimo_map_outliers (flimo_set_outlier_chunk)
  size_t fpfh_chunk = (size_t)1 << 20;      // points per search launch of flimo_map_fpfh (flimo_set_fpfh_chunk)
  size_t keypoints_chunk = (size_t)1 << 20; // points per search launch of flimo_map_keypoints (flimo_set_keypoints_chunk)
  size_t cluster_chunk = (size_t)1 << 20;   // points per link launch of flimo_map_clusters (flimo_set_cluster_chunk)
  size_t region_chunk = (size_t)1 << 20;    // points per link launch of flimo_map_regions (flimo_set_region_chunk)
  size_t plane_chunk = (size_t)1 << 10;     // hypotheses per chunk of flimo_map_planes (flimo_set_plane_chunk)
  int voxel_plan = 0;                       // lane plan of flimo_map_voxels' moments (flimo_set_voxel_plan; 0: by the voxel's count)
  size_t linearize_chunk = (size_t)1 << 20; // (pose, point) pairs per chunk of flimo_scan_linearize (flimo_set_linearize_chunk)
  size_t fitness_chunk = (size_t)1 << 22;   // (pose, point) pairs per chunk of flimo_scan_fitness (flimo_set_fitness_chunk)
  size_t corr_chunk = (size_t)1 << 16;      // hypotheses per chunk of flimo_corr_poses (flimo_set_corr_chunk)
  // the resident reference set of flimo_desc_match (flimo_desc_ref_set): the rows in the MFMA operand layout and their norms
  float* d_desc_rt = nullptr;
  float* d_desc_norm = nullptr;
  size_t desc_nr = 0;
  int desc_dim = 0;
  size_t desc_chunk = (size_t)1 << 16;      // queries per chunk of flimo_desc_match (flimo_set_desc_chunk)
  size_t desc_split = 0;                    // reference rows per split of its grid; 0: chosen per chunk, to fill the device
  float desc_last_ms = 0.f;                 // GPU time of the last call's launches (timing level >= 1)
  // the resident Scan Context database (flimo_sc_db_add): the raw rows, their normalised form (flimo_sc.h) and the bits of the
  // valid columns; independent of the map and of the scan
  float* d_sc_raw = nullptr;                // [sc_cap][sc_rings][sc_sectors]
  float* d_sc_un = nullptr;                 // [sc_cap][sc_rings][64]
  unsigned long long* d_sc_valid = nullptr; // [sc_cap]
  size_t sc_n = 0, sc_cap = 0;
  int sc_rings = 0, sc_sectors = 0;
  size_t sc_chunk = (size_t)1 << 12;        // queries per chunk of flimo_sc_match (flimo_set_sc_chunk)
  size_t sc_split = 0;                      // entries per split of its grid; 0: chosen per chunk, to fill the device
  float sc_last_ms = 0.f;                   // GPU time of the last call's launches (timing level >= 1)
  // the resident NDT cell models (flimo_ndt_build): each a SNAPSHOT of the map's voxels at its build -- inserts, removals and
  // flimo_map_clear leave it alone and only move map_epoch on, which is how flimo_ndt_info knows a model stale
  struct NdtModel {
    bool built = false;
    size_t nc = 0, map_n = 0;               // cells; stored points at the build
    float leaf = 0.f;
    int min_pts = 0;
    double eig_ratio = 0.0;
    uint64_t epoch = 0;                     // map_epoch at the build
    unsigned long long* d_keys = nullptr;   // [nc] ascending
    int32_t* d_count = nullptr;             // [nc]
    double* d_eval = nullptr;               // [nc][3] l0 <= l1 <= l2, before the clamp
    void* d_cells = nullptr;                // [nc] NdtCell (flimo_ndt.h)
    void release() {
      (void)hipFree(d_keys); (void)hipFree(d_count); (void)hipFree(d_eval); (void)hipFree(d_cells);
      *this = NdtModel{};
    }
  } ndt[FLIMO_NDT_SLOTS];
  uint64_t map_epoch = 0;                   // bumped whenever the stored points change: the insert, the clear, the removals' shared tail
  size_t ndt_chunk = (size_t)1 << 20;       // (pose, point) pairs per chunk of flimo_scan_ndt (flimo_set_ndt_chunk)
  // the resident GICP model (flimo_gicp_build): one regularised covariance per stored point, by INSERTION INDEX -- a snapshot like an
  // NDT model, but usable only for the map it was built from (a removal renumbers the points): flimo_scan_gicp refuses it once
  // map_epoch has moved
  struct GicpModel {
    bool built = false;
    size_t n = 0, n_cov = 0;                // stored points at the build; those that got a covariance
    flimo_gicp_cfg cfg{};
    uint64_t epoch = 0;                     // map_epoch at the build
    double* d_cov = nullptr;                // [n][6] xx xy xz yy yz zz, six NaN where there is none
    void release() {
      (void)hipFree(d_cov);
      *this = GicpModel{};
    }
  } gicp;
  // the covariances of the resident scan's points (flimo_scan_cov_set): the caller's, dropped whenever the scan is replaced
  double* d_scan_cov = nullptr;             // [scan_cov_n][6], body frame, the scan's order
  size_t scan_cov_n = 0, scan_cov_cap = 0;
  size_t gicp_chunk = (size_t)1 << 20;      // (pose, point) pairs per chunk of flimo_scan_gicp (flimo_set_gicp_chunk)
  bool sorted_follows = false;     // the raw buffer grew: the cell-sorted copy (3x its capacity) and the escape pool have to follow
  IndexTables idx;                 // the index of the main grid (GridView, flimo_types.h): tiles, directory, escapes, xstart
  GridView grid{};
  bool grid_valid = false;
  double map_last_time = -1.0;
  float bb[6] = {3.4e38f, 3.4e38f, 3.4e38f, -3.4e38f, -3.4e38f, -3.4e38f};   // bounding box of the stored points
  MapBuildScratch scratch;
  InsertBook* book = nullptr;      // host statement of the insert rule (flimo_insert.h): A/B checks and flimo_insert_rule_replay only
  GBook gbook;                     // the same tree on the device: every later batch is decided there
  float4* d_batch = nullptr;       // staging for host-supplied later batches
  size_t batch_cap = 0;
  // scan
  float4* d_scan = nullptr;        // pc2match (body frame), caller order
  float4* d_scan_sorted = nullptr; // the same points in Morton order, w = original index
  void* d_nbr = nullptr;           // per-query neighbour records (sorted order)
  int* d_wl = nullptr;             // worklist of queries that need the general ring search
  int* d_wl_count = nullptr;
  void* d_raw32 = nullptr;         // unfiltered sweep as 32-byte PointType records (flimo_raw_scan_filter_set)
  size_t raw32_cap = 0;
  unsigned long long* d_filt_ext = nullptr;
  unsigned long long* h_filt_ext = nullptr;   // pinned
  double resident_t_offset = 0.0;  // sweep offset of the resident raw scan's stamps (0: already contained in them)
  unsigned long long* d_tkey[2] = {nullptr, nullptr};   // ordered stamp keys of the kept points / the same sorted (device time order)
  uint32_t* d_tperm = nullptr;     // time rank -> position among the kept points (arrival order)
  double* d_t_tmp = nullptr;
  size_t tkey_cap = 0;
  bool raw_time_ordered = false;   // the resident raw scan is in the reference's time order (stamps pairwise different)
  float4* d_scan_raw = nullptr;    // raw lidar-frame points for deskew (caller order)
  float4* d_raw_sorted = nullptr;  // the same in Morton order, w = original index
  double* d_t_sorted = nullptr;
  size_t raw_sorted_cap = 0;       // capacity of the two above
  float4* d_scan_world = nullptr;
  double* d_scan_t = nullptr;
  size_t scan_n = 0, scan_cap = 0, raw_n = 0;
  size_t order_n = 0;              // points of the last input stage run HERE (d_tperm; stays when the sweep is handed over)
  size_t sorted_n = 0;             // points in d_scan_sorted: scan_n, or the MAX_NUM_PC2MATCH prefix once a pass asked for it
  void* d_frames = nullptr;
  size_t frames_cap = 0;
  char* d_frames_fg = nullptr;              // two slots of FRAMES_FG_SLOT bytes in fine-grained device memory the host stores into (large-BAR devices):
                                            // the IMU frames of a deskew without a copy launch (DeskewArgs::stage_words)
  void* h_frames[2] = {nullptr, nullptr};   // pinned staging of the IMU frames, alternating: the deskew call does not wait
  size_t h_frames_cap = 0;
  int frames_slot = 0, async_deskews = 0;   // copies possibly still in flight since the stream was last known idle
  // A deskew that has been set up (frames uploaded) but not run: the scan's first k-NN launch runs it on the way (DeskewArgs),
  // anything else that reads d_scan / d_scan_sorted first runs the stand-alone kernel (flush_deskew)
  DeskewArgs deskew_args{};
  size_t deskew_n = 0;
  bool deskew_pending = false;
  bool deskew_kept = false;        // deskew_args / deskew_n still describe the resident raw sweep (flimo_scan_debug_clouds)
  // per pass
  Rec16* d_recs = nullptr;
  RecDbg* d_dbg = nullptr;
  size_t rec_cap = 0;
  int last_nq = 0;
  int reduce_waves = 256;
  double* d_partials = nullptr;    // records-mode reduction partials [reduce_waves][256]
  double* d_fit_partials = nullptr;  // per fit-block partials [fit_blocks][256]
  size_t fit_partials_cap = 0;
  double* d_out256 = nullptr;
  double* h_out256 = nullptr;      // pinned + mapped: the last fit block writes the result straight to host memory
  double* d_out256_host = nullptr; // device alias of h_out256
  unsigned int* d_ticket = nullptr;
  // fit2 (per-pass fast path): per-block partials of the FIT_LIVE sums, granule slots in mapped host memory
  double* d_fit2_partials = nullptr;
  size_t fit2_partials_cap = 0;
  double* h_granules = nullptr;    // pinned + mapped: [FIT_GROUPS][FIT_LIVE_PAD] x {sum, pass number}
  double* d_granules_host = nullptr;
  unsigned char live_idx[FIT_LIVE_PAD];   // live sum k -> raw MFMA accumulator index (from the calibrated layout)
  bool fuse = true;                // FLIMO_FUSE=0: k-NN and fit stay separate dispatches in every pass (A/B checks)
  unsigned long long fused_passes = 0;
  unsigned long long pass_seq = 0;  // last pass number published by the fit kernel
  unsigned long long* d_cand = nullptr;
  unsigned long long* h_cand = nullptr;  // pinned
  double last_cand_per_query = 0.0;
  int mfma_idx[16][16];            // (i,j) -> raw index
  // staging
  void* h_stage = nullptr;         // pinned
  void* h_clouds = nullptr;        // pinned: the two clouds of flimo_scan_clouds
  void* h_dbg_clouds = nullptr;    // pinned: the two clouds of flimo_scan_debug_clouds
  float4* d_dbg_clouds = nullptr;  // their device side, [deskewed | final raw]
  size_t dbg_clouds_cap = 0, dbg_clouds_dcap = 0;   // bytes of h_dbg_clouds, points of each half of d_dbg_clouds
  void (*overlap_fn)(void*) = nullptr;   // flimo_match_reduce_overlap: host work of the caller to run while the pass is in flight
  void* overlap_arg = nullptr;
  size_t clouds_cap = 0;
  size_t stage_cap = 0;
  // timing
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // [0,1] k-NN / fused dispatch, [2,3] fit, [4,5] widening
  // deferred reading (flimo_set_timing_deferred): each timed pass takes the next set of a ring and nobody reads it until the totals
  // are asked for -- reading a pass's events right behind it costs the host tens of microseconds per pass, and a GPU that idles
  // through those lowers its clocks on some boxes (the same kernels then read 10-15 % long)
  static constexpr int EV_RING = 64;
  hipEvent_t ev_ring[EV_RING][6];
  unsigned char ev_kind[EV_RING];   // bit 0: one-launch pass, bit 1: fit2 layout, bit 2: the widening was timed
  int ev_pending = 0;
  bool ev_ring_made = false, timing_deferred = false;
  float last_knn_ms = 0.f, last_widen_ms = 0.f, last_fit_ms = 0.f;
  int* h_wl_count = nullptr;   // pinned
  int last_widen_count = 0;
  double tot_knn_ms = 0, tot_widen_ms = 0, tot_fit_ms = 0;
  long long tot_passes = 0, tot_queries = 0;
  // level-1 totals by kind of timed pass: [0] one-launch passes: total ms, count; [1] separate dispatches: k-NN ms, widening ms, fit ms, count
  double split_fused_ms = 0, split_knn_ms = 0, split_widen_ms = 0, split_fit_ms = 0;
  long long split_fused_n = 0, split_sep_n = 0;
  flimo_match_cfg last_cfg{};
  PoseMats last_P{};
  MatchParams last_mp{};
  int last_n_all = 0;
  bool recs_valid = false, dbg_valid = false;
  PrevPass prev{};                 // previous pass of the same resident scan (k-NN pruning bound); valid = 0 after any scan change
  bool prune = true;               // FLIMO_PRUNE=0 disables the bound (A/B checks)
  unsigned probe_min = 96;         // FLIMO_PROBE=<n>: first pass, a query with >= n candidates in its 3x3x3 block walks its own cell first for a bound (0: off)
  int stragglers_hist[4] = {1 << 30, 0, 0, 0};   // the same per pass position within a scan (0 = first pass .. 3 = fourth and later), last scan that reported
  int pass_in_scan = 0;
  int last_stragglers = -1;        // the same of the last pass (-1: not reported by that pass's path)
  // second level over crowded regions (flimo_map.hip): a grid with a quarter of the cell edge over the box around the cells near the
  // sensor that hold more than fine_threshold points, with a copy of every map point inside it
  bool fine_on = true;             // FLIMO_FINE=0 switches it off (A/B checks)
  unsigned fine_threshold = 64;    // FLIMO_FINE_THRESHOLD
  int fine_div = 4;                // FLIMO_FINE_DIV: fine cells per cell edge (power of two)
  unsigned fine_min_points = 32768;// FLIMO_FINE_MIN_POINTS: smaller crowded regions are not worth the extra dispatch (measured: 1M map, 7k points: +4 us)
  bool fine_valid = false;
  bool crowd_box_valid = false;    // the crowded-cell list (device bits + list, host copy) belongs to the current geometry
  GridView fine{};
  int fine_qlo[3] = {0, 0, 0}, fine_qhi[3] = {-1, -1, -1};
  float4 *d_fine_tmp = nullptr, *d_fine_pts = nullptr;
  size_t fine_pts_cap = 0;
  IndexTables fine_idx;
  uint32_t* d_fine_count = nullptr;
  void* d_crowd_list = nullptr;        // int4 (x, y, z, -) of every crowded cell of the current geometry, listed once
  uint32_t* d_crowd_count = nullptr;
  uint32_t* d_crowd_bits = nullptr;    // one bit per cell: listed
  size_t crowd_bits_cap = 0;
  uint32_t crowd_listed = 0;           // entries of the device list the host has fetched
  std::vector<std::array<int, 3>> crowd_cells;
  float fine_center[3] = {0.f, 0.f, 0.f};   // sensor position of the last inserted scan (world)
  bool have_fine_center = false;
  float fine_radius = 24.f;            // FLIMO_FINE_RADIUS [m]: crowded cells farther from the sensor (xy) stay out of the region
  uint64_t fine_builds = 0, fine_passes = 0;
  int xslabs = 2;                  // fine columns per cell along x (1, 2, 4, 8; power of two): a pass that has the
                                   // previous pass's bound walks only the half cells its ball reaches.  Measured (round 3, 1M map):
                                   // clean map no change (21.8 -> 22.1 us), after 50 raw 64k sweeps the later passes 30.9 -> 23.2 us
                                   // (1.05x the clean map's); inserts unchanged at 2 (0.28 ms), +14 % at 4; both tables twice the size
                                   // (the layout falls back to fewer columns where 32-bit indices would not do)
  int* d_tie_list = nullptr;       // queries of a pass whose five hinge on an exact distance tie (capacity = scan capacity)
  unsigned int* d_tie_count = nullptr;   // [2]: alternating by pass number (the pass's reduction re-arms the next one's)
  size_t tie_cap = 0;
  bool ties = true;                // FLIMO_TIES=0: leave ties to the position rule (A/B checks)
  unsigned long long tie_redos = 0, tie_queries = 0;
  unsigned long long* d_tie_settled = nullptr;   // queries whose ties were settled inside a reducing launch (tie_repair_wave), counted on the device
  void* d_nbrk = nullptr;          // neighbour records of the general pass
  size_t nbrk_cap = 0;
  int wait_timeout_ms = 2000;      // wall-clock bound of the wait for a pass's result (flimo_set_wait_timeout_ms)
  hipEvent_t adopt_ev = nullptr;   // flimo_scan_adopt: orders the two contexts' streams around the hand-over copies
  hipEvent_t timeout_ev = nullptr; // recorded behind the launches of a pass / chain whose wait ran out
  bool timeout_pending = false;    // ... and not yet seen complete: no new pass is queued on top of it (check_abandoned)
  // the whole iterated update enqueued at once (flimo_chain.h, flimo_update_chain)
  ChainState* d_chain = nullptr;         // device filter state
  void* d_chain_gran = nullptr;          // device copy of the granule slots: a chained pass publishes its sums here
  ChainPrior* h_chain_prior = nullptr;   // mapped: the prior of the scan's update (read by the first algebra kernel)
  ChainPrior* d_chain_prior = nullptr;   // its device alias
  double* h_chain_res = nullptr;         // mapped: CH_RES result granules {value, tag}
  void* d_chain_res = nullptr;
  double* h_chain_log = nullptr;         // mapped: CH_MAX_PASSES x CH_LOGN log granules
  void* d_chain_log = nullptr;
  unsigned long long chain_tag = 0x4000000000000000ull;   // tag of the last chain (own number space)
  // Host loop, pipelined (FLIMO_PIPELINE=0 switches it off): while a one-launch pass runs, the NEXT pass of the same update is already
  // queued behind it -- a chained-pass kernel whose workgroups wait, placed on the GPU, for their constants in `d_pipe_head`
  // (fine-grained device memory the host stores into through the PCIe BAR).  The next flimo_match_reduce then publishes the pose
  // instead of launching: no doorbell -> dispatch -> kernel start on the iteration's critical path.  A pass nobody asks for (the
  // update converged) is told to leave by the next call on the context (ctx_enter).
  struct Prelaunch {
    bool active = false;
    unsigned long long seq = 0;      // the pass number it will publish under
    size_t nq = 0;
    int n_all = 0, pos = 0;
    flimo_match_cfg cfg{};
    uint64_t grid_version = 0;
    unsigned int end_code = 0;
    double t_launch = 0.0;
    float prev_RT[16] = {0};   // the bound's reference pose the launch was given (a kernel argument)
  } pre;
  bool pipeline = false;                 // flimo_set_pass_pipeline (FLIMO_PIPELINE=0/1 presets it and wins)
  bool pipeline_env = false;
  PipeHead* d_pipe_head = nullptr;       // fine-grained device memory (host-writable); nullptr: not available on this system
  unsigned int pipe_tag = 0;
  bool pipe_last_hint = false;           // flimo_pass_pipeline_last: the next pass is its update's last -- nothing is queued behind it
  unsigned long long pipe_published = 0, pipe_cancelled = 0;   // statistics
  unsigned long long pipe_aged = 0, pipe_left = 0;             // passes found too old to be published to / that left before the publish reached them
  bool row_slack = true;                  // FLIMO_ROW_SLACK=0: a full layout packs the rows (A/B of the room behind every row)
  bool test_tight_array = false;          // FLIMO_TEST_TIGHT_ARRAY (tests): the cell-sorted array gets 4096 points of room instead of twice the map
  int test_publish_delay_ms = 0;         // FLIMO_TEST_PUBLISH_DELAY_MS (tests): a sleep between the age check of a waiting pass and the publish
  int test_publish_split_ms = 0;         // FLIMO_TEST_PUBLISH_SPLIT_MS (tests): a sleep between the two halves of the published head
  PrevPass prev_before{};                // `prev` as the pass in flight was given it (a pass that has to be launched a second time)
  // Which way the iterated update runs: the chain costs about 11 us per pass on top of the pass's kernels whatever the host (the
  // algebra launch and two dispatch boundaries); the host loop costs this host's launch -> result round trip + 2-3 us of algebra --
  // 9 us on a fast host, 15-19 us on a slow one (BENCH_r03: 5 497 scans/s where the builder's box gave 7 102).  The round trip is
  // measured once at context creation (launch_rtt_us) and REPORTED; update_mode 0 and 1 = host loop, 2 = chain (the caller's choice).
  int update_mode = 0;                   // FLIMO_HOST_UPDATE=1 -> 1, FLIMO_HOST_UPDATE=0 -> 2, unset -> 0 (flimo_set_update_mode)
  double launch_rtt_us = 0.0;            // launch -> granule seen (lower quartile) of a one-thread kernel on this host
  bool host_update = false;              // (the choice in force) flimo_update_chain always declines (the host loop runs the update; A/B)
  hipEvent_t chain_ev[CH_MAX_PASSES][8]; // per pass: [0,1] first launch, [2,3] fit launch, [4,5] algebra launch, [6,7] widening launch (lazy)
  bool chain_ev_made = false;
  double chain_alg_ms = 0;
  long long chain_alg_n = 0, chains_run = 0, chains_back = 0, chains_declined = 0;
  int fov_check = 0, fov_check_bad = 0;   // device atan2f vs this host's libm: 0 not checked yet, 1 equal, -1 different (the FoV filter is then declined)
  bool tail = true;                // FLIMO_TAIL=0: pending queries go to the worklist + widen_kernel dispatch instead of being finished inside the k-NN launch (A/B checks)
};

constexpr size_t FRAMES_FG_SLOT = 8192;             // bytes per slot of flimo_ctx::d_frames_fg (about 70 IMU frames)
static int fail(flimo_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}
#define HIPCHK(c, call)                                                                          \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) return fail(c, FLIMO_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

// Grows a pinned host buffer of the context (cap: its size in bytes) to hold `bytes`; the old contents are not kept.
static int ensure_pinned(flimo_ctx* c, void*& buf, size_t& cap, size_t bytes) {
  if (bytes <= cap) return FLIMO_OK;
  if (buf) (void)hipHostFree(buf);
  buf = nullptr;
  cap = 0;
  const size_t ncap = bytes + bytes / 4 + 4096;
  HIPCHK(c, hipHostMalloc(&buf, ncap, hipHostMallocDefault));
  cap = ncap;
  return FLIMO_OK;
}
static int ensure_stage(flimo_ctx* c, size_t bytes) { return ensure_pinned(c, c->h_stage, c->stage_cap, bytes); }

template <typename T>
static int ensure_dev(flimo_ctx* c, T*& p, size_t& cap, size_t need, bool keep, size_t keep_n) {
  if (need <= cap) return FLIMO_OK;
  size_t ncap = need + need / 4 + 1024;
  T* np = nullptr;
  HIPCHK(c, hipMalloc(&np, ncap * sizeof(T)));
  if (keep && p && keep_n) {
    HIPCHK(c, hipMemcpyAsync(np, p, keep_n * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (p) (void)hipFree(p);
  p = np;
  cap = ncap;
  return FLIMO_OK;
}

// The device scratch of one call: get<T>(count) allocates, the destructor frees whatever was got, on every exit path.  Nothing is
// kept from call to call.  A failed allocation is remembered, later ones are then not tried and return null: ok() after a group of
// them reports it.
struct DevScratch {
  std::vector<void*> got;
  hipError_t err = hipSuccess;
  DevScratch() = default;
  DevScratch(const DevScratch&) = delete;
  DevScratch& operator=(const DevScratch&) = delete;
  ~DevScratch() { for (void* p : got) (void)hipFree(p); }
  template <typename T>
  T* get(size_t count) {
    void* p = nullptr;
    if (err == hipSuccess) err = hipMalloc(&p, count * sizeof(T));
    if (err != hipSuccess) return nullptr;
    got.push_back(p);
    return static_cast<T*>(p);
  }
  void drop(void* p) {      // frees one buffer before the call ends
    got.erase(std::remove(got.begin(), got.end(), p), got.end());
    (void)hipFree(p);
  }
  int ok(flimo_ctx* c) const { return err == hipSuccess ? FLIMO_OK : fail(c, FLIMO_ERR_HIP, "hipMalloc failed: %s", hipGetErrorString(err)); }
};

// the waiting pass is told to leave (its workgroups poll the head's granules: granule 0's tag); cheap: one posted store when there
// is one, nothing otherwise
static inline void cancel_prelaunch(flimo_ctx* c) {
  if (!c->pre.active) return;
  c->pre.active = false;
  c->pipe_cancelled++;
  *reinterpret_cast<volatile unsigned long long*>(&c->d_pipe_head->gran[0]) = (unsigned long long)c->pre.end_code << 32;
  _mm_sfence();
}
// every entry point that queues work on the context's stream passes here first: nothing may line up behind a pass that waits
static inline void ctx_enter(flimo_ctx* c) {
  (void)hipSetDevice(c->device);
  cancel_prelaunch(c);
}

// every call that replaces the resident scan ends here: n points, no cell-sorted prefix yet to trust beyond them, no previous pass,
// and none of what the caller uploaded per point of the old scan (flimo_scan_cov_set)
static inline void scan_replaced(flimo_ctx* c, size_t n) {
  c->scan_n = n; c->sorted_n = n; c->prev.valid = 0;
  c->scan_cov_n = 0;
}

// defined in flimo_capi.hip, called from flimo_capi_query.hip too (hidden: the library exports nothing for them)
__attribute__((visibility("hidden"))) int ensure_index(flimo_ctx* c);
__attribute__((visibility("hidden"))) int flush_deskew(flimo_ctx* c);
__attribute__((visibility("hidden"))) int map_remove_masked(flimo_ctx* c, const unsigned char* d_mask, size_t first, size_t n, size_t marked,
                                                            uint64_t* calls, uint64_t* points, size_t* removed, const char* what);
