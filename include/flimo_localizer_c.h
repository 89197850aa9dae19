/* include/flimo_localizer_c.h -- C wrapper over the host C++ library (libfast_limo.so), i.e. over
 * fast_limo::Localizer / fast_limo::Mapper with the reference's API (Modules/Localizer.hpp:138-209,
 * Modules/Mapper.hpp:48-71).  It exists so that non-C++ callers (the Python tests and bench.py, or a
 * ROS-free replay tool) can drive the same objects the ROS wrapper would (src/main.cpp:14-95).
 * The hot-path boundary itself is include/flimo_c.h. */
#ifndef FLIMO_LOCALIZER_C_H
#define FLIMO_LOCALIZER_C_H
#include <stddef.h>
#include "flimo_c.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct flimo_loc flimo_loc;

/* hot-path subset of fast_limo::Config (Utils/Config.hpp:23-95); defaults: src/main.cpp:101-168 */
typedef struct flimo_loc_cfg {
  int NUM_MATCH_POINTS, MAX_NUM_MATCHES, MAX_NUM_PC2MATCH;
  int bucket_size;
  double MAX_DIST_PLANE, PLANE_THRESHOLD;
  float min_extent;
  int downsampling;
  int MAX_NUM_ITERS;
  int estimate_extrinsics;
  double LIMITS[23];
  double cov_gyro, cov_acc, cov_bias_gyro, cov_bias_acc;
  int time_offset, end_of_sweep, num_threads;
  float imu2baselink_t[3], imu2baselink_R[9];
  float lidar2baselink_t[3], lidar2baselink_R[9];
  float accel_bias[3], gyro_bias[3], imu_sm[9];
  /* filters (Config::Filters) */
  int voxel_active; float leaf_size;
  int crop_active; float cropBoxMin[3], cropBoxMax[3];
  int dist_active; double min_dist;
  int rate_active; int rate_value;
  int fov_active; float fov_angle;
  int sensor_type;
  /* IMU stand-still calibration (Config flags, Modules/Localizer.cpp:411-509) */
  int gravity_align, calibrate_accel, calibrate_gyro;
  double imu_calib_time;
  /* MI355X additions */
  int gpu_device;
  float gpu_cell_size;
  int debug;                   /* Config::debug (`debug` in the config yaml): keep original_scan / deskewed / matches for the caller */
} flimo_loc_cfg;

int    flimo_loc_create(const flimo_loc_cfg* cfg, flimo_loc** out);   /* Localizer::init */
void   flimo_loc_destroy(flimo_loc* L);
/* The Mapper's GPU context.  The map insert that ends a scan (reference Localizer.cpp:361-377) runs on a worker thread
 * and may still be in flight when flimo_loc_update_pointcloud* returns; this call (like every flimo_loc_* call that
 * touches the map) waits for it first.  Fetch the handle again after each scan rather than caching it. */
flimo_ctx* flimo_loc_ctx(flimo_loc* L);
void   flimo_loc_sync(flimo_loc* L);                                  /* wait for a running map insert */
void   flimo_loc_set_async_insert(flimo_loc* L, int on);              /* default on; FLIMO_SYNC_INSERT=1 turns it off */
/* default on: when no cap can bind and the voxel grid is off, the order of std::partial_sort_copy (Localizer.cpp:789-790) is not
 * observable by the registration; the GPU then gets the sweep in arrival order and the permutation is only computed for the
 * clouds handed back to the caller (set_flags download_clouds), while the GPU works.  off: always sort first. */
void   flimo_loc_set_lazy_time_order(flimo_loc* L, int on);
/* default on: NaN removal, crop box, rate and min-distance filters and the per-point stamps run on the GPU
 * (flimo_raw_scan_filter_set) whenever the arrival-order path applies and no host copies of the clouds are requested */
void   flimo_loc_set_gpu_filters(flimo_loc* L, int on);
/* default off.  A sweep whose stamps are not pairwise different (every spinning sensor: all rings of a column share one) and whose
 * time order is observable (MAX_NUM_PC2MATCH / MAX_NUM_MATCHES can bind, or the voxel grid is on): off = the device's stable
 * order, arrival order among equal stamps -- observable only as ulp-level voxel centroids and as which of several equally stamped
 * points a cap cuts off; on = the order std::partial_sort_copy leaves them in (Localizer.cpp:789-790), reproduced move for move
 * by the host front end (bit-exact against the reference's library call, 1.5 ms per 64k-point sweep). */
void   flimo_loc_set_exact_tied_order(flimo_loc* L, int on);
/* A local map, default off (the reference has no counterpart: its octree has no erase and only grows).  After the map insert of a
 * registered sweep at position p (the state's position), if no centre is set yet or max_a |p[a] - centre[a]| > recentre_dist,
 * then centre = p and the map is cropped to float(centre +- half_extent) (flimo_map_crop_box), on the insert's worker thread behind
 * the insert: the sweep does not wait for it.  half_extent[a] <= 0 on any axis, or a non-finite argument, switches the policy off.
 * Size the box as sensor range + MAX_DIST_PLANE + recentre_dist. */
void   flimo_loc_set_local_map(flimo_loc* L, const float half_extent[3], float recentre_dist);
/* The rule above as a pure host function.  centre / have_centre: the policy's state (in / out; *have_centre = 0 before the first
 * sweep).  Returns 1 when the map is to be cropped now -- centre = p, lo / hi = float(centre -+ half_extent) --, 0 when not (nothing
 * written), -1 when the arguments switch the policy off (nothing written). */
int    flimo_local_map_rule(const double p[3], const float half_extent[3], float recentre_dist, double centre[3], int* have_centre,
                            float lo[3], float hi[3]);
/* Map carving, default off (flimo_map_carve, include/flimo_c.h: forget the stored points a sweep looks through -- cars that left,
 * people who walked by).  On every every_n_sweeps-th registered sweep that is inserted into the map, a carve with that sweep's scan
 * and final state is queued on the insert's worker thread behind the insert: the sweep does not wait for it.  The sensor origin is
 * float(t + R * lidar-to-baselink translation), computed in float64 from the state (flimo_carve_sensor).  When the local-map rule
 * fires on the same sweep, ONE carve with the box is issued instead of a crop and a carve: one relayout.  every_n_sweeps <= 0, a
 * NULL cfg or one flimo_map_carve rejects switches the policy off.  Recommended: win >= 1, margin a few range sigmas. */
void   flimo_loc_set_map_carving(flimo_loc* L, int every_n_sweeps, const flimo_carve_cfg* cfg);
/* The counting rule above as a pure host function.  *count: the policy's state (in / out; 0 before the first sweep).  Called once
 * per inserted sweep: returns 1 when the map is to be carved now (*count = 0), 0 when not (*count advanced), -1 when every_n_sweeps
 * <= 0 or count is NULL (nothing written). */
int    flimo_carve_rule(int every_n_sweeps, int* count);
/* ... and the sensor origin of a state: sensor_xyz[a] = (float)(x26[a] + ((R[a][0] * l[0] + R[a][1] * l[1]) + R[a][2] * l[2])), R the
 * float64 rotation matrix of the state's attitude (x26[3..6], x y z w), l = x26[11..13] the lidar-to-baselink translation. */
void   flimo_carve_sensor(const double x26[26], float sensor_xyz[3]);
/* flimo_map_seen_through / flimo_map_carve (include/flimo_c.h: same arguments, same results, same error codes) on the map's context
 * with the scan resident there -- after updatePointCloud: pc2match --, after an insert, a crop or a carve still running behind the
 * last sweep has ended.  A Localizer that has no map yet answers like an empty one (count / removed 0). */
int    flimo_loc_map_seen_through(flimo_loc* L, const double x26[26], const float sensor_xyz[3], const flimo_carve_cfg* cfg,
                                  unsigned char* mask, size_t cap, size_t* count);
int    flimo_loc_map_carve(flimo_loc* L, const double x26[26], const float sensor_xyz[3], const flimo_carve_cfg* cfg, const float lo[3],
                           const float hi[3], size_t* removed);
/* points the last carve removed -- the policy's or flimo_loc_map_carve's (waits for one still running) */
size_t flimo_loc_last_carve_removed(flimo_loc* L);
/* flimo_map_outliers / flimo_map_remove_outliers (include/flimo_c.h: same arguments, same results, same error codes) on the map's
 * context, after an insert, a crop or a carve still running behind the last sweep has ended.  A Localizer that has no map yet
 * answers like an empty one (first = n = 0: zero counts, NaN statistics).  There is no policy that calls them: a whole-map
 * statistic plus a relayout belongs on the caller's schedule, not behind every sweep. */
int    flimo_loc_map_outliers(flimo_loc* L, size_t first, size_t n, const flimo_outlier_cfg* cfg, unsigned char* mask, double* mean_dist,
                              int32_t* cnt, flimo_outlier_stats* stats);
int    flimo_loc_map_remove_outliers(flimo_loc* L, size_t first, size_t n, const flimo_outlier_cfg* cfg, size_t* removed,
                                     flimo_outlier_stats* stats);
/* octree::Octree::radiusSearch (Objects/Octree.hpp:453-523) over the Localizer's map: flimo_radius_search (include/flimo_c.h: same
 * arguments, same results, same error codes) on the map's context, after an insert or a crop still running behind the last sweep
 * has ended.  A Localizer that has no map yet answers like an empty one (all offsets 0). */
int    flimo_loc_map_radius_search(flimo_loc* L, const float* q_xyz, size_t nq, float radius, unsigned flags, uint64_t* offsets,
                                   int32_t* idx, float* sqd, float* xyz, size_t cap, uint64_t* total);
/* octree::Octree::knn (Objects/Octree.hpp:526-555) for k up to FLIMO_KNN_MAX_K with a distance gate over the Localizer's map:
 * flimo_knn_k (include/flimo_c.h: same arguments, same results, same error codes) on the map's context, after an insert or a crop
 * still running behind the last sweep has ended.  A Localizer that has no map yet answers like an empty one (all cnt 0). */
int    flimo_loc_map_knn(flimo_loc* L, const float* q_xyz, size_t nq, int k, float max_dist, int32_t* idx, float* sqd, float* xyz,
                         int32_t* cnt);
/* Plane normals and covariances of the map's k-NN neighbourhoods over the Localizer's map: flimo_map_normals and
 * flimo_map_normals_range (include/flimo_c.h: same arguments, same results, same error codes) on the map's context, after an insert
 * or a crop still running behind the last sweep has ended.  A Localizer that has no map yet answers like an empty one (all cnt 0,
 * NaN results; a range other than first = 0, n = 0 lies beyond it). */
int    flimo_loc_map_normals(flimo_loc* L, const float* q_xyz, size_t nq, int k, float max_dist, int min_pts, const float viewpoint[3],
                             float* normal, int32_t* cnt, double* centroid, double* cov, double* eig);
int    flimo_loc_map_normals_range(flimo_loc* L, size_t first, size_t n, int k, float max_dist, int min_pts, const float viewpoint[3],
                                   float* normal, int32_t* cnt, double* centroid, double* cov, double* eig);
/* FPFH descriptors of the Localizer's stored points: flimo_map_fpfh (include/flimo_c.h: same arguments, same results, same error
 * codes) on the map's context, after an insert, a crop or a carve still running behind the last sweep has ended.  A Localizer that
 * has no map yet answers like an empty one (first = n = 0: nothing touched; any other range lies beyond it).  The Localizer's own
 * update does not use it. */
int    flimo_loc_map_fpfh(flimo_loc* L, size_t first, size_t n, const flimo_fpfh_cfg* cfg, float* fpfh, uint8_t* spfh, int32_t* cnt);
/* ISS keypoints of the Localizer's stored points: flimo_map_keypoints (include/flimo_c.h: same arguments, same results, same error
 * codes) on the map's context, after an insert, a crop or a carve still running behind the last sweep has ended.  A Localizer that
 * has no map yet answers like an empty one (first = n = 0: *count = 0; any other range lies beyond it).  The Localizer's own update
 * does not use it. */
int    flimo_loc_map_keypoints(flimo_loc* L, size_t first, size_t n, const flimo_keypoint_cfg* cfg, unsigned char* mask, double* saliency,
                               int32_t* cnt, size_t* count);
/* Euclidean clusters of the Localizer's stored points: flimo_map_clusters / flimo_map_remove_clusters (include/flimo_c.h: same
 * arguments, same results, same error codes) on the map's context, after an insert, a crop or a carve still running behind the
 * last sweep has ended.  A Localizer that has no map yet answers like an empty one (first = n = 0: every count 0; any other range
 * lies beyond it).  There is no policy that calls them: a whole-map relayout belongs on the caller's schedule, as for the outliers. */
int    flimo_loc_map_clusters(flimo_loc* L, size_t first, size_t n, const flimo_cluster_cfg* cfg, int32_t* label, int32_t* size,
                              unsigned char* mask, flimo_cluster_stats* stats);
int    flimo_loc_map_remove_clusters(flimo_loc* L, size_t first, size_t n, const flimo_cluster_cfg* cfg, size_t* removed,
                                     flimo_cluster_stats* stats);
/* RANSAC planes of the Localizer's stored points: flimo_map_planes / flimo_map_plane_mask / flimo_map_remove_plane
 * (include/flimo_c.h: same arguments, same results, same error codes) on the map's context, after an insert, a crop or a carve
 * still running behind the last sweep has ended.  A Localizer that has no map yet answers like an empty one (nh = 0, first = n = 0:
 * FLIMO_OK; anything else lies beyond it).  There is no policy that calls them. */
int    flimo_loc_map_planes(flimo_loc* L, const int32_t* tri, size_t nh, const flimo_plane_cfg* cfg, int32_t* status, int32_t* inliers,
                            double* sum_sq, double* plane);
int    flimo_loc_map_plane_mask(flimo_loc* L, size_t first, size_t n, const flimo_plane_sel* sel, unsigned char* mask, size_t* count);
int    flimo_loc_map_remove_plane(flimo_loc* L, size_t first, size_t n, const flimo_plane_sel* sel, size_t* removed);
/* Voxel statistics and thinning of the Localizer's stored points: flimo_map_voxels / flimo_map_voxel_mask / flimo_map_thin
 * (include/flimo_c.h: same arguments, same results, same error codes) on the map's context, after an insert, a crop or a carve
 * still running behind the last sweep has ended.  A Localizer that has no map yet answers like an empty one (first = n = 0:
 * FLIMO_OK, *nv = 0, stats 0; anything else lies beyond it).  There is no policy that calls them. */
int    flimo_loc_map_voxels(flimo_loc* L, const flimo_voxel_cfg* cfg, size_t cap, size_t* nv, int32_t* ijk, int32_t* count, int32_t* first,
                            int32_t* rep, double* centroid, double* cov, flimo_voxel_stats* stats);
int    flimo_loc_map_voxel_mask(flimo_loc* L, size_t first, size_t n, const flimo_voxel_cfg* cfg, int32_t* voxel, unsigned char* mask,
                                flimo_voxel_stats* stats);
int    flimo_loc_map_thin(flimo_loc* L, size_t first, size_t n, const flimo_voxel_cfg* cfg, size_t* removed, flimo_voxel_stats* stats);
/* Smooth-surface regions of the Localizer's stored points: flimo_map_regions / flimo_map_region_list / flimo_map_remove_regions
 * (include/flimo_c.h: same arguments, same results, same error codes) on the map's context, after an insert, a crop or a carve
 * still running behind the last sweep has ended.  A Localizer that has no map yet answers like an empty one (first = n = 0:
 * FLIMO_OK, *nr = 0, stats 0; any other range lies beyond it).  There is no policy that calls them: which regions to forget, and
 * when, is the caller's schedule. */
int    flimo_loc_map_regions(flimo_loc* L, size_t first, size_t n, const flimo_region_cfg* cfg, int32_t* label, int32_t* size,
                             unsigned char* mask, flimo_region_stats* stats);
int    flimo_loc_map_region_list(flimo_loc* L, const flimo_region_cfg* cfg, size_t cap, size_t* nr, int32_t* label, int32_t* count,
                                 int32_t* first, double* centroid, double* cov, flimo_region_stats* stats);
int    flimo_loc_map_remove_regions(flimo_loc* L, size_t first, size_t n, const flimo_region_cfg* cfg, size_t* removed,
                                    flimo_region_stats* stats);
/* Pose hypotheses from point correspondences: flimo_corr_poses (include/flimo_c.h: same arguments, same results, same error
 * codes) on the map's context, after an insert, a crop or a carve still running behind the last sweep has ended.  Neither the map
 * nor the resident scan is read; a Localizer that has no context yet creates it.  The Localizer's own update does not use it. */
int    flimo_loc_corr_poses(flimo_loc* L, const float* src_xyz, const float* dst_xyz, size_t m, const int32_t* tri, size_t nh,
                            const flimo_corr_cfg* cfg, int32_t* status, int32_t* inliers, double* sum_sqd, double* pose, float* pair_sqd);
/* The consistency graph of correspondences and its core numbers: flimo_corr_graph (include/flimo_c.h: same arguments, same results,
 * same error codes) on the map's context, under the rules of flimo_loc_corr_poses.  The Localizer's own update does not use it. */
int    flimo_loc_corr_graph(flimo_loc* L, const float* src_xyz, const float* dst_xyz, size_t m, const flimo_corr_graph_cfg* cfg,
                            int32_t* degree, int32_t* core, int32_t* max_core, uint64_t* adj);
/* Nearest descriptors: flimo_desc_ref_set / flimo_desc_match (include/flimo_c.h: same arguments, same results, same error codes) on
 * the map's context, after an insert, a crop or a carve still running behind the last sweep has ended.  The reference set stays
 * resident there (flimo_desc_ref_size(flimo_loc_ctx(L)) tells its size); neither the map nor the resident scan is read; a Localizer
 * that has no context yet creates it.  The Localizer's own update does not use them. */
int    flimo_loc_desc_ref_set(flimo_loc* L, const float* desc, size_t nr, int dim);
int    flimo_loc_desc_match(flimo_loc* L, const float* q, size_t nq, int dim, int k, int32_t* idx, float* dist, int32_t* cnt);
/* How well the scan resident in the map's context -- after updatePointCloud: pc2match -- fits the Localizer's map at each of np pose
 * hypotheses: flimo_scan_fitness (include/flimo_c.h: same arguments, same results, same error codes; n = the size of pc2match) on
 * the map's context, after an insert or a crop still running behind the last sweep has ended.  A Localizer that has no map yet
 * answers like an empty scan (all inliers and sums 0; nn_sqd / nn_idx have no element). */
int    flimo_loc_scan_fitness(flimo_loc* L, const double* x26, size_t np, float max_dist, int32_t* inliers, double* sum_sqd, float* nn_sqd,
                              int32_t* nn_idx);
/* One linearisation of a point-to-plane registration of that scan against the Localizer's map, per pose hypothesis:
 * flimo_scan_linearize (include/flimo_c.h: same arguments, same results, same error codes) on the map's context, after an insert
 * or a crop still running behind the last sweep has ended.  A Localizer that has no map yet answers like an empty scan (all sums and
 * valid 0; rows / pair_cnt have no element).  The Localizer's own update does not use it. */
int    flimo_loc_scan_linearize(flimo_loc* L, const double* x26, size_t np, int k, float max_dist, int min_pts, float max_curv, int32_t* valid,
                                double* H, double* g, double* cost, double* rows, int32_t* pair_cnt);
/* NDT against the Localizer's map (the reference has no counterpart): flimo_ndt_build / flimo_ndt_cells / flimo_ndt_info /
 * flimo_ndt_clear / flimo_scan_ndt (include/flimo_c.h: same arguments, same results, same error codes) on the map's context, after an
 * insert, a crop or a carve still running behind the last sweep has ended.  The models are snapshots: the sweeps' inserts and the
 * local map's crops leave them alone and flimo_ndt_info reports them stale.  A Localizer that has no map yet builds an empty model.
 * The Localizer's own update does not use them. */
int    flimo_loc_ndt_build(flimo_loc* L, int slot, const flimo_ndt_cfg* cfg, size_t* nc);
int    flimo_loc_ndt_cells(flimo_loc* L, int slot, size_t cap, size_t* nc, int32_t* ijk, int32_t* count, double* mean, double* evec, double* wgt,
                           double* eval);
int    flimo_loc_ndt_info(flimo_loc* L, int slot, flimo_ndt_model_info* info);
int    flimo_loc_ndt_clear(flimo_loc* L, int slot);
int    flimo_loc_scan_ndt(flimo_loc* L, int slot, const double* x26, size_t np, int hood, double d2, int32_t* valid, int64_t* cells, double* H,
                          double* g, double* score, double* terms, int32_t* term_cell);
/* GICP against the Localizer's map (the reference has no counterpart): flimo_gicp_build / flimo_gicp_model / flimo_gicp_info /
 * flimo_gicp_clear / flimo_scan_cov_set / flimo_scan_gicp (include/flimo_c.h: same arguments, same results, same error codes) on the
 * map's context, after an insert, a crop or a carve still running behind the last sweep has ended.  The model is a snapshot of the
 * stored points by insertion index: a sweep's insert or a local map's crop makes it stale, and flimo_scan_gicp then answers
 * FLIMO_ERR_NOMAP until it is rebuilt; every sweep replaces the resident scan and so drops its covariances
 * (flimo_scan_cov_size(flimo_loc_ctx(L)) tells how many there are).  The Localizer's own update does not use them. */
int    flimo_loc_gicp_build(flimo_loc* L, const flimo_gicp_cfg* cfg, size_t* n_cov);
int    flimo_loc_gicp_model(flimo_loc* L, size_t first, size_t n, double* cov);
int    flimo_loc_gicp_info(flimo_loc* L, flimo_gicp_model_info* info);
int    flimo_loc_gicp_clear(flimo_loc* L);
int    flimo_loc_scan_cov_set(flimo_loc* L, const double* cov6, size_t n);
int    flimo_loc_scan_gicp(flimo_loc* L, const double* x26, size_t np, float max_dist, int32_t* valid, double* H, double* g, double* cost,
                           int32_t* pair_idx, double* pair_m);
/* Scan Context on the Localizer's map context (the reference's loop/scancontext branch has it beside the Localizer, not in it):
 * flimo_scan_context / flimo_sc_db_add / flimo_sc_db_add_scan / flimo_sc_db_get / flimo_sc_db_clear / flimo_sc_match
 * (include/flimo_c.h: same arguments, same results, same error codes), after an insert, a crop or a carve still running behind
 * the last sweep has ended.  The resident scan is the last sweep's; the database stays on the map's context
 * (flimo_sc_db_size(flimo_loc_ctx(L)) tells its size) and no insert, crop or clear of the map touches it.  The Localizer's own
 * update does not use it. */
int    flimo_loc_scan_context(flimo_loc* L, const flimo_sc_cfg* cfg, const float* frame12, float* desc, int32_t* used);
int    flimo_loc_sc_db_add(flimo_loc* L, const float* desc, size_t n, int rings, int sectors, size_t* first_id);
int    flimo_loc_sc_db_add_scan(flimo_loc* L, const flimo_sc_cfg* cfg, const float* frame12, size_t* id);
int    flimo_loc_sc_db_get(flimo_loc* L, size_t first, size_t n, float* desc);
int    flimo_loc_sc_db_clear(flimo_loc* L);
int    flimo_loc_sc_match(flimo_loc* L, const float* q, size_t nq, int rings, int sectors, size_t first, size_t n,
                          const flimo_sc_match_cfg* cfg, int32_t* idx, float* dist, int32_t* shift, int32_t* cnt, float* profile);
/* Map segments on the Localizer's map (the reference has no loop closure): flimo_map_segment_mark / flimo_map_segments /
 * flimo_map_segments_reset / flimo_map_corrected / flimo_map_correct / flimo_map_transform / flimo_map_remove_range
 * (include/flimo_c.h: same arguments, same results, same error codes) on the map's context, after an insert, a crop or a carve
 * still running behind the last sweep has ended -- so a mark lands behind the last sweep's points.  The local map's crops and the
 * carving policy make the table stale like any removal.  THE FILTER'S POSE IS THE CALLER'S TO SET after a correction
 * (flimo_loc_set_x): the map moved, the state did not.  There is no policy that calls them. */
int    flimo_loc_map_segment_mark(flimo_loc* L, size_t* id);
int    flimo_loc_map_segments(flimo_loc* L, uint64_t* begin, size_t cap, size_t* n_seg, int* stale);
int    flimo_loc_map_segments_reset(flimo_loc* L);
int    flimo_loc_map_corrected(flimo_loc* L, const double* T, size_t n_seg, size_t first, size_t n, float* xyz, size_t* changed);
int    flimo_loc_map_correct(flimo_loc* L, const double* T, size_t n_seg, size_t* changed);
int    flimo_loc_map_transform(flimo_loc* L, const double T[12], size_t* changed);
int    flimo_loc_map_remove_range(flimo_loc* L, size_t first, size_t n, size_t* removed);
int    flimo_loc_last_sweep_tied(const flimo_loc* L);      /* 1: the last sweep of the device front end had equal stamps */
/* how long updatePointCloud waits for the IMU stream to reach the end of the sweep (Localizer::propagatedFromTimeRange,
 * Localizer.cpp:855-871).  The reference waits on its condition variable without bound, and so does fast_limo::Localizer used
 * through its C++ header (seconds < 0).  Handles made by flimo_loc_create start with 1 s, because their callers usually feed IMU
 * and sweeps from ONE thread, where an unbounded wait could never be satisfied. */
void   flimo_loc_set_propagation_wait(flimo_loc* L, double seconds);
double flimo_loc_last_insert_seconds(flimo_loc* L);                   /* duration of the last insert (waits for it) */
int    flimo_loc_update_imu(flimo_loc* L, double stamp, const float ang_vel[3], const float lin_accel[3]);
/* n samples in arrival order, one updateIMU each (a binding whose per-call cost matters -- ctypes: 25 us -- hands over the samples
 * between two sweeps at once) */
int    flimo_loc_update_imu_n(flimo_loc* L, size_t n, const double* stamps, const float* ang_vel3, const float* lin_accel3);
/* A recorded drive replayed at full speed from native code: before sweep k every IMU sample with stamp <= imu_until[k] goes to
 * updateIMU, then the sweep (PointType records, as flimo_loc_update_pointcloud_points takes them) to updatePointCloud.
 * status_out[k]: that sweep's status; seconds_out[k] (or NULL): when its call returned, since the start of the replay. */
int    flimo_loc_replay(flimo_loc* L, size_t n_sweeps, const void* const* sweeps32, const size_t* n_points, const double* sweep_stamps,
                        const double* imu_until, size_t n_imu, const double* imu_stamps, const float* ang_vel3, const float* lin_accel3,
                        int* status_out, double* seconds_out);
/* pts5: n x (x y z intensity time[s since sweep reference]).  Returns Localizer status:
 * 0 ok, 1 null iteration, <0 early return */
int    flimo_loc_update_pointcloud(flimo_loc* L, const float* pts5, size_t n, double stamp);
/* The same with points in the reference's PointType layout (Common.hpp:100-113): float x, y, z, w; float intensity;
 * 4 bytes of padding; 8-byte time union {uint32 t (OUSTER ns) | float time (VELODYNE s) | double timestamp
 * (HESAI s, LIVOX ns)} -- the view that is read follows flimo_loc_cfg.sensor_type. */
int    flimo_loc_update_pointcloud_points(flimo_loc* L, const void* points32, size_t n, double stamp);
int    flimo_loc_map_add(flimo_loc* L, const float* xyz, size_t n, double stamp);   /* Mapper::add */
size_t flimo_loc_map_size(flimo_loc* L);
void   flimo_loc_get_x(flimo_loc* L, double x26[26]);
void   flimo_loc_set_x(flimo_loc* L, const double x26[26]);
void   flimo_loc_get_P(flimo_loc* L, double P[529]);
void   flimo_loc_set_P(flimo_loc* L, const double P[529]);
void   flimo_loc_set_flags(flimo_loc* L, int add_to_map, int download_clouds, int keep_log);
int    flimo_loc_num_passes(flimo_loc* L);
void   flimo_loc_get_pass(flimo_loc* L, int i, int* M, double* HTH, double* HTh, double* dx, double* x_after);
size_t flimo_loc_get_pc2match(flimo_loc* L, float* xyz_out, size_t cap);
size_t flimo_loc_get_final_scan(flimo_loc* L, float* xyz_out, size_t cap);
/* The clouds Localizer keeps under config.debug (flimo_loc_cfg.debug), as full 32-byte PointType records: which = 0
 * get_orig_pointcloud() (the filtered sweep, LiDAR frame), 1 get_deskewed_pointcloud() (the sweep in time order, each point
 * deskewed into the world frame), 2 get_finalraw_pointcloud() (the un-voxelised deskewed sweep in the world frame of the corrected
 * pose).  Copies min(n, cap) records to points32_out (may be NULL when cap = 0) and returns n; (size_t)-1 for another `which`. */
size_t flimo_loc_get_debug_cloud(flimo_loc* L, int which, void* points32_out, size_t cap);
void   flimo_loc_get_stage_times(flimo_loc* L, double t[4]);
void   flimo_loc_get_pose_cov(flimo_loc* L, double cov36[36]);       /* getPoseCovariance */
/* host-side profile of register_resident: seconds in deskew call, whole update, flimo_match_reduce; passes */
void   flimo_loc_host_profile(flimo_loc* L, double out[4], int reset);
/* benchmark step: restore the prior (x26, P) and re-register the resident raw scan
 * (GPU deskew + iterated update) */
int    flimo_loc_register_resident(flimo_loc* L, const double x26_prior[26], const double P_prior[529]);
/* fast_limo::State::update (State.cpp:76-119) on a flat state p3 q4(xyzw) v3 g3 w3 a3 bg3 ba3 -- for unit tests */
void   flimo_host_state_update(float s[25], double time, double t);
/* fast_limo::Plane + Match object API in isolation (Plane.cpp:23-31, Match.cpp:23-28): returns good_fit(), the normal
 * (zeros when not a plane) and Match(p_global, ., plane).dist -- for unit tests */
/* Order in which Localizer::deskewPointCloud's std::partial_sort_copy (Localizer.cpp:789-790) leaves a sweep, ties included.
 * kind: 0 uint32 (OUSTER), 1 float (VELODYNE), 2 double (HESAI/LIVOX); use_library=1 runs the library call itself (tests). */
int    flimo_host_time_order(const void* keys, int kind, size_t n, int descending, int use_library, uint32_t* order_out);
int    flimo_host_plane(const float* xyz, const float* sqd, int n, int num_match_points, double max_dist_plane,
                        double plane_threshold, const float p_global[3], float n_out[4], float* dist_out);
/* IESKF algebra in isolation with a fixed measurement (H [M][12], h [M]) -- for unit tests */
int    flimo_eskf_update_fixed(double x26[26], double P[529], const double* H, const double* h, int M, int max_iters,
                               const double limits[23], double R, double D, int* n_passes);
int    flimo_eskf_predict(double x26[26], double P[529], double dt, const double Qdiag[12], const double acc[3],
                          const double gyro[3]);
/* Host twins of the device filter's developer entries (include/flimo_dev.h) -- for unit tests.
 * flimo_ieskf_gj12_host: the host filter's own elimination, flimo_host::inverse_gj / solve_gj with n = 12; op, in, out as
 * flimo_ieskf_eval takes FLIMO_IK_GJ12_INVERSE (7) / FLIMO_IK_GJ12_SOLVE (8).
 * flimo_ieskf_run_fixed_host: flimo_ieskf_run_fixed on flimo_host::Esekf, h_reduced returning the same sets, the eight partials
 * added in slot order.  log_out [max_iter + 1][207]: per completed pass M, HTH[144], HTh[12], dx[23], x_after[26] and the filter's own
 * count t of the passes that met `limits` so far, this one included (esekfom.hpp:1749-1757); *n_log passes;
 * loop[3]: the iteration the loop ended in, t then, passes. */
int    flimo_ieskf_gj12_host(int op, const double* in, size_t n, double* out);
int    flimo_ieskf_run_fixed_host(const double x26[26], const double P[529], const double limits[23], double R, double D,
                                  int max_iter, int n_sets, const double* partials, double* log_out, int* n_log, double x_out[26],
                                  double P_out[529], int loop[3]);
/* The filter's restatement of Eigen::EigenSolver<Matrix<double,6,6>> (IKFoM_toolkit/esekfom/esekfom.hpp:1736-1738, degeneracy
 * handling): A row-major; eigenvalues in the solver's order (real, imaginary part), real parts of the normalised eigenvectors as
 * the columns of V (row-major) -- for unit tests */
void   flimo_host_eigen_solver6(const double A[36], double wr[6], double wi[6], double V[36]);

#ifdef __cplusplus
}
#endif
#endif
