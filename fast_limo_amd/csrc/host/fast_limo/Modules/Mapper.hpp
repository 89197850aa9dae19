// fast_limo/Modules/Mapper.hpp -- GPU-resident map behind the reference's Mapper API
// (reference Modules/Mapper.hpp:48-71, Modules/Mapper.cpp:38-96).  The octree is replaced by the
// uniform-grid index of libflimo_hip; `match` keeps its signature for API compatibility, the
// filter itself uses the reduced seam (match_reduce) instead of materialising Matches.
#ifndef __FASTLIMO_MAPPER_HPP__
#define __FASTLIMO_MAPPER_HPP__
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>
#include <cstdint>
#include "fast_limo/Common.hpp"
#include "fast_limo/Objects/Match.hpp"
#include "fast_limo/Objects/State.hpp"
#include "fast_limo/Utils/Config.hpp"
#include "flimo_c.h"

struct flimo_ctx;

class fast_limo::Mapper {
 public:
  Matches matches;

  Mapper();
  ~Mapper();
  void set_num_threads(int n);
  void set_config(const Config::iKFoM::Mapping& cfg);
  bool exists();
  int size();
  double last_time();
  // Mapper::match (Mapper.cpp:59-86): matches of the RESIDENT scan (pc must be the cloud last
  // handed to the Localizer / set with set_scan) at state s.
  Matches match(State s, pcl::PointCloud<PointType>::Ptr& pc);
  void add(pcl::PointCloud<PointType>::Ptr& pc, double time);

  // --- MI355X additions -----------------------------------------------------------------------
  // one Mapper per GPU; getInstance() keeps the reference's process-wide singleton on device 0
  explicit Mapper(int device);
  bool attach(int device, float cell_size);     // creates the flimo_ctx; false + message on failure
  // The handle of the GPU context.  A map insert started by add_scan() may still be running on the Mapper's worker
  // thread: ctx() (like every other method of this class) waits for it first, so whoever holds the handle sees a
  // quiescent context.  Re-fetch it after each Localizer::updatePointCloud instead of caching it across scans.
  flimo_ctx* ctx() { sync(); return ctx_; }
  // A second context on the same GPU for the INPUT stage of a sweep (upload, filters, stamps, time order: nothing of it reads the
  // map): handed out WITHOUT waiting for a running insert, so that stage overlaps the previous sweep's Mapper::add; the sweep is
  // then handed over to ctx() with flimo_scan_adopt.  nullptr when it cannot be created (the caller uses ctx()).
  flimo_ctx* front_ctx();
  // Path exit of a scan (reference Localizer.cpp:361-377: transformPointCloud + Mapper::add) for the scan RESIDENT on
  // the GPU: returns at once, the insert runs on the worker thread and overlaps the host-side preparation (filters,
  // time sort) of the next scan.  FLIMO_SYNC_INSERT=1 (or set_async(false)) makes it synchronous.
  void add_scan(const double x26[26], double stamp);
  // A local map: forget the stored points outside [lo, hi] (flimo_map_crop_box; the reference's octree has no erase).  With
  // asynchronous inserts the crop runs on the same worker thread, BEHIND an insert that is running or queued: the sweep that
  // asked for it does not wait.  sync() waits for it like for an insert.
  void crop_box(const float lo[3], const float hi[3]);
  size_t last_crop_removed() { sync(); return crop_removed_; }   // points the last crop_box removed
  // Forget the stored points that the scan RESIDENT in the context looks through from `sensor` (world frame) at pose x26, and --
  // with a box (lo, hi both non-null) -- those outside it, in one pass (flimo_map_carve).  Queued like crop_box: with asynchronous
  // inserts a job on the worker thread BEHIND the insert of the sweep that asked for it, whose scan is still the resident one there.
  void carve(const double x26[26], const float sensor[3], const flimo_carve_cfg& cfg, const float* lo = nullptr, const float* hi = nullptr);
  size_t last_carve_removed() { sync(); return carve_removed_; }   // points the last carve removed
  // The stored points first .. first + n - 1 that belong to no surface, by the statistics of their k nearest neighbours
  // (flimo_map_outliers: PCL's StatisticalOutlierRemoval / RadiusOutlierRemoval): mask [n] (1 = outlier), and where a vector is
  // given mean_dist [n], cnt [n]; stats (may be null).  Changes nothing.  Returns a FLIMO_* code.
  int outliers(size_t first, size_t n, const flimo_outlier_cfg& cfg, std::vector<unsigned char>& mask, std::vector<double>* mean_dist = nullptr,
               std::vector<int32_t>* cnt = nullptr, flimo_outlier_stats* stats = nullptr);
  // ... and forget them (flimo_map_remove_outliers); afterwards the map is as after crop_box.  A whole-map statistic plus a relayout:
  // the caller's schedule decides when, so it runs at once -- after an insert, a crop or a carve still on the worker thread --
  // and is not queued.  removed / stats may be null.  Returns a FLIMO_* code.
  int remove_outliers(size_t first, size_t n, const flimo_outlier_cfg& cfg, size_t* removed = nullptr, flimo_outlier_stats* stats = nullptr);
  // The stored points first .. first + n - 1 that are ISS keypoints (flimo_map_keypoints: pcl::ISSKeypoint3D with k-bounded
  // neighbourhoods and broken ties): mask [n] (1 = keypoint), and where a vector is given saliency [n] (l0, NaN when not salient),
  // cnt [n]; count (may be null): the ones of the mask.  Changes nothing.  Returns a FLIMO_* code.
  int keypoints(size_t first, size_t n, const flimo_keypoint_cfg& cfg, std::vector<unsigned char>& mask, std::vector<double>* saliency = nullptr,
                std::vector<int32_t>* cnt = nullptr, size_t* count = nullptr);
  // The Euclidean clusters of the stored points (flimo_map_clusters: pcl::EuclideanClusterExtraction), for the stored points
  // first .. first + n - 1: where a vector is given label [n] (the smallest insertion index of the point's component), size [n],
  // mask [n] (1 = its component is selected by min_size / max_size); stats (may be null).  Changes nothing.  Returns a FLIMO_* code.
  int clusters(size_t first, size_t n, const flimo_cluster_cfg& cfg, std::vector<int32_t>* label, std::vector<int32_t>* size = nullptr,
               std::vector<unsigned char>* mask = nullptr, flimo_cluster_stats* stats = nullptr);
  // ... and forget the points of the range in selected components (flimo_map_remove_clusters); afterwards the map is as after
  // crop_box.  As remove_outliers: it runs at once and is not queued.  removed / stats may be null.  Returns a FLIMO_* code.
  int remove_clusters(size_t first, size_t n, const flimo_cluster_cfg& cfg, size_t* removed = nullptr, flimo_cluster_stats* stats = nullptr);
  // The voxels of the stored points on a lattice anchored at the world origin (flimo_map_voxels: pcl::VoxelGrid's leaves over the
  // map, float64 sums of one fixed shape): where a vector is given ijk [nv][3], count [nv], first [nv], rep [nv], centroid [nv][3],
  // cov [nv][6]; stats (may be null).  Changes nothing.  Returns a FLIMO_* code.
  int voxels(const flimo_voxel_cfg& cfg, std::vector<int32_t>* ijk, std::vector<int32_t>* count = nullptr, std::vector<int32_t>* first = nullptr,
             std::vector<int32_t>* rep = nullptr, std::vector<double>* centroid = nullptr, std::vector<double>* cov = nullptr,
             flimo_voxel_stats* stats = nullptr);
  // ... the voxel [n] and the thinning mask [n] of the stored points first .. first + n - 1 (flimo_map_voxel_mask) ...
  int voxel_mask(size_t first, size_t n, const flimo_voxel_cfg& cfg, std::vector<int32_t>* voxel, std::vector<unsigned char>* mask = nullptr,
                 flimo_voxel_stats* stats = nullptr);
  // ... and forget the masked points of the range (flimo_map_thin); afterwards the map is as after crop_box.  As remove_clusters: it
  // runs at once and is not queued.  removed / stats may be null.  Returns a FLIMO_* code.
  int thin(size_t first, size_t n, const flimo_voxel_cfg& cfg, size_t* removed = nullptr, flimo_voxel_stats* stats = nullptr);
  // The smooth-surface regions of the stored points (flimo_map_regions: pcl::RegionGrowing without its seed order), for the stored
  // points first .. first + n - 1: where a vector is given label [n] (the smallest insertion index of the region's smooth points,
  // -1: no region), size [n], mask [n] (1 = its region is selected by min_size / max_size); stats (may be null).  Changes nothing.
  // Returns a FLIMO_* code.
  int regions(size_t first, size_t n, const flimo_region_cfg& cfg, std::vector<int32_t>* label, std::vector<int32_t>* size = nullptr,
              std::vector<unsigned char>* mask = nullptr, flimo_region_stats* stats = nullptr);
  // ... the selected regions in ascending label (flimo_map_region_list): where a vector is given label [nr], count [nr], first [nr],
  // centroid [nr][3], cov [nr][6] ...
  int region_list(const flimo_region_cfg& cfg, std::vector<int32_t>* label, std::vector<int32_t>* count = nullptr, std::vector<int32_t>* first = nullptr,
                  std::vector<double>* centroid = nullptr, std::vector<double>* cov = nullptr, flimo_region_stats* stats = nullptr);
  // ... and forget the points of the range in selected regions (flimo_map_remove_regions); afterwards the map is as after crop_box.
  // As remove_clusters: it runs at once and is not queued.  removed / stats may be null.  Returns a FLIMO_* code.
  int remove_regions(size_t first, size_t n, const flimo_region_cfg& cfg, size_t* removed = nullptr, flimo_region_stats* stats = nullptr);
  // octree::Octree::radiusSearch (Objects/Octree.hpp:453-523) over the GPU map (flimo_radius_search).  The reference's Mapper hides
  // its octree, so this is an addition: the stored points with (p - query).squaredNorm() < radius * radius (strict, float32), in
  // ascending order of (distance, insertion index) -- the reference's traversal order is not reproduced.  As the template
  // (Octree.hpp:453-477): outputs untouched when the map is empty, cleared otherwise; only x, y, z of a neighbour are set.
  void radiusSearch(const PointType& query, float radius, std::vector<PointType>& neighbors, std::vector<float>& distances);
  // ... for a batch of packed xyz queries, CSR form: results of query i are [offsets[i], offsets[i + 1]) of idx (insertion
  // indices) / sqd / xyz (optional, packed).  sorted = false: an order only a change of the map changes.  Returns a FLIMO_* code.
  int radiusSearch(const float* q_xyz, size_t nq, float radius, bool sorted, std::vector<uint64_t>& offsets, std::vector<int32_t>& idx,
                   std::vector<float>& sqd, std::vector<float>* xyz = nullptr);
  // octree::Octree::knn (Objects/Octree.hpp:526-555) over the GPU map for any k up to FLIMO_KNN_MAX_K (flimo_knn_k): the k nearest
  // stored points in ascending order of (distance, insertion index) -- among exactly tied distances the reference's first-met
  // choice is not reproduced.  As the template: outputs untouched when the map is empty, cleared otherwise; only x, y, z of a
  // neighbour are set; distances are squared.
  void knn(const PointType& query, int k, std::vector<PointType>& neighbors, std::vector<float>& distances);
  // ... for a batch of packed xyz queries, with a distance gate (INFINITY: none; finite: only points with squared distance
  // < max_dist * max_dist): idx / sqd [nq][k] (-1 / 0 beyond cnt[q]), cnt [nq], xyz (optional) [nq][k][3].  Returns a FLIMO_* code.
  int knn(const float* q_xyz, size_t nq, int k, float max_dist, std::vector<int32_t>& idx, std::vector<float>& sqd, std::vector<int32_t>& cnt,
          std::vector<float>* xyz = nullptr);
  // Plane normals and covariances of the map's k-NN neighbourhoods (flimo_map_normals: what pcl::NormalEstimation computes), the
  // neighbour lists never leaving the GPU.  normal [nq][4] = nx ny nz curvature, cnt [nq]; centroid [nq][3], cov [nq][6] (xx xy xz
  // yy yz zz) and eig [nq][6] (ascending eigenvalues, the float64 normal) are filled where a vector is given.  viewpoint (may be
  // null): the normals face it.  A query with fewer than max(3, min_pts) neighbours has NaN results.  Returns a FLIMO_* code.
  int normals(const float* q_xyz, size_t nq, int k, float max_dist, int min_pts, const float* viewpoint, std::vector<float>& normal,
              std::vector<int32_t>& cnt, std::vector<double>* centroid = nullptr, std::vector<double>* cov = nullptr,
              std::vector<double>* eig = nullptr);
  // ... of the stored points first .. first + n - 1 themselves (insertion order), nothing uploaded (flimo_map_normals_range)
  int normals_range(size_t first, size_t n, int k, float max_dist, int min_pts, const float* viewpoint, std::vector<float>& normal,
                    std::vector<int32_t>& cnt, std::vector<double>* centroid = nullptr, std::vector<double>* cov = nullptr,
                    std::vector<double>* eig = nullptr);
  // How well the scan resident in this Mapper's context -- after Localizer::updatePointCloud: pc2match -- fits the map at each of np
  // pose hypotheses x26 [np][26] (flimo_scan_fitness: what pcl::Registration::getFitnessScore computes for one pose).  inliers [np]:
  // scan points whose nearest stored point is closer than max_dist (INFINITY: no gate); sum_sqd [np]: the float64 sum of their
  // squared distances; nn_sqd / nn_idx [np][scan size] (optional): that distance (-1: none) and the stored point's insertion index.
  // Returns a FLIMO_* code.
  int fitness(const double* x26, size_t np, float max_dist, std::vector<int32_t>& inliers, std::vector<double>& sum_sqd,
              std::vector<float>* nn_sqd = nullptr, std::vector<int32_t>* nn_idx = nullptr);
  // One linearisation of a point-to-plane registration of that scan at each of np pose hypotheses (flimo_scan_linearize): per pose
  // the plane of every moved scan point's k nearest stored points (gate max_dist, at least max(3, min_pts) of them, curvature at
  // most max_curv) and the sums of the 6 x 6 normal equations over the valid pairs.  valid [np]; H [np][21]: the upper triangle,
  // row-major; g [np][6]; cost [np]; rows [np][scan size][7] (optional): J0..J5, d per pair, NaN when invalid; pair_cnt
  // [np][scan size] (optional): neighbours per pair.  The step solves H xi = -g, xi = (drho, dphi) in the body frame.  Returns a
  // FLIMO_* code.
  int linearize(const double* x26, size_t np, int k, float max_dist, int min_pts, float max_curv, std::vector<int32_t>& valid,
                std::vector<double>& H, std::vector<double>& g, std::vector<double>& cost, std::vector<double>* rows = nullptr,
                std::vector<int32_t>* pair_cnt = nullptr);
  // NDT (flimo_ndt_build / flimo_scan_ndt, same arguments and results): a resident cell model of the map's voxels at cfg->leaf in one
  // of FLIMO_NDT_SLOTS slots -- a snapshot that later inserts and crops leave alone --, and per pose hypothesis the score and the 6 x 6
  // Gauss-Newton normal equations of the resident scan against it.  Both run after an insert, a crop or a carve on the worker thread
  // has ended.  Return a FLIMO_* code.
  int ndt_build(int slot, const flimo_ndt_cfg* cfg, size_t* nc = nullptr);
  int ndt(int slot, const double* x26, size_t np, int hood, double d2, int32_t* valid, int64_t* cells, double* H, double* g, double* score,
          double* terms = nullptr, int32_t* term_cell = nullptr);
  // Pose hypotheses from point correspondences (flimo_corr_poses, same arguments and results): src[i] in the body frame is dst[i] in
  // the map's; per triplet of tri the pre-rejection, the closed-form pose and the correspondences it explains.  Reads neither the map
  // nor the resident scan: it only runs on this Mapper's context (created here if there is none yet), after an insert, a crop or a
  // carve on the worker thread has ended.  Returns a FLIMO_* code.
  int corr_poses(const float* src_xyz, const float* dst_xyz, size_t m, const int32_t* tri, size_t nh, const flimo_corr_cfg* cfg,
                 int32_t* status, int32_t* inliers, double* sum_sqd, double* pose = nullptr, float* pair_sqd = nullptr);
  // The consistency graph of those correspondences and its core numbers (flimo_corr_graph, same arguments and results): which
  // pairs can be true together.  Runs under the rules of corr_poses.  Returns a FLIMO_* code.
  int corr_graph(const float* src_xyz, const float* dst_xyz, size_t m, const flimo_corr_graph_cfg* cfg, int32_t* degree, int32_t* core,
                 int32_t* max_core = nullptr, uint64_t* adj = nullptr);
  // Nearest descriptors (flimo_desc_ref_set / flimo_desc_match, same arguments and results): the reference set stays resident in
  // this Mapper's context (created here if there is none yet); neither call reads the map or the resident scan, both run after an
  // insert, a crop or a carve on the worker thread has ended.  Return a FLIMO_* code.
  int desc_ref_set(const float* desc, size_t nr, int dim);
  int desc_match(const float* q, size_t nq, int dim, int k, int32_t* idx, float* dist, int32_t* cnt);
  void sync();                                  // wait for a running insert or crop (no-op when idle)
  void set_async(bool on) { sync(); async_ = on; }
  double last_insert_seconds() { sync(); return insert_seconds_; }
  double last_handoff_time() const { return handoff_time_; }      // developer timing
  const Config::iKFoM::Mapping& config_ref() const { return config; }
  const std::string& last_error() const { return err_; }

  static Mapper& getInstance() {
    static Mapper* mapper = new Mapper();
    return *mapper;
  }

 private:
  Config::iKFoM::Mapping config;
  int num_threads_;
  flimo_ctx* ctx_;
  flimo_ctx* front_;            // the input stage's context (front_ctx())
  int normals_run(const float* q_xyz, size_t first, size_t nq, int k, float max_dist, int min_pts, const float* viewpoint,
                  std::vector<float>& normal, std::vector<int32_t>& cnt, std::vector<double>* centroid, std::vector<double>* cov,
                  std::vector<double>* eig);
  int device_;
  float cell_size_;
  std::string err_;
  // worker of add_scan()
  bool async_;
  std::thread worker_;
  std::mutex wm_;
  std::condition_variable wcv_;
  std::atomic<bool> busy_{false}, quit_{false};   // written under wm_, also polled without it (short spins before the condition-variable waits)
  bool job_insert_ = false, job_crop_ = false;    // what the worker's next round holds (both under wm_)
  double job_x_[26];
  double job_stamp_ = 0.0;
  float job_lo_[3] = {0, 0, 0}, job_hi_[3] = {0, 0, 0};
  size_t crop_removed_ = 0;
  struct CarveJob { double x26[26]; float sensor[3]; flimo_carve_cfg cfg; bool has_box = false; float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}; };
  bool job_carve_ = false;                        // (under wm_, as job_crop_)
  CarveJob carve_job_;
  size_t carve_removed_ = 0;
  void run_carve(const CarveJob& j);
  double handoff_time_ = 0.0;
  double insert_seconds_ = 0.0;
  void run_insert(const double x26[26], double stamp);
  void run_crop(const float lo[3], const float hi[3]);
  void worker_main();
  Mapper(const Mapper&) = delete;
  Mapper& operator=(const Mapper&) = delete;
};
#endif
