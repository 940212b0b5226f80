// lidar_odometry.h — host-side drop-in for the reference's odometry facade.
//
// Public surface identical to the reference's src/odometry/lidar_odometry.h:11-25
//     LidarOdometry();  void AddImuData(const ImuData&);  void AddLidarScan(const pcl::PointCloud<hilti_ros::Point>::Ptr&);
// so that src/wildcat_slam_node.cc (:42, :51, :66) compiles against it unchanged where ROS / PCL exist.  Everything the
// reference does between lidar_odometry.cc:520 and :566 (sweep undistortion, surfel extraction, surfel pose update, correspondence,
// factor construction, the Ceres solve) goes through the C-ABI of libwildcat_hip.so; the window bookkeeping around it
// (point pre-filter :489-496, SyncHeadingMsgs :457-485, PredictImuStatesAndSampleStates :365-455, BuildSweep :134-141,
// UpdateImuPoses + B-spline corrector :22-54,:187-215, UpdateSamplePoses :172-179,
// ShrinkToFit :228-250) is restated here as plain host C++.  All state is per instance (the reference keeps some of it
// in function-local statics).  ROS publishing is replaced by the accessors at the bottom.
#pragma once
#include <cstdint>
#include <deque>
#include <memory>
#include <string>
#include <vector>

#ifndef WC_HAVE_REFERENCE_TYPES
#include "shim/common.h"
#endif
#include "../../include/wildcat_hip.h"
#include "lio_config.h"
#include "wire_formats.h"

// the wc_params a configuration stands for (needs no context): wc_params_default with the IMU cost weights of lio_config.h:42-45 formed
// from c's noise model, imu_rate and imu_factor_weight, imu_dt = 1 / imu_rate, max_iterations = inner_iter_num_max and the two switches
void WcParamsFromConfig(const LioConfig &c, wc_params *P);

class LidarOdometry {
 public:
  LidarOdometry();
  explicit LidarOdometry(int device);
  ~LidarOdometry();
  LidarOdometry(const LidarOdometry &) = delete;
  LidarOdometry &operator=(const LidarOdometry &) = delete;

  /** Add raw imu measurements to queue (lidar_odometry.h:14-18) */
  void AddImuData(const ImuData &msg);
  /** Add raw lidar points with timestamp (lidar_odometry.h:20-25) */
  void AddLidarScan(const pcl::PointCloud<hilti_ros::Point>::Ptr &msg);

  // ---- not in the reference: read-outs instead of ROS topics / TF (lidar_odometry.cc:582-602) ----
  struct SampleStateView {
    double timestamp;
    double pos[3];
    double quat[4];  // w, x, y, z
    double bg[3], ba[3];
  };
  int sweeps_done() const { return sweep_id_; }
  bool latest_state(SampleStateView *out) const;
  size_t num_sample_states() const { return samples_.size(); }
  bool sample_state(size_t i, SampleStateView *out) const;
  size_t sliding_window_surfels() const { return n_surfels_ - sld_begin_; }
  size_t fixed_window_surfels() const { return fix_end_ - fix_start_; }
  // timestamps of the fixed window in its own order (newest first, like the reference's deque after push_front, Q11)
  const std::deque<double> &fixed_window_times() const { return fix_times_; }
  const wc_solve_summary &last_solve() const { return last_summary_; }
  // wall time [ms] of the last completed sweep's stages: predict + undistort, extract + poses, match, build, solve, update, shrink
  const double *last_stage_ms() const { return last_stage_ms_; }
  int last_lm_iterations() const { return last_lm_iterations_; }
  // wall time [ms] the message that completed the last sweep spent in front of the stages: upload + pre-filter of its points
  // (AppendScanOnDevice) and the heading synchronisation
  double last_append_ms() const { return last_append_ms_; }
  uint64_t last_correspondences(int which) const { return last_corr_[which]; }
  // test hook: keep, for the last completed sweep's last outer iteration, the two surfel timestamps of every correspondence
  // (which = 0: sliding window, 1: fixed window) - what a comparison with another run can match pairs on when surfel ORDER differs
  void set_keep_pair_stamps(bool on) { keep_pair_stamps_ = on; }
  const std::vector<double> &last_pair_stamps(int which) const { return pair_stamps_[which]; }
  // sweeps whose extraction was completed by the default (integer-moment) path / by the reference-order path (configured, or
  // fallen back to because a gate lay inside the reference's own rounding noise)
  int sweeps_fast_path() const { return sweeps_fast_; }
  int sweeps_exact_path() const { return sweeps_exact_; }
  // what the reference publishes after a sweep (lidar_odometry.cc:582-602), as plain data (config().fill_outputs)
  struct SweepOutputs {
    std::vector<wc_wire::SurfelMarker> markers;  // PubSurfels(surfels_sld_win_) (:582), one SPHERE per sliding-window surfel
    wc_wire::PointCloud2 scan_in_world;          // the sweep undistorted with the final IMU poses (:584-595), frame "world"
    double scan_stamp = 0;                       // msg.header.stamp = time of the sweep's first point (:592)
    wc_wire::StampedTransform tf{};              // world -> imu_link at the last sample state (:596-602)
  };
  const SweepOutputs &last_outputs() const { return outputs_; }
  // the residual histograms of the last completed sweep (config().log_residual_histograms; lidar_odometry.cc:56-94)
  const std::string &last_residual_log() const { return residual_log_; }
  // the accumulated, voxel-downsampled map (config().map_voxel_size > 0): every sweep undistorted with its final poses - the points
  // of last_outputs().scan_in_world - goes into a hash table in HBM (wc_map_*, DownSamplingVoxel over all sweeps).  The counts wait
  // for the device; 0 without a map
  bool SetMapVoxel(double voxel);  // config().map_voxel_size = voxel, the map re-created empty (0: removed); false: voxel out of range
  uint64_t map_voxels() const;
  uint64_t map_points() const;
  uint64_t map_rejected() const;  // points with a non-finite coordinate or a voxel index beyond 2^20 (not inserted)
  // centroids (n x 3 floats) and point counts in ascending voxel-index order; returns n, writes nothing when cap < n
  size_t ExportMap(float *xyz, uint32_t *counts, size_t cap);
  void ClearMap();
  // nearest map voxel of n host points (xyz: n x 3 floats) within max_dist (> 0, may be +inf): hits[n] as wc_map_nearest defines them;
  // returns the number found.  Without a map: 0, every hit a miss
  size_t QueryMap(const float *xyz, size_t n, double max_dist, wc_map_hit *hits);
  // wc_map_knn for n host points (xyz: n x 3 floats): hits[n * p.k], within[n] (may be null); returns the number of queries with a
  // neighbour (as QueryMap).  Without a map: 0, every record a miss and every count 0.  Parameters the library would refuse (k outside
  // 1 .. 16 among them, so the size of hits is unknown): 0, nothing written
  size_t QueryMapKnn(const float *xyz, size_t n, const wc_map_knn_params &p, wc_map_hit *hits, uint32_t *within);
  // drops the voxels that do not intersect the box [lo, hi] and compacts the table (wc_map_crop); returns the voxels removed
  size_t CropMap(const double lo[3], const double hi[3]);
  // config().map_surfels = on, the map re-created empty (as SetMapVoxel does)
  void SetMapSurfels(bool on);
  // the map's voxels as wc_map_export_surfels writes them (the order and number of ExportMap); returns the number of voxels, nothing
  // written when cap is too small.  Without a map, or with map_surfels off: 0
  size_t ExportMapSurfels(wc_map_surfel *surfels, size_t cap);
  // wc_map_nearest_plane for n host points (xyz: n x 3 floats): hits[n]; returns the number of voxels found (as QueryMap).  Without a
  // map, with map_surfels off or min_points < 3: 0, every hit a miss
  size_t QueryMapPlanes(const float *xyz, size_t n, double max_dist, uint32_t min_points, wc_map_plane_hit *hits);
  // registration of n host points (xyz: n x 3 floats) against the map's planes (wc_map_align): T_io (row-major 3 x 4) in, the aligned
  // pose out, *summary (may be null) as wc_map_align leaves it.  false - nothing touched - without a map, with map_surfels off, or when
  // the library refuses the arguments.  Nothing in AddLidarScan calls it
  bool AlignToMap(const float *xyz, size_t n, double T_io[12], const wc_map_align_opts &opts, wc_map_align_summary *summary);
  // registration of a RAW sweep in continuous time (wc_map_align_ct): n 48-byte point records on the host, in the body frame, with stamps;
  // pose_begin_io is the body -> map pose at the sweep's smallest finite stamp, pose_end_io at its largest (the two stamp bounds of the
  // call); the aligned poses out, *summary (may be null) as wc_map_align_ct leaves it.  insert: the registered sweep - the moved points
  // wc_map_linearize_ct writes at the final poses - is inserted into the map.  false - nothing touched - where AlignToMap returns false,
  // for n = 0, and for a sweep whose finite stamps do not span an interval.  Nothing in AddLidarScan calls it
  bool AlignSweepToMap(const void *points48, size_t n, wc_pose *pose_begin_io, wc_pose *pose_end_io, const wc_map_ct_align_opts &opts,
                       wc_map_ct_align_summary *summary, bool insert);
  // AlignToMap from a rough pose, coarse to fine: levels 1 .. n_levels - 1 are built from the map by chained wc_map_coarsen(factor) - level
  // l has voxel size (double)factor * that of level l - 1 -, the pyramid (wc_map_align_pyramid_batch with this one start: byte for byte
  // wc_map_align_pyramid, whose error is the start's status) runs them coarsest first and the map itself last, each with
  // `finest` except reg.max_dist, which is multiplied by (double)factor^l; then the built levels are destroyed.  summaries (may be null):
  // n_levels records, coarsest first.  Nothing is cached: the levels are rebuilt per call (a relocalisation is rare; DESIGN 8.9 has the
  // cost).  false - nothing touched - where AlignToMap returns false, for factor < 1, n_levels outside 1 .. 8, and when a level's voxel
  // size would exceed 4.0.  Nothing in AddLidarScan calls it
  bool RelocalizeToMap(const float *xyz, size_t n, double T_io[12], uint32_t factor, uint32_t n_levels, const wc_map_align_opts &finest,
                       wc_map_align_summary *summaries);
  // RelocalizeToMap when the heading is unknown: n_yaw starts T_k = (Rz(2 pi k / n_yaw) R | t) of T_io (wc_pose_yaw_grid), all of them through
  // the levels RelocalizeToMap builds in ONE wc_map_align_pyramid_batch, the winner chosen by wc_map_align_best on the finest level with
  // finest.min_used; T_io becomes the winner's pose and the built levels are destroyed.  summaries (may be null): n_levels x n_yaw records,
  // level-major, coarsest first; best (may be null): the winner's index.  false - nothing touched - where RelocalizeToMap returns false, for
  // n_yaw outside 1 .. 1024, and when no hypothesis is eligible.  n_yaw = 1 gives RelocalizeToMap's pose byte for byte.  Nothing in
  // AddLidarScan calls it
  bool RelocalizeSearch(const float *xyz, size_t n, double T_io[12], uint32_t n_yaw, uint32_t factor, uint32_t n_levels,
                        const wc_map_align_opts &finest, wc_map_align_summary *summaries, int32_t *best);
  // RelocalizeToMap when neither heading nor position is known: the levels RelocalizeToMap builds; the n_yaw x n_xyz[0] x n_xyz[1] x n_xyz[2]
  // poses wc_pose_grid makes around T_io (spacing step, world axes); wc_map_score_batch of all of them on the COARSEST level with
  // min_points = 1; the top_m best by wc_map_score_top (min_hit = finest.min_used) through ONE wc_map_align_pyramid_batch in rank order; the
  // winner by wc_map_align_best on the finest level with finest.min_used; T_io becomes its pose and the built levels are destroyed.
  // summaries (may be null): n_levels x top_m records, level-major, coarsest first, in rank order (zero where fewer candidates were
  // eligible); best (may be null): the winner's rank.  false - nothing touched - where RelocalizeToMap returns false, for top_m outside
  // 1 .. 1024, for a grid wc_pose_grid or wc_map_score_batch refuses, and when no candidate or no aligned hypothesis is eligible.  A
  // 1 x (1, 1, 1) grid with top_m = 1 and an eligible start gives RelocalizeToMap's pose byte for byte.  Nothing in AddLidarScan calls it
  bool RelocalizeGlobal(const float *xyz, size_t n, double T_io[12], uint32_t n_yaw, const uint32_t n_xyz[3], const double step[3], uint32_t top_m,
                        uint32_t factor, uint32_t n_levels, const wc_map_align_opts &finest, wc_map_align_summary *summaries, int32_t *best);
  // one linearisation at T (wc_map_linearize): *out, and rows[n] when rows is not null; false as AlignToMap
  bool LinearizeAgainstMap(const float *xyz, size_t n, const double T[12], const wc_map_reg_params &params, wc_map_normal_eq *out,
                           wc_map_reg_row *rows);
  bool SetMapKeepRadius(double radius);  // config().map_keep_radius = radius; false: negative or NaN
  // wc_map_carve for the rays origin -> each of n host points (xyz: n x 3 floats, the map's frame): *result (may be null) as the library
  // leaves it - what the rays select; the map is not modified.  false without a map or with arguments the library refuses
  bool CarveMap(const float *xyz, size_t n, const double origin[3], const wc_map_carve_params &params, wc_map_carve_result *result);
  // CarveMap that also removes what it selects, in place (wc_map_carve_remove): *result is what CarveMap would have returned
  bool CarveMapRemove(const float *xyz, size_t n, const double origin[3], const wc_map_carve_params &params, wc_map_carve_result *result);
  // wc_map_remove_keys for n host voxel indices (keys: n x 3 int32): out[3] = voxels removed, points removed, keys that removed nothing.
  // false - nothing touched - without a map, with out null, or with n > 0 and keys null
  bool RemoveMapVoxels(const int32_t *keys, size_t n, uint64_t out[3]);
  // wc_map_components of the map into host arrays: labels (cap entries; null: a query for the sizes) and keys (cap x 3; may be null) in
  // ExportMap's order, comps (cap_comps records; may be null), out[4] = voxels, nodes, components, voxels of the largest.  false without a
  // map, with out null, with params the library refuses (out untouched), or when cap or cap_comps is too small (out filled, nothing
  // else written).  The map is not modified.  Nothing in AddLidarScan calls it
  bool MapComponents(const wc_map_cc_params &params, int32_t *keys, uint32_t *labels, size_t cap, wc_map_component *comps, size_t cap_comps,
                     uint64_t out[4]);
  // wc_map_remove_small: out[4] = components before, components removed, voxels removed, points removed; false - nothing touched - without
  // a map, with out null or with params the library refuses.  Nothing in AddLidarScan calls it, and there is no per-sweep option: a
  // surface first seen at the edge of range is a small component for a sweep or two, and removing it every sweep would restart its sums
  // from zero each time - when to call it is the caller's policy
  bool RemoveSmallMapComponents(const wc_map_cc_params &params, uint32_t min_voxels, uint64_t min_comp_points, uint64_t out[4]);
  // config().map_carve_range / _shell / _min_rays (the per-sweep carve; range 0 = off); false - nothing changed - for a negative or NaN
  // range, shell > 8 or min_rays < 1
  bool SetMapCarve(double range, uint32_t shell, uint32_t min_rays);
  // wc_map_raycast for the rays origin -> each of n host points (xyz: n x 3 floats, the map's frame): hits receives n records - per ray the
  // first occupied voxel its walk tests -, *result (may be null) the call's counters; the map is not modified.  false without a map or with
  // arguments the library refuses.  Nothing in AddLidarScan calls it
  bool CastMap(const float *xyz, size_t n, const double origin[3], const wc_map_raycast_params &params, wc_map_ray_hit *hits,
               wc_map_raycast_result *result);
  // the map's exact state (wc_map_export_state) as the canonical file of host/map_file.h; false - no file is left behind -
  // without a map or when the file cannot be written.  Nothing in AddLidarScan calls SaveMap or LoadMap
  bool SaveMap(const std::string &path);
  // a file SaveMap wrote, absorbed (wc_map_absorb) into the map: re-created empty first, with room for the file's voxels (merge = false),
  // or as it is (merge = true: counts and sums add up).  false - nothing touched - without a map, when the file is refused
  // (wc_map_file::Decode), when its voxel size is not bitwise config().map_voxel_size, or when map_surfels is on and the file has no
  // moments (a file with moments loads into a map without: they are dropped)
  bool LoadMap(const std::string &path, bool merge = false);
  // a file SaveMap wrote in ANOTHER frame, aligned to the map and merged into it under the pose found: the file is decoded
  // into a temporary map of the facade's voxel size with moments; that map's centroids (wc_map_export, on the device) go through the level
  // chain of RelocalizeToMap from T_io (the file's frame to the map's) with `opts` as its `finest`; when the finest level ends with
  // termination 0 or 1 and n_used >= opts.min_used, wc_map_merge_moved adds the temporary map to the facade's under the found pose, T_io
  // becomes that pose and summaries (may be null) receives n_levels records, coarsest first.  false - the map and T_io untouched - where
  // LoadMap(path) or RelocalizeToMap would return false (map_surfels off included), when the alignment ends with termination 2 or too few
  // points, and when the library refuses the pose.  The call's wall time goes to last_map_ms().  Nothing in AddLidarScan calls it
  bool MergeMapFile(const std::string &path, double T_io[12], uint32_t factor, uint32_t n_levels, const wc_map_align_opts &opts,
                    wc_map_align_summary *summaries);
  // wall time [ms] of the last completed sweep's map step (the undistortion when fill_outputs does not already form it, the insert's
  // enqueue - its kernel runs behind on the stream -, with map_carve_range the carve, which waits, and, with map_keep_radius, the crop,
  // which waits too).  Not part of last_stage_ms()
  double last_map_ms() const { return last_map_ms_; }
  LioConfig &config() { return config_; }
  void ApplyConfig();  // push config() changes (IMU model, quirks, extraction arithmetic, iteration cap, extrinsics) into the device context
  // replace the whole configuration, checked first: false - nothing changed, config_error() says why - after the first AddImuData /
  // AddLidarScan, for a window or timing value that is not finite and positive, or when the derived wc_params fail wc_params_check
  bool SetConfig(const LioConfig &c);
  const std::string &config_error() const { return config_error_; }
  bool ImportState(const double *samples23, size_t ns, const wc_imu_state *imu, size_t n_imu);  // test hook, see .cc

 private:
  struct Sample {  // reference SampleState (surfel.h:9-23)
    double timestamp;
    double cor[12];  // rot_cor, pos_cor, bg, ba
    double grav[3];
    double quat[4];
    double pos[3];
  };
  void PredictImuStatesAndSampleStates(double end_time);
  bool SyncHeadingMsgs();
  void UploadImuStates();
  void LogResiduals(const std::vector<double> &x, const char *when);
  void UpdateImuPoses();
  void UpdateSamplePoses();
  void UpdateSurfelPosesOnDevice();
  void ShrinkToFit();
  void EnsureSurfelCapacity(size_t n);
  void EnsureFixedCapacity(size_t extra);
  void AppendScanOnDevice(const pcl::PointCloud<hilti_ros::Point> &msg);
  void DropBufferedPoints(size_t k);
  void Fatal(const char *what, int rc) const;

  LioConfig config_;
  std::string config_error_;
  bool data_added_ = false;  // an IMU or lidar message has arrived: SetConfig is refused from then on
  wc_ctx *ctx_ = nullptr;
 public:
  // the library context behind this object (tests and profiling scripts set development options on it: wc_ctx_set_dev_option)
  wc_ctx *gpu_context() const { return ctx_; }
 private:
  std::deque<ImuData> imu_buff_;
  // points_buff_ of the reference (lidar_odometry.h:56) lives in HBM: the pre-filtered points of the scans not yet
  // consumed are d_pts_[pts_cur_][pts_begin_ .. pts_end_); the host keeps only their timestamps
  std::deque<double> point_times_;
  void *d_pts_[2] = {nullptr, nullptr};
  void *d_scan_raw_ = nullptr;
  size_t cap_pts_[2] = {0, 0}, cap_scan_raw_ = 0, pts_begin_ = 0, pts_end_ = 0;
  int pts_cur_ = 0;
  std::deque<Sample> samples_;
  std::deque<wc_imu_state> imu_states_;
  // contiguous copy of imu_states_ (the C-ABI takes arrays) and whether the device copy follows it: rebuilt / uploaded only after a change
  // (prediction, post-solve correction, shrink, import) - a sweep flattened and uploaded the ~0.3 MB four to five times
  std::vector<wc_imu_state> imu_flat_;
  bool imu_flat_stale_ = true, imu_dev_stale_ = true;
  void TouchImu() { imu_flat_stale_ = imu_dev_stale_ = true; }
  const std::vector<wc_imu_state> &FlatImu();
  double ext_quat_[4];
  bool init_sld_win_ = false, sync_done_ = false, first_sample_known_ = false;
  double first_sample_time_ = 0.0;
  int sweep_id_ = 0, sweeps_fast_ = 0, sweeps_exact_ = 0;
  // sliding window in HBM, time ordered: d_surf_[sld_begin_ .. n_surfels_) ([0, sld_begin_) has moved to the fixed window and
  // is dropped at the next reallocation).  Fixed window: d_fix_surf_[fix_start_ .. fix_end_), NEWEST first - the array is
  // filled from the back because the reference push_front()s (lidar_odometry.cc:243-246, Q11)
  wc_surfel *d_surf_ = nullptr;
  wc_surfel *d_fix_surf_ = nullptr;
  wc_pose *d_fix_pose_ = nullptr;
  size_t fix_cap_ = 0, fix_start_ = 0, fix_end_ = 0;
  std::deque<double> fix_times_;
  wc_pose *d_pose_ = nullptr;
  uint8_t *d_inbody_ = nullptr;
  wc_pair *d_pairs_sld_ = nullptr, *d_pairs_fix_ = nullptr;
  wc_imu_state *d_imu_ = nullptr;
  void *d_sweep_xyz_ = nullptr, *d_sweep_t_ = nullptr;  // the undistorted sweep, packed: 3 floats | 1 double per point
  void *d_kept_t_ = nullptr;  // stamps of the points the pre-filter kept (scratch of AppendScanOnDevice)
  size_t cap_kept_t_ = 0;
  size_t cap_surfels_ = 0, n_surfels_ = 0, sld_begin_ = 0, cap_imu_ = 0, cap_sweep_ = 0;
  std::deque<double> surfel_times_;  // host copy of the sliding window's surfel timestamps (window bookkeeping only)
  SweepOutputs outputs_;
  void FillOutputs(const void *d_world_sweep, size_t n_sweep);
  const void *UndistortFinal(const void *d_raw_sweep, size_t n_sweep);  // the sweep with the final poses, 48-byte records, in d_world_
  void EnsureMap();
  void *d_world_ = nullptr;
  size_t cap_world_ = 0;
  wc_map *map_ = nullptr;
  double map_voxel_ = 0.0;  // voxel size map_ was created with
  bool map_moments_ = false;  // ... and whether with WC_MAP_MOMENTS
  double last_map_ms_ = 0.0;
  std::string residual_log_;
  void *d_res_ = nullptr;
  size_t cap_res_ = 0;
  wc_solve_summary last_summary_{};
  double last_stage_ms_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int last_lm_iterations_ = 0;  // over the sweep's outer iterations
  double last_append_ms_ = 0.0;
  uint64_t last_corr_[2] = {0, 0};
  bool keep_pair_stamps_ = false;
  std::vector<double> pair_stamps_[2];  // (first, second) stamps, pair after pair
};
