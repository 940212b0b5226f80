// odom_c_api.cc — a flat C wrapper around the LidarOdometry facade so that scripts (tests, bench) can drive the same
// object wildcat_slam_node.cc would drive through its C++ interface.
#include <cstring>

#include <algorithm>

#include "../csrc/extract_plan.h"
#include "../csrc/lm_loop.h"
#include "../csrc/map_room.h"
#include "cubic_bspline.h"
#include "histogram.h"
#include "imu_resampler.h"
#include "lidar_odometry.h"
#include "map_file.h"

extern "C" {

void *wc_odom_create(int device) { return new LidarOdometry(device); }
void wc_odom_destroy(void *h) { delete (LidarOdometry *)h; }
// a development option of the facade's library context (include/wildcat_hip.h: wc_ctx_set_dev_option) - stress scripts only
int wc_odom_set_dev_option(void *h, const char *name, int value) { return wc_ctx_set_dev_option(((LidarOdometry *)h)->gpu_context(), name, value); }

void wc_odom_add_imu(void *h, double t, const double acc[3], const double gyr[3]) {
  ImuData d;
  d.timestamp = t;
  for (int i = 0; i < 3; ++i) d.linear_acceleration[i] = acc[i], d.angular_velocity[i] = gyr[i];
  ((LidarOdometry *)h)->AddImuData(d);
}

// points: n records of the 48-byte hilti_ros::Point layout, in the LIDAR frame, time ascending
void wc_odom_add_scan(void *h, const void *points, uint64_t n) {
  auto cloud = std::make_shared<pcl::PointCloud<hilti_ros::Point>>();
  cloud->points.resize(n);
  if (n) std::memcpy(cloud->points.data(), points, n * sizeof(hilti_ros::Point));
  ((LidarOdometry *)h)->AddLidarScan(cloud);
}

int wc_odom_sweeps(void *h) { return ((LidarOdometry *)h)->sweeps_done(); }
uint64_t wc_odom_num_samples(void *h) { return ((LidarOdometry *)h)->num_sample_states(); }

// out[15] = t, pos[3], quat[4] (w,x,y,z), bg[3], ba[3], spare
int wc_odom_sample(void *h, uint64_t i, double *out) {
  LidarOdometry::SampleStateView v;
  if (!((LidarOdometry *)h)->sample_state(i, &v)) return 1;
  out[0] = v.timestamp;
  std::memcpy(out + 1, v.pos, 24);
  std::memcpy(out + 4, v.quat, 32);
  std::memcpy(out + 8, v.bg, 24);
  std::memcpy(out + 11, v.ba, 24);
  return 0;
}

// stats[8] = sliding surfels, fixed surfels, binary corr, unary corr, LM iterations, initial cost, final cost, termination
void wc_odom_stats(void *h, double *stats) {
  LidarOdometry *o = (LidarOdometry *)h;
  stats[0] = (double)o->sliding_window_surfels();
  stats[1] = (double)o->fixed_window_surfels();
  stats[2] = (double)o->last_correspondences(0);
  stats[3] = (double)o->last_correspondences(1);
  stats[4] = o->last_solve().iterations;
  stats[5] = o->last_solve().initial_cost;
  stats[6] = o->last_solve().final_cost;
  stats[7] = o->last_solve().termination;
}

// wall time [ms] of the last completed sweep's stages (predict + undistort, extract + poses, match, build, solve, update, shrink)
// and, in out[7], the LM iterations of its outer iterations together
void wc_odom_stage_ms(void *h, double out[8]) {
  const LidarOdometry *o = (const LidarOdometry *)h;
  for (int i = 0; i < 7; ++i) out[i] = o->last_stage_ms()[i];
  out[7] = (double)o->last_lm_iterations();
}

// wall time [ms] of the completing message's part in front of those stages (upload + pre-filter of its points, heading synchronisation)
double wc_odom_append_ms(void *h) { return ((const LidarOdometry *)h)->last_append_ms(); }

// out[2] = sweeps extracted by the default (integer-moment) arithmetic, sweeps extracted in the reference's summation order
void wc_odom_extract_paths(void *h, int out[2]) {
  out[0] = ((LidarOdometry *)h)->sweeps_fast_path();
  out[1] = ((LidarOdometry *)h)->sweeps_exact_path();
}

// timestamps of the fixed window in its stored order (newest first, Q11); returns the window size
uint64_t wc_odom_fixed_times(void *h, double *out, uint64_t cap) {
  const std::deque<double> &t = ((LidarOdometry *)h)->fixed_window_times();
  for (uint64_t i = 0; i < t.size() && i < cap; ++i) out[i] = t[i];
  return t.size();
}
// test hook: the surfel timestamps (first, second) of the last sweep's correspondences; which = 0 sliding, 1 fixed window
void wc_odom_set_keep_pair_stamps(void *h, int on) { ((LidarOdometry *)h)->set_keep_pair_stamps(on != 0); }
uint64_t wc_odom_pair_stamps(void *h, int which, double *out, uint64_t cap) {
  const std::vector<double> &v = ((LidarOdometry *)h)->last_pair_stamps(which ? 1 : 0);
  for (uint64_t i = 0; i < v.size() && i < cap; ++i) out[i] = v[i];
  return v.size();
}
// both setters re-derive the device context's parameters (Q1 / Q3 Jacobians, extraction arithmetic), not only the host flags
void wc_odom_set_quirks(void *h, int on) {
  ((LidarOdometry *)h)->config().reference_quirks = on != 0;
  ((LidarOdometry *)h)->ApplyConfig();
}
void wc_odom_set_exact_sums(void *h, int on) {
  ((LidarOdometry *)h)->config().exact_sums = on != 0;
  ((LidarOdometry *)h)->ApplyConfig();
}
// ---- the configuration (host/lio_config.h: wc_odom_config = LioConfig's reference fields) --------------------------------------------
void wc_odom_get_config(void *h, wc_odom_config *out) { ConfigToC(((LidarOdometry *)h)->config(), out); }
// 0: taken - the context's wc_params re-derived (IMU cost weights, imu_dt, iteration cap) and the extrinsic quaternion with them.
// WC_ERR_ARG: refused and nothing changed - IMU or lidar data has been added already, a window or timing value is not finite and positive,
// or wc_params_check refuses the derived parameters; wc_odom_config_error says which
int wc_odom_set_config(void *h, const wc_odom_config *c) {
  LidarOdometry *o = (LidarOdometry *)h;
  if (!c) return WC_ERR_ARG;
  LioConfig next = o->config();
  ConfigFromC(*c, &next);
  return o->SetConfig(next) ? WC_OK : WC_ERR_ARG;
}
const char *wc_odom_config_error(void *h) { return ((LidarOdometry *)h)->config_error().c_str(); }
// the wc_params the facade's context holds
int wc_odom_ctx_params(void *h, wc_params *out) { return wc_ctx_get_params(((LidarOdometry *)h)->gpu_context(), out); }
// the wc_params a configuration stands for, without a context (c NULL: the default LioConfig); the return value is wc_params_check's
int wc_host_params_from_config(const wc_odom_config *c, wc_params *out) {
  LioConfig cfg;
  if (c) ConfigFromC(*c, &cfg);
  WcParamsFromConfig(cfg, out);
  return wc_params_check(out, nullptr);
}
void wc_host_default_config(wc_odom_config *out) { ConfigToC(LioConfig(), out); }

// the reference's residual log (PrintSurfelResiduals / PrintImuResiduals, lidar_odometry.cc:56-94): switch + the last sweep's text
void wc_odom_set_residual_log(void *h, int on) { ((LidarOdometry *)h)->config().log_residual_histograms = on != 0; }
uint64_t wc_odom_residual_log(void *h, char *out, uint64_t cap) {
  const std::string &s = ((LidarOdometry *)h)->last_residual_log();
  if (out && cap) {
    const size_t n = std::min<size_t>(s.size(), cap - 1);
    std::memcpy(out, s.data(), n);
    out[n] = 0;
  }
  return s.size();
}
// Histogram::ToString (src/common/histogram.cc:27-76) through the facade's restatement, for a known-answer test
uint64_t wc_host_histogram(const double *values, uint64_t n, int buckets, char *out, uint64_t cap) {
  Histogram hst;
  for (uint64_t i = 0; i < n; ++i) hst.Add(values[i]);
  const std::string s = hst.ToString(buckets);
  if (out && cap) {
    const size_t m = std::min<size_t>(s.size(), cap - 1);
    std::memcpy(out, s.data(), m);
    out[m] = 0;
  }
  return s.size();
}

// ---- the ROS-free wire formats (host/wire_formats.h) ------------------------------------------------------------------------
void wc_odom_set_fill_outputs(void *h, int on) { ((LidarOdometry *)h)->config().fill_outputs = on != 0; }
// markers of the last sweep: out = n x 14 doubles (position 3, orientation wxyz 4, scale 3, colour rgba 4); returns n
uint64_t wc_odom_markers(void *h, double *out, uint64_t cap) {
  const auto &m = ((LidarOdometry *)h)->last_outputs().markers;
  for (uint64_t i = 0; i < m.size() && i < cap; ++i) {
    double *o = out + 14 * i;
    std::memcpy(o, m[i].position, 24);
    std::memcpy(o + 3, m[i].orientation, 32);
    std::memcpy(o + 7, m[i].scale, 24);
    for (int c = 0; c < 4; ++c) o[10 + c] = m[i].color[c];
  }
  return m.size();
}
// the published sweep: its 48-byte point records (the PointCloud2 payload), header stamp; tf8 = stamp, origin, rotation xyzw
uint64_t wc_odom_scan_in_world(void *h, void *points48, uint64_t cap, double *stamp, double tf8[8]) {
  const LidarOdometry::SweepOutputs &o = ((LidarOdometry *)h)->last_outputs();
  const uint64_t n = o.scan_in_world.width;
  if (points48 && cap >= n && n) std::memcpy(points48, o.scan_in_world.data.data(), 48 * n);
  if (stamp) *stamp = o.scan_stamp;
  if (tf8) {
    tf8[0] = o.tf.stamp;
    std::memcpy(tf8 + 1, o.tf.origin, 24);
    std::memcpy(tf8 + 4, o.tf.rotation_xyzw, 32);
  }
  return n;
}
// pcl::fromROSMsg for hilti_ros::Point on a described payload: nf fields (names: zero-terminated strings back to back),
// returns the number of registered fields matched (-1: refused); out48 must hold width * height records
int wc_host_cloud2_to_points(const char *names, const uint32_t *offsets, const uint8_t *datatypes, const uint32_t *counts, int nf, uint32_t width,
                             uint32_t height, uint32_t point_step, uint32_t row_step, int is_bigendian, const uint8_t *data, uint64_t nbytes,
                             void *out48) {
  wc_wire::PointCloud2 msg;
  msg.width = width, msg.height = height, msg.point_step = point_step, msg.row_step = row_step, msg.is_bigendian = is_bigendian != 0;
  const char *p = names;
  for (int f = 0; f < nf; ++f) {
    msg.fields.push_back({std::string(p), offsets[f], datatypes[f], counts[f]});
    p += std::strlen(p) + 1;
  }
  msg.data.assign(data, data + nbytes);
  std::vector<hilti_ros::Point> pts;
  const int m = wc_wire::PointsFromCloud2(msg, pts);
  if (m >= 0 && !pts.empty()) std::memcpy(out48, pts.data(), 48 * pts.size());
  return m;
}
// pcl::toROSMsg: the field table (6 x {offset, datatype, count}) and point_step for hilti_ros::Point; names_out gets
// "x\0y\0z\0intensity\0timestamp\0ring\0"
int wc_host_points_to_cloud2_layout(uint32_t table18[18], char *names_out, uint64_t cap) {
  wc_wire::PointCloud2 msg;
  wc_wire::Cloud2FromPoints(nullptr, 0, msg);
  std::string names;
  for (size_t f = 0; f < msg.fields.size(); ++f) {
    table18[3 * f] = msg.fields[f].offset, table18[3 * f + 1] = msg.fields[f].datatype, table18[3 * f + 2] = msg.fields[f].count;
    names += msg.fields[f].name;
    names.push_back('\0');
  }
  if (names_out && cap >= names.size()) std::memcpy(names_out, names.data(), names.size());
  return (int)msg.point_step;
}
// makeRightHanded (surfel_extraction.cc:340-358) and the marker of one surfel, for known-answer tests
void wc_host_make_right_handed(double evec9[9], double eval3[3]) { wc_wire::MakeRightHanded(evec9, eval3); }
void wc_host_marker(const wc_surfel *s, const wc_pose *p, double out14[14]) {
  const wc_wire::SurfelMarker m = wc_wire::MarkerFromSurfel(*s, *p);
  std::memcpy(out14, m.position, 24);
  std::memcpy(out14 + 3, m.orientation, 32);
  std::memcpy(out14 + 7, m.scale, 24);
  for (int c = 0; c < 4; ++c) out14[10 + c] = m.color[c];
}

// ---- the accumulated map (LioConfig::map_voxel_size; include/wildcat_hip.h: wc_map_*) -------------------------------------
// voxel side [m]: 0 removes the map, 0.01 .. 4.0 (re-)creates it empty; returns 0, or WC_ERR_ARG for any other value
int wc_odom_set_map_voxel(void *h, double voxel) { return ((LidarOdometry *)h)->SetMapVoxel(voxel) ? 0 : WC_ERR_ARG; }
// out3 = voxels, points inserted, points rejected (non-finite or beyond 2^20 voxels from the origin)
void wc_odom_map_size(void *h, uint64_t out3[3]) {
  const LidarOdometry *o = (const LidarOdometry *)h;
  out3[0] = o->map_voxels(), out3[1] = o->map_points(), out3[2] = o->map_rejected();
}
// centroids (n x 3 floats) and counts in ascending voxel-index order; returns n (nothing written when cap < n)
uint64_t wc_odom_map_export(void *h, float *xyz, uint32_t *counts, uint64_t cap) { return ((LidarOdometry *)h)->ExportMap(xyz, counts, cap); }
void wc_odom_map_clear(void *h) { ((LidarOdometry *)h)->ClearMap(); }
double wc_odom_map_ms(void *h) { return ((const LidarOdometry *)h)->last_map_ms(); }
// nearest map voxel of n host points (n x 3 floats) within max_dist -> hits[n] (wc_map_hit); returns the number found
uint64_t wc_odom_map_query(void *h, const float *xyz, uint64_t n, double max_dist, wc_map_hit *hits) {
  return ((LidarOdometry *)h)->QueryMap(xyz, n, max_dist, hits);
}
// wc_map_knn for n host points (n x 3 floats) -> hits[n * params->k] (wc_map_hit), within[n] (may be NULL); returns the queries with a neighbour
uint64_t wc_odom_map_query_knn(void *h, const float *xyz, uint64_t n, const wc_map_knn_params *params, wc_map_hit *hits, uint32_t *within) {
  return params ? ((LidarOdometry *)h)->QueryMapKnn(xyz, n, *params, hits, within) : 0;
}
// keeps the voxels that intersect the box [lo, hi]; returns the voxels removed
uint64_t wc_odom_map_crop(void *h, const double lo[3], const double hi[3]) { return ((LidarOdometry *)h)->CropMap(lo, hi); }
// LioConfig::map_surfels: the map re-created empty, with (1) or without (0) second moments
void wc_odom_set_map_surfels(void *h, int on) { ((LidarOdometry *)h)->SetMapSurfels(on != 0); }
int wc_odom_map_surfels_on(void *h) { return ((LidarOdometry *)h)->config().map_surfels ? 1 : 0; }
// the map's voxels as wc_map_surfel records (wc_map_export_surfels); returns the number of voxels (nothing written when cap is smaller)
uint64_t wc_odom_map_surfels(void *h, wc_map_surfel *surfels, uint64_t cap) { return ((LidarOdometry *)h)->ExportMapSurfels(surfels, cap); }
// wc_map_nearest_plane for n host points (n x 3 floats) -> hits[n] (wc_map_plane_hit); returns the number of voxels found
uint64_t wc_odom_map_query_planes(void *h, const float *xyz, uint64_t n, double max_dist, uint32_t min_points, wc_map_plane_hit *hits) {
  return ((LidarOdometry *)h)->QueryMapPlanes(xyz, n, max_dist, min_points, hits);
}
// LidarOdometry::AlignToMap / LinearizeAgainstMap for n host points (n x 3 floats); 1 = done, 0 = no map, map_surfels off or refused arguments
int wc_odom_map_align(void *h, const float *xyz, uint64_t n, double T_io[12], const wc_map_align_opts *opts, wc_map_align_summary *summary) {
  return opts && ((LidarOdometry *)h)->AlignToMap(xyz, n, T_io, *opts, summary) ? 1 : 0;
}
// LidarOdometry::AlignSweepToMap for n host records of 48 bytes; 1 = done, 0 = as wc_odom_map_align, an empty sweep or one without a stamp interval
int wc_odom_map_align_sweep(void *h, const void *points48, uint64_t n, wc_pose *pose_begin_io, wc_pose *pose_end_io,
                            const wc_map_ct_align_opts *opts, wc_map_ct_align_summary *summary, int insert) {
  return opts && ((LidarOdometry *)h)->AlignSweepToMap(points48, n, pose_begin_io, pose_end_io, *opts, summary, insert != 0) ? 1 : 0;
}
// LidarOdometry::RelocalizeToMap; summaries: n_levels records, coarsest first (may be null); 1 = done, 0 = as wc_odom_map_align, or levels refused
int wc_odom_map_relocalize(void *h, const float *xyz, uint64_t n, double T_io[12], uint32_t factor, uint32_t n_levels,
                           const wc_map_align_opts *finest, wc_map_align_summary *summaries) {
  return finest && ((LidarOdometry *)h)->RelocalizeToMap(xyz, n, T_io, factor, n_levels, *finest, summaries) ? 1 : 0;
}
// LidarOdometry::RelocalizeSearch; summaries: n_levels x n_yaw records, level-major (may be null); best: the winner's index (may be null);
// 1 = done, 0 = as wc_odom_map_relocalize, n_yaw outside 1 .. 1024, or no eligible hypothesis
int wc_odom_map_relocalize_search(void *h, const float *xyz, uint64_t n, double T_io[12], uint32_t n_yaw, uint32_t factor, uint32_t n_levels,
                                  const wc_map_align_opts *finest, wc_map_align_summary *summaries, int32_t *best) {
  return finest && ((LidarOdometry *)h)->RelocalizeSearch(xyz, n, T_io, n_yaw, factor, n_levels, *finest, summaries, best) ? 1 : 0;
}
// LidarOdometry::RelocalizeGlobal; summaries: n_levels x top_m records, level-major, rank order (may be null); best: the winner's rank (may be
// null); 1 = done, 0 = as wc_odom_map_relocalize, top_m outside 1 .. 1024, a refused grid, or no eligible candidate or hypothesis
int wc_odom_map_relocalize_global(void *h, const float *xyz, uint64_t n, double T_io[12], uint32_t n_yaw, const uint32_t n_xyz[3],
                                  const double step[3], uint32_t top_m, uint32_t factor, uint32_t n_levels, const wc_map_align_opts *finest,
                                  wc_map_align_summary *summaries, int32_t *best) {
  return finest && ((LidarOdometry *)h)->RelocalizeGlobal(xyz, n, T_io, n_yaw, n_xyz, step, top_m, factor, n_levels, *finest, summaries, best) ? 1 : 0;
}
int wc_odom_map_linearize(void *h, const float *xyz, uint64_t n, const double T[12], const wc_map_reg_params *params, wc_map_normal_eq *out,
                          wc_map_reg_row *rows) {
  return params && ((LidarOdometry *)h)->LinearizeAgainstMap(xyz, n, T, *params, out, rows) ? 1 : 0;
}
// LidarOdometry::CarveMap for n host points (n x 3 floats); 1 = done, 0 = no map or refused arguments
int wc_odom_map_carve(void *h, const float *xyz, uint64_t n, const double origin[3], const wc_map_carve_params *params, wc_map_carve_result *result) {
  return params && ((LidarOdometry *)h)->CarveMap(xyz, n, origin, *params, result) ? 1 : 0;
}
// LidarOdometry::CarveMapRemove, RemoveMapVoxels (keys: n x 3 int32 on the host) and SetMapCarve; 1 = done, 0 = no map or refused arguments
int wc_odom_map_carve_remove(void *h, const float *xyz, uint64_t n, const double origin[3], const wc_map_carve_params *params,
                             wc_map_carve_result *result) {
  return params && ((LidarOdometry *)h)->CarveMapRemove(xyz, n, origin, *params, result) ? 1 : 0;
}
int wc_odom_map_remove_keys(void *h, const int32_t *keys, uint64_t n, uint64_t out3[3]) {
  return ((LidarOdometry *)h)->RemoveMapVoxels(keys, n, out3) ? 1 : 0;
}
// LidarOdometry::MapComponents (host arrays; keys, comps and - for a size query - labels may be null) and RemoveSmallMapComponents;
// 1 = done, 0 = no map, refused arguments, or (wc_odom_map_components, out4 filled) too little room
int wc_odom_map_components(void *h, const wc_map_cc_params *params, int32_t *keys, uint32_t *labels, uint64_t cap, wc_map_component *comps,
                           uint64_t cap_comps, uint64_t out4[4]) {
  return params && ((LidarOdometry *)h)->MapComponents(*params, keys, labels, cap, comps, cap_comps, out4) ? 1 : 0;
}
int wc_odom_map_remove_small(void *h, const wc_map_cc_params *params, uint32_t min_voxels, uint64_t min_comp_points, uint64_t out4[4]) {
  return params && ((LidarOdometry *)h)->RemoveSmallMapComponents(*params, min_voxels, min_comp_points, out4) ? 1 : 0;
}
// LioConfig::map_carve_range / _shell / _min_rays; returns 0, or WC_ERR_ARG for a negative or NaN range, shell > 8 or min_rays < 1
int wc_odom_set_map_carve(void *h, double range, uint32_t shell, uint32_t min_rays) {
  return ((LidarOdometry *)h)->SetMapCarve(range, shell, min_rays) ? 0 : WC_ERR_ARG;
}
// csrc/map_room.h without a GPU: 0 = keep, 1 = grow, 2 = purge (*new_cap: the table's slots afterwards), negative: beyond 2^32 slots
int wc_host_map_room(uint64_t cap, uint64_t live_bound, uint64_t tombs, uint64_t n, uint64_t *new_cap) {
  uint64_t c = cap;
  const int rc = map_room(cap, live_bound, tombs, n, &c);
  if (new_cap) *new_cap = c;
  return rc;
}
// LidarOdometry::CastMap for n host points (n x 3 floats) into n host records; 1 = done, 0 = no map or refused arguments
int wc_odom_map_raycast(void *h, const float *xyz, uint64_t n, const double origin[3], const wc_map_raycast_params *params, wc_map_ray_hit *hits,
                        wc_map_raycast_result *result) {
  return params && ((LidarOdometry *)h)->CastMap(xyz, n, origin, *params, hits, result) ? 1 : 0;
}
// LidarOdometry::SaveMap / LoadMap (the canonical state file of host/map_file.h); 1 = done, 0 = refused (nothing touched)
int wc_odom_map_save(void *h, const char *path) { return path && ((LidarOdometry *)h)->SaveMap(path) ? 1 : 0; }
int wc_odom_map_load(void *h, const char *path, int merge) { return path && ((LidarOdometry *)h)->LoadMap(path, merge != 0) ? 1 : 0; }
// LidarOdometry::MergeMapFile: a file of another frame aligned from T_io and merged under the pose found; summaries: n_levels records,
// coarsest first (may be null); 1 = done, 0 = refused (the map and T_io untouched)
int wc_odom_map_merge_file(void *h, const char *path, double T_io[12], uint32_t factor, uint32_t n_levels, const wc_map_align_opts *opts,
                           wc_map_align_summary *summaries) {
  return path && opts && ((LidarOdometry *)h)->MergeMapFile(path, T_io, factor, n_levels, *opts, summaries) ? 1 : 0;
}
// host/map_file.h without a GPU.  encode: the file of n records (vox: n x 40 bytes as wc_map_voxel; mom: n x 9 int64, read with flags
// bit 0) -> its size in bytes; written when cap is at least that.  decode: wc_map_file::Decode's code (0 = accepted; then *voxel, *flags
// and *n describe the file, and vox / mom - either may be NULL - receive its records when cap >= n)
uint64_t wc_host_map_file_encode(double voxel, uint32_t flags, const void *vox, const int64_t *mom, uint64_t n, uint8_t *out, uint64_t cap) {
  const uint64_t bytes = wc_map_file::EncodedBytes(n, (flags & wc_map_file::kFlagMoments) != 0);
  if (out && cap >= bytes) wc_map_file::Encode(voxel, flags, (const wc_map_file::Voxel *)vox, mom, n, out);
  return bytes;
}
int wc_host_map_file_decode(const uint8_t *buf, uint64_t len, double *voxel, uint32_t *flags, uint64_t *n, void *vox, int64_t *mom, uint64_t cap) {
  wc_map_file::Header h;
  const int rc = wc_map_file::Decode(buf, len, &h);
  if (rc != wc_map_file::kOk) return rc;
  if (voxel) *voxel = h.voxel;
  if (flags) *flags = h.flags;
  if (n) *n = h.n;
  if (vox && cap >= h.n) wc_map_file::Unpack(buf, h, (wc_map_file::Voxel *)vox, mom);
  return rc;
}
// LioConfig::map_keep_radius: 0 = unbounded map; returns 0, or WC_ERR_ARG for a negative or NaN radius
int wc_odom_set_map_keep_radius(void *h, double radius) { return ((LidarOdometry *)h)->SetMapKeepRadius(radius) ? 0 : WC_ERR_ARG; }
// Cloud2FromXyz (host/wire_formats.h): the field table (3 x {offset, datatype, count}), point_step and the payload of n points
int wc_host_xyz_to_cloud2(const float *xyz, uint64_t n, uint32_t table9[9], char *names_out, uint64_t cap, uint8_t *data_out) {
  wc_wire::PointCloud2 msg;
  wc_wire::Cloud2FromXyz(xyz, n, msg);
  std::string names;
  for (size_t f = 0; f < msg.fields.size() && f < 3; ++f) {
    table9[3 * f] = msg.fields[f].offset, table9[3 * f + 1] = msg.fields[f].datatype, table9[3 * f + 2] = msg.fields[f].count;
    names += msg.fields[f].name;
    names.push_back('\0');
  }
  if (names_out && cap >= names.size()) std::memcpy(names_out, names.data(), names.size());
  if (data_out && !msg.data.empty()) std::memcpy(data_out, msg.data.data(), msg.data.size());
  return (int)msg.point_step;
}

// test hook: start the next sweep from another run's states (LidarOdometry::ImportState); 0 = done, 1 = the counts differ
int wc_odom_import_state(void *h, const double *samples23, uint64_t ns, const wc_imu_state *imu, uint64_t n_imu) {
  return ((LidarOdometry *)h)->ImportState(samples23, ns, imu, n_imu) ? 0 : 1;
}

// ---- known-answer hooks for the host-side product code (the g++ instantiation of csrc/dmath.h, the facade's spline, the
// resampler): the reference's own unit tests are run against these in tests/test_host_kat.py -------------------------------

// csrc/extract_plan.h - which pipeline an extraction starts on and repeats on - driven step by step (tests/test_extract_plan_cpu.py).
// mem11 = ExMemory's general_calls, lds_cap, unordered, fx_backoff, fx_skip_calls, fx_spill_full, fx_fallbacks, fx_last_flags,
// fx_last_why, fx_dirty, fx_ctrl_ready; *path_bits = ex_path_bits.  op 0: ex_first_path(fx_ok = a, no_bucket_sort = b);
// op 1: ex_next_path(flags = a, reason words set = bits of b) -> its return value; op 2: ex_learn_unordered(run count = a, n = b);
// op 3: ex_reset_backoff
int wc_host_ex_plan(int op, uint32_t mem11[11], uint32_t *path_bits, uint32_t a, uint64_t b) {
  ExMemory m;
  m.general_calls = (int)mem11[0], m.lds_cap = mem11[1], m.unordered = mem11[2] != 0, m.fx_backoff = mem11[3], m.fx_skip_calls = mem11[4];
  m.fx_spill_full = mem11[5] != 0, m.fx_fallbacks = mem11[6], m.fx_last_flags = mem11[7], m.fx_last_why = mem11[8];
  m.fx_dirty = mem11[9] != 0, m.fx_ctrl_ready = mem11[10] != 0;
  ExPath p;
  p.fx = *path_bits & 1u, p.wide = *path_bits & 2u, p.run_sort = *path_bits & 4u, p.bin_order = *path_bits & 8u;
  int rc = 0;
  if (op == 0) {
    p = ex_first_path(m, a != 0, b != 0);
  } else if (op == 1) {
    uint32_t why[24];
    for (int i = 0; i < 24; ++i) why[i] = (uint32_t)((b >> i) & 1u);
    rc = ex_next_path(p, a, why, m) ? 1 : 0;
  } else if (op == 2) {
    ex_learn_unordered(m, p, a, b);
  } else {
    ex_reset_backoff(m);
  }
  const uint32_t out[11] = {(uint32_t)m.general_calls, m.lds_cap, m.unordered, m.fx_backoff, m.fx_skip_calls, m.fx_spill_full,
                            m.fx_fallbacks, m.fx_last_flags, m.fx_last_why, m.fx_dirty, m.fx_ctrl_ready};
  std::memcpy(mem11, out, sizeof(out));
  *path_bits = ex_path_bits(p);
  return rc;
}
// ... and its sizes: out5 = total slots, slot bin capacity, default-path tiles, node grid, layer-2 grid
void wc_host_ex_sizes(uint64_t n, int max_layer, int cluster_min, uint64_t floor, uint32_t last_splits, uint64_t out5[5]) {
  out5[0] = ex_total_slots(n, max_layer, cluster_min, floor);
  out5[1] = ex_slot_bin_cap(out5[0]);
  out5[2] = ex_fx_tiles(n);
  out5[3] = ex_fx_node_grid(n);
  out5[4] = ex_fx_layer2_grid((unsigned)out5[3], last_splits);
}
// ... and the early count's two mailbox words (tests/test_extract_mail_cpu.py).  pack: out2 = word A (ticket, count), word B (ticket,
// overflow, queued).  unpack: out3 = count, queued, overflow; returns ex_mail_arrived(a, b, ticket).  next_ticket: the sequence.
void wc_host_ex_mail_pack(uint32_t ticket, uint32_t count, uint32_t queued, int overflow, uint64_t out2[2]) {
  out2[0] = ex_mail_pack_count(ticket, count);
  out2[1] = ex_mail_pack_queue(ticket, overflow != 0, queued);
}
int wc_host_ex_mail_unpack(uint64_t a, uint64_t b, uint32_t ticket, uint32_t out3[3]) {
  out3[0] = ex_mail_count(a), out3[1] = ex_mail_queued(b), out3[2] = ex_mail_overflow(b) ? 1u : 0u;
  return ex_mail_arrived(a, b, ticket) ? 1 : 0;
}
uint32_t wc_host_ex_mail_next_ticket(uint32_t seq) { return ex_mail_next_ticket(seq); }

// csrc/lm_loop.h - the decisions of the window solver's LM loop - driven step by step over a caller-owned state block
// (tests/test_lm_loop_cpu.py).  op -1: -> the block's size in bytes.  op 0, lm_begin: in = max_iterations, lm_radius0,
// lm_dense_radius, lm_dense, ns, late_gradient, cost, max |g|, |x|.  op 1, lm_next -> LmAction.  op 2, lm_judge: in = fail,
// model_change, step_norm, cand_cost, cand_gmax, late_gmax -> LmVerdict.  op 3, lm_accepted: in = |x|, late slot -> 1: best so far.
// out22 (may be NULL), after the op: cost, gmax, min_cost, radius, decrease, x_norm, iter, consecutive_invalid, first_recorded,
// first_step_now, late_pending, late_at, then lm_summary: initial_cost, final_cost, iterations, successful_steps,
// unsuccessful_steps, termination, n_linearizations, n_cost_evaluations, first_step[0], first_step[1].  -2: bad op or block
int wc_host_lm_loop(int op, void *state, uint64_t state_bytes, const double *in, double *out22) {
  if (op == -1) return (int)sizeof(LmLoop);
  if (!state || state_bytes < sizeof(LmLoop) || (op != 1 && !in)) return -2;
  LmLoop L;
  std::memcpy(&L, state, sizeof(L));
  int rc = 0;
  if (op == 0)
    L = lm_begin(LmConfig{(int)in[0], (int)in[1], (int)in[2], in[3] != 0, (int)in[4], in[5] != 0}, in[6], in[7], in[8]);
  else if (op == 1)
    rc = (int)lm_next(L);
  else if (op == 2)
    rc = (int)lm_judge(L, LmMail{(int)in[0], in[1], in[2], in[3], in[4], in[5]});
  else if (op == 3)
    rc = lm_accepted(L, in[0], (int)in[1]) ? 1 : 0;
  else
    return -2;
  std::memcpy(state, &L, sizeof(L));
  if (out22) {
    const wc_solve_summary s = lm_summary(L);
    const double o[22] = {L.cost, L.gmax, L.min_cost, L.radius, L.decrease, L.x_norm, (double)L.iter, (double)L.consecutive_invalid,
                          (double)L.first_recorded, (double)L.first_step_now, (double)L.late_pending, (double)L.late_at,
                          s.initial_cost, s.final_cost, (double)s.iterations, (double)s.successful_steps, (double)s.unsuccessful_steps,
                          (double)s.termination, (double)s.n_linearizations, (double)s.n_cost_evaluations, s.first_step[0], s.first_step[1]};
    std::memcpy(out22, o, sizeof(o));
  }
  return rc;
}

// utils_test.cc:5-21 inputs -> out52 = Exp(v) | Log(Exp(v)) | Jl | Jl_inv | Jr | Jr_inv | Hat (layout of wc_selftest_so3)
void wc_host_so3(const double v3[3], double out52[52]) {
  using namespace wc;
  const V3 v = mk3(v3[0], v3[1], v3[2]);
  const Q4 q = so3_exp(v);
  const V3 l = so3_log(q);
  double *o = out52;
  o[0] = q.w, o[1] = q.x, o[2] = q.y, o[3] = q.z, o[4] = l.x, o[5] = l.y, o[6] = l.z;
  const M3 ms[5] = {so3_Jl(v), so3_Jl_inv(v), so3_Jr(v), so3_Jr_inv(v), hat(v)};
  for (int m = 0; m < 5; ++m)
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) o[7 + 9 * m + 3 * i + j] = ms[m].m[i][j];
}

// CubicBSplineInterpolator(timestamps, points).Interp(t) (spline_interpolation.h:42-113) through the facade's class.
// ctrl3 (may be NULL) receives the np control points.
void wc_host_bspline_fit_eval(const double *ts, const double *pts3, uint64_t np, const double *query, uint64_t nq, double *out3,
                              uint8_t *valid, double *ctrl3) {
  using namespace wc;
  std::vector<double> t(ts, ts + np);
  std::vector<V3> p(np);
  for (uint64_t i = 0; i < np; ++i) p[i] = mk3(pts3[3 * i], pts3[3 * i + 1], pts3[3 * i + 2]);
  const CubicBSpline sp(t, p);
  for (uint64_t i = 0; i < nq; ++i) {
    V3 o = mk3(0, 0, 0);
    valid[i] = sp.Interp(query[i], o) ? 1 : 0;
    out3[3 * i] = o.x, out3[3 * i + 1] = o.y, out3[3 * i + 2] = o.z;
  }
  if (ctrl3)
    for (uint64_t i = 0; i < np; ++i)
      ctrl3[3 * i] = sp.control_points()[i].x, ctrl3[3 * i + 1] = sp.control_points()[i].y, ctrl3[3 * i + 2] = sp.control_points()[i].z;
}

void *wc_host_resampler_create(int freq) { return new ImuResampler(freq); }
void wc_host_resampler_destroy(void *h) { delete (ImuResampler *)h; }
void wc_host_resampler_add(void *h, double t, const double acc[3], const double gyr[3]) {
  ImuData d;
  d.timestamp = t;
  for (int i = 0; i < 3; ++i) d.linear_acceleration[i] = acc[i], d.angular_velocity[i] = gyr[i];
  ((ImuResampler *)h)->AddImuData(d);
}
// out7 = t, acc, gyr; returns 1 when a resampled measurement was due (the shared_ptr was non-null)
int wc_host_resampler_advance(void *h, double out7[7]) {
  const std::shared_ptr<ImuData> r = ((ImuResampler *)h)->AdvanceGetResampledImuData();
  if (!r) return 0;
  out7[0] = r->timestamp;
  for (int i = 0; i < 3; ++i) out7[1 + i] = r->linear_acceleration[i], out7[4 + i] = r->angular_velocity[i];
  return 1;
}
}
