// lio_config.h — the reference's hard-coded configuration (src/odometry/lio_config.h:8-46), values unchanged.
#pragma once
#include <cmath>
#include <cstdint>

struct LioConfig {
  // IMU noise model (lio_config.h:10-14)
  double gyroscope_noise_density = 0.00015198973532354657;
  double accelerometer_noise_density = 0.006308226052016165;
  double gyroscope_random_walk = 0.00011673723527962174;
  double accelerometer_random_walk = 2.664506559330434e-06;
  double imu_factor_weight = 0.01;
  // preprocessing (lio_config.h:18-30)
  double max_range = 120;
  double min_range = 0.3;
  double blind_min[3] = {-0.8, -0.5, -0.4};  // Eigen::AlignedBox in imu_link
  double blind_max[3] = {0.3, 0.5, 0.4};
  double ext_translation[3] = {-0.001, -0.00855, 0.055};  // lidar -> imu
  double ext_rotation[9] = {-5.32125e-08, -1, 0, -1, -5.32125e-08, -0, 0, 0, -1};
  // windows (lio_config.h:32-36)
  double imu_rate = 200;
  double sample_dt = 0.08;
  double fixed_window_duration = 20.0;
  double sliding_window_duration = 6.0;
  double sweep_duration = 0.5;
  // optimisation (lio_config.h:39-45)
  double gravity_norm = 9.81;
  int outer_iter_num_max = 1;
  int inner_iter_num_max = 100;
  // not in the reference: true = reproduce its quirks (Q1/Q3 Jacobians, Q11 fixed window never trimmed); false = the
  // mathematically intended behaviour (accumulated Jacobians, fixed window trimmed to fixed_window_duration)
  bool reference_quirks = true;
  // not in the reference (which always does it): log the residual histograms of the three factor families before and
  // after every solve (PrintSurfelResiduals / PrintImuResiduals, lidar_odometry.cc:56-94, :547-549, :568-570) - two more passes
  // over the factors and a read-back of every residual per sweep
  bool log_residual_histograms = false;
  // not in the reference (which always publishes): fill LidarOdometry::last_outputs() after every sweep with what the reference
  // hands to ROS there (lidar_odometry.cc:582-602): the sliding window's surfel markers, the sweep undistorted with the final
  // poses as a PointCloud2 payload, the world -> imu_link transform.  Costs a read-back of the window's surfels per sweep.
  bool fill_outputs = false;
  // not in the reference: surfel-extraction arithmetic (wc_params.exact_sums).  false (default) = the order-independent integer
  // moments every benchmark number is quoted on (ids / counts exact, geometry ~1e-9); true = every sum in the reference's order
  bool exact_sums = false;
  // not in the reference (whose accumulated map is built by RViz from /scan_in_imu_frame, lidar_odometry.cc:584-595): voxel side [m] of
  // the device-resident map every sweep is inserted into after its solve (DownSamplingVoxel, surfel_extraction.cc:228-261, over all
  // sweeps; include/wildcat_hip.h: wc_map_*).  0 (default) = no map: nothing allocated or launched.  Otherwise 0.01 <= v <= 4.0
  double map_voxel_size = 0.0;
  // not in the reference: half-side [m] of the axis-aligned cube, centred on the sweep's world -> imu_link origin (the tf of
  // last_outputs()), that the map is cropped to after every sweep's insert (wc_map_crop: the voxels outside are dropped and the table
  // is compacted).  0 (default) = the map is unbounded and nothing extra is launched.  Needs map_voxel_size > 0
  double map_keep_radius = 0.0;
  // the map also accumulates every voxel's second moments (wc_map_create_ex, WC_MAP_MOMENTS): ExportMapSurfels and QueryMapPlanes answer
  // with the plane through a voxel's points.  false (default) = the plain map: nothing more allocated or launched.  Needs map_voxel_size > 0
  bool map_surfels = false;
  // not in the reference: per-sweep carving of the map (wc_map_carve_remove).  After a sweep's insert, the occupied voxels that at least
  // map_carve_min_rays of the rays sensor -> point (the points the insert took; the sensor: the sweep's world -> imu_link origin, the tf of
  // last_outputs()) no longer than map_carve_range [m] pass through, farther than map_carve_shell voxels from the ray's end, and in which no
  // point of the sweep lies, are removed in place - before the keep-radius crop.  0 (default) = off: nothing allocated or launched.
  // Needs map_voxel_size > 0.  Set through LidarOdometry::SetMapCarve
  double map_carve_range = 0.0;
  uint32_t map_carve_shell = 1;
  uint32_t map_carve_min_rays = 2;
};

// LioConfig's reference fields (lio_config.h:8-41) as a plain C struct: what wc_odom_get_config / wc_odom_set_config of the flat C
// wrapper (odom_c_api.cc) exchange.  The switches that are not in the reference keep their own setters.
extern "C" {
typedef struct wc_odom_config {
  double gyroscope_noise_density, accelerometer_noise_density, gyroscope_random_walk, accelerometer_random_walk, imu_factor_weight;
  double max_range, min_range;
  double blind_min[3], blind_max[3];
  double ext_translation[3];
  double ext_rotation[9];  // row-major, lidar -> imu
  double imu_rate, sample_dt, fixed_window_duration, sliding_window_duration, sweep_duration;
  double gravity_norm;
  int32_t outer_iter_num_max, inner_iter_num_max;
} wc_odom_config;
}

inline void ConfigToC(const LioConfig &c, wc_odom_config *o) {
  o->gyroscope_noise_density = c.gyroscope_noise_density, o->accelerometer_noise_density = c.accelerometer_noise_density;
  o->gyroscope_random_walk = c.gyroscope_random_walk, o->accelerometer_random_walk = c.accelerometer_random_walk;
  o->imu_factor_weight = c.imu_factor_weight;
  o->max_range = c.max_range, o->min_range = c.min_range;
  for (int i = 0; i < 3; ++i) o->blind_min[i] = c.blind_min[i], o->blind_max[i] = c.blind_max[i], o->ext_translation[i] = c.ext_translation[i];
  for (int i = 0; i < 9; ++i) o->ext_rotation[i] = c.ext_rotation[i];
  o->imu_rate = c.imu_rate, o->sample_dt = c.sample_dt, o->fixed_window_duration = c.fixed_window_duration;
  o->sliding_window_duration = c.sliding_window_duration, o->sweep_duration = c.sweep_duration;
  o->gravity_norm = c.gravity_norm;
  o->outer_iter_num_max = c.outer_iter_num_max, o->inner_iter_num_max = c.inner_iter_num_max;
}

// the reference fields of *c from o; every other field of *c stays
inline void ConfigFromC(const wc_odom_config &o, LioConfig *c) {
  c->gyroscope_noise_density = o.gyroscope_noise_density, c->accelerometer_noise_density = o.accelerometer_noise_density;
  c->gyroscope_random_walk = o.gyroscope_random_walk, c->accelerometer_random_walk = o.accelerometer_random_walk;
  c->imu_factor_weight = o.imu_factor_weight;
  c->max_range = o.max_range, c->min_range = o.min_range;
  for (int i = 0; i < 3; ++i) c->blind_min[i] = o.blind_min[i], c->blind_max[i] = o.blind_max[i], c->ext_translation[i] = o.ext_translation[i];
  for (int i = 0; i < 9; ++i) c->ext_rotation[i] = o.ext_rotation[i];
  c->imu_rate = o.imu_rate, c->sample_dt = o.sample_dt, c->fixed_window_duration = o.fixed_window_duration;
  c->sliding_window_duration = o.sliding_window_duration, c->sweep_duration = o.sweep_duration;
  c->gravity_norm = o.gravity_norm;
  c->outer_iter_num_max = o.outer_iter_num_max, c->inner_iter_num_max = o.inner_iter_num_max;
}
