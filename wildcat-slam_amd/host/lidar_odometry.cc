// lidar_odometry.cc — host orchestration of one odometry instance around the MI355X C-ABI (see lidar_odometry.h).
// Every block names the reference lines it stands in for (src/odometry/lidar_odometry.cc unless noted).
#include "lidar_odometry.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <limits>
#include <memory>

#include "../csrc/dmath.h"
#include "cubic_bspline.h"
#include "histogram.h"
#include "map_file.h"

using namespace wc;

namespace {

inline V3 v3(const double *p) { return mk3(p[0], p[1], p[2]); }
inline Q4 q4(const double *p) { return Q4{p[0], p[1], p[2], p[3]}; }
inline void st3(double *d, V3 v) { d[0] = v.x, d[1] = v.y, d[2] = v.z; }
inline void stq(double *d, Q4 q) { d[0] = q.w, d[1] = q.x, d[2] = q.y, d[3] = q.z; }

// rotation matrix (row-major) -> unit quaternion; stands in for Eigen::Quaterniond(Matrix3d) + Rigid3's normalisation
Q4 quat_from_matrix(const double *m) {
  const double tr = m[0] + m[4] + m[8];
  Q4 q;
  if (tr > 0) {
    double s = std::sqrt(tr + 1.0) * 2;
    q = {0.25 * s, (m[7] - m[5]) / s, (m[2] - m[6]) / s, (m[3] - m[1]) / s};
  } else if (m[0] > m[4] && m[0] > m[8]) {
    double s = std::sqrt(1.0 + m[0] - m[4] - m[8]) * 2;
    q = {(m[7] - m[5]) / s, 0.25 * s, (m[1] + m[3]) / s, (m[2] + m[6]) / s};
  } else if (m[4] > m[8]) {
    double s = std::sqrt(1.0 + m[4] - m[0] - m[8]) * 2;
    q = {(m[2] - m[6]) / s, (m[1] + m[3]) / s, 0.25 * s, (m[5] + m[7]) / s};
  } else {
    double s = std::sqrt(1.0 + m[8] - m[0] - m[4]) * 2;
    q = {(m[3] - m[1]) / s, (m[2] + m[6]) / s, (m[5] + m[7]) / s, 0.25 * s};
  }
  const double n = std::sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  return {q.w / n, q.x / n, q.y / n, q.z / n};
}

// PredictPoseOfNewImuState (:106-123): constant-acceleration / mid-point gyro dead reckoning
void PredictPoseOfNewImuState(const wc_imu_state &i1, const wc_imu_state &i2, V3 ba, V3 bg, V3 grav, wc_imu_state &i3) {
  const double dt = i3.t - i2.t;
  stq(i3.quat, qmul(q4(i2.quat), so3_exp(((v3(i2.gyr) + v3(i3.gyr)) / 2 - bg) * dt)));
  st3(i3.pos, ((qrot(q4(i1.quat), v3(i1.acc) - ba) + grav) * dt) * dt + 2 * v3(i2.pos) - v3(i1.pos));
}

// a library call that failed: the reference aborts through glog CHECK / LOG(FATAL); so does the facade
[[noreturn]] void FatalCall(const wc_ctx *ctx, const char *what, int rc) {
  std::fprintf(stderr, "[wildcat] FATAL %s (rc=%d): %s\n", what, rc, ctx ? wc_last_error(ctx) : "");
  std::abort();
}

}  // namespace

void LidarOdometry::Fatal(const char *what, int rc) const { FatalCall(ctx_, what, rc); }
#define WC_CHECK(cond)                                                                           \
  do {                                                                                           \
    if (!(cond)) {                                                                               \
      std::fprintf(stderr, "[wildcat] CHECK failed: %s (%s:%d)\n", #cond, __FILE__, __LINE__);   \
      std::abort();                                                                              \
    }                                                                                            \
  } while (0)
#define WC_CALL(expr)                  \
  do {                                 \
    int rc_ = (expr);                  \
    if (rc_ != WC_OK) Fatal(#expr, rc_); \
  } while (0)

namespace {

// A device allocation of the context that lives as long as its scope: freed on every path out of it.  bytes = 0: nothing is allocated
// and p stays null.  A failing library call aborts, as WC_CALL does.
void CheckCall(const wc_ctx *ctx, const char *what, int rc) {
  if (rc != WC_OK) FatalCall(ctx, what, rc);
}
struct DevBuf {
  wc_ctx *ctx;
  void *p = nullptr;
  DevBuf(wc_ctx *c, size_t bytes) : ctx(c) {
    if (bytes) CheckCall(ctx, "wc_dev_alloc", wc_dev_alloc(ctx, bytes, &p));
  }
  ~DevBuf() {
    if (p) CheckCall(ctx, "wc_dev_free", wc_dev_free(ctx, p));
  }
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  void ToHost(void *dst, size_t bytes) const { CheckCall(ctx, "wc_d2h", wc_d2h(ctx, dst, p, bytes)); }
};
// n x 3 host floats into `buf` (allocated for them) and the descriptor the library takes; n = 0: an empty cloud, nothing is copied
wc_points UploadXyz(const DevBuf &buf, const float *xyz, size_t n) {
  if (n) CheckCall(buf.ctx, "wc_h2d", wc_h2d(buf.ctx, buf.p, xyz, n * 3 * sizeof(float)));
  return wc_points{buf.p, nullptr, 12, 0, n};
}

// every record of a query's answer a miss: zeros, d2 = +inf (a wc_map_plane_hit begins with its wc_map_hit)
static_assert(offsetof(wc_map_plane_hit, hit) == 0, "FillMisses writes the wc_map_hit at the start of either record");
template <class Rec>
void FillMisses(Rec *hits, size_t n) {
  wc_map_hit miss;
  std::memset(&miss, 0, sizeof(miss));
  miss.d2 = std::numeric_limits<double>::infinity();
  for (size_t i = 0; i < n; ++i) {
    std::memset(&hits[i], 0, sizeof(Rec));
    std::memcpy(&hits[i], &miss, sizeof(miss));
  }
}

}  // namespace

LidarOdometry::LidarOdometry() : LidarOdometry(0) {}

// the library parameters that follow LioConfig: the four IMU cost weights (lio_config.h:42-45, the expressions and operation order of
// wc_params_default, so that the default LioConfig gives wc_params_default's bytes), imu_dt, solver iterations, the quirk Jacobians
// (Q1 / Q3) and the extraction arithmetic
void WcParamsFromConfig(const LioConfig &c, wc_params *P) {
  wc_params_default(P);
  const double rate = c.imu_rate, k = c.imu_factor_weight;
  P->w_gyr = 1 / (c.gyroscope_noise_density * std::sqrt(rate)) * k;
  P->w_acc = 1 / (c.accelerometer_noise_density * std::sqrt(rate)) * k;
  P->w_bg = 1 / (c.gyroscope_random_walk / std::sqrt(rate)) * k;
  P->w_ba = 1 / (c.accelerometer_random_walk / std::sqrt(rate)) * k;
  P->imu_dt = 1 / rate;
  P->max_iterations = c.inner_iter_num_max;
  P->reference_quirks = c.reference_quirks ? 1 : 0;
  P->exact_sums = c.exact_sums ? 1 : 0;
}
static void ParamsFromConfig(const LioConfig &c, wc_params *P) { WcParamsFromConfig(c, P); }

LidarOdometry::LidarOdometry(int device) {
  wc_params P;
  ParamsFromConfig(config_, &P);
  int rc = wc_ctx_create(&P, device, &ctx_);
  if (rc != WC_OK) {
    std::fprintf(stderr, "[wildcat] FATAL: no MI355X context (rc=%d); there is no CPU fallback\n", rc);
    std::abort();
  }
  // one-time costs out of the first sweeps: code objects, the matcher's helper context and thread, 2 GB of HBM taken into the pool
  // the library's scratch buffers grow from (a 6.5 s window of a 640 k points/s scanner uses ~1 GB of them)
  rc = wc_ctx_warmup(ctx_, (size_t)2 << 30);
  if (rc != WC_OK) std::fprintf(stderr, "[wildcat] wc_ctx_warmup: %s\n", wc_last_error(ctx_));
  stq(ext_quat_, quat_from_matrix(config_.ext_rotation));
}

// config() hands out a mutable LioConfig; the values the library holds a copy of (wc_params) and the extrinsic quaternion are
// re-derived here.  Call after changing config() and before the next AddLidarScan.
void LidarOdometry::ApplyConfig() {
  wc_params P;
  ParamsFromConfig(config_, &P);
  WC_CALL(wc_ctx_set_params(ctx_, &P));
  stq(ext_quat_, quat_from_matrix(config_.ext_rotation));
}

// a whole configuration at once, checked before anything of it is taken: false - config() and the context's parameters as they were,
// config_error() says why - once IMU or lidar data has been added (a change in mid-stream is not supported), when a window or timing value
// cannot be run with, or when wc_params_check refuses the parameters derived from c (a zero noise density gives an infinite weight,
// imu_rate = 0 an infinite imu_dt)
bool LidarOdometry::SetConfig(const LioConfig &c) {
  config_error_.clear();
  if (data_added_) {
    config_error_ = "the configuration cannot change once IMU or lidar data has been added";
    return false;
  }
  const struct {
    const char *name;
    double v;
  } positive[] = {{"imu_rate", c.imu_rate},
                  {"sample_dt", c.sample_dt},
                  {"sweep_duration", c.sweep_duration},
                  {"sliding_window_duration", c.sliding_window_duration},
                  {"fixed_window_duration", c.fixed_window_duration},
                  {"gravity_norm", c.gravity_norm},
                  {"max_range", c.max_range}};
  for (const auto &f : positive)
    if (!(std::isfinite(f.v) && f.v > 0)) {
      config_error_ = std::string(f.name) + " must be finite and > 0";
      return false;
    }
  bool finite = std::isfinite(c.min_range);
  for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(c.blind_min[i]) && std::isfinite(c.blind_max[i]) && std::isfinite(c.ext_translation[i]);
  for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(c.ext_rotation[i]);
  if (!finite || c.outer_iter_num_max < 0) {
    config_error_ = !finite ? "min_range, the blind box and the extrinsics must be finite" : "outer_iter_num_max must be >= 0";
    return false;
  }
  wc_params P;
  ParamsFromConfig(c, &P);
  const char *field = nullptr;
  if (wc_params_check(&P, &field) != WC_OK) {
    config_error_ = std::string("the derived parameter ") + (field ? field : "?") + " is refused (wc_params_check)";
    return false;
  }
  config_ = c;
  ApplyConfig();
  return true;
}

// test hook (not in the reference): overwrite the window's sample states and IMU states with another run's (23 doubles per
// sample state: timestamp, cor[12], grav[3], quat[4], pos[3]) and re-attach the surfel poses, so that every sweep of a
// comparison starts from the same states.  The counts must equal the facade's own.
bool LidarOdometry::ImportState(const double *samples23, size_t ns, const wc_imu_state *imu, size_t n_imu) {
  if (ns != samples_.size() || n_imu != imu_states_.size()) return false;
  for (size_t i = 0; i < ns; ++i) {
    const double *p = samples23 + 23 * i;
    Sample &s = samples_[i];
    if (s.timestamp != p[0]) return false;
    std::memcpy(s.cor, p + 1, 96);
    std::memcpy(s.grav, p + 13, 24);
    std::memcpy(s.quat, p + 16, 32);
    std::memcpy(s.pos, p + 20, 24);
  }
  for (size_t i = 0; i < n_imu; ++i) imu_states_[i] = imu[i];
  TouchImu();
  UpdateSurfelPosesOnDevice();
  return true;
}

LidarOdometry::~LidarOdometry() {
  if (!ctx_) return;
  if (d_res_) wc_dev_free(ctx_, d_res_);
  if (map_) wc_map_destroy(ctx_, map_);
  void *bufs[] = {d_surf_, d_pose_, d_inbody_, d_pairs_sld_, d_pairs_fix_, d_imu_, d_sweep_xyz_, d_sweep_t_, d_kept_t_, d_scan_raw_, d_pts_[0], d_pts_[1], d_fix_surf_, d_fix_pose_, d_world_};
  for (void *b : bufs)
    if (b) wc_dev_free(ctx_, b);
  wc_ctx_destroy(ctx_);
}

void LidarOdometry::AddImuData(const ImuData &msg) {  // :607-611
  data_added_ = true;
  imu_buff_.push_back(msg);
}

bool LidarOdometry::latest_state(SampleStateView *out) const {
  return !samples_.empty() && sample_state(samples_.size() - 1, out);
}
bool LidarOdometry::sample_state(size_t i, SampleStateView *out) const {
  if (i >= samples_.size()) return false;
  const Sample &s = samples_[i];
  out->timestamp = s.timestamp;
  std::memcpy(out->pos, s.pos, 24);
  std::memcpy(out->quat, s.quat, 32);
  std::memcpy(out->bg, s.cor + 6, 24);
  std::memcpy(out->ba, s.cor + 9, 24);
  return true;
}

// room for n more sliding-window surfels behind n_surfels_; a reallocation drops the dead prefix [0, sld_begin_)
void LidarOdometry::EnsureSurfelCapacity(size_t n) {
  if (n_surfels_ + n <= cap_surfels_) return;
  const size_t live = n_surfels_ - sld_begin_;
  const size_t cap = std::max<size_t>((live + n) + (live + n) / 2, 1 << 18);  // (262 k surfels = 57 MB from the start: the room stream's window crossed 65 k in its fifth sweep - five allocations and three copies, 0.5 ms)
  void *ns = nullptr, *np = nullptr, *nb = nullptr, *p1 = nullptr, *p2 = nullptr;
  WC_CALL(wc_dev_alloc(ctx_, cap * sizeof(wc_surfel), &ns));
  WC_CALL(wc_dev_alloc(ctx_, cap * sizeof(wc_pose), &np));
  WC_CALL(wc_dev_alloc(ctx_, cap, &nb));
  WC_CALL(wc_dev_alloc(ctx_, cap * sizeof(wc_pair), &p1));
  WC_CALL(wc_dev_alloc(ctx_, cap * sizeof(wc_pair), &p2));
  if (live) {
    WC_CALL(wc_d2d(ctx_, ns, d_surf_ + sld_begin_, live * sizeof(wc_surfel)));
    WC_CALL(wc_d2d(ctx_, np, d_pose_ + sld_begin_, live * sizeof(wc_pose)));
    WC_CALL(wc_d2d(ctx_, nb, d_inbody_ + sld_begin_, live));
  }
  void *old[] = {d_surf_, d_pose_, d_inbody_, d_pairs_sld_, d_pairs_fix_};
  for (void *b : old)
    if (b) WC_CALL(wc_dev_free(ctx_, b));
  d_surf_ = (wc_surfel *)ns, d_pose_ = (wc_pose *)np, d_inbody_ = (uint8_t *)nb;
  d_pairs_sld_ = (wc_pair *)p1, d_pairs_fix_ = (wc_pair *)p2;
  cap_surfels_ = cap;
  n_surfels_ = live;
  sld_begin_ = 0;
}

// room for `extra` more surfels in FRONT of the fixed window (it is filled from the back of its array)
void LidarOdometry::EnsureFixedCapacity(size_t extra) {
  if (extra <= fix_start_) return;
  const size_t live = fix_end_ - fix_start_;
  const size_t cap = std::max<size_t>(2 * (live + extra), 1 << 16);
  void *ns = nullptr, *np = nullptr;
  WC_CALL(wc_dev_alloc(ctx_, cap * sizeof(wc_surfel), &ns));
  WC_CALL(wc_dev_alloc(ctx_, cap * sizeof(wc_pose), &np));
  if (live) {
    WC_CALL(wc_d2d(ctx_, (wc_surfel *)ns + (cap - live), d_fix_surf_ + fix_start_, live * sizeof(wc_surfel)));
    WC_CALL(wc_d2d(ctx_, (wc_pose *)np + (cap - live), d_fix_pose_ + fix_start_, live * sizeof(wc_pose)));
  }
  if (d_fix_surf_) WC_CALL(wc_dev_free(ctx_, d_fix_surf_));
  if (d_fix_pose_) WC_CALL(wc_dev_free(ctx_, d_fix_pose_));
  d_fix_surf_ = (wc_surfel *)ns, d_fix_pose_ = (wc_pose *)np;
  fix_cap_ = cap, fix_end_ = cap, fix_start_ = cap - live;
}

// the per-point loop of AddLidarScan (:489-496) on the device: upload the raw message, wc_prefilter_points (extrinsic,
// range / blind-box filter) appends the survivors to the device-resident points_buff_; only their timestamps come back
void LidarOdometry::AppendScanOnDevice(const pcl::PointCloud<hilti_ros::Point> &msg) {
  const size_t n = msg.size();
  if (n == 0) return;
  if (n > cap_scan_raw_) {
    if (d_scan_raw_) WC_CALL(wc_dev_free(ctx_, d_scan_raw_));
    cap_scan_raw_ = n + n / 2;
    WC_CALL(wc_dev_alloc(ctx_, cap_scan_raw_ * sizeof(hilti_ros::Point), &d_scan_raw_));
  }
  WC_CALL(wc_h2d(ctx_, d_scan_raw_, msg.points.data(), n * sizeof(hilti_ros::Point)));
  // make room behind pts_end_: consumed points in front are dropped by moving the live range to the other buffer
  const size_t live = pts_end_ - pts_begin_;
  if (pts_end_ + n > cap_pts_[pts_cur_]) {
    const int other = pts_cur_ ^ 1;
    if (live + n > cap_pts_[other]) {
      if (d_pts_[other]) WC_CALL(wc_dev_free(ctx_, d_pts_[other]));
      cap_pts_[other] = 2 * (live + n);
      WC_CALL(wc_dev_alloc(ctx_, cap_pts_[other] * sizeof(hilti_ros::Point), &d_pts_[other]));
    }
    if (live)
      WC_CALL(wc_d2d(ctx_, d_pts_[other], (const char *)d_pts_[pts_cur_] + pts_begin_ * sizeof(hilti_ros::Point), live * sizeof(hilti_ros::Point)));
    pts_cur_ = other, pts_begin_ = 0, pts_end_ = live;
  }
  uint64_t kept = 0;
  char *dst = (char *)d_pts_[pts_cur_] + pts_end_ * sizeof(hilti_ros::Point);
  if (n > cap_kept_t_) {
    if (d_kept_t_) WC_CALL(wc_dev_free(ctx_, d_kept_t_));
    cap_kept_t_ = n + n / 2;
    WC_CALL(wc_dev_alloc(ctx_, cap_kept_t_ * sizeof(double), &d_kept_t_));
  }
  // CHECK(points_buff_.empty() || pt.time >= points_buff_.back().time) (:491) runs on the device too: every incoming point,
  // filtered or not, against the last BUFFERED point at that moment; the survivors' stamps come back packed
  int monotonic = 1;
  WC_CALL(wc_prefilter_points_checked(ctx_, d_scan_raw_, n, ext_quat_, config_.ext_translation, config_.min_range, config_.max_range,
                                      config_.blind_min, config_.blind_max, dst, cap_pts_[pts_cur_] - pts_end_, &kept,
                                      point_times_.empty() ? -INFINITY : point_times_.back(), (double *)d_kept_t_, &monotonic));
  WC_CHECK(monotonic);
  std::vector<double> kt(kept);
  if (kept) WC_CALL(wc_d2h(ctx_, kt.data(), d_kept_t_, kept * sizeof(double)));
  point_times_.insert(point_times_.end(), kt.begin(), kt.end());
  pts_end_ += kept;
}

void LidarOdometry::DropBufferedPoints(size_t k) {
  pts_begin_ += k;
  point_times_.erase(point_times_.begin(), point_times_.begin() + (long)k);
}

// SyncHeadingMsgs (:457-485)
bool LidarOdometry::SyncHeadingMsgs() {
  if (sync_done_) return true;
  if (imu_buff_.empty() || point_times_.empty()) return false;
  if (imu_buff_.back().timestamp < point_times_.front()) return false;
  while (imu_buff_.front().timestamp < point_times_.front()) {
    imu_buff_.pop_front();
    WC_CHECK(!imu_buff_.empty());
  }
  while (point_times_.front() < imu_buff_.front().timestamp) {
    DropBufferedPoints(1);
    WC_CHECK(!point_times_.empty());
  }
  sync_done_ = true;
  return true;
}

// PredictImuStatesAndSampleStates (:365-455)
void LidarOdometry::PredictImuStatesAndSampleStates(double end_time) {
  WC_CHECK(imu_buff_.size() >= 2);
  TouchImu();
  const double dt = 1 / config_.imu_rate;
  if (!init_sld_win_) {
    for (int i = 0; i < 2; ++i) {
      const ImuData m = imu_buff_.front();
      imu_buff_.pop_front();
      wc_imu_state s{};
      s.t = m.timestamp;
      for (int d = 0; d < 3; ++d) s.acc[d] = m.linear_acceleration[d], s.gyr[d] = m.angular_velocity[d], s.pos[d] = 0;
      if (i == 0)
        stq(s.quat, Q4{1, 0, 0, 0});
      else
        stq(s.quat, so3_exp(((v3(imu_states_.back().gyr) + v3(s.gyr)) / 2) * dt));
      imu_states_.push_back(s);
    }
    Sample ss{};
    ss.timestamp = imu_states_.front().t;
    const V3 a0 = v3(imu_states_.front().acc);
    st3(ss.grav, (-config_.gravity_norm) * (a0 / norm(a0)));
    std::memcpy(ss.quat, imu_states_.front().quat, 32);
    std::memcpy(ss.pos, imu_states_.front().pos, 24);
    samples_.push_back(ss);
    first_sample_time_ = ss.timestamp;
    first_sample_known_ = true;
    init_sld_win_ = true;
  }
  const double old_last = samples_.back().timestamp;
  const int add_size = (int)((end_time - old_last) / config_.sample_dt);
  const double add_last = old_last + config_.sample_dt * add_size;
  const V3 ba = v3(samples_.back().cor + 9), bg = v3(samples_.back().cor + 6), grav = v3(samples_.back().grav);
  while (!imu_buff_.empty()) {
    const size_t size = imu_states_.size();
    const ImuData m = imu_buff_.front();
    imu_buff_.pop_front();
    wc_imu_state s{};
    s.t = m.timestamp;
    for (int d = 0; d < 3; ++d) s.acc[d] = m.linear_acceleration[d], s.gyr[d] = m.angular_velocity[d];
    WC_CHECK(std::fabs((s.t - imu_states_[size - 1].t) - (imu_states_[size - 1].t - imu_states_[size - 2].t)) <= 1e-6);
    PredictPoseOfNewImuState(imu_states_[size - 2], imu_states_[size - 1], ba, bg, grav, s);
    imu_states_.push_back(s);
    if (s.t >= add_last) break;  // enough imu states
  }
  for (int i = 1; i <= add_size; ++i) {
    const double t = old_last + i * config_.sample_dt;
    Sample ss{};
    ss.timestamp = t;
    st3(ss.cor + 9, ba), st3(ss.cor + 6, bg), st3(ss.grav, grav);
    size_t idx = std::lower_bound(imu_states_.begin(), imu_states_.end(), t,
                                  [](const wc_imu_state &a, double b) { return a.t < b; }) - imu_states_.begin();
    WC_CHECK(idx != 0 && idx != imu_states_.size());
    const wc_imu_state &a = imu_states_[idx - 1], &b = imu_states_[idx];
    const double f = (t - a.t) / (b.t - a.t);
    stq(ss.quat, qslerp(q4(a.quat), f, q4(b.quat)));
    st3(ss.pos, (1 - f) * v3(a.pos) + f * v3(b.pos));
    WC_CHECK(f >= 0 && f <= 1);
    samples_.push_back(ss);
  }
}

// PrintSurfelResiduals x 2 + PrintImuResiduals (:56-94) on the problem wc_window_build holds: ONE wc_window_evaluate (the
// reference's three problem.Evaluate calls, each on one family's blocks, apply_loss_function = true) gives the loss-corrected
// residuals in the reference's block order - binary, unary, 12 per IMU factor.  The cost the reference prints is problem.Evaluate's
// 0.5 * sum rho(s): for the IMU family (TrivialLoss) half the squared norm; for the surfel families (CauchyLoss(0.4), cc:273,311)
// the corrected residual is r' = sqrt(rho'(s)) r with rho(s) = b log(1 + s / b), b = 0.16, so s = r'^2 / (1 - r'^2 / b) is
// recovered and rho summed - half the squared norm of r' would understate it (0.08 against 0.111 at s = b).  The
// text goes to last_residual_log() (and to stderr with WC_ODOM_DEBUG): the reference's LOG(INFO) lines, glog prefix aside.
void LidarOdometry::LogResiduals(const std::vector<double> &x, const char *when) {
  uint64_t cnt[4] = {0, 0, 0, 0};
  WC_CALL(wc_window_counts(ctx_, cnt));
  const size_t nb = cnt[0], nu = cnt[1], ni = cnt[2], nres = nb + nu + 12 * ni;
  if (nres == 0) return;
  if (nres > cap_res_) {
    if (d_res_) WC_CALL(wc_dev_free(ctx_, d_res_));
    cap_res_ = nres + nres / 2;
    WC_CALL(wc_dev_alloc(ctx_, cap_res_ * sizeof(double), &d_res_));
  }
  double cost = 0;
  WC_CALL(wc_window_evaluate(ctx_, x.data(), &cost, (double *)d_res_));
  std::vector<double> r(nres);
  WC_CALL(wc_d2h(ctx_, r.data(), d_res_, nres * sizeof(double)));
  char buf[96];
  wc_params P;
  ParamsFromConfig(config_, &P);
  const double cb = P.cauchy_a * P.cauchy_a;
  auto surfel = [&](size_t first, size_t n, const char *window_type) {
    if (n == 0) return;  // (:57-59)
    Histogram hist;
    double c = 0;
    for (size_t i = first; i < first + n; ++i) {
      hist.Add(r[i]);
      // (r'^2 = s / (1 + s / b) < b; for a strong outlier r'^2 rounds to b itself: the denominator is clamped, the logged cost stays
      // finite where the reference prints a finite rho - ADVICE r4)
      const double q = r[i] * r[i], s = q / std::max(1.0 - q / cb, 2.220446049250313e-16);
      c += cb * std::log1p(s / cb);
    }
    std::snprintf(buf, sizeof(buf), " Surfel residuals, cost: %g, dist: ", 0.5 * c);
    residual_log_ += std::string(when) + window_type + buf + hist.ToString(10) + "\n";
  };
  surfel(0, nb, "Sliding Window");
  surfel(nb, nu, "Fixed Window");
  if (ni) {  // (:74-93)
    Histogram hist[4];
    const char *types[4] = {"gyro", "acc", "gyro_bias", "acc_bias"};
    double c = 0;
    for (size_t i = nb + nu; i < nres; i += 12)
      for (int j = 0; j < 4; ++j) {
        const double *p = &r[i + 3 * j];
        const double s2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
        hist[j].Add(std::sqrt(s2));
        c += s2;
      }
    for (int j = 0; j < 4; ++j) {
      std::snprintf(buf, sizeof(buf), ", cost: %g, dist: ", 0.5 * c);
      residual_log_ += std::string(when) + "Imu residuals with type " + types[j] + buf + hist[j].ToString(10) + "\n";
    }
  }
}

// the sweep undistorted once more with the poses the solve left behind (:584-595): what FillOutputs publishes and the map takes in
const void *LidarOdometry::UndistortFinal(const void *d_raw_sweep, size_t n_sweep) {
  if (n_sweep > cap_world_) {
    if (d_world_) WC_CALL(wc_dev_free(ctx_, d_world_));
    cap_world_ = n_sweep * 2;
    WC_CALL(wc_dev_alloc(ctx_, cap_world_ * sizeof(hilti_ros::Point), &d_world_));
  }
  UploadImuStates();
  WC_CALL(wc_undistort_sweep(ctx_, d_raw_sweep, n_sweep, d_imu_, imu_states_.size(), d_world_));
  return d_world_;
}

// what the reference hands to ROS at the end of AddLidarScan (:582-602), as plain data
void LidarOdometry::FillOutputs(const void *d_world_sweep, size_t n_sweep) {
  // PubSurfels(surfels_sld_win_, ...) (:582, surfel_extraction.cc:360-434)
  const size_t n = n_surfels_ - sld_begin_;
  std::vector<wc_surfel> surf(n);
  std::vector<wc_pose> pose(n);
  if (n) {
    WC_CALL(wc_d2h(ctx_, surf.data(), d_surf_ + sld_begin_, n * sizeof(wc_surfel)));
    WC_CALL(wc_d2h(ctx_, pose.data(), d_pose_ + sld_begin_, n * sizeof(wc_pose)));
  }
  outputs_.markers.resize(n);
  for (size_t i = 0; i < n; ++i) outputs_.markers[i] = wc_wire::MarkerFromSurfel(surf[i], pose[i]);
  // the sweep with the final poses (:584-595)
  std::vector<hilti_ros::Point> pts(n_sweep);
  if (n_sweep) WC_CALL(wc_d2h(ctx_, pts.data(), d_world_sweep, n_sweep * sizeof(hilti_ros::Point)));
  wc_wire::Cloud2FromPoints(pts.data(), pts.size(), outputs_.scan_in_world);
  outputs_.scan_stamp = n_sweep ? pts[0].time : 0.0;
  // tf world -> imu_link (:596-602)
  const Sample &b = samples_.back();
  outputs_.tf.stamp = b.timestamp;
  std::memcpy(outputs_.tf.origin, b.pos, 24);
  outputs_.tf.rotation_xyzw[0] = b.quat[1], outputs_.tf.rotation_xyzw[1] = b.quat[2], outputs_.tf.rotation_xyzw[2] = b.quat[3], outputs_.tf.rotation_xyzw[3] = b.quat[0];
}

// ---- the accumulated map (config().map_voxel_size) ----------------------------------------------------------------------------
bool LidarOdometry::SetMapVoxel(double voxel) {
  if (voxel != 0.0 && !(voxel >= 0.01 && voxel <= 4.0)) return false;
  config_.map_voxel_size = voxel;
  if (map_) WC_CALL(wc_map_destroy(ctx_, map_));
  map_ = nullptr;
  EnsureMap();
  return true;
}
// the map follows config().map_voxel_size: created on first use, re-created (empty) when the size changed, removed at 0
void LidarOdometry::EnsureMap() {
  const double v = config_.map_voxel_size;
  if (map_ && map_voxel_ == v && map_moments_ == config_.map_surfels) return;
  if (map_) WC_CALL(wc_map_destroy(ctx_, map_));
  map_ = nullptr;
  if (v == 0.0) return;
  WC_CALL(wc_map_create_ex(ctx_, v, (size_t)1 << 20, config_.map_surfels ? WC_MAP_MOMENTS : 0u, &map_));
  map_voxel_ = v;
  map_moments_ = config_.map_surfels;
}
void LidarOdometry::SetMapSurfels(bool on) {
  config_.map_surfels = on;
  if (map_) WC_CALL(wc_map_destroy(ctx_, map_));
  map_ = nullptr;
  EnsureMap();
}
size_t LidarOdometry::ExportMapSurfels(wc_map_surfel *surfels, size_t cap) {
  if (!map_ || !map_moments_) return 0;
  uint64_t n = map_voxels();
  if (n == 0 || cap < n || !surfels) return n;
  const DevBuf d_out(ctx_, n * sizeof(wc_map_surfel));
  WC_CALL(wc_map_export_surfels(ctx_, map_, (wc_map_surfel *)d_out.p, n, &n));
  d_out.ToHost(surfels, n * sizeof(wc_map_surfel));
  return n;
}
size_t LidarOdometry::QueryMapPlanes(const float *xyz, size_t n, double max_dist, uint32_t min_points, wc_map_plane_hit *hits) {
  if (!n || !xyz || !hits) return 0;
  if (!map_ || !map_moments_ || min_points < 3) {
    FillMisses(hits, n);
    return 0;
  }
  const DevBuf d_xyz(ctx_, n * 3 * sizeof(float)), d_hits(ctx_, n * sizeof(wc_map_plane_hit));
  const wc_points desc = UploadXyz(d_xyz, xyz, n);
  uint64_t found = 0;
  WC_CALL(wc_map_nearest_plane(ctx_, map_, &desc, max_dist, min_points, (wc_map_plane_hit *)d_hits.p, &found));
  d_hits.ToHost(hits, n * sizeof(wc_map_plane_hit));
  return found;
}
bool LidarOdometry::AlignToMap(const float *xyz, size_t n, double T_io[12], const wc_map_align_opts &opts, wc_map_align_summary *summary) {
  if (!map_ || !map_moments_ || !T_io || (n && !xyz)) return false;
  const DevBuf d_xyz(ctx_, n * 3 * sizeof(float));
  const wc_points desc = UploadXyz(d_xyz, xyz, n);
  double T[12];
  std::memcpy(T, T_io, sizeof(T));
  wc_map_align_summary s;
  if (wc_map_align(ctx_, map_, &desc, T, &opts, &s) != WC_OK) return false;  // (an argument the library refuses is the caller's: no abort)
  std::memcpy(T_io, T, sizeof(T));
  if (summary) *summary = s;
  return true;
}
bool LidarOdometry::AlignSweepToMap(const void *points48, size_t n, wc_pose *pose_begin_io, wc_pose *pose_end_io, const wc_map_ct_align_opts &opts,
                                    wc_map_ct_align_summary *summary, bool insert) {
  if (!map_ || !map_moments_ || !pose_begin_io || !pose_end_io || !n || !points48) return false;
  double t_begin = std::numeric_limits<double>::infinity(), t_end = -t_begin;
  for (size_t i = 0; i < n; ++i) {
    double t;
    std::memcpy(&t, (const char *)points48 + i * WC_HILTI_POINT_BYTES + WC_HILTI_POINT_TIME_OFFSET, sizeof(t));
    if (std::isfinite(t)) t_begin = std::min(t_begin, t), t_end = std::max(t_end, t);
  }
  if (!(t_begin < t_end)) return false;
  const DevBuf d_pts(ctx_, n * WC_HILTI_POINT_BYTES), d_out(ctx_, insert ? n * 3 * sizeof(float) : 0);
  CheckCall(ctx_, "wc_h2d", wc_h2d(ctx_, d_pts.p, points48, n * WC_HILTI_POINT_BYTES));
  const wc_points desc{d_pts.p, (const char *)d_pts.p + WC_HILTI_POINT_TIME_OFFSET, WC_HILTI_POINT_BYTES, WC_HILTI_POINT_BYTES, n};
  wc_pose b = *pose_begin_io, e = *pose_end_io;
  wc_map_ct_align_summary s;
  // (an argument the library refuses is the caller's: no abort, as in AlignToMap)
  if (wc_map_align_ct(ctx_, map_, &desc, &b, &e, t_begin, t_end, &opts, &s) != WC_OK) return false;
  if (insert) {  // the registered sweep at the final poses, straight from the linearisation's own moved points
    wc_map_ct_normal_eq ne;
    if (wc_map_linearize_ct(ctx_, map_, &desc, &b, &e, t_begin, t_end, &opts.reg, &ne, nullptr, (float *)d_out.p) != WC_OK) return false;
    const wc_points moved{d_out.p, nullptr, 12, 0, n};
    WC_CALL(wc_map_insert(ctx_, map_, &moved, nullptr));
  }
  *pose_begin_io = b, *pose_end_io = e;
  if (summary) *summary = s;
  return true;
}
namespace {
constexpr uint32_t kMaxLevels = 8;  // wc_map_align_pyramid's
// the levels of a relocalisation: levels[0] = the coarsest ... levels[n_levels - 1] = the map itself, built finest first, each from the one
// before it by wc_map_coarsen(factor); opts[l]: `finest` with reg.max_dist multiplied by (double)factor per level above the map.  false:
// a level's voxel size would exceed 4.0 (nothing built), or a level could not be built (FreeLevels drops those that were)
bool BuildLevels(wc_ctx *ctx, wc_map *map, double voxel, uint32_t factor, uint32_t n_levels, const wc_map_align_opts &finest,
                 wc_map *(&levels)[kMaxLevels], wc_map_align_opts (&opts)[kMaxLevels]) {
  double V = voxel, scale[kMaxLevels] = {1.0};
  for (uint32_t l = 1; l < n_levels; ++l) {
    V = (double)factor * V;  // (as wc_map_coarsen forms it)
    scale[l] = scale[l - 1] * (double)factor;
    if (!(V <= 4.0)) return false;
  }
  levels[n_levels - 1] = map;
  bool ok = true;
  for (uint32_t l = 1; ok && l < n_levels; ++l)
    ok = wc_map_coarsen(ctx, levels[n_levels - l], factor, WC_MAP_MOMENTS, &levels[n_levels - 1 - l]) == WC_OK;
  for (uint32_t l = 0; l < n_levels; ++l) {
    opts[n_levels - 1 - l] = finest;
    opts[n_levels - 1 - l].reg.max_dist = finest.reg.max_dist * scale[l];
  }
  return ok;
}
void FreeLevels(wc_ctx *ctx, wc_map *(&levels)[kMaxLevels], uint32_t n_levels) {
  for (uint32_t l = 0; l + 1 < n_levels; ++l)
    if (levels[l]) {
      const int rc = wc_map_destroy(ctx, levels[l]);
      if (rc != WC_OK) FatalCall(ctx, "wc_map_destroy", rc);
    }
}
// What the three relocalisations share: the levels built (BuildLevels), the points uploaded once, the candidate starts in T through ONE
// wc_map_align_pyramid_batch, the built levels destroyed.  seed(coarsest level, points) runs ahead of the alignment and may still fill T;
// false from it ends the call.  T: K x 12 doubles, the starts in and the aligned poses out; s: n_levels x K summaries, level-major;
// status: K codes.  false: BuildLevels' cases, the seed's, or arguments the library refuses (no abort: as in AlignToMap)
// (upload(): the points' descriptor, called once the levels stand - the host cloud uploaded into a buffer of the call, or points that are
// in device memory already, as MergeMapFile's exported centroids)
template <class Upload, class Seed>
bool AlignCandidatesOf(wc_ctx *ctx, wc_map *map, double voxel, Upload upload, uint32_t factor, uint32_t n_levels, const wc_map_align_opts &finest,
                       Seed seed, std::vector<double> &T, std::vector<wc_map_align_summary> &s, std::vector<int32_t> &status) {
  wc_map *levels[kMaxLevels] = {};
  wc_map_align_opts opts[kMaxLevels];
  bool ok = BuildLevels(ctx, map, voxel, factor, n_levels, finest, levels, opts);
  if (ok) {
    const wc_points desc = upload();
    ok = seed(levels[0], desc);
    if (ok) {
      const uint32_t K = (uint32_t)(T.size() / 12);
      s.resize((size_t)n_levels * K), status.resize(K);
      ok = wc_map_align_pyramid_batch(ctx, levels, n_levels, &desc, T.data(), K, opts, s.data(), status.data()) == WC_OK;
    }
  }
  FreeLevels(ctx, levels, n_levels);
  return ok;
}
template <class Seed>
bool AlignCandidates(wc_ctx *ctx, wc_map *map, double voxel, const float *xyz, size_t n, uint32_t factor, uint32_t n_levels,
                     const wc_map_align_opts &finest, Seed seed, std::vector<double> &T, std::vector<wc_map_align_summary> &s,
                     std::vector<int32_t> &status) {
  std::unique_ptr<DevBuf> d_xyz;  // (allocated by upload(): behind BuildLevels, as before)
  const auto upload = [&] {
    d_xyz.reset(new DevBuf(ctx, n * 3 * sizeof(float)));
    return UploadXyz(*d_xyz, xyz, n);
  };
  return AlignCandidatesOf(ctx, map, voxel, upload, factor, n_levels, finest, seed, T, s, status);
}
const auto kNoSeed = [](wc_map *, const wc_points &) { return true; };
}  // namespace
bool LidarOdometry::RelocalizeToMap(const float *xyz, size_t n, double T_io[12], uint32_t factor, uint32_t n_levels, const wc_map_align_opts &finest,
                                    wc_map_align_summary *summaries) {
  if (!map_ || !map_moments_ || !T_io || (n && !xyz) || factor < 1 || n_levels < 1 || n_levels > kMaxLevels) return false;
  std::vector<double> T(T_io, T_io + 12);
  std::vector<wc_map_align_summary> s;
  std::vector<int32_t> status;
  // (one hypothesis: by the batched form's contract what wc_map_align_pyramid leaves; its error is the hypothesis's status)
  if (!AlignCandidates(ctx_, map_, map_voxel_, xyz, n, factor, n_levels, finest, kNoSeed, T, s, status) || status[0] != WC_OK) return false;
  std::memcpy(T_io, T.data(), 12 * sizeof(double));
  if (summaries) std::memcpy(summaries, s.data(), s.size() * sizeof(s[0]));
  return true;
}
bool LidarOdometry::RelocalizeSearch(const float *xyz, size_t n, double T_io[12], uint32_t n_yaw, uint32_t factor, uint32_t n_levels,
                                     const wc_map_align_opts &finest, wc_map_align_summary *summaries, int32_t *best) {
  if (!map_ || !map_moments_ || !T_io || (n && !xyz) || factor < 1 || n_levels < 1 || n_levels > kMaxLevels || n_yaw < 1 || n_yaw > 1024)
    return false;
  std::vector<double> T((size_t)n_yaw * 12);
  std::vector<wc_map_align_summary> s;
  std::vector<int32_t> status;
  int32_t win = -1;
  if (wc_pose_yaw_grid(T_io, n_yaw, T.data()) != WC_OK ||
      !AlignCandidates(ctx_, map_, map_voxel_, xyz, n, factor, n_levels, finest, kNoSeed, T, s, status) ||
      wc_map_align_best(s.data() + (size_t)(n_levels - 1) * n_yaw, status.data(), n_yaw, finest.min_used, &win) != WC_OK || win < 0)
    return false;
  std::memcpy(T_io, T.data() + (size_t)win * 12, 12 * sizeof(double));
  if (summaries) std::memcpy(summaries, s.data(), s.size() * sizeof(s[0]));
  if (best) *best = win;
  return true;
}
bool LidarOdometry::RelocalizeGlobal(const float *xyz, size_t n, double T_io[12], uint32_t n_yaw, const uint32_t n_xyz[3], const double step[3],
                                     uint32_t top_m, uint32_t factor, uint32_t n_levels, const wc_map_align_opts &finest,
                                     wc_map_align_summary *summaries, int32_t *best) {
  if (!map_ || !map_moments_ || !T_io || (n && !xyz) || factor < 1 || n_levels < 1 || n_levels > kMaxLevels || top_m < 1 || top_m > 1024 ||
      !n_xyz || !step)
    return false;
  uint64_t K = n_yaw;  // (wc_pose_grid refuses what is out of range; here only the size of its output is needed)
  for (int a = 0; a < 3; ++a) K = K > ((uint64_t)1 << 20) ? K : K * n_xyz[a];
  if (K == 0 || K > ((uint64_t)1 << 20)) return false;
  std::vector<double> grid((size_t)K * 12), T;
  std::vector<wc_map_align_summary> s;
  std::vector<int32_t> status;
  uint32_t cnt = 0;
  // the starts: the top_m best of the grid by their occupancy score on the coarsest level, in rank order
  const auto seed = [&](wc_map *coarsest, const wc_points &desc) {
    std::vector<wc_map_score> scores((size_t)K);
    std::vector<int32_t> idx(top_m);
    const wc_map_score_params sp = {1u, 0u};
    if (wc_map_score_batch(ctx_, coarsest, &desc, grid.data(), (uint32_t)K, &sp, scores.data()) != WC_OK ||
        wc_map_score_top(scores.data(), (uint32_t)K, top_m, finest.min_used, idx.data(), &cnt) != WC_OK || cnt < 1)
      return false;
    T.resize((size_t)cnt * 12);
    for (uint32_t r = 0; r < cnt; ++r) std::memcpy(T.data() + (size_t)r * 12, grid.data() + (size_t)idx[r] * 12, 12 * sizeof(double));
    return true;
  };
  int32_t win = -1;
  if (wc_pose_grid(T_io, n_yaw, n_xyz, step, grid.data()) != WC_OK ||
      !AlignCandidates(ctx_, map_, map_voxel_, xyz, n, factor, n_levels, finest, seed, T, s, status) ||
      wc_map_align_best(s.data() + (size_t)(n_levels - 1) * cnt, status.data(), cnt, finest.min_used, &win) != WC_OK || win < 0)
    return false;
  std::memcpy(T_io, T.data() + (size_t)win * 12, 12 * sizeof(double));
  if (summaries) {  // (level-major with top_m records per level; the candidates that did not exist: zero)
    std::memset(summaries, 0, (size_t)n_levels * top_m * sizeof(summaries[0]));
    for (uint32_t l = 0; l < n_levels; ++l) std::memcpy(summaries + (size_t)l * top_m, s.data() + (size_t)l * cnt, cnt * sizeof(s[0]));
  }
  if (best) *best = win;
  return true;
}
bool LidarOdometry::LinearizeAgainstMap(const float *xyz, size_t n, const double T[12], const wc_map_reg_params &params, wc_map_normal_eq *out,
                                        wc_map_reg_row *rows) {
  if (!map_ || !map_moments_ || !T || !out || (n && !xyz)) return false;
  const DevBuf d_xyz(ctx_, n * 3 * sizeof(float)), d_rows(ctx_, rows ? n * sizeof(wc_map_reg_row) : 0);
  const wc_points desc = UploadXyz(d_xyz, xyz, n);
  wc_map_normal_eq ne;
  if (wc_map_linearize(ctx_, map_, &desc, T, &params, &ne, (wc_map_reg_row *)d_rows.p) != WC_OK) return false;  // (as in AlignToMap)
  if (d_rows.p) d_rows.ToHost(rows, n * sizeof(wc_map_reg_row));
  *out = ne;
  return true;
}
uint64_t LidarOdometry::map_voxels() const {
  uint64_t v = 0;
  if (map_) WC_CALL(wc_map_size(ctx_, map_, &v, nullptr));
  return v;
}
uint64_t LidarOdometry::map_points() const {
  uint64_t p = 0;
  if (map_) WC_CALL(wc_map_size(ctx_, map_, nullptr, &p));
  return p;
}
uint64_t LidarOdometry::map_rejected() const {
  uint64_t info[4] = {0, 0, 0, 0};
  if (map_) WC_CALL(wc_map_info(ctx_, map_, info));
  return info[2];
}
size_t LidarOdometry::ExportMap(float *xyz, uint32_t *counts, size_t cap) {
  if (!map_) return 0;
  uint64_t n = map_voxels();
  if (n == 0 || cap < n || !xyz || !counts) return n;
  const DevBuf d_xyz(ctx_, n * 3 * sizeof(float)), d_cnt(ctx_, n * sizeof(uint32_t));
  WC_CALL(wc_map_export(ctx_, map_, (float *)d_xyz.p, (uint32_t *)d_cnt.p, nullptr, n, &n));
  d_xyz.ToHost(xyz, n * 3 * sizeof(float));
  d_cnt.ToHost(counts, n * sizeof(uint32_t));
  return n;
}
void LidarOdometry::ClearMap() {
  if (map_) WC_CALL(wc_map_clear(ctx_, map_));
}
size_t LidarOdometry::QueryMap(const float *xyz, size_t n, double max_dist, wc_map_hit *hits) {
  if (!n || !xyz || !hits) return 0;
  if (!map_) {
    FillMisses(hits, n);
    return 0;
  }
  const DevBuf d_xyz(ctx_, n * 3 * sizeof(float)), d_hits(ctx_, n * sizeof(wc_map_hit));
  const wc_points desc = UploadXyz(d_xyz, xyz, n);
  uint64_t found = 0;
  WC_CALL(wc_map_nearest(ctx_, map_, &desc, max_dist, (wc_map_hit *)d_hits.p, &found));
  d_hits.ToHost(hits, n * sizeof(wc_map_hit));
  return found;
}
size_t LidarOdometry::QueryMapKnn(const float *xyz, size_t n, const wc_map_knn_params &p, wc_map_hit *hits, uint32_t *within) {
  if (!n || !xyz || !hits) return 0;
  if (!(p.max_dist > 0.0) || p.k < 1 || p.k > 16 || (p.reach != 1 && p.reach != 2) || p.min_points < 1 || (p.flags & ~(uint32_t)WC_MAP_KNN_NOT_OWN))
    return 0;
  if (!map_) {
    FillMisses(hits, n * p.k);
    if (within) std::memset(within, 0, n * sizeof(uint32_t));
    return 0;
  }
  const DevBuf d_xyz(ctx_, n * 3 * sizeof(float)), d_hits(ctx_, n * p.k * sizeof(wc_map_hit)), d_within(ctx_, n * sizeof(uint32_t));
  const wc_points desc = UploadXyz(d_xyz, xyz, n);
  uint64_t out[3] = {0, 0, 0};
  WC_CALL(wc_map_knn(ctx_, map_, &desc, &p, (wc_map_hit *)d_hits.p, (uint32_t *)d_within.p, out));
  d_hits.ToHost(hits, n * p.k * sizeof(wc_map_hit));
  if (within) d_within.ToHost(within, n * sizeof(uint32_t));
  return out[0];
}
size_t LidarOdometry::CropMap(const double lo[3], const double hi[3]) {
  uint64_t removed = 0;
  if (map_) WC_CALL(wc_map_crop(ctx_, map_, lo, hi, &removed));
  return removed;
}
bool LidarOdometry::CarveMap(const float *xyz, size_t n, const double origin[3], const wc_map_carve_params &params, wc_map_carve_result *result) {
  if (!map_ || !origin || (n && !xyz)) return false;
  const DevBuf d_xyz(ctx_, n * 3 * sizeof(float));
  const wc_points desc = UploadXyz(d_xyz, xyz, n);
  wc_map_carve_result r;
  if (wc_map_carve(ctx_, map_, &desc, origin, &params, &r) != WC_OK) return false;  // (as in AlignToMap)
  if (result) *result = r;
  return true;
}
bool LidarOdometry::CarveMapRemove(const float *xyz, size_t n, const double origin[3], const wc_map_carve_params &params,
                                   wc_map_carve_result *result) {
  if (!map_ || !origin || (n && !xyz)) return false;
  const DevBuf d_xyz(ctx_, n * 3 * sizeof(float));
  const wc_points desc = UploadXyz(d_xyz, xyz, n);
  wc_map_carve_result r;
  if (wc_map_carve_remove(ctx_, map_, &desc, origin, &params, &r) != WC_OK) return false;  // (as in AlignToMap)
  if (result) *result = r;
  return true;
}
bool LidarOdometry::RemoveMapVoxels(const int32_t *keys, size_t n, uint64_t out[3]) {
  if (!map_ || !out || (n && !keys)) return false;
  const DevBuf d_keys(ctx_, n * 3 * sizeof(int32_t));
  if (n) CheckCall(ctx_, "wc_h2d", wc_h2d(ctx_, d_keys.p, keys, n * 3 * sizeof(int32_t)));
  return wc_map_remove_keys(ctx_, map_, (const int32_t *)d_keys.p, n, out) == WC_OK;
}
bool LidarOdometry::MapComponents(const wc_map_cc_params &params, int32_t *keys, uint32_t *labels, size_t cap, wc_map_component *comps,
                                  size_t cap_comps, uint64_t out[4]) {
  if (!map_ || !out) return false;
  // (device room for what the caller can take: a call with too little of either fills out[] and writes nothing there)
  const DevBuf d_keys(ctx_, keys ? cap * 3 * sizeof(int32_t) : 0), d_labels(ctx_, labels ? cap * sizeof(uint32_t) : 0),
      d_comps(ctx_, comps ? std::max<size_t>(cap_comps, 1) * sizeof(wc_map_component) : 0);
  uint64_t o[4] = {0, 0, 0, 0};
  const int rc = wc_map_components(ctx_, map_, &params, (int32_t *)d_keys.p, (uint32_t *)d_labels.p, labels ? cap : 0, (wc_map_component *)d_comps.p,
                                   comps ? cap_comps : 0, o);
  if (rc != WC_OK && rc != WC_ERR_CAPACITY) return false;  // (as in AlignToMap)
  std::memcpy(out, o, sizeof(o));
  if (rc != WC_OK) return false;
  if (o[0] && keys) d_keys.ToHost(keys, o[0] * 3 * sizeof(int32_t));
  if (o[0] && labels) d_labels.ToHost(labels, o[0] * sizeof(uint32_t));
  if (o[2] && comps) d_comps.ToHost(comps, o[2] * sizeof(wc_map_component));
  return true;
}
bool LidarOdometry::RemoveSmallMapComponents(const wc_map_cc_params &params, uint32_t min_voxels, uint64_t min_comp_points, uint64_t out[4]) {
  if (!map_ || !out) return false;
  uint64_t o[4] = {0, 0, 0, 0};
  if (wc_map_remove_small(ctx_, map_, &params, min_voxels, min_comp_points, o) != WC_OK) return false;  // (as in AlignToMap)
  std::memcpy(out, o, sizeof(o));
  return true;
}
bool LidarOdometry::SetMapCarve(double range, uint32_t shell, uint32_t min_rays) {
  if (!(range >= 0.0) || shell > 8 || min_rays < 1) return false;
  config_.map_carve_range = range, config_.map_carve_shell = shell, config_.map_carve_min_rays = min_rays;
  return true;
}
bool LidarOdometry::CastMap(const float *xyz, size_t n, const double origin[3], const wc_map_raycast_params &params, wc_map_ray_hit *hits,
                            wc_map_raycast_result *result) {
  if (!map_ || !origin || (n && (!xyz || !hits))) return false;
  const DevBuf d_xyz(ctx_, n * 3 * sizeof(float)), d_hits(ctx_, n * sizeof(wc_map_ray_hit));
  const wc_points desc = UploadXyz(d_xyz, xyz, n);
  wc_map_raycast_result r;
  if (wc_map_raycast(ctx_, map_, &desc, origin, &params, (wc_map_ray_hit *)d_hits.p, &r) != WC_OK) return false;  // (as in AlignToMap)
  if (n) d_hits.ToHost(hits, n * sizeof(wc_map_ray_hit));
  if (result) *result = r;
  return true;
}
// ---- the map's exact state as a file (host/map_file.h) ---------------------------------------------------------------------------
static_assert(sizeof(wc_map_voxel) == sizeof(wc_map_file::Voxel) && offsetof(wc_map_voxel, count) == offsetof(wc_map_file::Voxel, count) &&
                  offsetof(wc_map_voxel, sum) == offsetof(wc_map_file::Voxel, sum),
              "the file's record is the library's wc_map_voxel");
bool LidarOdometry::SaveMap(const std::string &path) {
  if (!map_) return false;
  uint64_t n = map_voxels();
  std::vector<wc_map_file::Voxel> vox(n);
  std::vector<int64_t> mom(map_moments_ ? 9 * n : 0);
  if (n) {
    const DevBuf d_vox(ctx_, n * sizeof(wc_map_voxel)), d_mom(ctx_, mom.size() * sizeof(int64_t));
    WC_CALL(wc_map_export_state(ctx_, map_, (wc_map_voxel *)d_vox.p, (int64_t *)d_mom.p, n, &n));
    d_vox.ToHost(vox.data(), n * sizeof(wc_map_voxel));
    if (d_mom.p) d_mom.ToHost(mom.data(), mom.size() * sizeof(int64_t));
  }
  std::vector<uint8_t> file(wc_map_file::EncodedBytes(n, map_moments_));
  wc_map_file::Encode(map_voxel_, map_moments_ ? wc_map_file::kFlagMoments : 0u, vox.data(), mom.data(), n, file.data());
  if (wc_map_file::Decode(file.data(), file.size(), nullptr) != wc_map_file::kOk) return false;  // (a voxel beyond 2^30 points)
  std::FILE *f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool written = std::fwrite(file.data(), 1, file.size(), f) == file.size();
  const bool closed = std::fclose(f) == 0;
  if (!(written && closed)) std::remove(path.c_str());
  return written && closed;
}
namespace {
// what LoadMap and MergeMapFile begin with: the file read, decoded and held against the map's voxel size and flags; the records (and,
// with `moments`, their moment words) unpacked.  false: the file cannot be read, Decode refuses it, its voxel size is not bitwise
// `voxel`, or `moments` is asked of a file without
bool ReadMapFile(const std::string &path, double voxel, bool moments, std::vector<wc_map_file::Voxel> &vox, std::vector<int64_t> &mom) {
  std::FILE *f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  std::vector<uint8_t> file;
  uint8_t chunk[65536];
  for (size_t got; (got = std::fread(chunk, 1, sizeof(chunk), f)) > 0;) file.insert(file.end(), chunk, chunk + got);
  const bool read_ok = std::ferror(f) == 0;
  std::fclose(f);
  wc_map_file::Header h;
  if (!read_ok || wc_map_file::Decode(file.data(), file.size(), &h) != wc_map_file::kOk) return false;
  const bool file_moments = (h.flags & wc_map_file::kFlagMoments) != 0;
  if (std::memcmp(&h.voxel, &voxel, sizeof(double)) != 0 || (moments && !file_moments)) return false;
  vox.resize(h.n);
  mom.resize(moments ? 9 * h.n : 0);
  wc_map_file::Unpack(file.data(), h, vox.data(), moments ? mom.data() : nullptr);
  return true;
}
// ... and the records absorbed into `map`
void AbsorbRecords(wc_ctx *ctx, wc_map *map, const std::vector<wc_map_file::Voxel> &vox, const std::vector<int64_t> &mom) {
  const uint64_t n = vox.size();
  if (!n) return;
  const DevBuf d_vox(ctx, n * sizeof(wc_map_voxel)), d_mom(ctx, mom.size() * sizeof(int64_t));
  CheckCall(ctx, "wc_h2d", wc_h2d(ctx, d_vox.p, vox.data(), n * sizeof(wc_map_voxel)));
  if (d_mom.p) CheckCall(ctx, "wc_h2d", wc_h2d(ctx, d_mom.p, mom.data(), mom.size() * sizeof(int64_t)));
  uint64_t rejected = 0;  // (asked for: the call waits, so the host vectors and device buffers outlive the kernel)
  CheckCall(ctx, "wc_map_absorb", wc_map_absorb(ctx, map, (const wc_map_voxel *)d_vox.p, (const int64_t *)d_mom.p, n, &rejected));
  WC_CHECK(rejected == 0);  // (Decode refuses every record the absorb rejects)
}
}  // namespace
bool LidarOdometry::LoadMap(const std::string &path, bool merge) {
  if (!map_) return false;
  std::vector<wc_map_file::Voxel> vox;
  std::vector<int64_t> mom;
  if (!ReadMapFile(path, map_voxel_, map_moments_, vox, mom)) return false;
  if (!merge) {  // as SetMapVoxel re-creates it, with room for the file's voxels: no growth and no wc_map_clear
    WC_CALL(wc_map_destroy(ctx_, map_));
    map_ = nullptr;
    WC_CALL(wc_map_create_ex(ctx_, map_voxel_, vox.size(), map_moments_ ? WC_MAP_MOMENTS : 0u, &map_));
  }
  AbsorbRecords(ctx_, map_, vox, mom);
  return true;
}
bool LidarOdometry::MergeMapFile(const std::string &path, double T_io[12], uint32_t factor, uint32_t n_levels, const wc_map_align_opts &opts,
                                 wc_map_align_summary *summaries) {
  if (!map_ || !map_moments_ || !T_io || factor < 1 || n_levels < 1 || n_levels > kMaxLevels) return false;
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<wc_map_file::Voxel> vox;
  std::vector<int64_t> mom;
  if (!ReadMapFile(path, map_voxel_, true, vox, mom)) return false;
  wc_map *other = nullptr;  // the file's map, in the file's frame
  WC_CALL(wc_map_create_ex(ctx_, map_voxel_, vox.size(), WC_MAP_MOMENTS, &other));
  AbsorbRecords(ctx_, other, vox, mom);
  std::vector<double> T(T_io, T_io + 12);
  std::vector<wc_map_align_summary> s;
  std::vector<int32_t> status;
  bool ok;
  {
    // its centroids, exported on the device, are the points RelocalizeToMap's level chain aligns to the facade's map
    uint64_t n = vox.size();
    const DevBuf d_xyz(ctx_, n * 3 * sizeof(float)), d_count(ctx_, n * sizeof(uint32_t));
    const auto exported = [&] {
      CheckCall(ctx_, "wc_map_export", wc_map_export(ctx_, other, (float *)d_xyz.p, (uint32_t *)d_count.p, nullptr, n, &n));
      return wc_points{d_xyz.p, nullptr, 12, 0, n};
    };
    ok = AlignCandidatesOf(ctx_, map_, map_voxel_, exported, factor, n_levels, opts, kNoSeed, T, s, status) && status[0] == WC_OK;
  }
  if (ok) {
    const wc_map_align_summary &last = s[n_levels - 1];
    ok = last.termination != 2 && last.n_used >= opts.min_used;
  }
  // (a T the library refuses - no rotation, from a start that was none - is the caller's: no abort, as in AlignToMap)
  if (ok) ok = wc_map_merge_moved(ctx_, map_, other, T.data(), nullptr) == WC_OK;
  WC_CALL(wc_map_destroy(ctx_, other));
  if (!ok) return false;
  std::memcpy(T_io, T.data(), 12 * sizeof(double));
  if (summaries) std::memcpy(summaries, s.data(), s.size() * sizeof(s[0]));
  last_map_ms_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return true;
}
bool LidarOdometry::SetMapKeepRadius(double radius) {
  if (!(radius >= 0.0)) return false;
  config_.map_keep_radius = radius;
  return true;
}

void LidarOdometry::UploadImuStates() {
  const size_t n_imu = imu_states_.size();
  if (n_imu > cap_imu_) {
    if (d_imu_) WC_CALL(wc_dev_free(ctx_, d_imu_));
    cap_imu_ = n_imu * 2;
    void *p = nullptr;
    WC_CALL(wc_dev_alloc(ctx_, cap_imu_ * sizeof(wc_imu_state), &p));
    d_imu_ = (wc_imu_state *)p;
    imu_dev_stale_ = true;
  }
  if (!imu_dev_stale_) return;
  const std::vector<wc_imu_state> &flat = FlatImu();
  WC_CALL(wc_h2d(ctx_, d_imu_, flat.data(), n_imu * sizeof(wc_imu_state)));
  imu_dev_stale_ = false;
}

const std::vector<wc_imu_state> &LidarOdometry::FlatImu() {
  if (imu_flat_stale_) {
    imu_flat_.assign(imu_states_.begin(), imu_states_.end());
    imu_flat_stale_ = false;
  }
  return imu_flat_;
}

void LidarOdometry::UpdateSurfelPosesOnDevice() {  // UpdateSurfelPoses (:160-170) over the sliding window
  UploadImuStates();
  const size_t n = n_surfels_ - sld_begin_;
  if (n)
    WC_CALL(wc_update_surfel_poses(ctx_, d_imu_, imu_states_.size(), d_surf_ + sld_begin_, d_pose_ + sld_begin_, d_inbody_ + sld_begin_, n));
}

// UpdateImuPoses (:187-215) with the CubicBSplineSampleCorrector (:22-54)
void LidarOdometry::UpdateImuPoses() {
  TouchImu();
  std::vector<double> ts;
  std::vector<V3> rc, pc;
  for (const Sample &s : samples_) {
    ts.push_back(s.timestamp);
    rc.push_back(v3(s.cor));
    pc.push_back(v3(s.cor + 3));
  }
  CubicBSpline rot_interp(ts, rc), pos_interp(ts, pc);
  long first = -1, last = -1;
  for (size_t i = 0; i < imu_states_.size(); ++i) {
    V3 r{0, 0, 0}, p{0, 0, 0};
    const bool ok = rot_interp.Interp(imu_states_[i].t, r);
    const bool ok2 = pos_interp.Interp(imu_states_[i].t, p);
    WC_CHECK(ok == ok2);
    if (!ok) continue;
    stq(imu_states_[i].quat, qmul(so3_exp(r), q4(imu_states_[i].quat)));
    st3(imu_states_[i].pos, p + v3(imu_states_[i].pos));
    if (first < 0) first = (long)i;
    last = (long)i;
  }
  if (first != -1) {
    WC_CHECK(first == 0);
    WC_CHECK(last == (long)imu_states_.size() - 2);
    const size_t n = imu_states_.size();
    const Sample &b = samples_.back();
    PredictPoseOfNewImuState(imu_states_[n - 3], imu_states_[n - 2], v3(b.cor + 9), v3(b.cor + 6), v3(b.grav), imu_states_[n - 1]);
  }
}

void LidarOdometry::UpdateSamplePoses() {  // :172-179
  for (Sample &s : samples_) {
    stq(s.quat, qmul(so3_exp(v3(s.cor)), q4(s.quat)));
    st3(s.pos, v3(s.cor + 3) + v3(s.pos));
    for (int d = 0; d < 6; ++d) s.cor[d] = 0;
  }
}

// ShrinkToFit (:228-250).  The oldest sliding-window surfels move to the FRONT of the fixed window, oldest first
// (push_front, :243-246), so the fixed window is newest-first: one reversed device copy per sweep.  Like the reference
// (Q11: :247-249 compares back() with itself) the fixed window is never trimmed while reference_quirks is set; without the
// quirk it is cut to fixed_window_duration from its old end.
void LidarOdometry::ShrinkToFit() {
  if (samples_.empty() || samples_.back().timestamp - samples_.front().timestamp <= config_.sliding_window_duration) return;
  while (samples_.back().timestamp - samples_.front().timestamp > config_.sliding_window_duration) samples_.pop_front();
  while (imu_states_.front().t < samples_.front().timestamp) imu_states_.pop_front();
  TouchImu();
  size_t k = 0;
  while (k < surfel_times_.size() && surfel_times_[k] < imu_states_.front().t) ++k;
  if (k) {
    EnsureFixedCapacity(k);
    WC_CALL(wc_reverse_copy_surfels(ctx_, d_surf_ + sld_begin_, d_pose_ + sld_begin_, k, d_fix_surf_ + (fix_start_ - k), d_fix_pose_ + (fix_start_ - k)));
    WC_CALL(wc_sync(ctx_));
    fix_start_ -= k;
    for (size_t i = 0; i < k; ++i) fix_times_.push_front(surfel_times_[i]);
    surfel_times_.erase(surfel_times_.begin(), surfel_times_.begin() + (long)k);
    sld_begin_ += k;
  }
  if (!config_.reference_quirks)
    while (!fix_times_.empty() && fix_times_.front() - fix_times_.back() > config_.fixed_window_duration) {
      fix_times_.pop_back();
      --fix_end_;
    }
}

void LidarOdometry::AddLidarScan(const pcl::PointCloud<hilti_ros::Point>::Ptr &msg) {
  // lidar frame -> imu frame, range / blind-box filter (:489-496): on the device, the points stay there
  const auto t_entry = std::chrono::steady_clock::now();
  data_added_ = true;
  AppendScanOnDevice(*msg);
  if (!SyncHeadingMsgs()) return;

  // 1. collect scan to sweep (:501-509)
  double sweep_endtime = point_times_.front() + config_.sweep_duration;
  if (point_times_.back() < sweep_endtime || imu_buff_.empty() || imu_buff_.back().timestamp < sweep_endtime) return;

  // wall time of the stages of a completed sweep (last_stage_ms(); WC_ODOM_DEBUG=1 also prints them on stderr)
  static const bool dbg_t = getenv("WC_ODOM_DEBUG") != nullptr;  // (prints only; the one variable the facade reads)
  auto t_prev = std::chrono::steady_clock::now();
  last_append_ms_ = std::chrono::duration<double, std::milli>(t_prev - t_entry).count();
  double (&t_stage)[8] = last_stage_ms_;
  for (double &v : t_stage) v = 0.0;
  last_lm_iterations_ = 0;
  auto lap = [&](int i) {
    const auto now = std::chrono::steady_clock::now();
    t_stage[i] += std::chrono::duration<double, std::milli>(now - t_prev).count();
    t_prev = now;
  };
  // 2. integrate IMU poses in windows (:512-513)
  PredictImuStatesAndSampleStates(sweep_endtime);
  sweep_endtime = samples_.back().timestamp;
  size_t n_sweep = 0;  // BuildSweep (:134-141): the leading points with time < sweep_endtime
  // (the stamps ascend - the CHECK of :491 holds on the device, AppendScanOnDevice -, so the first one that is not earlier is found by
  // bisection; counted one by one through the deque, 300 k stamps were 0.25 ms of every completed sweep)
  n_sweep = (size_t)(std::lower_bound(point_times_.begin(), point_times_.end(), sweep_endtime) - point_times_.begin());
  WC_CHECK(n_sweep > 0);
  const double sweep_t0 = point_times_.front(), sweep_t1 = point_times_[n_sweep - 1];

  // 3. undistort sweep by IMU poses (:519-520) — wc_undistort_sweep_packed replaces UndistortSweep :143-158 and leaves the
  //    sweep as the 20 bytes per point BuildSurfels reads (x, y, z, time: surfel_extraction.cc:317-324); neither the raw nor the
  //    undistorted sweep ever comes back to the host, and the undistorted 48-byte records are never formed
  if (n_sweep > cap_sweep_) {
    if (d_sweep_xyz_) WC_CALL(wc_dev_free(ctx_, d_sweep_xyz_));
    if (d_sweep_t_) WC_CALL(wc_dev_free(ctx_, d_sweep_t_));
    cap_sweep_ = n_sweep * 2;
    WC_CALL(wc_dev_alloc(ctx_, cap_sweep_ * 3 * sizeof(float), &d_sweep_xyz_));
    WC_CALL(wc_dev_alloc(ctx_, cap_sweep_ * sizeof(double), &d_sweep_t_));
  }
  UploadImuStates();
  WC_CALL(wc_undistort_sweep_packed(ctx_, (const char *)d_pts_[pts_cur_] + pts_begin_ * sizeof(hilti_ros::Point), n_sweep, d_imu_, imu_states_.size(),
                                    (float *)d_sweep_xyz_, (double *)d_sweep_t_));
  const void *d_raw_sweep = (const char *)d_pts_[pts_cur_] + pts_begin_ * sizeof(hilti_ros::Point);  // (stays where it is until the next scan arrives)
  lap(0);

  // 4. ---- hot path: extract surfels, attach poses (:523-527) ----
  const size_t max_new = (3 * n_sweep) / 20 + 1;
  EnsureSurfelCapacity(max_new);
  wc_points desc{d_sweep_xyz_, d_sweep_t_, 3 * sizeof(float), sizeof(double), n_sweep};
  uint64_t n_new = 0;
  // (the sweep's stamps leave the host's buffer - 300 k deque entries, ~0.1 ms - while the extraction runs)
  WC_CALL(wc_extract_surfels_enqueue(ctx_, &desc, sweep_t0, sweep_t1, d_surf_ + n_surfels_, nullptr, max_new));
  DropBufferedPoints(n_sweep);
  WC_CALL(wc_extract_surfels_finish(ctx_, &n_new));
  {
    uint32_t st[64];
    WC_CALL(wc_debug_status(ctx_, st));
    ++(st[61] ? sweeps_fast_ : sweeps_exact_);  // which arithmetic completed this sweep (read-out for tests / logs)
  }
  if (n_new) {
    WC_CALL(wc_memset(ctx_, d_inbody_ + n_surfels_, 0, n_new));
    std::vector<double> fresh(n_new);  // only the timestamps travel (8 of 144 bytes per surfel)
    WC_CALL(wc_d2h_strided(ctx_, fresh.data(), d_surf_ + n_surfels_, 8, sizeof(wc_surfel), n_new));
    surfel_times_.insert(surfel_times_.end(), fresh.begin(), fresh.end());
    n_surfels_ += n_new;
  }
  UpdateSurfelPosesOnDevice();
  lap(1);

  for (int iter = 0; iter < config_.outer_iter_num_max; ++iter) {
    const size_t n_sld = n_surfels_ - sld_begin_;
    // correspondences (:530-538)
    uint64_t n_b = 0, n_u = 0;
    const size_t n_fix = fix_end_ - fix_start_;
    WC_CALL(wc_match_pair(ctx_, d_surf_ + sld_begin_, d_pose_ + sld_begin_, n_sld, d_fix_surf_ + fix_start_, d_fix_pose_ + fix_start_, n_fix,
                          d_pairs_sld_, cap_surfels_, &n_b, d_pairs_fix_, cap_surfels_, &n_u));
    last_corr_[0] = n_b, last_corr_[1] = n_u;
    if (keep_pair_stamps_) {  // (test hook: outside the stage clocks' interest, a few strided read-backs)
      std::vector<double> ts_sld(n_sld), ts_fix(n_fix);
      if (n_sld) WC_CALL(wc_d2h_strided(ctx_, ts_sld.data(), d_surf_ + sld_begin_, 8, sizeof(wc_surfel), n_sld));
      if (n_fix) WC_CALL(wc_d2h_strided(ctx_, ts_fix.data(), d_fix_surf_ + fix_start_, 8, sizeof(wc_surfel), n_fix));
      for (int which = 0; which < 2; ++which) {
        const uint64_t n = which ? n_u : n_b;
        std::vector<wc_pair> pr(n);
        if (n) WC_CALL(wc_d2h(ctx_, pr.data(), which ? d_pairs_fix_ : d_pairs_sld_, n * sizeof(wc_pair)));
        pair_stamps_[which].clear();
        for (const wc_pair &q : pr) {
          pair_stamps_[which].push_back(which ? ts_fix[(size_t)q.first] : ts_sld[(size_t)q.first]);  // (fixed window: first = its surfel)
          pair_stamps_[which].push_back(ts_sld[(size_t)q.second]);
        }
      }
    }
    lap(2);
    // 5. solve poses in windows (:541-562)
    std::vector<double> ts, x;
    for (const Sample &s : samples_) {
      ts.push_back(s.timestamp);
      x.insert(x.end(), s.cor, s.cor + 12);
    }
    const std::vector<wc_imu_state> &flat = FlatImu();
    const bool fix_first = first_sample_known_ && samples_.front().timestamp == first_sample_time_;  // :556-560
    WC_CALL(wc_window_build(ctx_, d_surf_ + sld_begin_, d_pose_ + sld_begin_, d_pairs_sld_, n_b, d_fix_surf_ + fix_start_, d_fix_pose_ + fix_start_, d_pairs_fix_, n_u,
                            flat.data(), flat.size(), ts.data(), ts.size(), samples_.back().grav, fix_first ? 1 : 0));
    lap(3);
    if (config_.log_residual_histograms) {  // :547-549
      residual_log_.clear();
      LogResiduals(x, "[before solve] ");
    }
    WC_CALL(wc_window_solve(ctx_, x.data(), &last_summary_, nullptr));
    last_lm_iterations_ += (int)last_summary_.iterations;
    lap(4);
    for (size_t i = 0; i < samples_.size(); ++i) std::memcpy(samples_[i].cor, &x[12 * i], 96);
    // state update (:564-566)
    UpdateImuPoses();
    UpdateSurfelPosesOnDevice();
    UpdateSamplePoses();
    if (config_.log_residual_histograms) {
      // :568-570 - AFTER UpdateSamplePoses: the factors still hold the poses they were built with, the sample states' rotation
      // and position corrections have just been zeroed (:176-177), the biases stay: the reference's second log shows the
      // residuals at (0, 0, bg, ba), not at the optimum.  Reproduced as it is.
      std::vector<double> x_after;
      for (const Sample &s : samples_) x_after.insert(x_after.end(), s.cor, s.cor + 12);
      LogResiduals(x_after, "[after update] ");
      if (dbg_t) fputs(residual_log_.c_str(), stderr);
    }
    lap(5);
  }
  ShrinkToFit();  // :574-580
  // the sweep with the final poses (:584-595) is formed once, for the outputs and for the map alike
  const void *d_world = nullptr;
  if (config_.fill_outputs) {
    d_world = UndistortFinal(d_raw_sweep, n_sweep);
    FillOutputs(d_world, n_sweep);  // :582-602
  }
  lap(6);
  last_map_ms_ = 0.0;
  if (config_.map_voxel_size != 0.0) {  // (the reference accumulates in RViz; off by default: nothing allocated or launched)
    const auto t_map = std::chrono::steady_clock::now();
    EnsureMap();
    if (!d_world) d_world = UndistortFinal(d_raw_sweep, n_sweep);
    const wc_points desc{d_world, (const char *)d_world + WC_HILTI_POINT_TIME_OFFSET, WC_HILTI_POINT_BYTES, WC_HILTI_POINT_BYTES, n_sweep};
    WC_CALL(wc_map_insert(ctx_, map_, &desc, nullptr));
    if (config_.map_carve_range > 0.0) {  // the sweep's own rays from the sensor's position (the tf of FillOutputs) take what they contradict
      const wc_map_carve_params cp{0.0, config_.map_carve_range, config_.map_carve_shell, config_.map_carve_min_rays, 4096, 0};
      wc_map_carve_result cr;
      WC_CALL(wc_map_carve_remove(ctx_, map_, &desc, samples_.back().pos, &cp, &cr));
    }
    if (config_.map_keep_radius > 0.0) {  // the cube around this sweep's world -> imu_link origin (the tf of FillOutputs)
      const double *c = samples_.back().pos, r = config_.map_keep_radius;
      const double lo[3] = {c[0] - r, c[1] - r, c[2] - r}, hi[3] = {c[0] + r, c[1] + r, c[2] + r};
      WC_CALL(wc_map_crop(ctx_, map_, lo, hi, nullptr));
    }
    t_prev = std::chrono::steady_clock::now();
    last_map_ms_ = std::chrono::duration<double, std::milli>(t_prev - t_map).count();
  }
  if (dbg_t)
    fprintf(stderr, "[odom] sweep %d: predict + undistort %.2f, extract + poses %.2f, match %.2f, build %.2f, solve %.2f (%d iterations), update %.2f, shrink %.2f ms\n",
            (int)sweep_id_, t_stage[0], t_stage[1], t_stage[2], t_stage[3], t_stage[4], (int)last_summary_.iterations, t_stage[5], t_stage[6]);
  ++sweep_id_;
}
