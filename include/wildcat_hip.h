/*
 * wildcat_hip.h — C-ABI of libwildcat_hip.so, the MI355X (gfx950) implementation of the sliding-window
 * odometry hot path of kekeliu-whu/Wildcat-SLAM (reference call site src/odometry/lidar_odometry.cc:523-566).
 *
 * The reference has no FFI / plugin boundary: the seam is a set of C++ free functions and classes inside
 * src/odometry.  Each entry point below names the reference interface it replaces; INTEGRATION.md shows the
 * C++ glue a maintainer adds inside LidarOdometry::AddLidarScan to call them.
 *
 * Conventions
 *   - every function returns an int status: WC_OK (0) or a WC_ERR_* code; wc_last_error() gives the text.
 *     (The reference aborts through glog CHECKs instead; the host facade turns non-zero into a fatal log.)
 *   - pointers named d_* are DEVICE (HBM) pointers, h_* are host pointers.  Records are the PODs of wc_types.h.
 *   - one caller thread per wc_ctx; a ctx owns one HIP stream (replaceable through wc_ctx_set_stream) and all
 *     scratch memory.  Calls are synchronous on return unless stated otherwise.
 *   - no C++ types, exceptions or torch types cross this boundary.
 */
#ifndef WILDCAT_HIP_H_
#define WILDCAT_HIP_H_

#include "wc_types.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
  WC_OK = 0,
  WC_ERR_CAPACITY = 1,  /* output buffer too small; *n_out holds the needed count                   */
  WC_ERR_RANGE = 2,     /* timestamp outside the IMU / sample-state range (reference CHECKs)        */
  WC_ERR_ORDER = 3,     /* correspondence not (older, newer)  (CHECK_LT lidar_odometry.cc:256,301)  */
  WC_ERR_HIP = 10,      /* HIP runtime error                                                        */
  WC_ERR_ARG = 11,      /* bad argument                                                             */
  WC_ERR_NOGPU = 12,    /* no gfx950 device visible                                                 */
  WC_ERR_NUMERIC = 13,  /* linear solve failed                                                      */
  WC_ERR_INTERNAL = 14  /* a bounded loop of a kernel ran past its bound: a defect, reported instead of a hang */
};

typedef struct wc_ctx wc_ctx;

/* library / device --------------------------------------------------------------------------------------------- */
const char *wc_version(void);
int wc_device_count(void);
void wc_params_default(wc_params *p); /* SURVEY.md §2.1 values: surfel_extraction.cc:327, knn_surfel_matcher.h:37-41,
                                         lio_config.h:10-14,32-45 */
/* Host only, no context, no GPU: WC_OK when every field of p is a value the library can run with, else WC_ERR_ARG and, in *field
 * (may be NULL), the name of the first field that is not (a static string; NULL when p passes).  The rules: voxel_size, surfel_sigma0,
 * cauchy_a and imu_dt finite and > 0; planer_threshold, cluster_gap and the four IMU weights finite and >= 0; min_plane_likeness and
 * view_point finite; center_scale and angular_scale finite and not 0 (a negative scale is a scale); surfel_dist_max and time_diff_min
 * anything but NaN (an infinite gate is a gate that is always open or always shut); max_layer 0..2, min_points >= 0,
 * cluster_min_points >= 1, knn_k 1..16, max_iterations >= 0.  Every one of these is divided by, or scales what goes into a kernel:
 * a value outside them would put NaN or infinity into the kd-tree's features, the loss or the IMU Jacobians. */
int wc_params_check(const wc_params *p, const char **field);
/* params NULL: wc_params_default.  Parameters that fail wc_params_check: WC_ERR_ARG, no context. */
int wc_ctx_create(const wc_params *params, int device, wc_ctx **out);
void wc_ctx_destroy(wc_ctx *ctx);
const char *wc_last_error(const wc_ctx *ctx);
int wc_ctx_set_stream(wc_ctx *ctx, void *hip_stream); /* NULL = the ctx's own stream */
/* Replaces the context's parameters.  Parameters that fail wc_params_check are refused before anything is launched: WC_ERR_ARG,
 * wc_last_error names the field and its rule, and the context keeps the parameters it had.
 * When a parameter is read: extraction and matcher parameters by the call that extracts or matches; the factor parameters
 * (surfel_sigma0, cauchy_a, w_gyr, w_acc, w_bg, w_ba, imu_dt, reference_quirks) by wc_window_build, which copies them into the
 * problem - a wc_ctx_set_params between the build and wc_window_linearize / _evaluate / _solve does not change the problem built;
 * max_iterations by wc_window_solve, at the solve. */
int wc_ctx_set_params(wc_ctx *ctx, const wc_params *params);
int wc_ctx_get_params(const wc_ctx *ctx, wc_params *out); /* the parameters in force (a copy; host only) */
/* Development options of ONE context - the only way to change what the release library executes besides wc_params.  The release
 * build reads no environment variable that alters a result or a code path (a stray WC_* variable cannot change what a node runs);
 * the variables it does read only PRINT: WC_ALLOC_DEBUG, WC_FX_DEBUG, WC_MATCH_DEBUG, WC_MATCH_TIMING, WC_WIN_DEBUG, WC_DEBUG_GATHER
 * (libwildcat_hip.so) and WC_ODOM_DEBUG (the facade).  A `-DWC_DEV_KNOBS` build (profiles/dev) additionally seeds the options below
 * from the upper-case WC_<NAME> variables when a context is created.  Options (value 0 / 1 unless stated; -1 = the library decides):
 *   exact_sums         contexts behave as if wc_params.exact_sums were 1
 *   debug_skip         knock-out bits of the default extraction path (timing runs only: results are wrong; the bits exist in a
 *                      -DWC_DEV_KNOBS build only - the release kernels carry no profiling branch and ignore the option)
 *   fx_merge_min       list length from which the next sweep merges record lists first (default 3)
 *   fx_split           node stage of the default extraction: 0 fused kernel, 1 two kernels, -1 by size
 *   fx_acc_form        form of the default extraction's first kernel: bit 0 - the per-point part runs per load round, under the loads;
 *                      bit 1 - records are linked into their lists before their sums exist; 0 - neither (the earlier kernel's order
 *                      WITHOUT its early first hash probe, which bit 1 replaced: slower than that kernel was); -1 - the library's
 *                      own choice (both bits; bit 0 alone for sweeps above 2 M points that are not packed).  The layer-2 kernel has bit 1 only.  Every form writes the same bytes
 *   no_bucket_sort     exact path: radix sort instead of the run-binned sort
 *   ex_sync            wc_extract_surfels_finish waits for the stream instead of the sweep's completion ticket
 *   match_pair_serial  wc_match_pair runs its two searches one after the other on the ctx
 *   lm_dense           round 2's LM step: dense Cholesky of all unknowns instead of the bias elimination
 *   lm_one_collective  sharded windows: rounds 3 - 5's ONE all-reduce per linearisation (IMU triples sharded too) instead of the
 *                      two-collective form (IMU factors replicated; 16-byte cost collective, then the pose corners)
 *   lm_side_stream (1) two-collective form: the large collective on a side stream beside the bias elimination (1: with the in-library RCCL
 *                      binding, 0: never, 2: always - the choreography with a communicator of callbacks, for tests)
 *   lm_dense_radius    iterations whose trust-region radius exceeds 10^value take the dense step (default 7: the largest radius at which
 *                      the bias elimination's backward error stays below 1e-9 - tests/test_lm_step_gpu.py; 0 = never)
 *   map_mom_pts (1)    wc_map_insert into a WC_MAP_MOMENTS map: points per lane - 1: tiles of 256 points, 54 KB of LDS; 2: the plain
 *                      insert's tiles of 512 points, 108 KB of LDS, one workgroup per CU (same sums either way)
 *   map_lin_groups (0) wc_map_linearize, wc_map_linearize_batch and the align calls on them: workgroups of their one first kernel (0:
 *                      chosen from the point count and K); H, g and cost are byte-equal whatever the value
 *   map_score_groups (0) wc_map_score_batch: workgroups of its kernel (0: chosen from the point count and K); every record is the same
 *                      whatever the value
 *   map_carve_groups (0) wc_map_carve: workgroups of its ray kernel (0: chosen from the point count); the five counts are the same
 *                      whatever the value
 *   map_cast_groups (0) wc_map_raycast: workgroups of its kernel (0: chosen from the point count); every output byte is the same
 *                      whatever the value
 *   map_absorb_groups (0) wc_map_absorb: workgroups of its kernel (0: chosen from the record count); the map is the same whatever the
 *                      value
 *   map_remove_groups (0) wc_map_remove_keys: workgroups of its kernel (0: chosen from the key count); the map and the three counts are
 *                      the same whatever the value
 *   map_cc_groups (0)  wc_map_components, wc_map_remove_small: workgroups of their per-voxel kernels (0: chosen from the voxel count);
 *                      every output byte and the map are the same whatever the value
 *   lm_radius0         initial trust-region radius of wc_window_solve: 10^value (default -1 = the library's 1e4); tests use it to
 *                      look at the first step at other damping levels
 * Tests use it to run both forms of a choice on the same data.  Unknown names return WC_ERR_ARG. */
int wc_ctx_set_dev_option(wc_ctx *ctx, const char *name, int value);
/* Optional, for long-running callers (the facade calls it from its constructor): takes one-time costs out of the first calls - loads
 * the code object of every translation unit of the library, creates wc_match_pair's helper context and host thread, and takes
 * `reserve_bytes` (0: nothing) of HBM into the device's stream-ordered memory pool, from which every scratch buffer of a context grows
 * (growing a buffer is then an enqueue of microseconds, not a hipFree + hipMalloc).  No reference counterpart. */
int wc_ctx_warmup(wc_ctx *ctx, size_t reserve_bytes);

/* device memory helpers so that a host program needs no HIP headers ---------------------------------------------- */
int wc_dev_alloc(wc_ctx *ctx, size_t bytes, void **d_ptr);
int wc_dev_free(wc_ctx *ctx, void *d_ptr);
int wc_h2d(wc_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int wc_d2h(wc_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int wc_d2d(wc_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);
int wc_memset(wc_ctx *ctx, void *d_dst, int value, size_t bytes);
/* one field of every record: n elements of elem_bytes, src_stride bytes apart on the device, packed on the host */
int wc_d2h_strided(wc_ctx *ctx, void *h_dst, const void *d_src, size_t elem_bytes, size_t src_stride, size_t n);
int wc_sync(wc_ctx *ctx);
/* HIP-event timing on the ctx stream (used by bench.py: torch.cuda.Event only sees torch's stream) */
int wc_timer_start(wc_ctx *ctx);
int wc_timer_stop_ms(wc_ctx *ctx, float *h_ms);

/* known-answer hooks for the library's own math (csrc/dmath.h), so that the reference's KATs (src/common/utils_test.cc:5-21)
 * run against the product code: on_device != 0 evaluates in a one-thread kernel on the ctx's GPU, on_device == 0 with the
 * host instantiation of the same header (ctx may be NULL).
 *   wc_selftest_so3 : out52 = Exp(v) quat (w,x,y,z) | Log(Exp(v)) | Jl | Jl_inv | Jr | Jr_inv | Hat   (3x3 row-major)
 *   wc_selftest_eig3: a9 symmetric row-major -> out12 = ascending eigenvalues | eigenvectors in columns (row-major)
 *   wc_selftest_quat: in12 = a(4) b(4) f p(3) -> out11 = slerp(a,f,b) | a*p (rotation) | a*b
 *   wc_selftest_so3_fused (device only): the fused forms the factor kernels evaluate (csrc/so3_fused.h) ->
 *                     out25 = Exp(v) quat | Jr(v) | Log(Exp(v)) | Jr_inv(Log(Exp(v)))
 *   wc_selftest_fx_eig3 (device only): the closed-form eigen-solver of the default extraction path (csrc/extract_fast.inc: fx_eig3,
 *                     what every surfel's normal and sigma come from) -> out8 = ascending eigenvalues | eigenvector of the
 *                     smallest | 1.0 closed form accepted / 0.0 the Jacobi fall-back ran | 0 */
int wc_selftest_so3(wc_ctx *ctx, const double v[3], int on_device, double out52[52]);
int wc_selftest_so3_fused(wc_ctx *ctx, const double v[3], double out25[25]);
int wc_selftest_eig3(wc_ctx *ctx, const double a9[9], int on_device, double out12[12]);
int wc_selftest_quat(wc_ctx *ctx, const double in12[12], int on_device, double out11[11]);
int wc_selftest_fx_eig3(wc_ctx *ctx, const double a9[9], double out8[8]);
/* the damped solve's diagonal-block kernel on its own (tests/test_kat_gpu.py, profiles/dev/factor32.py): Cholesky factor L and L^-1 of a
 * 32 x 32 SPD matrix (row-major, lower part read); variant 0 = the library's block form (256 threads, fp64 matrix-core rank-4 updates);
 * h_clk[0] = shader clocks of the fastest of `reps` runs, h_clk[1] = 1 when every pivot was positive */
int wc_selftest_factor32(wc_ctx *ctx, int variant, int reps, const double *h_A, double *h_L, double *h_X, long long *h_clk);

/* surfel extraction --------------------------------------------------------------------------------------------- */
/* Replaces BuildSurfels(const std::vector<hilti_ros::Point>&, std::deque<Surfel::Ptr>&, GlobalMap&)
 * (src/odometry/surfel_extraction.h:145-147, .cc:316-337; call site lidar_odometry.cc:523-525).
 *   pts          descriptor with DEVICE pointers (time ascending, as the reference CHECKs at lidar_odometry.cc:491)
 *   d_out/d_ids  caller-allocated, capacity `cap` records; d_ids may be NULL
 *   h_n_out      number of surfels, sorted by ascending timestamp (surfel_extraction.cc:334), ties by id
 *   t_lo, t_hi   optional hint: all point timestamps lie in [t_lo, t_hi] (pass t_lo > t_hi to let the
 *                library read the first/last timestamp back from the device)
 * NON-FINITE POINTS.  A point with a NaN or infinite x, y or z contributes to nothing: it is in no node's count, sums, time bins
 * or clusters, it raises no status flag whatever its stamp is (the hint binds the stamps of the finite points only; without a hint
 * the first and the last record's stamps are read, whatever their coordinates), it does not decide the key origin (that is the
 * first FINITE point's root voxel, or voxel 0 of a sweep without one) and by itself it does not move a sweep off the default path.
 * The surfels of a cloud are the surfels of the same cloud with those points removed; a cloud without a finite point gives 0
 * surfels and WC_OK.  (The reference drops them too, without saying so: VoxelLoc's cast puts them in voxels of their own kind,
 * whose covariance is not finite and passes no gate.)  This holds for every form of the call - _enqueue / _finish, _batch_*,
 * wc_extract_surfels_sharded - in both arithmetics.  FINITE coordinates beyond the key range (2^20 root voxels around the first
 * finite point) and finite points with a stamp outside the hint remain WC_ERR_ARG. */
int wc_extract_surfels(wc_ctx *ctx, const wc_points *pts, double t_lo, double t_hi, wc_surfel *d_out,
                       wc_surfel_id *d_ids, uint64_t cap, uint64_t *h_n_out);
/* asynchronous split of the same call for pipelined / benchmarked use: enqueue does no host synchronisation; finish returns once
 * the sweep's count and status are final.  d_out / d_ids are then complete IN THE ORDER OF THE CONTEXT'S STREAM - the sweep's last
 * kernel may still be copying surfels when finish returns.  Every library call on the context sees them complete (wc_d2h*, wc_d2d,
 * the next enqueue, wc_match*, the window calls and their side streams, which wait on events of the ctx stream; wc_dev_free waits for
 * the stream).  Whoever reads or frees the buffers any other way - a kernel or copy on another stream, another device or process, a
 * framework's allocator - calls wc_sync(ctx) first.  wc_extract_surfels, the one-call form above, is complete on return for any
 * reader, and so are the batch calls; the development option ex_sync = 1 makes finish wait for the stream as well. */
int wc_extract_surfels_enqueue(wc_ctx *ctx, const wc_points *pts, double t_lo, double t_hi, wc_surfel *d_out,
                               wc_surfel_id *d_ids, uint64_t cap);
int wc_extract_surfels_finish(wc_ctx *ctx, uint64_t *h_n_out);
/* K sweeps (1 <= K <= 64) through ONE launch chain: BuildSurfels is called once per sweep with a fresh GlobalMap
 * (lidar_odometry.cc:523-525), so sweeps are independent; when several are known together (a window replayed from a log, C3 / C4's
 * 5 / 20-sweep windows, several sensors) their kernels run as one launch each over all sweeps instead of three launches per
 * sweep - a 1 M-point sweep is launch-latency bound on its own.  Every sweep gets its own output buffers, count and - should a
 * gate fall inside the noise band - its own repetition on the exact path; results are those of K wc_extract_surfels calls, byte for
 * byte.  enqueue returns without waiting; finish fills h_n_out[K]. */
int wc_extract_surfels_batch_enqueue(wc_ctx *ctx, const wc_sweep_job *jobs, int K);
int wc_extract_surfels_batch_finish(wc_ctx *ctx, uint64_t *h_n_out, int K);
/* per-stage device time of the LAST enqueued extraction, measured with HIP events on the ctx stream:
 * h_ms5 = {per-call fills, voxel grouping of the points, root + layer-1 streaming, node tests + emission (+ layer 2),
 * time ordering + gather of the surfels}.  Enable first: 1 = an event after every kernel group (each event costs ~5 us of
 * stream time), 2 = one pair of events around the whole stage (the stage's time is then reported in h_ms5[1], the other
 * entries are 0), 0 = off. */
int wc_extract_profile(wc_ctx *ctx, int enable);
int wc_extract_stage_ms(wc_ctx *ctx, float *h_ms5);
/* raw status words of the last extraction (profiling aid; words 56..58: pipelines the last sweep enqueued (1 = no repeat), path bits of the run that
 * completed it (1 default path, 2 wide keys, 4 run-binned point sort, 8 time-bin surfel order), LDS capacity of the run-binned
 * sort; words 59..63: long lists, fall-backs so far, completed by the default path, its last flags and reasons) */
int wc_debug_status(wc_ctx *ctx, uint32_t *h_out64);
/* root-voxel index of every point: VoxelLoc (src/odometry/surfel_extraction.h:55-64); d_keys_xyz = 3 int32 per point.  An axis
 * whose coordinate is NaN or infinite, or whose quotient does not fit an int32, gives INT32_MIN (what the reference's cast gives on
 * x86-64; the other axes of the point are unaffected). */
int wc_voxel_keys(wc_ctx *ctx, const wc_points *pts, int32_t *d_keys_xyz);

/* one cloud over several GPUs (BASELINE config 5) --------------------------------------------------- */
/* The reference has no counterpart (single thread): root voxels are independent after binning (surfel_extraction.cc:217-219,
 * :330-332) but each needs all its points in time order (:22-29), so a cloud shards by root voxel - see csrc/route.hip. */
/* Installing a communicator makes NO existing entry point a collective: only the *_sharded calls (wc_extract_surfels_sharded,
 * wc_gather_surfels, wc_match_sharded, wc_match_pair_sharded, wc_window_build_sharded and the solve of a problem built by it) use it. */
int wc_ctx_set_comm(wc_ctx *ctx, const wc_comm *comm); /* NULL removes it */
/* the in-library RCCL communicator (csrc/comm.hip; librccl.so is dlopen()ed): rank 0 creates the 128-byte unique id, the
 * launcher hands it to every rank, each rank calls wc_comm_rccl_init on its ctx.  Collectives run on the ctx's stream. */
int wc_comm_rccl_unique_id(char out128[128]);
int wc_comm_rccl_init(wc_ctx *ctx, int rank, int world, const char id128[128]);
int wc_comm_rccl_destroy(wc_ctx *ctx);
/* measurement helper (bench.py): microseconds per in-place all-reduce of `count` doubles through the ctx's communicator, `reps` of
 * them enqueued back to back on the ctx stream between two HIP events; a collective - every rank of the communicator calls it */
int wc_comm_allreduce_probe(wc_ctx *ctx, uint64_t count, int reps, double *h_us);
/* owner rank of a root voxel (VoxelLoc index, surfel_extraction.h:59-64): hash(kx,ky,kz) mod world; needs no GPU */
int wc_route_owner(int32_t kx, int32_t ky, int32_t kz, int world);
/* stable partition of this rank's points by owner: d_send (capacity pts->n records) receives `world` consecutive segments
 * (owner 0, 1, ...), time order preserved inside each; h_counts[world] = their lengths */
int wc_route_partition(wc_ctx *ctx, const wc_points *pts, int world, wc_route_point *d_send, uint64_t *h_counts);
/* the whole sharded call on one rank: partition the local time-contiguous slice, ONE all-to-all of 24-byte records through
 * the ctx's communicator, wc_extract_surfels on the points of the voxels this rank owns.  t_lo <= t_hi: the time range of
 * the WHOLE cloud.  Output: this rank's surfels (disjoint from the other ranks' by voxel), time sorted.
 * h_n_points_owned (may be NULL): points this rank received.  A point with a non-finite coordinate is routed like any other (an
 * index of INT32_MIN on that axis, see wc_voxel_keys: ONE owner, counted in its h_n_points_owned) and dropped by the owner's
 * extraction, as wc_extract_surfels drops it. */
int wc_extract_surfels_sharded(wc_ctx *ctx, const wc_points *pts, double t_lo, double t_hi, wc_surfel *d_out, wc_surfel_id *d_ids,
                               uint64_t cap, uint64_t *h_n_out, uint64_t *h_n_points_owned);
/* k time-sorted surfel lists, concatenated in d_in (h_counts[k] lengths) -> one list in the extraction's canonical order
 * (timestamp, ties by root voxel index and node id; without ids: timestamp, ties by list).  d_out must not alias d_in. */
int wc_merge_surfels(wc_ctx *ctx, const wc_surfel *d_in, const wc_surfel_id *d_in_ids, const uint64_t *h_counts, int k,
                     wc_surfel *d_out, wc_surfel_id *d_out_ids);
/* all-gather of every rank's surfel list + merge: every rank ends with the unsharded call's output (replicated window) */
int wc_gather_surfels(wc_ctx *ctx, const wc_surfel *d_local, const wc_surfel_id *d_local_ids, uint64_t n_local, wc_surfel *d_out,
                      wc_surfel_id *d_out_ids, uint64_t cap, uint64_t *h_n_out);

/* sweep preparation ("next" row f-1 of SURVEY.md §8: the per-point stages right in front of the hot path) ------------ */
/* Replaces the per-point loop of LidarOdometry::AddLidarScan (src/odometry/lidar_odometry.cc:489-496): lidar->imu
 * extrinsic in double (quat = w,x,y,z), cast to float, drop points with |p| < min_range, |p| > max_range or inside the
 * blind box; survivors keep their order.  Records are the 48-byte hilti_ros::Point (common.h:12-28). */
int wc_prefilter_points(wc_ctx *ctx, const void *d_pts_in, uint64_t n, const double ext_quat[4], const double ext_t[3],
                        double min_range, double max_range, const double blind_min[3], const double blind_max[3],
                        void *d_pts_out, uint64_t cap, uint64_t *h_n_out);
/* The same loop including its CHECK(points_buff_.empty() || pt.time >= points_buff_.back().time) (:491), evaluated on the device
 * for EVERY incoming point against the last point buffered at that moment: prev_time = stamp of the last buffered point before this
 * message (-INFINITY: buffer empty).  *h_monotonic = 0 when the CHECK would have fired.  d_kept_times (may be NULL, capacity
 * `cap`): the survivors' stamps, packed - the only thing a host-side window bookkeeping needs back.  The CHECK knows no capacity:
 * with WC_ERR_CAPACITY, *h_monotonic still covers every point of the message. */
int wc_prefilter_points_checked(wc_ctx *ctx, const void *d_pts_in, uint64_t n, const double ext_quat[4], const double ext_t[3],
                                double min_range, double max_range, const double blind_min[3], const double blind_max[3],
                                void *d_pts_out, uint64_t cap, uint64_t *h_n_out, double prev_time, double *d_kept_times,
                                int *h_monotonic);
/* Replaces UndistortSweep(sweep_in, imu_states, sweep_out) (src/odometry/lidar_odometry.cc:143-158).
 * WC_ERR_RANGE mirrors the CHECK at :149. */
int wc_undistort_sweep(wc_ctx *ctx, const void *d_pts_in, uint64_t n, const wc_imu_state *d_imu, uint64_t n_imu, void *d_pts_out);
/* The same, but the sweep leaves as the 20 bytes per point BuildSurfels reads (surfel_extraction.cc:317-324 copies x, y, z, time
 * and nothing else): d_xyz_out = n x 3 floats, d_time_out = n doubles, i.e. the wc_points {d_xyz_out, d_time_out, 12, 8, n}.
 * The undistorted 48-byte records are never written or read: 48 + 20 + 20 bytes of traffic per point up to and including the
 * extraction's pass instead of 48 + 48 + 48. */
int wc_undistort_sweep_packed(wc_ctx *ctx, const void *d_pts_in, uint64_t n, const wc_imu_state *d_imu, uint64_t n_imu, float *d_xyz_out,
                              double *d_time_out);

/* surfel pose update --------------------------------------------------------------------------------------------- */
/* Replaces UpdateSurfelPoses(const std::deque<ImuState>&, std::deque<Surfel::Ptr>&) (src/odometry/lidar_odometry.cc:160-170)
 * + Surfel::UpdatePose (src/odometry/surfel.h:48-58).  d_in_body[i] == 0 marks a surfel still in the world frame
 * (fresh from wc_extract_surfels); it is converted to the body frame and the flag set.  WC_ERR_RANGE mirrors the
 * CHECK at lidar_odometry.cc:164. */
int wc_update_surfel_poses(wc_ctx *ctx, const wc_imu_state *d_imu, uint64_t n_imu, wc_surfel *d_surf, wc_pose *d_pose,
                           uint8_t *d_in_body, uint64_t n);

/* ShrinkToFit (src/odometry/lidar_odometry.cc:243-246) moves the oldest sliding-window surfels to the fixed window with
 * push_front, oldest first: the fixed window is kept NEWEST-first.  dst[j] = src[n-1-j]; asynchronous on the
 * ctx stream. */
int wc_reverse_copy_surfels(wc_ctx *ctx, const wc_surfel *d_src_surf, const wc_pose *d_src_pose, uint64_t n,
                            wc_surfel *d_dst_surf, wc_pose *d_dst_pose);

/* correspondence -------------------------------------------------------------------------------------------------- */
/* Replaces KnnSurfelMatcher::BuildIndex(const std::deque<Surfel::Ptr>&) + Match(std::deque<Surfel::Ptr>&,
 * std::vector<SurfelCorrespondence>&) (src/odometry/knn_surfel_matcher.h:17-19, .cc:3-49; calls lidar_odometry.cc:532-538).
 *   same_set != 0 : sliding-window matcher, the targets ARE the queries (pass the same arrays twice); pairs are
 *                   (older, newer) indices into that set, at most one per query, in query order
 *   same_set == 0 : fixed-window matcher; pair.first indexes the targets (fixed window), pair.second the queries
 *   d_knn_idx / d_knn_d2 (may be NULL): the raw exact k nearest neighbours per query (k = wc_params.knn_k), the output
 *                   of FLANNKNearestSearch (cc:75-89), for known-answer tests; asking for them gives the plain k-NN walk.  With
 *                   them NULL the walk is bounded by the nearest gate-passing candidate as well as by the k-th distance - Match
 *                   takes the FIRST of the k neighbours that passes the gates (cc:24-46), so the pair list is the same, byte for byte
 * Surfels must be in the body frame with poses attached (wc_update_surfel_poses). */
int wc_match(wc_ctx *ctx, const wc_surfel *d_q_surf, const wc_pose *d_q_pose, uint64_t nq, const wc_surfel *d_t_surf,
             const wc_pose *d_t_pose, uint64_t nt, int same_set, wc_pair *d_pairs, uint64_t cap, uint64_t *h_n_pairs,
             uint32_t *d_knn_idx, double *d_knn_d2);

/* What the walk of the last wc_match on this context touched (the index is a 6-D kd-tree with bounding boxes, csrc/match_tree.inc),
 * from a sample of its wavefronts: h_out[0 .. 3] = wide nodes opened, leaves scanned, points looked at, exact
 * fp64 distances - sums over h_out[4] sampled queries; h_out[5] = depth of the tree, h_out[6] = levels above the buckets,
 * h_out[7] = targets.  Measurement only (bench.py's candidates-per-query figure). */
int wc_match_stats(wc_ctx *ctx, double h_out[8]);

/* Multi-GPU form of wc_match (the queries are independent, knn_surfel_matcher.cc:22-48): a COLLECTIVE of the ctx's
 * communicator - every rank calls it with the same replicated arguments; each searches a contiguous share of the queries (in
 * tree-leaf order) and ONE all-gather of the gated neighbour lists (4 k bytes per query) gives every rank the whole table, on
 * which the order-dependent de-duplication (cc:35-38) runs replicated: every rank ends with the unsharded call's pairs, byte for
 * byte.  wc_match itself is never a collective, whatever is installed on the ctx.  Without a communicator (or a world of one) this
 * is wc_match.  A rank that fails locally BEFORE the all-gather (an allocation, a HIP error) returns its error without entering it:
 * treat a non-zero return of any rank as fatal for the job (wc_window_build_sharded, whose local part can fail on its arguments,
 * joins its share check with a poisoned share instead). */
int wc_match_sharded(wc_ctx *ctx, const wc_surfel *d_q_surf, const wc_pose *d_q_pose, uint64_t nq, const wc_surfel *d_t_surf,
                     const wc_pose *d_t_pose, uint64_t nt, int same_set, wc_pair *d_pairs, uint64_t cap, uint64_t *h_n_pairs);
/* both searches of an outer iteration as collectives (one after the other: their all-gathers share the ctx stream) */
int wc_match_pair_sharded(wc_ctx *ctx, const wc_surfel *d_sld_surf, const wc_pose *d_sld_pose, uint64_t n_sld,
                          const wc_surfel *d_fix_surf, const wc_pose *d_fix_pose, uint64_t n_fix, wc_pair *d_pairs_sld, uint64_t cap_sld,
                          uint64_t *h_n_pairs_sld, wc_pair *d_pairs_fix, uint64_t cap_fix, uint64_t *h_n_pairs_fix);

/* Both correspondence searches of one outer iteration (the two KnnSurfelMatcher objects of lidar_odometry.cc:530-538) at
 * once.  Same results, bit for bit, as
 *   wc_match(ctx, sld, sld_pose, n_sld, sld, sld_pose, n_sld, 1, d_pairs_sld, ...) followed by
 *   wc_match(ctx, sld, sld_pose, n_sld, fix, fix_pose, n_fix, 0, d_pairs_fix, ...),
 * but the fixed-window search runs on a helper context of its own (own stream and scratch, created on first use, ordered
 * behind the work already enqueued on the ctx stream): the builds of the two trees are chains of small launches and a search is a
 * single round of wavefronts of unequal length, so each fills the slots the other leaves.  Never a collective
 * (wc_match_pair_sharded is). */
int wc_match_pair(wc_ctx *ctx, const wc_surfel *d_sld_surf, const wc_pose *d_sld_pose, uint64_t n_sld,
                  const wc_surfel *d_fix_surf, const wc_pose *d_fix_pose, uint64_t n_fix, wc_pair *d_pairs_sld, uint64_t cap_sld,
                  uint64_t *h_n_pairs_sld, wc_pair *d_pairs_fix, uint64_t cap_fix, uint64_t *h_n_pairs_fix);

/* window problem: factors + Levenberg-Marquardt ----------------------------------------------------------------- */
/* Replaces the ceres::Problem construction of lidar_odometry.cc:541-545:
 *   BuildSldWinLidarResiduals (cc:254-297) — d_pairs_sld index the sliding-window surfels (older, newer),
 *   BuildFixWinLidarResiduals (cc:299-317) — d_pairs_fix: first = fixed-window surfel, second = sliding-window surfel,
 *   BuildImuResiduals         (cc:319-363) — h_imu: the window's IMU states (host; a few thousand records),
 * with SampleState timestamps h_sample_times[ns] (ascending), gravity of the last sample state and the
 * SubsetParameterization gauge flag (cc:556-560).  Surfels must already carry poses (wc_update_surfel_poses).
 * The packed per-correspondence records are built once here; the calls below reuse them.
 * 2 <= ns <= 340 (dense normal equations of 12 ns unknowns; the reference's default 6.5 s window has 82 sample states),
 * otherwise WC_ERR_ARG.
 * Refusals that restate the reference's CHECKs: WC_ERR_ORDER for a correspondence whose first stamp is not below its second (cc:256, :301;
 * reported ahead of RANGE), WC_ERR_RANGE for a bracketed surfel stamp outside [times[0], times[ns-1]) (cc:259-265, :304-305; the fixed
 * surfel of d_pairs_fix is not bracketed) and for an IMU triple whose second or third stamp lies outside the sample states of its factor,
 * [times[sp1], times[sp1+2]] - [times[sp1], times[sp1+1]] in the last interval - (ImuFactor::ComputeStateCorr, cost_functor.h:367, :390).
 * Ordering: every host argument (h_imu, h_sample_times, h_grav) has been consumed when the call returns, and argument errors the
 * device finds (a surfel stamp outside the sample-state range, a correspondence that is not (older, newer)) are reported by it;
 * the call's LAST device work - the records and one copy of host-built lists - may still be in flight on the ctx stream.  The
 * calls that use the problem (wc_window_solve / _linearize / _evaluate) are enqueued behind it on that stream; a caller that reads
 * the device arguments' buffers on ANOTHER stream orders itself with an event on the ctx stream, as after any asynchronous call.
 * Parameters: the build copies the context's factor parameters (surfel_sigma0, cauchy_a, w_gyr, w_acc, w_bg, w_ba, imu_dt,
 * reference_quirks) into the problem; every later linearisation, evaluation and solve of this problem uses that copy, whatever
 * wc_ctx_set_params is given in between.  max_iterations alone is read by wc_window_solve when it is called. */
int wc_window_build(wc_ctx *ctx, const wc_surfel *d_sld_surf, const wc_pose *d_sld_pose, const wc_pair *d_pairs_sld,
                    uint64_t n_pairs_sld, const wc_surfel *d_fix_surf, const wc_pose *d_fix_pose, const wc_pair *d_pairs_fix,
                    uint64_t n_pairs_fix, const wc_imu_state *h_imu, uint64_t n_imu, const double *h_sample_times, uint64_t ns,
                    const double *h_grav, int fix_first_pos);
/* Multi-GPU form (correspondences and IMU factors sharded, unknowns replicated): a COLLECTIVE of the ctx's
 * communicator.  EVERY rank passes the SAME replicated arguments as it would to wc_window_build; the library takes this rank's
 * contiguous share of both correspondence lists - the IMU factors, a few hundred to two thousand, stay on EVERY rank -, and one small
 * all-reduce checks that the shares add up to the whole problem (WC_ERR_ARG otherwise).  From then on wc_window_linearize / _evaluate /
 * _solve on this problem are collectives, two per linearisation (round 6): {cost of the surfel factors, spare} - 16 bytes, all the
 * trust-region decision waits for - and {6 x 6 pose corner of every upper block pair, pose half of g} (surfel factors reach nothing
 * else: 0.60 MB at 64 sample states, 2.35 MB at 127), which the in-library RCCL binding runs on a side stream beside the bias
 * elimination; every rank takes identical accept / reject decisions on identical numbers.  (Development option lm_one_collective:
 * rounds 3 - 5's ONE all-reduce of {upper block pairs of H, g, cost} with the IMU triples sharded too: 0.76 / 2.7 MB.)
 * A problem built with wc_window_build is never a collective, whatever is installed on the ctx (a caller that shards the factors
 * itself opts in with wc_window_set_allreduce).  Without a communicator (or a world of one) this is wc_window_build. */
int wc_window_build_sharded(wc_ctx *ctx, const wc_surfel *d_sld_surf, const wc_pose *d_sld_pose, const wc_pair *d_pairs_sld,
                            uint64_t n_pairs_sld, const wc_surfel *d_fix_surf, const wc_pose *d_fix_pose, const wc_pair *d_pairs_fix,
                            uint64_t n_pairs_fix, const wc_imu_state *h_imu, uint64_t n_imu, const double *h_sample_times, uint64_t ns,
                            const double *h_grav, int fix_first_pos);
/* counts[4] = {binary factors, unary factors, imu factors, assembly pieces} (of THIS rank's share for a sharded problem);
 * wc_window_reduce_bytes: bytes one linearisation's collectives carry (0: the problem is not sharded).  A problem built by
 * wc_window_build_sharded has two per linearisation since round 6 - {cost of the surfel factors, spare} (16 bytes) and {6 x 6 pose corner of
 * every upper block pair, pose half of g} -, the IMU factors being replicated; the figure is their sum */
uint64_t wc_window_reduce_bytes(wc_ctx *ctx);
int wc_window_counts(wc_ctx *ctx, uint64_t counts[4]);
/* problem.Evaluate(apply_loss_function = true) (lidar_odometry.cc:62-65): cost = 1/2 sum rho; d_residuals (may be NULL)
 * receives the loss-corrected residuals in the reference's block order: binary, unary, 12 per IMU factor.
 * h_x = the 12*ns correction blocks (SampleState::data_cor, surfel.h:13-17). */
int wc_window_evaluate(wc_ctx *ctx, const double *h_x, double *h_cost, double *d_residuals);
/* one linearisation: dense row-major H = J^T J (12ns x 12ns) and g = J^T r, loss-corrected, gauge columns zeroed */
int wc_window_linearize(wc_ctx *ctx, const double *h_x, double *d_H, double *d_g, double *h_cost);
/* measurement: `reps` linearisations at h_x back to back on the ctx stream between two HIP events; *h_ms = device time of one
 * (the kernels and the gap between them - no upload, no wait for the mailbox, no caller between two of them) */
int wc_window_linearize_timed(wc_ctx *ctx, const double *h_x, int reps, float *h_ms_per_linearisation);
/* ceres::Solve with the reference's options (lidar_odometry.cc:551-561): trust-region LM, <= max_iterations.
 * h_x_inout: corrections in / optimised corrections out; h_first_step (may be NULL) receives the first LM increment. */
int wc_window_solve(wc_ctx *ctx, double *h_x_inout, wc_solve_summary *summary, double *h_first_step);
/* multi-GPU, for a caller that shards the factors ITSELF (each rank builds its own slices with wc_window_build): install a
 * "sum this device buffer over all ranks" callback; called once per linearisation on the packed {upper block pairs of H, g, cost}
 * buffer (layout: wc_window_build_sharded above) and once per candidate-cost evaluation (one double).  NULL removes it.  On a
 * problem built by wc_window_build_sharded - before or after the callback is installed - the callback runs THAT build's collectives
 * in place of the communicator's (the two-collective form: {cost, spare}, then the pose corners); the form is the build's. */
int wc_window_set_allreduce(wc_ctx *ctx, int (*fn)(void *user, double *d_buf, uint64_t count), void *user);

/* voxel-downsampled point map (device resident) ------------------------------------------------------------------------------- */
/* The accumulated map of the reference's README (pics/point_cloud_accumulated.jpg): every sweep undistorted with its final poses and
 * published on /scan_in_imu_frame (lidar_odometry.cc:584-595), gathered in world coordinates, thinned by DownSamplingVoxel
 * (src/odometry/surfel_extraction.cc:228-261: every occupied voxel replaced by the centroid of its points).  The reference leaves the
 * accumulation to RViz and DownSamplingVoxel has no callers; here the map is a hash table in HBM that every insert grows (csrc/map.hip).
 *   voxel of a point  VoxelLoc(p, v) = floor((double)p / v) per axis (surfel_extraction.h:59-64)
 *   centroid          center / count (:258) from per-voxel 64-bit fixed-point sums (unit 2^-32 m, relative to a point of the voxel on
 *                     the 2^-10 m grid) rounded to float once: order independent, so the map after inserting A, B, C is, bit for bit,
 *                     the map of A u B u C inserted in any split, order or schedule
 *   limits            0.01 <= v <= 4.0 (below 0.01 the reference does nothing, :232-234) else WC_ERR_ARG; |k| < 2^20 per axis (keys
 *                     packed 21 bits per axis).  A point with a non-finite coordinate or a key out of range is NOT inserted and is
 *                     counted (the reference's int32 cast has no range check); at most 2^30 points per voxel (2^28 in a map created
 *                     with WC_MAP_MOMENTS, below)
 * Several maps per context are independent.  Every call works on the ctx's stream. */
typedef struct wc_map wc_map;
/* reserve_voxels: voxels the table holds before its first growth (0: none) */
int wc_map_create(wc_ctx *ctx, double voxel, uint64_t reserve_voxels, wc_map **out);
/* wc_map_create with flags (wc_types.h: WC_MAP_MOMENTS; 0 = wc_map_create; any other bit: WC_ERR_ARG) */
int wc_map_create_ex(wc_ctx *ctx, double voxel, uint64_t reserve_voxels, uint32_t flags, wc_map **out);
int wc_map_destroy(wc_ctx *ctx, wc_map *m);
/* DownSamplingVoxel's accumulation (:236-254) for the points of `pts` (DEVICE pointers, any xyz_stride >= 12 that is a multiple of 4:
 * the 48-byte hilti_ros::Point or packed xyz; pts->time is ignored and may be NULL).  h_n_rejected (may be NULL) receives the number
 * of this call's points that were not inserted; asking for it waits for the call, passing NULL returns without waiting.  The table
 * grows on the device before an insert that could fill more than half of it. */
int wc_map_insert(wc_ctx *ctx, wc_map *m, const wc_points *pts, uint64_t *h_n_rejected);
/* occupied voxels and points inserted so far (both may be NULL); waits for the ctx stream */
int wc_map_size(wc_ctx *ctx, wc_map *m, uint64_t *h_voxels, uint64_t *h_points);
/* h_info[4] = {table slots, growths so far, points rejected so far, bytes of HBM the table holds}; waits for the ctx stream */
int wc_map_info(wc_ctx *ctx, wc_map *m, uint64_t h_info[4]);
/* the map as DownSamplingVoxel's output (:255-260), in ascending (kx, ky, kz) order (the reference's is hash-map order):
 * d_xyz = n x 3 float centroids, d_count = n point counts, d_keys (may be NULL) = n x 3 voxel indices; *h_n = n.
 * WC_ERR_CAPACITY with *h_n = the needed count when cap < n.  Reads the size back, then enqueues its kernels on the ctx stream and
 * returns: the outputs are complete for whatever is ordered behind it on that stream (wc_d2h, wc_sync) */
int wc_map_export(wc_ctx *ctx, wc_map *m, float *d_xyz, uint32_t *d_count, int32_t *d_keys, uint64_t cap, uint64_t *h_n);
/* empties the map (the table keeps its size) */
int wc_map_clear(wc_ctx *ctx, wc_map *m);
/* Nearest-voxel query.  For every query point q (DEVICE pointers, the wc_points rules of wc_map_insert; pts->time is ignored) d_hits
 * receives one wc_map_hit:
 *   voxel of the query  kq = floor((double)q / v) per axis (VoxelLoc).  A non-finite coordinate or |kq| >= 2^20 on any axis cannot be
 *                       searched: flags = 1, count = 0, d2 = +inf
 *   candidates          the occupied voxels with index kq + {-1, 0, 1}^3 (neighbour indices outside the key range are skipped)
 *   distance            to a candidate's centroid c, the float triple wc_map_export returns for it:
 *                       d2 = (dx*dx + dy*dy) + dz*dz in fp64 with dx = (double)q.x - (double)c.x, no fused multiply-add
 *   result              the candidate of smallest d2, ties to the smaller (kx, ky, kz) lexicographically; accepted iff
 *                       d2 <= max_dist * max_dist (the product formed once on the host in fp64), otherwise a miss (count = 0)
 * so a restatement on the exported map reproduces every hit bit for bit.  max_dist must be > 0 (NaN or <= 0: WC_ERR_ARG); +inf means
 * "the nearest of the 27 voxels, whatever its distance".  Consequence: a centroid within max_dist <= v of q lies in one of the 27
 * voxels, so for max_dist <= v the result is the globally nearest centroid within max_dist - the only exception is a centroid that
 * the rounding to float carried across a face of its own voxel.
 * h_n_found (may be NULL) receives the number of accepted hits; asking for it waits for the stream, passing NULL returns without
 * waiting.  queries->n == 0 is WC_OK; NULL d_hits with n > 0 or a map of another context is WC_ERR_ARG.  The map is not modified. */
int wc_map_nearest(wc_ctx *ctx, wc_map *m, const wc_points *queries, double max_dist, wc_map_hit *d_hits, uint64_t *h_n_found);
/* k nearest voxels within a radius.  For every query point q (the wc_points rules of wc_map_nearest) d_hits receives params->k
 * wc_map_hit records, d_hits[i * k + j], j = 0 .. k - 1, and d_within[i] (may be NULL) one count; a pure function of the exported map
 * and the query:
 *   voxel of the query  kq and the query that cannot be searched: exactly wc_map_nearest's
 *   candidates          the occupied voxels with index kq + {-reach .. reach}^3 (27 for reach 1, 125 for reach 2) whose every index
 *                       lies inside the key range (others are skipped), with count >= min_points and, with WC_MAP_KNN_NOT_OWN, an
 *                       index other than kq
 *   distance            wc_map_nearest's d2: to the float centroid wc_map_export returns, (dx*dx + dy*dy) + dz*dz in fp64, no fused
 *                       multiply-add
 *   acceptance          a candidate is accepted iff d2 <= max_dist * max_dist (the product formed once on the host in fp64)
 *   answer              the accepted candidates in ascending d2, ties in ascending (kx, ky, kz): the first min(k, within) of them are the
 *                       query's first records, ordinary wc_map_hit records; its remaining records are the miss record (zeros, d2 = +inf)
 *   d_within[i]         the number of accepted candidates, NOT capped by k: the neighbour count of a radius filter
 *   unsearchable query  all k records are the miss record with flags = 1, and d_within[i] = 0
 * so a restatement on the exported map reproduces every record bit for bit.  Consequence: a centroid within max_dist <= reach * v of q
 * lies in one of the candidate voxels, so for max_dist <= reach * v the answer is the k globally nearest centroids within max_dist, with
 * wc_map_nearest's one exception (a centroid that the rounding to float carried across a face of its own voxel).  With k = 1, reach = 1,
 * min_points = 1 and flags = 0 the records are byte for byte wc_map_nearest's.
 * h_out (may be NULL) receives {queries with within > 0, records written = sum of min(k, within), sum of within}; asking for it waits
 * for the stream, passing NULL returns without waiting.  queries->n == 0 is WC_OK.  WC_ERR_ARG, with every output untouched: NULL params,
 * NULL d_hits with n > 0, k outside 1 .. 16, reach other than 1 or 2, min_points == 0, an unknown flag, max_dist NaN or <= 0, a map of
 * another context.  The map is not modified; plain and WC_MAP_MOMENTS maps behave alike; a removed voxel is never a candidate. */
int wc_map_knn(wc_ctx *ctx, wc_map *m, const wc_points *queries, const wc_map_knn_params *params, wc_map_hit *d_hits, uint32_t *d_within,
               uint64_t h_out[3]);
/* Crop and compact.  A voxel k is kept iff floor(lo[a] / v) <= k[a] <= floor(hi[a] / v) on all three axes (the voxels that intersect
 * the box); +-inf bounds are allowed and clamped to the key range, NaN or lo[a] > hi[a] is WC_ERR_ARG.  The kept voxels keep their
 * integer sums and counts: the result is, bit for bit, the map of exactly those inserted points whose voxel is kept.  They are
 * rehashed into a fresh table of the smallest power of two >= 2 * max(kept, 1) slots (an all-infinite box: "shrink to fit"), and
 * the old table's memory is released.  The voxel and point counts (wc_map_size) become those of the kept voxels; the rejected and
 * growth counts stay.  *h_removed_voxels (may be NULL) receives the number of voxels dropped.  Waits for the ctx stream either way:
 * the new table is sized from the kept count. */
int wc_map_crop(wc_ctx *ctx, wc_map *m, const double lo[3], const double hi[3], uint64_t *h_removed_voxels);

/* Carving: free space by visibility.  A lidar return also says that the space between the sensor and the return is empty: every point p
 * of `pts` (DEVICE pointers, the wc_points rules of wc_map_insert: either stride, pts->time ignored; every k-th ray: a larger xyz_stride)
 * is the end of a ray from `origin` - ONE sensor position for the whole call, in the map's frame - and an occupied voxel that enough
 * rays of the call passed through, and in which none of them ended, is SELECTED.  This call counts what it selects and
 * leaves the map as it is: voxels_removed and points_removed say what a removal would take (wc_map_carve_remove, below, takes
 * it).  Every expression is fp64 without fused multiply-add, so a restatement (tests/map_carve_ref.py) reproduces the counts exactly:
 *   ray           o = origin, P = (double)p, d = P - o, len2 = (d_x d_x + d_y d_y) + d_z d_z; k0 = floor(o / v), ke = floor(P / v) per
 *                 axis (VoxelLoc, true division); M = sum over the axes of |ke_a - k0_a|
 *   end mark      a point with finite coordinates and |ke_a| < 2^20 marks its end voxel ke, whether or not its ray is used
 *   used          iff p is finite, |k0_a| and |ke_a| < 2^20, min_range^2 <= len2 <= max_range^2 (the squares formed once on the host)
 *                 and M <= max_steps; every other point counts in rays_skipped
 *   walk          k^(0) = k0, ..., k^(M) = ke.  At a step the candidate axes are those with k_a != ke_a; for a candidate
 *                 b_a = (double)(k_a + (ke_a > k0_a ? 1 : 0)) * v, t_a = (b_a - o_a) * inv_a, inv_a = 1.0 / d_a formed once per ray; the
 *                 lowest candidate axis steps by sign(ke_a - k0_a) unless a later candidate's t is strictly smaller (ties: the lowest
 *                 axis).  b_a comes from the integer at every step (nothing drifts), a non-candidate axis is never used, and
 *                 ke_a != k0_a implies d_a != 0: the walk reaches ke after exactly M steps for any input - a counted loop
 *   seen through  k^(i) is seen through by the ray iff max_a |k^(i)_a - ke_a| > shell; a walk visits a voxel at most once;
 *                 through(k) = the number of used rays that see through k; steps = the sum of M over the used rays
 *   selection     an occupied voxel is selected iff through(k) >= min_rays and no point of this call marked it as an end voxel: integer
 *                 functions of the call's point set, independent of order, split, grid size and schedule
 * Plain and WC_MAP_MOMENTS maps alike.  The call waits and fills *h_out.  A uint32 word per slot of scratch is taken on the first call
 * and grows with the table.
 * WC_ERR_ARG: a NULL argument; a non-finite origin; a NaN or negative range; min_range > max_range; shell > 8; min_rays = 0; max_steps
 * outside 1..65536; reserved != 0; pts->n >= 2^31; a map of another context.  pts->n = 0 or an empty map: WC_OK, nothing selected.
 * Limits: one origin per call - sensor motion within the sweep and the lever arm are ignored, `shell` is the margin for
 * both; a ray grazing a surface passes through surface voxels no return of the call fell into (min_rays and the end marks reduce
 * this and do not remove it). */
int wc_map_carve(wc_ctx *ctx, wc_map *m, const wc_points *pts, const double origin[3], const wc_map_carve_params *params,
                 wc_map_carve_result *h_out);

/* Removal in place.  A removed voxel's slot keeps a TOMBSTONE - a key word no voxel can have - instead of its key; the table
 * keeps its size, and the next replacement of the table (a growth, a crop's, or a purge: a fresh table of the same size, made when live
 * voxels + tombstones + the voxels a call may add would fill more than half of it) drops the tombstones.  After a removal the map is,
 * through every call that reads it (wc_map_size, _export, _export_surfels, _export_state, _nearest, _nearest_plane, _linearize, _carve,
 * _raycast, _merge as either side, _crop), bit for bit the map of the inserted points whose voxel was not removed.  A voxel that is
 * removed and inserted again starts from zero sums.  wc_map_size reports the live voxels and their points; wc_map_info keeps its four
 * words and their meaning (a purge is not a growth; the cumulative rejected count is untouched).
 *
 * wc_map_carve_remove: the definition, argument rules and errors are wc_map_carve's, word for word (reserved != 0 included); *h_out is
 * what wc_map_carve would have returned on the same map, and the voxels it selects are then gone.  The call waits.  pts->n = 0 or an
 * empty map: WC_OK, nothing removed. */
int wc_map_carve_remove(wc_ctx *ctx, wc_map *m, const wc_points *pts, const double origin[3], const wc_map_carve_params *params,
                        wc_map_carve_result *h_out);
/* Removes the voxels with the n indices d_keys (DEVICE, n x 3 int32 (kx, ky, kz), 4-aligned, in any order).
 * h_out[3] = {voxels removed, points removed, keys that removed nothing}; the last counts the keys that are absent, the keys with
 * |k_a| >= 2^20 on any axis, and the second and later copies of a key in the list - integer functions of the key set, independent of
 * order, grid size (development option map_remove_groups) and schedule.  The call waits.  n = 0: WC_OK, nothing is launched and d_keys is
 * not looked at.  WC_ERR_ARG: n > 2^31, a NULL or misaligned d_keys, a NULL h_out, a map of another context. */
int wc_map_remove_keys(wc_ctx *ctx, wc_map *m, const int32_t *d_keys, uint64_t n, uint64_t h_out[3]);
/* h_out[2] = {tombstones in the table now, purges so far}; host state, no wait */
int wc_map_tombstones(wc_ctx *ctx, wc_map *m, uint64_t h_out[2]);

/* Connected components of the occupied voxels, and removal of the small ones.  params: wc_map_cc_params (wc_types.h).
 *   nodes       the occupied voxels (tombstones are not voxels) whose point count is >= min_points.  min_points >= 1
 *   edges       two nodes a, b are adjacent iff a != b, max_axis |a - b| == 1 and sum_axis |a - b| <= c, with c = 1, 2, 3 for
 *               connectivity 6, 18, 26; any other value of connectivity is WC_ERR_ARG.  A neighbour index outside the key range
 *               (|k_a| >= 2^20) does not exist: the packed key's 21-bit fields never wrap into another axis or to the other end of the range
 *   component   the classes of the transitive closure
 *   root        the root of a component is its voxel of smallest (kx, ky, kz), which is the smallest packed key
 *   numbering   components are numbered 0 .. C-1 in ascending order of their root
 *   labels      voxels are listed in the order of wc_map_export (ascending key); label[i] is the component number of export entry i; an
 *               occupied voxel that is not a node gets WC_MAP_NO_COMPONENT = 0xFFFFFFFF
 *   record      wc_map_component, 40 bytes, 8-aligned: first = export index of the root; voxels; points; kmin[3], kmax[3] = the key
 *               bounding box.  All fields are integers, so every field is order independent
 * A component is a function of the set of occupied keys (and their counts, through min_points) alone: every output is independent of
 * table layout, grid size (development option map_cc_groups) and schedule, and a restatement on the exported map (tests/map_components_ref.py)
 * reproduces it byte for byte.
 *
 * wc_map_components: d_keys (DEVICE, n x 3 int32, 4-aligned, may be NULL) receives the voxel indices and d_label (DEVICE, n uint32) the
 * labels of the n occupied voxels, cap = the entries either holds; d_comps (DEVICE, 8-aligned, may be NULL) receives the C records, cap_comps
 * = the records it holds.  h_out[4] = {voxels n, nodes, components C, voxels of the largest component}.  WC_ERR_CAPACITY with h_out filled
 * when cap < n (nothing is written to d_keys / d_label) or when d_comps != NULL and cap_comps < C (nothing is written to d_comps).  An empty
 * map is WC_OK with zeros.  The map is read, never written, and so is every scratch whose content another call of the map relies on: the
 * call has a uint32 word per slot and its per-voxel arrays of its own (taken on the first call, grow-only), and shares only the export's
 * sort buffers, which every export fills afresh.  The call waits.  Plain and WC_MAP_MOMENTS maps alike.
 * WC_ERR_ARG: a NULL ctx, map, params or h_out; a map of another context; connectivity not 6 / 18 / 26; min_points = 0; an unknown flag;
 * reserved != 0; a misaligned pointer; cap > 0 with d_label NULL.  WC_ERR_INTERNAL (map untouched): a bounded loop of the labelling
 * ran past its bound. */
int wc_map_components(wc_ctx *ctx, wc_map *m, const wc_map_cc_params *params, int32_t *d_keys, uint32_t *d_label, uint64_t cap,
                      wc_map_component *d_comps, uint64_t cap_comps, uint64_t h_out[4]);
/* Removes, in place and through tombstones (above), every voxel of a component with voxels < min_voxels or points < min_comp_points.  A
 * threshold of 0 switches its test off; both 0 removes nothing.  With flag WC_MAP_CC_DROP_SPARSE it also removes the occupied voxels that
 * are not nodes; without it they stay.  h_out[4] = {components before, components removed, voxels removed, points removed}.  After it the
 * map is, through every call that reads it, bit for bit the map of the points whose voxel stayed.  The call is idempotent: components are
 * disjoint, so what stays keeps its components, and a second call removes nothing.  The call waits.  Argument errors as wc_map_components;
 * every error leaves the map as it was. */
int wc_map_remove_small(wc_ctx *ctx, wc_map *m, const wc_map_cc_params *params, uint32_t min_voxels, uint64_t min_comp_points, uint64_t h_out[4]);
/* The same function of an exported map on the host, without a GPU or a context: keys (n x 3 int32) and count (n uint32) as wc_map_export
 * returns them; label_out (n uint32), comps_out (may be NULL; cap_comps records) and h_out as wc_map_components fills them.
 * WC_ERR_ARG: keys that are not strictly ascending in (kx, ky, kz) (unsorted or duplicate) or have |k_a| >= 2^20; n > 2^31; a NULL
 * argument (keys, count, label_out with n > 0; params; h_out); params as above.  WC_ERR_CAPACITY with h_out (and label_out) filled when
 * comps_out != NULL and cap_comps < C. */
int wc_map_label_keys(const int32_t *keys, const uint32_t *count, uint64_t n, const wc_map_cc_params *params, uint32_t *label_out,
                      wc_map_component *comps_out, uint64_t cap_comps, uint64_t h_out[4]);

/* Ray casting: what does the map put along a ray?  Every point p of `pts` (DEVICE pointers, the wc_points rules of wc_map_insert: either
 * stride, pts->time ignored) is the END of a ray from `origin` - ONE position for the whole call, in the map's frame; "in a direction up to
 * a reach" is the end point origin + reach * direction, and it is the end point that defines the ray - and d_hits (DEVICE, 8-aligned)
 * receives one wc_map_ray_hit per point: the first occupied voxel among the positions of the ray's walk that are tested.  The map is read,
 * never written, and so is every scratch another call of the map uses.  The ray and its walk are wc_map_carve's, word for word, in fp64
 * without fused multiply-add, so a restatement on the exported map (tests/map_raycast_ref.py) reproduces every record byte for byte:
 *   ray      o = origin, P = (double)p, d = P - o, len2 = (d_x d_x + d_y d_y) + d_z d_z; k0 = floor(o / v), ke = floor(P / v) per axis
 *            (VoxelLoc, true division); M = sum over the axes of |ke_a - k0_a|
 *   cast     iff p is finite, |k0_a| and |ke_a| < 2^20, min_range^2 <= len2 <= max_range^2 (the squares formed once on the host) and
 *            M <= max_steps - wc_map_carve's "used"; every other point counts in rays_skipped and its record has flags = 1
 *   walk     k^(0) = k0, ..., k^(M) = ke.  At a step the candidate axes are those with k_a != ke_a; for a candidate
 *            b_a = (double)(k_a + (ke_a > k0_a ? 1 : 0)) * v, t_a = (b_a - o_a) * inv_a, inv_a = 1.0 / d_a formed once per ray; the lowest
 *            candidate axis steps by sign(ke_a - k0_a) unless a later candidate's t is strictly smaller (ties: the lowest axis); the walk
 *            reaches ke after exactly M steps for any input - a counted loop
 *   tested   position i is tested iff i >= first_step and max_a |k^(i)_a - ke_a| >= end_shell.  end_shell = 0 tests all M + 1 positions,
 *            ke included; end_shell = s + 1 tests exactly the positions a wc_map_carve with shell = s sees through.  The distance to ke
 *            never grows along a walk: the tested positions are one contiguous run, and the walk ends behind it
 *   hit      the first tested position whose voxel is occupied with count >= min_points; the walk ends there
 *   t        the parameter at which the ray enters the hit voxel, a point of the ray being o + t d: 0.0 for i = 0, otherwise the
 *            winning t_a of the step from k^(i-1) to k^(i), the very double the step rule compared.  The range is t * |d|; it is left
 *            to the caller and no square root is formed
 *   record   xyz = the hit voxel's centroid, the float triple wc_map_export returns for it; count = its point count; key = k^(i);
 *            step = i; tested = the number of positions this ray tested, the hit included.  A miss: xyz = key = 0, count = 0, step = 0,
 *            t = +inf, tested as walked.  A ray that is not cast: the same with tested = 0 and flags = 1
 * h_out (may be NULL): rays_cast, rays_skipped, hits and tested, the sum of the records' field - integer functions of the call, independent
 * of grid size (development option map_cast_groups), order and schedule.  Asking for it waits for the stream; passing NULL returns
 * without waiting, as wc_map_nearest does.  Plain and WC_MAP_MOMENTS maps alike; an empty map makes every cast ray a miss; pts->n = 0 is
 * WC_OK.
 * WC_ERR_ARG: a NULL argument other than h_out (d_hits with n > 0 included); d_hits not 8-aligned; a non-finite origin; a NaN or negative
 * range; min_range > max_range; first_step > 65536; end_shell > 9; min_points = 0; max_steps outside 1..65536; pts->n >= 2^31; a wc_points
 * the insert would refuse; a map of another context.
 * Limits: one origin per call; a ray that grazes a surface is stopped by surface voxels well before its own return (what
 * end_shell = 1 hits on a static scene); every step is a hash probe - no coarse level skips empty space. */
int wc_map_raycast(wc_ctx *ctx, wc_map *m, const wc_points *pts, const double origin[3], const wc_map_raycast_params *params,
                   wc_map_ray_hit *d_hits, wc_map_raycast_result *h_out);

/* map surfels: the plane through every voxel's points (WC_MAP_MOMENTS) ------------------------------------------------------------ */
/* A map created with WC_MAP_MOMENTS holds nine more 64-bit words per slot (112 instead of 40 bytes, wc_map_info).  Per inserted point
 * p of voxel k, from the quantity the insert already forms:
 *   q_a = llrint((p_a - r_a) * 2^32)      r = the voxel's reference point on the 2^-10 m grid (unchanged: the centroid's sums)
 *   u_a = (q_a + 2^15) >> 16              arithmetic shift: the coordinate in units of 2^-16 m (about 15 um), a function of the point alone
 *   U_a = sum u_a,  M_ab = sum u_a u_b    ab = xx, xy, xz, yy, yz, zz; two's-complement 64-bit sums
 * |p - r| <= 2.0005 m gives |u| < 2^17.001 and products < 2^34.01: at most 2^28 points per voxel of such a map (2^30 otherwise).  All
 * sums are integers, so the moments - like the centroids - are bit-identical however the same points are split, ordered or scheduled,
 * and everything a plain map returns (wc_map_export, wc_map_nearest, wc_map_size) is byte-equal for a moments map of the same input.
 * Growth, crop and clear carry, keep and clear the moments with their voxels.
 *   covariance   population covariance of the quantised points: exactly N_ab / (n^2 2^32) m^2 with the integer N_ab = n M_ab - U_a U_b,
 *                formed in 128 bits, rounded once and divided by n^2 (csrc/map.hip: map_plane_of): within 2 ulp of the rational.
 *                Coincident points give exactly 0; points on one plane of the 2^-16 m grid across an axis give an exactly zero row
 *   ev, normal   eigenvalues ascending and the unit eigenvector of ev[0], by the closed-form solver of the extraction (csrc/fx_eig3.h;
 *                cyclic Jacobi where the matrix is diagonal or the closed form's residual exceeds 8 x 2^-53 of the scale); the normal
 *                is negated when its component of largest magnitude is negative, the lowest axis deciding a tie in magnitude
 *   plane bit    count >= 3 and ev[2] > 0
 * wc_map_export_surfels writes one wc_map_surfel per occupied voxel, in the order and number of wc_map_export, under its capacity and
 * error rules (WC_ERR_CAPACITY with *h_n = the needed count; d_out 8-aligned).  A map without moments: WC_ERR_ARG. */
int wc_map_export_surfels(wc_ctx *ctx, wc_map *m, wc_map_surfel *d_out, uint64_t cap, uint64_t *h_n);
/* the exact state: export, absorb, merge --------------------------------------------------------------------------------------- */
/* wc_map_export and wc_map_export_surfels round the table's sums; the state is the sums themselves.  A voxel k of a map of voxel size v
 * holds count, sum[a] = the sum over its points of q_a = round((p_a - r_a) * 2^32) with r_a = rint((k_a + 0.5) * v * 1024) / 1024 (a
 * function of k_a and v alone), and in a WC_MAP_MOMENTS map nine more words, in this order: U_x, U_y, U_z (sums of u = (q + 2^15) >> 16),
 * M_xx, M_xy, M_xz, M_yy, M_yz, M_zz (sums of u_a u_b).  All of them are integers, so a state that is exported and absorbed again gives
 * the map back bit for bit, and the states of two maps of one voxel size add up to the map of the points of both.
 *
 * wc_map_export_state writes one wc_map_voxel per occupied voxel into d_vox (DEVICE, 8-aligned), in the order and number of
 * wc_map_export, under its capacity and error rules: WC_ERR_CAPACITY with *h_n = the needed count when cap < n; the size is read back,
 * the kernels are enqueued on the ctx stream and the call returns.  d_mom (DEVICE, 8-aligned, may be NULL) receives n x 9 int64 moment
 * words in the order above; NULL: they are not written; non-NULL with a map created without WC_MAP_MOMENTS: WC_ERR_ARG.  A misaligned
 * pointer is WC_ERR_ARG.  The map is not modified. */
int wc_map_export_state(wc_ctx *ctx, wc_map *m, wc_map_voxel *d_vox, int64_t *d_mom, uint64_t cap, uint64_t *h_n);
/* Every one of the n records (DEVICE, 8-aligned) adds its count, its three sums and - in a WC_MAP_MOMENTS map - its nine moment words
 * (d_mom: n x 9 int64, DEVICE, 8-aligned) to the voxel of its key; the voxel is created where it is new.  The records need not be sorted
 * and the keys need not be distinct: duplicates add up.
 *   rejected   a record with |key[a]| >= 2^20 on any axis, count == 0 or count > 2^30 is counted and not applied
 *   the sums   are taken as they are, neither checked against the count nor against the voxel's extent: a state no insert could have
 *              produced gives a map no insert could have produced (centroids outside their voxel, negative variances)
 *   moments    a WC_MAP_MOMENTS map with d_mom == NULL is WC_ERR_ARG; a plain map ignores d_mom, so a moments state loads into a plain map
 *   n == 0     WC_OK, nothing is launched and no pointer is looked at; n > 2^31 is WC_ERR_ARG
 * h_n_rejected follows wc_map_insert's convention: NULL returns without waiting, non-NULL waits and receives this call's rejected
 * records.  The map's cumulative count of rejected POINTS (wc_map_info[2]) is not touched.  The voxel count grows by the new voxels and the
 * point count by the accepted records' counts.  The table grows as before an insert, the n records counting as n possible new voxels. */
int wc_map_absorb(wc_ctx *ctx, wc_map *m, const wc_map_voxel *d_vox, const int64_t *d_mom, uint64_t n, uint64_t *h_n_rejected);
/* dst becomes, bit for bit, the map of the points of both maps; src is not modified.  Table to table on the device: no export, no sort,
 * no host copy.  WC_ERR_ARG when dst == src, when either map belongs to another context, when the two voxel sizes are not bitwise equal
 * doubles, or when dst has moments and src has none (a moments src merges into a plain dst, the moments are dropped).  Waits once, to
 * read src's exact voxel count for dst's growth bound; the merge itself is enqueued on the ctx stream. */
int wc_map_merge(wc_ctx *ctx, wc_map *dst, wc_map *src);
/* A map built in another frame, merged under a rigid pose.  T is wc_map_linearize's row-major 3 x 4 (R | t) in fp64: it
 * takes src's frame to dst's.  Every live voxel of src - key k, count n, sums S and, where both maps hold moments, words U, M - is moved
 * as ONE Gaussian and added to the voxel of dst its centroid moves into; table to table on the device, in integers.  With v the voxel
 * size and r(k, v) = rint((k + 0.5) * v * 1024) / 1024, every fp64 operation below is a single IEEE operation in the stated association
 * (no fused multiply-add), so the state of dst afterwards is a pure function of the two states and T: byte-equal for every run, grid
 * size and slot order of src, and reproducible with integers plus IEEE fp64 (tests/map_moved_ref.py).
 *   1 centroid   c_a  = r(k_a, v) + ((double)S_a / (double)n) * 2^-32
 *                c'_a = ((T[4a] c_x + T[4a+1] c_y) + T[4a+2] c_z) + T[4a+3]
 *   2 key        K_a  = floor(c'_a / v), the insert's rule on the fp64 centroid.  The voxel is REJECTED - counted, not applied - when a
 *                c'_a is not finite or |K_a| >= 2^20 on an axis (and by the count cap under "limits")
 *   3 sums       m_a  = llrint((c'_a - r(K_a, v)) * 2^32),  S'_a = n m_a in wrapping 64-bit arithmetic: the moved centroid is kept to
 *                the 2^-32 m grid
 *   4 moments    N_ab = n M_ab - U_a U_b in 128 bits, rounded once to fp64 on its magnitude (as the surfel export rounds it);
 *                C_ab = fp64(N_ab) / (double)n, one division;  B_ij = (R_i0 C_0j + R_i1 C_1j) + R_i2 C_2j;
 *                C'_ij = (B_i0 R_j0 + B_i1 R_j1) + B_i2 R_j2 for i <= j;  e_a = (m_a + 2^15) >> 16;  U'_a = n e_a;
 *                M'_ab = llrint(C'_ab) + n e_a e_b.  The moved voxel's integer covariance numerator n M' - U' U' is thus exactly
 *                n llrint((R C R^T)_ab), and adding the words into a voxel that already holds points obeys the parallel-axis rule by
 *                construction.  Skipped when dst is a plain map (a moments src merges into a plain dst)
 *   5 deposit    count, S' and (U', M') are added to voxel K of dst, which is created where it is new
 * WC_ERR_ARG, with dst and a pre-filled h_out untouched: dst == src; a map of another context; voxel sizes that are not bitwise equal;
 * moments in dst and none in src; T == NULL; a non-finite entry of T; |(R^T R - I)_ij| > 1e-9 for some entry, with (R^T R)_ij =
 * (R_0i R_0j + R_1i R_1j) + R_2i R_2j - a design threshold against passing something that is no rotation, not a measurement.
 * Tombstoned slots of src are skipped; src is never modified.  dst grows as wc_map_merge grows it, by src's live voxel count, whose
 * read-back is the call's one wait before the launch.  h_out (may be NULL: the call then returns without waiting) receives {voxels
 * applied, points applied, voxels rejected, points rejected} of this call; dst's voxel and point counts grow by what is new and what was
 * applied.  An empty src is WC_OK with four zeros.
 * Limits.
 *   extent    all n points of a source voxel go to the ONE voxel their centroid moves into: nothing is split over the voxels the moved
 *             voxel straddles, so a voxel's points can reach v sqrt(3) from its far corner and its Gaussian describes them, not a
 *             sample of that voxel's own cube
 *   overflow  c' lies in voxel K, so |c'_a - r(K_a, v)| <= v / 2 + 2^-11 m (+ rounding) <= 2.0005 m for v <= 4: |m| < 2^33.001 and
 *             |e| < 2^17.001, the bound of a point's u ("map surfels" above).  The second moments do not stay inside that section's
 *             product bound: the points of a cube of side v have a variance of up to 3 v^2 / 4 along its diagonal, which a rotation can
 *             turn onto an axis, so M'_aa / n <= 3 v^2 / 4 + e_a^2 in units of 2^-32 m^2 - below 2^34.003 for v <= 2 (2^28 points per
 *             voxel hold, as for an insert), below 2^36.003 for v <= 4.  The call therefore enforces a cap: with v > 2 a source voxel of
 *             more than 2^26 points is rejected.  This holds for a source whose voxels hold points of their own cube (inserted,
 *             merged, coarsened); a source that is itself the result of a move has wider voxels ("extent") and no such bound
 *   counts    what the counts of a destination voxel reach is not checked against 2^28 / 2^30, as in wc_map_merge
 *   exactness a coincident source voxel (C = 0) stays exactly so: M'_ab = n e_a e_b.  A voxel that is exactly planar stays exactly planar
 *             only where R C R^T rounds to a singular matrix on the integer grid; in general its smallest eigenvalue becomes a rounding
 *             residue of the order of 2^-32 / n m^2
 *   identity  T = identity does NOT give wc_map_merge's bits: S' = n llrint(S / n) is not S in general, and the moments are re-based to
 *             the rounded centroid.  Use wc_map_merge for maps of one frame */
int wc_map_merge_moved(wc_ctx *ctx, wc_map *dst, wc_map *src, const double T[12], uint64_t h_out[4]);
/* Steps 1 - 4 above over n exported records on the HOST: no context, no GPU, the same per-voxel function (csrc/map.hip: map_move_voxel).
 * out_vox[i] receives the record (K, n, S') of vox[i] and out_mom[9 i ..] its nine words; a rejected record - by step 2, by the count
 * cap, or one wc_map_absorb would reject (|key| >= 2^20, count 0 or > 2^30) - is written as all zeros (count 0, which wc_map_absorb
 * skips) and counted in *n_rejected (may be NULL).  mom and out_mom are both NULL (step 4 is skipped) or both given.  wc_map_absorb of
 * the output into dst gives, bit for bit, the map wc_map_merge_moved gives.  The output keys need not be distinct or sorted.
 * WC_ERR_ARG, with every output untouched: voxel outside [0.01, 4.0]; T as above; n > 0 with vox or out_vox NULL; one of mom, out_mom NULL. */
int wc_map_move_state(const wc_map_voxel *vox, const int64_t *mom, uint64_t n, double voxel, const double T[12], wc_map_voxel *out_vox,
                      int64_t *out_mom, uint64_t *n_rejected);
/* A coarser level, exactly.  *out becomes a NEW map of voxel size V = (double)factor * v (one fp64 product; v = src's voxel size) that
 * holds the voxels of src gathered factor^3 to one; src is not modified.  With r(k, v) = rint((k + 0.5) * v * 1024) / 1024, the reference
 * point of wc_map_export_state:
 *   key     K_a = floor(k_a / factor) per axis, toward minus infinity for negative k_a; |K| < 2^20 follows from |k| < 2^20
 *   shift   D_a = (r(k_a, v) - r(K_a, V)) * 2^32: both reference points lie on the 2^-10 m grid below 2^23 m, so the difference and the
 *           product are exact in fp64 and D_a is an integer multiple of 2^22;  E_a = D_a >> 16, exact
 *   words   of a fine voxel (count n, sums S, moment words U, M), re-based in 64-bit two's-complement arithmetic:
 *             S'_a = S_a + n D_a,   U'_a = U_a + n E_a,   M'_ab = M_ab + (E_a U_b + E_b U_a) + n E_a E_b     (U: the fine voxel's)
 *           because a point's q' = q + D and u' = (q + D + 2^15) >> 16 = u + E.  The re-based words are added to voxel K of the new map,
 *           which is created where it is new.  Integer sums: no order matters
 *   flags   0: a plain map (a WC_MAP_MOMENTS src drops its moments); WC_MAP_MOMENTS: needs a WC_MAP_MOMENTS src, else WC_ERR_ARG; any
 *           other bit: WC_ERR_ARG
 *   limits  factor >= 1 (factor 1: an exact copy, D = 0); V <= 4.0; a NULL argument or a map of another context: WC_ERR_ARG.  A src that
 *           holds more points in total (wc_map_size) than ONE voxel of the result may - 2^28 with WC_MAP_MOMENTS in flags, 2^30 without -
 *           is WC_ERR_CAPACITY: the simple sufficient condition under which no coarse voxel overflows.  *out is untouched by every error
 *   table   removed voxels (tombstones) are skipped; the new table has the slots wc_map_merge gives an empty destination: the smallest
 *           power of two >= twice src's exact live voxel count, whose read-back is the call's one wait; the kernel is enqueued on the
 *           ctx stream.  The result's voxel and point counts are those of its content; an empty src gives an empty map
 * Through every call that reads a map the result is, bit for bit, the map wc_map_absorb builds from the re-based records; and bit for
 * bit the map of src's points inserted at V whenever every point p has floor((double)p / V) == floor(floor((double)p / v) / factor) on
 * every axis.  That condition always holds in exact arithmetic, and in fp64 for every p when v is a power of two (the divisions are then
 * exact).  For another v it can fail only for a point whose quotient rounds onto an integer: a point on a voxel face to within rounding
 * (measured with points placed on the faces on purpose, tests/test_map_coarsen_ref.py: v = 0.1, factor 3: 333 of 3000; v = 0.1, factor 2
 * and v = 0.2, factor 5: none; uniformly random float points: none of 17 000 at any tested v).  Such a point is counted in the neighbouring coarse voxel, and its
 * offset from that voxel's reference point is still exact.  The result is an ordinary map: it grows, merges (with a map of voxel size
 * bitwise V) and is destroyed like any other. */
int wc_map_coarsen(wc_ctx *ctx, wc_map *src, uint32_t factor, uint32_t flags, wc_map **out);

/* Plane query.  The voxel is chosen as wc_map_nearest chooses it (candidates, distance, ties, max_dist, argument checks), and the first
 * 40 bytes of a wc_map_plane_hit are that call's wc_map_hit, except that bit 1 of flags is set iff a voxel was found, its
 * count >= min_points and its plane bit is set.  Then normal and sigma2 are the voxel's wc_map_surfel.normal and .ev[0], byte for byte, and
 *   dist = (n_x e_x + n_y e_y) + n_z e_z,  e = (double)q - (double)xyz as in d2, no fused multiply-add;
 * otherwise normal, sigma2 and dist are 0.  The eigen-solve runs once per query, for the winning voxel.  h_n_found counts the hits of
 * wc_map_nearest, not the planes.  min_points < 3 or a map without moments: WC_ERR_ARG. */
int wc_map_nearest_plane(wc_ctx *ctx, wc_map *m, const wc_points *queries, double max_dist, uint32_t min_points,
                         wc_map_plane_hit *d_hits, uint64_t *h_n_found);

/* registration against the map: point-to-plane normal equations on the device ------------------------------------------------------ */
/* wc_map_linearize moves every point of `pts` (DEVICE pointers, the wc_points rules of wc_map_insert) by the pose T - row-major 3 x 4
 * (R | t), fp64, not checked for orthonormality -, finds its plane exactly as wc_map_nearest_plane finds a query's, and reduces the
 * point-to-plane normal equations to the 240 bytes of a wc_map_normal_eq on the host.  Nothing but those 240 bytes travels back; the
 * call waits for them.  One point, with x, y, z its floats cast to double and no fused multiply-add anywhere:
 *   P_a = ((T[4a] x + T[4a+1] y) + T[4a+2] z) + T[4a+3],  q_a = (float)P_a
 *   q is searched as wc_map_nearest_plane searches a query q (same device functions: candidates, ties, max_dist, min_points, flags);
 *   the point is USED iff that record would carry flags bit 1.  Then, with Q = (double)q, n and sigma2 the record's normal and sigma2:
 *   d      the record's dist
 *   J[0] = Q_y n_z - Q_z n_y,  J[1] = Q_z n_x - Q_x n_z,  J[2] = Q_x n_y - Q_y n_x  (differences of two rounded products),  J[3..5] = n:
 *          d(dist) / d(omega, upsilon) for T <- Exp(xi) T, xi = (omega, upsilon)
 *   w2   = 1.0 / (sigma0 * sigma0 + sigma2),  s = (w2 * d) * d         (sigma0 * sigma0, a * a, max_dist * max_dist: formed once, on the host)
 *   no loss (cauchy_a = 0):  k = w2,  rho = s
 *   Cauchy loss of scale a:  k = w2 / (1.0 + s / (a * a)),  rho = (a * a) * log1p(s / (a * a))
 * k has no square root on purpose: every field of a row is a chain of IEEE multiplications, additions and divisions, so a restatement
 * reproduces a wc_map_reg_row bit for bit.  A point that is not used contributes nothing and its row is all zero.
 *   H_ab = sum (k J_a) J_b  (a <= b),   g_a = sum (k J_a) d,   cost = 0.5 * sum rho,   n_used, n_found (wc_map_nearest_plane's found count)
 * d_rows (DEVICE, 8-aligned, may be NULL) receives one wc_map_reg_row per point.
 * Order of the sums - a function of the point count alone, so H, g and cost are byte-equal from run to run, for every grid size
 * (development option map_lin_groups), for both point layouts, with and without d_rows: tile t = points [256 t, 256 t + 256); within
 * a tile the terms of rows 32 c .. 32 c + 31 are added in ascending order (chunk c, 31 additions), then the eight chunk sums in
 * ascending order (7); then, level by level, partials 32 j .. 32 j + 31 in ascending order into partial j until one is left.  The
 * largest number of floating-point additions a term passes through:
 *   A(n) = 38 + sum over the levels of (min(32, m_l) - 1),   m_0 = ceil(n / 256),  m_(l+1) = ceil(m_l / 32),  while m_l > 1
 * A(n) = 38 for n <= 256, <= 69 for n <= 8192, <= 100 for n <= 2^18 and A(2^20) = 38 + 31 + 31 + 3 = 103 (<= 128 for every n <= 2^20).
 * WC_ERR_ARG: a non-finite entry of T; a T that sends a finite point to a non-finite q; a map created without WC_MAP_MOMENTS or owned by
 * another context; max_dist not > 0 (+inf allowed), min_points < 3, reserved != 0, sigma0 not > 0 or not finite, cauchy_a < 0 or not
 * finite; a NULL argument other than d_rows.  pts->n == 0: WC_OK, h_out all zero.  The map is not modified. */
int wc_map_linearize(wc_ctx *ctx, wc_map *m, const wc_points *pts, const double T[12], const wc_map_reg_params *params,
                     wc_map_normal_eq *h_out, wc_map_reg_row *d_rows);
/* Gauss-Newton on wc_map_linearize: T_io (host, row-major 3 x 4) in, the aligned pose out.  Each iteration: linearise at T; stop with
 * termination 2 if n_used < min_used; scale H to unit diagonal (H_ab / sqrt(H_aa H_bb), the diagonal exactly 1) and factorise it by
 * Cholesky in fp64 on the host; stop with termination 2 - T_io as it was before this iteration - when a pivot (the number under the
 * square root) is not finite or below min_pivot; solve H xi = -g; R <- Rod(omega) R, t <- Rod(omega) t + upsilon with Rodrigues' formula
 * Rod(w) = I + (sin th / th) K + ((sin(th/2) / (th/2))^2 / 2) K^2, K = [w]x, th = |w|; stop with termination 0 when |omega| <= tol_rot
 * and |upsilon| <= tol_trans.  Termination 1: max_iterations steps were taken without meeting the tolerances.  One more linearisation at
 * the final T gives final_cost, n_used and n_found (after termination 2 that is the iteration's own).
 * min_pivot is a design choice, not a measurement: the pivots of the unit-diagonal matrix lie in (0, 1], and 1 / min_pivot caps how far
 * the least-determined pose direction may be amplified (a single wall leaves three directions free: pivots at rounding level).  The
 * Python binding's default is 1e-9.  WC_ERR_ARG: max_iterations < 1, tol_rot / tol_trans / min_pivot not > 0, min_used < 6, and
 * whatever wc_map_linearize refuses. */
int wc_map_align(wc_ctx *ctx, wc_map *m, const wc_points *pts, double T_io[12], const wc_map_align_opts *opts, wc_map_align_summary *h_out);
/* Coarse to fine.  levels[0] runs first - the caller passes the coarsest map first -, and level l is exactly one
 *   wc_map_align(ctx, levels[l], pts, T_io, &opts[l], &h_out[l])
 * from the pose level l - 1 left (opts and h_out: n_levels records each).  A level that ends with termination 1 or 2 leaves T_io as
 * wc_map_align defines, and the next level runs.  The levels need not be related to one another (wc_map_coarsen makes related ones: a
 * plane is searched in the 27 voxels around a point, so a level of voxel size V catches offsets of the order of V).
 * 1 <= n_levels <= 8.  The arguments of ALL levels are checked before any work, and WC_ERR_ARG then leaves T_io and h_out untouched: a
 * NULL argument, a non-finite entry of T_io, and per level everything wc_map_align and wc_map_linearize refuse (a map of another
 * context or one created without WC_MAP_MOMENTS, the options' ranges, reserved != 0).  Returns WC_OK otherwise, unless a level's call
 * itself fails (a pose that sends a finite point to a non-finite one: that level's error, the levels before it have run). */
int wc_map_align_pyramid(wc_ctx *ctx, wc_map *const *levels, uint32_t n_levels, const wc_points *pts, double T_io[12],
                         const wc_map_align_opts *opts, wc_map_align_summary *h_out);

/* many pose hypotheses in one pass ------------------------------------------------------------------------------------- */
/* wc_map_linearize for K poses of ONE point set: T is K x 12 doubles on the HOST, h_out K records, h_status K codes.
 * Contract: where h_status[h] == WC_OK, h_out[h] is byte-equal to what wc_map_linearize(ctx, m, pts, T + 12 h, params, &out, NULL)
 * writes - for every K, every grid size (development option map_lin_groups: the workgroups of the first kernel, as for the single
 * call) and both point layouts.  Per hypothesis the summation order is wc_map_linearize's, unchanged: tiles of 256 points, chunks of 32
 * rows in ascending order, the eight chunk sums in ascending order, reduce levels of fan 32 in ascending order.  One launch works on all
 * (hypothesis, tile) pairs, one launch per level reduces that level of all hypotheses, ONE copy of K x 256 bytes travels back and the
 * call waits once.  There is no d_rows.
 * A pose that sends a finite point to a non-finite one: h_status[h] = WC_ERR_ARG and h_out[h] all zero; the other hypotheses are
 * unaffected and the call returns WC_OK.
 * WC_ERR_ARG for the whole call, h_out and h_status untouched: a NULL argument; a non-finite entry anywhere in T; whatever
 * wc_map_linearize refuses of its map, points descriptor and params; K > 1024.
 * WC_ERR_CAPACITY, outputs untouched: K * ceil(n / 256) > 2^20 (hypothesis, tile) pairs - a design cap, about 270 MB of partial sums
 * (it is checked before anything of the points is read).
 * K == 0: WC_OK, nothing is touched or launched.  pts->n == 0: WC_OK, every h_out[h] zero and every status WC_OK. */
int wc_map_linearize_batch(wc_ctx *ctx, wc_map *m, const wc_points *pts, const double *T, uint32_t K, const wc_map_reg_params *params,
                           wc_map_normal_eq *h_out, int32_t *h_status);
/* wc_map_align for K starts in lockstep: T_io is K x 12 doubles on the host, in and out.  Round r linearises, in one
 * wc_map_linearize_batch launch chain, every hypothesis that still iterates together with the closing linearisation (final_cost at the
 * final T) of those that ended in round r - 1; the poses of that set are compacted on the host.  A call makes at most
 * max_iterations + 1 rounds, however large K is.  The host arithmetic per hypothesis is wc_map_align's own (one copy of it).
 * Contract: T_io + 12 h, h_out[h] and h_status[h] are, byte for byte, what wc_map_align leaves and returns for that start - a start
 * whose linearisation fails part-way (WC_ERR_ARG: T_io and the summary as they stood) included.  The call returns WC_OK then.
 * Refused as a whole, everything untouched: what wc_map_linearize_batch and wc_map_align refuse of their arguments. */
int wc_map_align_batch(wc_ctx *ctx, wc_map *m, const wc_points *pts, double *T_io, uint32_t K, const wc_map_align_opts *opts,
                       wc_map_align_summary *h_out, int32_t *h_status);
/* wc_map_align_pyramid for K starts: level l is one wc_map_align_batch over the hypotheses from the poses level l - 1 left, levels[0]
 * (the coarsest) first.  h_out is level-major: n_levels x K records, record l * K + h.  A hypothesis whose status becomes an error is
 * skipped on the later levels: its T stays, its later summaries are zero.  All levels' arguments are checked before any work
 * (wc_map_align_pyramid's refusals and wc_map_align_batch's; everything untouched).  For every hypothesis that ends with status WC_OK,
 * T_io and the summaries equal those of a single wc_map_align_pyramid call from that start, byte for byte. */
int wc_map_align_pyramid_batch(wc_ctx *ctx, wc_map *const *levels, uint32_t n_levels, const wc_points *pts, double *T_io, uint32_t K,
                               const wc_map_align_opts *opts, wc_map_align_summary *h_out, int32_t *h_status);
/* The winner of a batch; host only, no context, no GPU.  Hypothesis h is eligible iff status[h] == WC_OK, termination != 2,
 * n_used >= min_used and final_cost is finite.  Ranking: larger n_used first, then smaller final_cost, then the smaller index;
 * *best = -1 when none is eligible (K == 0 included).  The inlier count comes first on purpose: a wrong heading can end with a LOWER
 * cost than the right one, on few points that sit on floor and ceiling.  WC_ERR_ARG: a NULL argument (s and status may
 * be NULL when K == 0). */
int wc_map_align_best(const wc_map_align_summary *s, const int32_t *status, uint32_t K, uint64_t min_used, int32_t *best);
/* K yaw hypotheses around a pose; host only, no context, no GPU.  T_k = (Rz(2 pi k / K) R0 | t0), T0 = (R0 | t0) row-major 3 x 4: the
 * scan turned about the sensor's position, around the world z axis.  T_0 is T0 bitwise and every translation is t0 bitwise.  Sine and
 * cosine are rounded once from extended precision; an entry is c r - s r' or s r + c r' (two rounded products and one sum).  K == 0:
 * nothing is written.  WC_ERR_ARG: a NULL argument (T_out may be NULL when K == 0). */
int wc_pose_yaw_grid(const double T0[12], uint32_t K, double *T_out);

/* registration of a stamped sweep in continuous time: two poses ------------------------------------------------------------ */
/* wc_map_linearize_ct is wc_map_linearize for a RAW sweep: every point carries a stamp (pts->time, doubles, DEVICE), and the unknowns are
 * the pose at t_begin and the pose at t_end (wc_pose: pos, quat = (w, x, y, z); body -> map), 12 degrees of freedom.  A point's pose is
 * interpolated between the two by its stamp on the device.  On the host, once: span = t_end - t_begin, and quat_end is negated where
 * (((w0 w1 + x0 x1) + y0 y1) + z0 z1) < 0; the quaternions need not be unit.  One point, with p = its floats cast to double, t its stamp, no
 * fused multiply-add anywhere, q0 / p0 the begin pose's quat / pos and q1 / p1 the end's:
 *   s = (t - t_begin) / span,  a = 1.0 - s;  the point is IN SPAN iff t_begin <= t <= t_end (a NaN stamp is not)
 *   q_c = a * q0_c + s * q1_c  (c = w, x, y, z),   c_c = a * p0_c + s * p1_c  (c = x, y, z)
 *   nn = ((qw qw + qx qx) + qy qy) + qz qz,  f = 2.0 / nn
 *   u = v x p,  r = v x u,  v = (qx, qy, qz):  u_x = qy p_z - qz p_y, u_y = qz p_x - qx p_z, u_z = qx p_y - qy p_x, r likewise from v and u
 *   P_c = (p_c + f * (qw * u_c + r_c)) + c_c,   the moved point is (float)P_c
 * - the normalised linear blend of the two quaternions without a square root or a trigonometric function: every field is a chain of
 * IEEE multiplications, additions and one division, so a restatement reproduces it bit for bit (wc_pose_interp_move is the host's).  It is
 * NOT wc_undistort_sweep's slerp: it follows the same great arc at a slightly different speed.  With Theta the rotation angle between the
 * two poses, the blend's rotation at s leads the slerp's by
 *   delta(s) = 2 atan2(s sin(Theta / 2), (1 - s) + s cos(Theta / 2)) - s Theta
 * about the common axis: zero at s = 0, 1/2, 1, extremal near s = 0.21 and 0.79, about 0.004 Theta^3 there (DESIGN 8.12 has the value
 * at Theta = 0.2 rad).
 * A point out of span is unused, counts in n_outside, and is not searched.  A point in span: its moved float point is searched exactly
 * as wc_map_linearize searches its q (the same device functions, max_dist, min_points, flags), and J = (Q x n, n), d, w2, s2 = (w2 d) d, k
 * and rho are wc_map_linearize's, the Cauchy form included.  The unknown is xi = (xi_begin, xi_end), each (omega, upsilon), applied as
 * T_u <- Exp(xi_u) T_u, and the linearisation is  d(dist) ~ a J . xi_begin + s J . xi_end  (CT-ICP's): exact at T_begin = T_end and first
 * order in the inter-pose motion otherwise - for a point p with |p_end - p_begin| = D and Theta as above, an entry of the true gradient
 * with respect to omega_begin differs from a J_i by at most a (s D + (Theta / 2 + Theta^2 / 8) |p|), with respect to omega_end by at most
 * s (a D + (Theta / 2 + Theta^2 / 8) |p|) (the neglected translation term is a s omega x (p_end - p_begin), the rotation term is of the
 * order of the inter-pose angle), and the upsilon entries are exact.  Weights kaa = (k a) a, kab = (k a) s, kbb = (k s) s, ka = k a, kb = k s:
 *   H00_ij = sum (kaa J_i) J_j,  H01_ij = sum (kab J_i) J_j,  H11_ij = sum (kbb J_i) J_j  (i <= j; all three symmetric)
 *   g0_i = sum (ka J_i) d,  g1_i = sum (kb J_i) d,  cost = 0.5 * sum rho:   76 sums
 *   n_used, n_found (in-span points whose search found a voxel), n_outside
 * Order of the sums: wc_map_linearize's, unchanged - tiles of 256 points, chunks of 32 rows in ascending order, the eight chunk sums in
 * ascending order, reduce levels of fan 32 - so A(n) carries over, and the 640 bytes are byte-equal from run to run, for every grid size
 * (map_lin_groups), for both point layouts, with and without the optional outputs.  One 640-byte record travels back; the call waits once.
 * d_rows (DEVICE, 8-aligned, may be NULL): one wc_map_ct_row per point (J, d, k, s), all zero for an unused point.
 * d_xyz_out (DEVICE, 4-aligned, may be NULL): n x 3 floats, the moved point of every point in span and three quiet NaNs (0x7fc00000) for a
 * point out of span - the registered sweep, ready for wc_map_insert (which rejects the NaN rows).
 * WC_ERR_ARG: what wc_map_linearize refuses of its map, points and params; a NULL pts->time (with n > 0) or a time_stride that is 0 or not
 * a multiple of 8; a NULL pose or h_out; a non-finite pose entry; a quaternion whose squared norm is 0 or not finite; t_end <= t_begin or
 * a non-finite stamp bound or span; poses that send a finite point in span to a non-finite one (h_out is then zero).  pts->n == 0: WC_OK,
 * h_out all zero.  The map is not modified. */
int wc_map_linearize_ct(wc_ctx *ctx, wc_map *m, const wc_points *pts, const wc_pose *pose_begin, const wc_pose *pose_end, double t_begin,
                        double t_end, const wc_map_reg_params *params, wc_map_ct_normal_eq *h_out, wc_map_ct_row *d_rows, float *d_xyz_out);
/* Gauss-Newton on wc_map_linearize_ct: the two poses in, the aligned poses out.  Each iteration: linearise; termination 2 if
 * n_used < min_used; the 12 x 12 system of wc_map_ct_step - H = (H00 H01; H01 H11), g = (g0, g1), plus the prior - solved by
 * wc_map_align's rules (unit-diagonal scaling, Cholesky in fp64 on the host, min_pivot; one solver of a size parameter serves both); then
 *   quat_u <- quat(Rod(omega_u)) * quat_u, divided by its norm;   pos_u <- Rod(omega_u) pos_u + upsilon_u       (u = begin, end)
 * with quat(Rod(w)) = (cos(th / 2), (sin(th / 2) / th) w), th = |w| ((1, w / 2) at th = 0).  Termination 0 when |omega| <= tol_rot and
 * |upsilon| <= tol_trans for both poses; 1 after max_iterations updates; a closing linearisation gives final_cost and the counts.
 * The prior is first order: with acc the running sum of the applied steps, H_ii += w_i and g_i += w_i acc_i (w = prior[0] on the begin
 * rotation's three entries, prior[1] on the begin translation's, prior[2], prior[3] on the end's).  It is a regulariser for sweeps whose
 * geometry leaves a direction of one pose free - it pulls the SUM of the steps to zero -, not a prior on the manifold: the sum of rotation
 * vectors is the rotation's logarithm only to first order.  prior_cost = 0.5 sum w_i acc_i^2.
 * WC_ERR_ARG: max_iterations < 1, tol_rot / tol_trans / min_pivot not > 0, min_used < 12, a prior weight that is negative or not finite,
 * and whatever wc_map_linearize_ct refuses (the poses then stay as they were passed in, or as the last accepted step left them). */
int wc_map_align_ct(wc_ctx *ctx, wc_map *m, const wc_points *pts, wc_pose *pose_begin_io, wc_pose *pose_end_io, double t_begin, double t_end,
                    const wc_map_ct_align_opts *opts, wc_map_ct_align_summary *h_out);
/* The host restatement of the device's interpolation and move, same associations; host only, no context, no GPU.  xyz: n x 3 floats,
 * times: n doubles, xyz_out: n x 3 floats - the moved point, or three quiet NaNs (0x7fc00000) for a stamp out of span.  WC_ERR_ARG: a NULL
 * argument (the arrays may be NULL when n == 0), a non-finite pose entry, a zero quaternion, t_end <= t_begin or a non-finite bound. */
int wc_pose_interp_move(const wc_pose *pose_begin, const wc_pose *pose_end, double t_begin, double t_end, const float *xyz,
                        const double *times, uint64_t n, float *xyz_out);
/* The host's 12 x 12 step; host only, no context, no GPU.  A = (H00 H01; H01 H11) + diag(w), b = (g0, g1) + w * acc; xi12 solves
 * A xi = -b by wc_map_align's Cholesky of the matrix scaled to unit diagonal.  prior: 4 weights (wc_map_ct_align_opts), acc: 12 doubles.
 * WC_OK: xi12 written.  WC_ERR_NUMERIC: a pivot is not finite or below min_pivot, or the step is not finite (xi12 untouched).
 * WC_ERR_ARG: a NULL argument, min_pivot not > 0, a prior weight that is negative or not finite. */
int wc_map_ct_step(const wc_map_ct_normal_eq *ne, const double prior[4], const double acc[12], double min_pivot, double xi12[12]);

/* occupancy score of pose hypotheses ------------------------------------------------------------------------------------ */
/* For K poses of ONE point set, how many points land in an occupied voxel of the map: T is K x 12 doubles on the HOST, h_out K records on
 * the host.  Hypothesis h has the pose T + 12 h.  One point, with x, y, z its floats cast to double and no fused multiply-add anywhere:
 *   P_a = ((T[4a] x + T[4a+1] y) + T[4a+2] z) + T[4a+3],  q_a = (float)P_a          (wc_map_linearize's lines: one device function)
 *   a point with a non-finite coordinate counts nowhere; a finite point whose q is not finite counts in n_bad; otherwise
 *   k_a = floor((double)q_a / v), true fp64 division (wc_map_insert's rule: one function); the point counts in n_in iff |k_a| < 2^20
 *   on every axis, and in n_hit iff, further, voxel k is live in the table - neither empty nor removed - and holds at least
 *   params->min_points points.
 * The point's own voxel only: one probe chain per (point, pose), no neighbourhood, no plane; plain and WC_MAP_MOMENTS maps alike.
 * The counts are integers: every record is the same for every grid size (development option map_score_groups), schedule and run, and a
 * restatement reproduces it byte for byte.  reserved is written as 0.  One copy of K x 16 bytes travels back and the call waits once; the
 * map and the scratch of its other calls are only read.
 * WC_ERR_ARG, h_out untouched: a NULL argument; a non-finite entry of T; min_points = 0 or reserved != 0 in params; a points descriptor
 * wc_map_insert refuses; a map of another context; n >= 2^31; K > 2^20.
 * WC_ERR_CAPACITY, h_out untouched: K * n > 2^34 (point, pose) pairs, checked before anything is read.  Both caps are design choices, not
 * measurements.
 * K == 0: WC_OK, nothing is touched or launched (T and h_out may be NULL).  pts->n == 0: every record zero.  An empty map: n_hit = 0, n_in
 * and n_bad as defined. */
int wc_map_score_batch(wc_ctx *ctx, wc_map *m, const wc_points *pts, const double *T, uint32_t K, const wc_map_score_params *params,
                       wc_map_score *h_out);
/* Pose hypotheses on a lattice of headings and positions; host only, no context, no GPU.  K = n_yaw * n[0] * n[1] * n[2] poses, pose
 * ((k n[0] + i0) n[1] + i1) n[2] + i2 = (R_k | t): R_k the rotation of wc_pose_yaw_grid(T0, n_yaw)'s entry k, bitwise, and
 *   t_a = t0_a + ((double)(2 i_a - (n[a] - 1)) * 0.5) * step[a]       (the integer and the half are exact: one rounded product, one rounded sum)
 * - the lattice is centred on t0 in WORLD axes.  n[a] = 1 gives t0_a itself, except that -0.0 becomes +0.0.
 * WC_ERR_ARG, T_out untouched: a NULL argument; n_yaw or an n[a] of 0; K > 2^20; a step that is negative or not finite; a non-finite entry
 * of T0. */
int wc_pose_grid(const double T0[12], uint32_t n_yaw, const uint32_t n[3], const double step[3], double *T_out);
/* The M best of K scores; host only, no context, no GPU.  Hypothesis h is eligible iff n_bad == 0 and n_hit >= min_hit.  Order: larger
 * n_hit first, then the smaller index.  idx_out (M entries) receives the first min(M, eligible) indices in that order and -1 in the rest;
 * *n_out receives that count.  There is no non-maximum suppression: the neighbours of a peak may fill the list.
 * WC_ERR_ARG: a NULL n_out; a NULL scores with K > 0; a NULL idx_out with M > 0. */
int wc_map_score_top(const wc_map_score *scores, uint32_t K, uint32_t M, uint32_t min_hit, int32_t *idx_out, uint32_t *n_out);

#ifdef __cplusplus
}
#endif
#endif /* WILDCAT_HIP_H_ */
