/*
 * wc_types.h — plain-old-data records that cross the C-ABI of the MI355X hot path.
 *
 * Every record is a flat run of doubles / ints so that it can live in HBM, in a numpy array, or
 * in a C++ host struct without translation.  Each one names the reference type it stands for
 * (paths relative to the reference checkout).
 */
#ifndef WC_TYPES_H_
#define WC_TYPES_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Input point buffer.  The reference hands `std::vector<hilti_ros::Point>` (src/common/common.h:12-28,
 * a 48-byte AoS record: float x,y,z,pad @0, float intensity @16, double time @24, uint16 ring @32) to
 * BuildSurfels (src/odometry/surfel_extraction.cc:316).  The descriptor accepts that record in place
 * (xyz = base, xyz_stride = 48, time = base + 24, time_stride = 48) or a packed SoA
 * (xyz_stride = 12 or 16, time_stride = 8).  Pointers are DEVICE pointers for the wc_* entry points and
 * host pointers for the oracle. */
typedef struct wc_points {
  const void *xyz;      /* first float of point 0 (x, y, z consecutive floats)            */
  const void *time;     /* first double (timestamp of point 0), ascending                  */
  uint32_t xyz_stride;  /* bytes between consecutive points' x                             */
  uint32_t time_stride; /* bytes between consecutive points' timestamps                    */
  uint64_t n;           /* number of points                                                */
} wc_points;

#define WC_HILTI_POINT_BYTES 48
#define WC_HILTI_POINT_TIME_OFFSET 24

/* One surfel as `BuildSurfels` emits it: reference `Surfel` ctor arguments
 * (src/odometry/surfel.h:39-40, src/odometry/surfel_extraction.cc:62).  144 bytes.
 * Right after extraction center/cov/normal are in the world frame; after the first pose update they are in
 * the body frame (surfel.h:48-58). */
typedef struct wc_surfel {
  double t;          /* mean timestamp of the cluster                       */
  double center[3];  /* mean point                                          */
  double cov[9];     /* population covariance, row-major 3x3 (symmetric)    */
  double normal[3];  /* eigenvector of the smallest eigenvalue, view-flipped */
  double resolution; /* 4 * quarter_length of the emitting octree node      */
  double sigma;      /* sqrt(lambda_min)                                    */
} wc_surfel;

/* Identity of the octree node + temporal cluster a surfel came from.  Not a reference type: the
 * reference's emission order is hash-map order, so parity is checked by matching surfels
 * on this id.  node = layer | o1 << 2 | o2 << 5 | cluster << 8, where o1/o2 are the octant codes
 * 4*[x>cx] + 2*[y>cy] + [z>cz] (surfel_extraction.cc:147-158) of the layer-1 / layer-2 node and
 * `cluster` is the ordinal of the temporal cluster inside the node (dropped clusters count). */
typedef struct wc_surfel_id {
  int32_t kx, ky, kz; /* root voxel index, floor(p / voxel_size)  (surfel_extraction.h:59-64) */
  uint32_t node;
} wc_surfel_id;

/* Body->world pose attached to a surfel (surfel.h:114-115). quat = (w, x, y, z). 56 bytes. */
typedef struct wc_pose {
  double pos[3];
  double quat[4];
} wc_pose;

/* Reference `ImuState` (src/odometry/surfel.h:25-33) flattened: 112 bytes. quat = (w, x, y, z). */
typedef struct wc_imu_state {
  double t;
  double pos[3];
  double quat[4];
  double acc[3];
  double gyr[3];
} wc_imu_state;

/* Index pair produced by the matcher: reference `SurfelCorrespondence{s1, s2}`
 * (src/odometry/surfel.h:124-127) with s1 the older surfel (knn_surfel_matcher.cc:41-45).
 * For the sliding-window matcher both are indices into the query/target set (the same set);
 * for the fixed-window matcher `first` indexes the fixed-window (target) set and `second` the query set. */
typedef struct wc_pair {
  int32_t first;
  int32_t second;
} wc_pair;

/* Record of the ONE exchange step of the sharded extraction: the 20 used bytes of a point
 * (float xyz + double time) padded to 24.  A received buffer is a valid wc_points input (xyz_stride = time_stride = 24). */
typedef struct wc_route_point {
  float x, y, z;
  uint32_t src; /* spare (keeps t 8-aligned) */
  double t;
} wc_route_point;

/* Answer of wc_map_nearest for one query (not a reference type).  40 bytes, 8-aligned. */
typedef struct wc_map_hit {
  float xyz[3];   /* centroid of the voxel found: the very float triple wc_map_export returns for it          */
  uint32_t count; /* its point count; 0 = nothing found (then xyz = key = 0, d2 = +inf)                       */
  int32_t key[3]; /* its voxel index                                                                          */
  uint32_t flags; /* bit 0: the query could not be searched (non-finite coordinate or its own voxel index out of range) */
  double d2;      /* squared distance query -> centroid                                                      */
} wc_map_hit;

/* wc_map_knn (wildcat_hip.h: "k nearest voxels within a radius"; not a reference type) */
#define WC_MAP_KNN_NOT_OWN 1u /* skip the candidate whose voxel index equals the query's own kq */
typedef struct wc_map_knn_params { /* 24 bytes */
  double max_dist;     /* > 0, may be +inf; NaN or <= 0: WC_ERR_ARG                                       */
  uint32_t k;          /* 1 .. 16: records per query                                                      */
  uint32_t reach;      /* 1 or 2: candidates are the voxels kq + {-reach .. reach}^3 (27 or 125)          */
  uint32_t min_points; /* >= 1: a candidate needs count >= min_points                                     */
  uint32_t flags;      /* WC_MAP_KNN_NOT_OWN or 0; any other bit: WC_ERR_ARG                              */
} wc_map_knn_params;

/* wc_map_create_ex flags */
#define WC_MAP_MOMENTS 1u /* every voxel also accumulates the second moments of its points: surfel export and plane queries */

/* One voxel of a WC_MAP_MOMENTS map as wc_map_export_surfels writes it (not a reference type).  128 bytes, 8-aligned.  The plane
 * through the voxel's points, from exact integer moments of the points quantised to 2^-16 m (wildcat_hip.h: "map surfels"). */
typedef struct wc_map_surfel {
  int32_t key[3];   /* the voxel index                                                                          */
  uint32_t count;   /* its point count                                                                          */
  float xyz[3];     /* its centroid: the very float triple wc_map_export returns for it                         */
  uint32_t flags;   /* bit 0 "plane": count >= 3 and ev[2] > 0                                                  */
  double cov[6];    /* population covariance (xx, xy, xz, yy, yz, zz) of the quantised points, m^2              */
  double ev[3];     /* its eigenvalues, ascending                                                               */
  double normal[3]; /* unit eigenvector of ev[0]; its component of largest magnitude (lowest axis on a tie) > 0 */
} wc_map_surfel;

/* One voxel of the map's exact state (wildcat_hip.h: wc_map_export_state, wc_map_absorb; not a reference type).  40 bytes, 8-aligned;
 * the first 16 bytes are laid out as wc_map_surfel's.  The nine moment words of a WC_MAP_MOMENTS map travel in an array of their own. */
typedef struct wc_map_voxel {
  int32_t key[3];  /* the voxel index                                                                                       */
  uint32_t count;  /* its point count                                                                                       */
  int64_t sum[3];  /* the table's integer sums per axis: sum of round((p - r) * 2^32), r = the voxel's reference point      */
} wc_map_voxel;

/* Answer of wc_map_nearest_plane for one query (not a reference type).  80 bytes, 8-aligned. */
typedef struct wc_map_plane_hit {
  wc_map_hit hit;   /* what wc_map_nearest writes for the query; hit.flags bit 1 is added: "the plane below is valid"          */
  double normal[3]; /* the found voxel's wc_map_surfel.normal, byte for byte (0 without bit 1)                                */
  double sigma2;    /* its ev[0] (0 without bit 1)                                                                            */
  double dist;      /* signed distance of the query to the plane through the centroid: (nx ex + ny ey) + nz ez, e = q - xyz   */
} wc_map_plane_hit;

/* wc_map_linearize / wc_map_align (wildcat_hip.h: "registration against the map"; not reference types) */
typedef struct wc_map_reg_params { /* 32 bytes */
  double max_dist;     /* wc_map_nearest_plane's: > 0, may be +inf                                            */
  uint32_t min_points; /* wc_map_nearest_plane's: >= 3                                                        */
  uint32_t reserved;   /* 0, anything else WC_ERR_ARG                                                         */
  double sigma0;       /* > 0: w2 = 1 / (sigma0^2 + sigma2)  (wc_params.surfel_sigma0)                        */
  double cauchy_a;     /* > 0: Cauchy loss of scale a (the window's: wc_params.cauchy_a); 0: none             */
} wc_map_reg_params;

typedef struct wc_map_reg_row { /* 64 bytes: one point's share, optional output */
  double J[6]; /* d(dist) / d(omega, upsilon) for T <- Exp(xi) T: (Q x n, n); 0 if the point is unused */
  double d;    /* the plane hit's dist                                                                */
  double k;    /* w2 * rho'; 0 if the point is unused                                                 */
} wc_map_reg_row;

typedef struct wc_map_normal_eq { /* 240 bytes */
  double H[21];     /* upper triangle, row-major (00 01 .. 05 11 12 ..): sum (k J_a) J_b */
  double g[6];      /* sum (k J_a) d                                                     */
  double cost;      /* 0.5 * sum rho                                                     */
  uint64_t n_used;  /* points with a valid plane (flags bit 1)                           */
  uint64_t n_found; /* wc_map_nearest_plane's found count                                */
} wc_map_normal_eq;

typedef struct wc_map_align_opts { /* 64 bytes */
  wc_map_reg_params reg;
  uint32_t max_iterations; /* >= 1                                                                             */
  uint32_t min_used;       /* >= 6: fewer used points end the loop with termination 2                          */
  double tol_rot;          /* > 0 [rad]:  converged when |omega| <= tol_rot and ...                            */
  double tol_trans;        /* > 0 [m]:    ... |upsilon| <= tol_trans                                           */
  double min_pivot;        /* > 0: smallest accepted Cholesky pivot of H scaled to unit diagonal (a design
                              choice, wildcat_hip.h: wc_map_align; the Python binding's default is 1e-9)      */
} wc_map_align_opts;

typedef struct wc_map_align_summary { /* 88 bytes */
  double initial_cost;  /* cost at the T_io passed in                                                */
  double final_cost;    /* cost at the T_io returned                                                 */
  int32_t iterations;   /* pose updates applied                                                      */
  int32_t termination;  /* as wc_solve_summary: 0 = convergence, 1 = max_iterations, 2 = failure     */
  uint64_t n_used;      /* at the T_io returned                                                      */
  uint64_t n_found;
  double last_step[6];  /* the last update applied (omega, upsilon); 0 if none                       */
} wc_map_align_summary;

/* wc_map_linearize_ct / wc_map_align_ct (wildcat_hip.h: "registration of a stamped sweep in continuous time"; not reference types) */
typedef struct wc_map_ct_normal_eq { /* 640 bytes */
  double H00[21];     /* upper triangle, row-major: sum (kaa J_i) J_j, kaa = (k a) a; the begin pose's block           */
  double H01[21];     /* sum (kab J_i) J_j, kab = (k a) s: the block between the poses (symmetric as well)              */
  double H11[21];     /* sum (kbb J_i) J_j, kbb = (k s) s; the end pose's block                                        */
  double g0[6];       /* sum (ka J_i) d, ka = k a                                                                      */
  double g1[6];       /* sum (kb J_i) d, kb = k s                                                                      */
  double cost;        /* 0.5 * sum rho                                                                                 */
  uint64_t n_used;    /* points in span with a valid plane                                                             */
  uint64_t n_found;   /* points in span whose search found a voxel                                                     */
  uint64_t n_outside; /* points whose stamp is not in [t_begin, t_end] (a NaN stamp included)                          */
  uint64_t reserved;  /* written as 0                                                                                  */
} wc_map_ct_normal_eq;

typedef struct wc_map_ct_row { /* 72 bytes: one point's share, optional output; all zero for an unused point */
  double J[6]; /* wc_map_reg_row's J at the moved point                         */
  double d;    /* the plane hit's dist                                          */
  double k;    /* w2 * rho'                                                     */
  double s;    /* (t - t_begin) / span: the end pose's share, 1.0 - s the begin's */
} wc_map_ct_row;

typedef struct wc_map_ct_align_opts { /* 96 bytes */
  wc_map_reg_params reg;
  uint32_t max_iterations; /* >= 1                                                                             */
  uint32_t min_used;       /* >= 12: fewer used points end the loop with termination 2                         */
  double tol_rot;          /* > 0 [rad]: converged when both |omega| <= tol_rot and ...                        */
  double tol_trans;        /* > 0 [m]:   ... both |upsilon| <= tol_trans                                       */
  double min_pivot;        /* > 0: wc_map_align_opts' min_pivot, for the 12 x 12 matrix                        */
  double prior[4];         /* >= 0, finite: information weights holding the begin rotation [rad^-2], the begin
                              translation [m^-2], the end rotation and the end translation to their input
                              values (first order: wildcat_hip.h); 0: none                                     */
} wc_map_ct_align_opts;

typedef struct wc_map_ct_align_summary { /* 152 bytes */
  double initial_cost;  /* cost at the poses passed in (the points' share alone)                     */
  double final_cost;    /* cost at the poses returned (the points' share alone)                      */
  int32_t iterations;   /* pose updates applied                                                      */
  int32_t termination;  /* as wc_map_align_summary: 0 = convergence, 1 = max_iterations, 2 = failure */
  uint64_t n_used;      /* at the poses returned                                                     */
  uint64_t n_found;
  uint64_t n_outside;
  double last_step[12]; /* the last update applied (omega, upsilon of begin, then of end); 0 if none */
  double prior_cost;    /* 0.5 * sum w_i acc_i^2 at the poses returned, acc = the sum of the steps   */
} wc_map_ct_align_summary;

/* wc_map_score_batch (wildcat_hip.h: "occupancy score of pose hypotheses"; not reference types) */
typedef struct wc_map_score { /* 16 bytes: one hypothesis */
  uint32_t n_hit;    /* points whose own voxel is live in the map with count >= min_points              */
  uint32_t n_in;     /* points moved to a voxel inside the key range, |k| < 2^20 on every axis          */
  uint32_t n_bad;    /* finite points the pose sent to a non-finite one                                 */
  uint32_t reserved; /* written as 0                                                                    */
} wc_map_score;

typedef struct wc_map_score_params { /* 8 bytes */
  uint32_t min_points; /* >= 1: a voxel counts when it holds at least this many points */
  uint32_t reserved;   /* 0, anything else WC_ERR_ARG                                   */
} wc_map_score_params;

/* wc_map_carve (wildcat_hip.h): which rays of a call are used and what they select. */
typedef struct wc_map_carve_params { /* 32 bytes */
  double min_range;   /* [m] 0 <= min_range <= max_range: a ray is used iff min_range^2 <= |p - origin|^2 <= max_range^2   */
  double max_range;   /* [m] may be +inf                                                                            */
  uint32_t shell;     /* 0..8: Chebyshev radius, in voxels, around a ray's end voxel that the ray does not see through */
  uint32_t min_rays;  /* >= 1: a voxel is selected when at least this many rays of THIS call saw through it         */
  uint32_t max_steps; /* 1..65536: rays whose walk is longer are skipped and counted                                */
  uint32_t reserved;  /* 0                                                                                          */
} wc_map_carve_params;

typedef struct wc_map_carve_result { /* 40 bytes */
  uint64_t rays_used;      /* rays that were walked                                             */
  uint64_t rays_skipped;   /* every other point of the call                                     */
  uint64_t steps;          /* sum of the used rays' walk lengths M                              */
  uint64_t voxels_removed; /* occupied voxels selected (wc_map_carve_remove: and removed)       */
  uint64_t points_removed; /* ... and the points they hold                                      */
} wc_map_carve_result;

/* Answer of wc_map_raycast for one ray (wildcat_hip.h; not a reference type).  48 bytes, 8-aligned; the first 32 bytes are laid out as
 * wc_map_hit's. */
typedef struct wc_map_ray_hit {
  float xyz[3];    /* centroid of the hit voxel: the very float triple wc_map_export returns for it                     */
  uint32_t count;  /* its point count; 0 = no hit (then xyz = key = 0, step = 0, t = +inf)                             */
  int32_t key[3];  /* its voxel index                                                                                  */
  uint32_t flags;  /* bit 0: the ray was not cast (then tested = 0 too)                                                */
  double t;        /* parameter at which the ray enters the hit voxel: origin + t (p - origin); 0 at the origin's voxel */
  uint32_t step;   /* i: the hit voxel is k^(i) of the ray's walk                                                      */
  uint32_t tested; /* positions of the walk this ray tested, the hit included                                          */
} wc_map_ray_hit;

/* wc_map_raycast (wildcat_hip.h): which rays of a call are cast, which positions of a walk are tested, what counts as occupied. */
typedef struct wc_map_raycast_params { /* 32 bytes */
  double min_range;    /* [m] 0 <= min_range <= max_range: a ray is cast iff min_range^2 <= |p - origin|^2 <= max_range^2       */
  double max_range;    /* [m] may be +inf                                                                                  */
  uint32_t first_step; /* 0..65536: positions k^(i) with i < first_step are not tested                                     */
  uint32_t end_shell;  /* 0..9: positions nearer than this to the end voxel (Chebyshev, in voxels) are not tested; 0: none */
  uint32_t min_points; /* >= 1: a voxel with fewer points does not stop a ray                                              */
  uint32_t max_steps;  /* 1..65536: rays whose walk is longer are not cast and counted                                     */
} wc_map_raycast_params;

typedef struct wc_map_raycast_result { /* 32 bytes */
  uint64_t rays_cast;    /* rays that were walked                             */
  uint64_t rays_skipped; /* every other point of the call (flags bit 0)       */
  uint64_t hits;         /* rays with count != 0                              */
  uint64_t tested;       /* sum of the rays' `tested`                         */
} wc_map_raycast_result;

/* wc_map_components / wc_map_remove_small / wc_map_label_keys (wildcat_hip.h): which voxels are nodes and which of them are adjacent. */
#define WC_MAP_NO_COMPONENT 0xFFFFFFFFu /* label of an occupied voxel that is not a node */
#define WC_MAP_CC_DROP_SPARSE 1u        /* wc_map_remove_small: the occupied voxels that are not nodes are removed too */
typedef struct wc_map_cc_params { /* 16 bytes */
  uint32_t connectivity; /* 6, 18 or 26: the sum of |a - b| over the axes is at most 1, 2 or 3; anything else WC_ERR_ARG */
  uint32_t min_points;   /* >= 1: an occupied voxel is a node when it holds at least this many points                  */
  uint32_t flags;        /* 0 or WC_MAP_CC_DROP_SPARSE; any other bit WC_ERR_ARG                                       */
  uint32_t reserved;     /* 0, anything else WC_ERR_ARG                                                                */
} wc_map_cc_params;

/* One connected component (wildcat_hip.h: wc_map_components).  40 bytes, 8-aligned; integers only, so every field is independent of
 * order and schedule. */
typedef struct wc_map_component {
  uint32_t first;  /* export index of the root: the component's voxel of smallest (kx, ky, kz) */
  uint32_t voxels; /* nodes in the component                                                   */
  uint64_t points; /* ... and the points they hold                                             */
  int32_t kmin[3]; /* the key bounding box, per axis                                           */
  int32_t kmax[3];
} wc_map_component;

/* Communicator of a multi-GPU job: one process (and one wc_ctx) per GPU. The library calls these for its few collectives;
 * wc_comm_rccl_init() installs an in-library RCCL implementation, tests / other runtimes install callbacks.
 * All buffers are DEVICE pointers on the ctx's GPU; a callback returns 0 on success and must have completed (or be
 * stream-ordered on the ctx's stream) when it returns.  Byte counts are per rank, data consecutive in rank order. */
typedef struct wc_comm {
  void *user;
  int32_t rank, world;
  int (*allreduce_f64)(void *user, double *d_buf, uint64_t count); /* in-place sum over ranks */
  int (*alltoallv)(void *user, const void *d_send, const uint64_t *send_bytes, void *d_recv, const uint64_t *recv_bytes);
  int (*allgatherv)(void *user, const void *d_send, uint64_t send_bytes, void *d_recv, const uint64_t *recv_bytes);
  int32_t stream_ordered; /* 1: the callbacks enqueue on the ctx's stream themselves (the in-library RCCL binding): the library
                             does not synchronise around them.  0: the library drains its stream before every call and the
                             callback must have completed when it returns */
} wc_comm;

/* One sweep of a batched extraction (wc_extract_surfels_batch_*): the arguments of wc_extract_surfels_enqueue. */
typedef struct wc_sweep_job {
  wc_points pts;
  double t_lo, t_hi;   /* time range hint of THIS sweep (t_lo > t_hi: read back from the device) */
  wc_surfel *d_out;
  wc_surfel_id *d_ids; /* may be NULL */
  uint64_t cap;
} wc_sweep_job;

/* Hard-coded reference parameters of the path.  wc_params_default() fills the
 * reference values; tests may override them to reach edge cases. */
typedef struct wc_params {
  /* extraction: src/odometry/surfel_extraction.cc:327 */
  float voxel_size;          /* 0.8f  (float in the reference signature)               */
  int32_t max_layer;         /* 2                                                     */
  int32_t min_points;        /* node is tested when n > min_points (20)               */
  float planer_threshold;    /* 0.01f                                                 */
  double min_plane_likeness; /* 0.1                                                   */
  double view_point[3];      /* (0,0,0)                                               */
  double cluster_gap;        /* 0.05 s  (surfel_extraction.cc:24)                     */
  int32_t cluster_min_points;/* clusters with fewer points are dropped (20, cc:33)    */
  /* matcher: src/odometry/knn_surfel_matcher.h:37-41 */
  double center_scale;       /* 1.0                                                   */
  double angular_scale;      /* 5 deg in rad                                          */
  double surfel_dist_max;    /* 0.1                                                   */
  int32_t knn_k;             /* 10                                                    */
  double time_diff_min;      /* 0.06                                                  */
  /* factors / solver: src/odometry/lio_config.h:10-14,32-45, lidar_odometry.cc:270,551-560 */
  double surfel_sigma0;      /* 0.05 / 6 (cost_functor.h:24)                          */
  double cauchy_a;           /* 0.4                                                   */
  double w_gyr, w_acc, w_bg, w_ba; /* IMU cost weights                                */
  double imu_dt;             /* 1 / imu_rate = 0.005                                  */
  int32_t max_iterations;    /* 100                                                   */
  int32_t reference_quirks;  /* 1: reproduce Q1 (Jacobian overwrite) and Q3           */
  /* extraction arithmetic (not a reference parameter).  0 (default): order-independent integer moments - counts / ids exact,
   * geometry ~1e-9, surfel time stamp = the correctly rounded mean, sweeps with a gate inside the reference's own rounding
   * noise are repeated on the exact path.  1: every sum formed in the reference's order (bit-identical to the CPU path,
   * including the output order among surfels whose stamps differ by less than the running sum's rounding). */
  int32_t exact_sums;
} wc_params;

/* Solver summary (subset of ceres::Solver::Summary the reference logs, lidar_odometry.cc:562). */
typedef struct wc_solve_summary {
  double initial_cost;
  double final_cost;
  int32_t iterations;            /* LM iterations performed (iteration 0 excluded)   */
  int32_t successful_steps;
  int32_t unsuccessful_steps;
  int32_t termination;           /* 0 = convergence, 1 = no convergence (max iters), 2 = failure */
  int32_t n_linearizations;
  int32_t n_cost_evaluations;
  double first_step[16];         /* [0] first_step_norm; [1] steps re-formed by the dense factorisation (a rejected or
                                  * invalid step of the bias elimination, wildcat_hip.h: wc_window_solve); rest unused */
} wc_solve_summary;

#ifdef __cplusplus
}
#endif
#endif /* WC_TYPES_H_ */
