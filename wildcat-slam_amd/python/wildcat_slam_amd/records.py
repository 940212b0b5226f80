"""numpy / ctypes mirrors of the C-ABI records in include/wc_types.h.

Every dtype here is byte-compatible with the C struct of the same name, so a numpy array can be handed to
the C-ABI (or copied to HBM) without conversion.
"""
import ctypes as C

import numpy as np

# reference hilti_ros::Point (src/common/common.h:12-28): 48-byte AoS record
POINT = np.dtype(
    {
        "names": ["x", "y", "z", "intensity", "time", "ring"],
        "formats": ["f4", "f4", "f4", "f4", "f8", "u2"],
        "offsets": [0, 4, 8, 16, 24, 32],
        "itemsize": 48,
    }
)
SURFEL = np.dtype(
    [("t", "f8"), ("center", "f8", 3), ("cov", "f8", 9), ("normal", "f8", 3), ("resolution", "f8"), ("sigma", "f8")]
)
SURFEL_ID = np.dtype([("kx", "i4"), ("ky", "i4"), ("kz", "i4"), ("node", "u4")])
POSE = np.dtype([("pos", "f8", 3), ("quat", "f8", 4)])
IMU_STATE = np.dtype([("t", "f8"), ("pos", "f8", 3), ("quat", "f8", 4), ("acc", "f8", 3), ("gyr", "f8", 3)])
PAIR = np.dtype([("first", "i4"), ("second", "i4")])

ROUTE_POINT = np.dtype([("x", "f4"), ("y", "f4"), ("z", "f4"), ("src", "u4"), ("t", "f8")])  # wc_route_point
assert ROUTE_POINT.itemsize == 24

MAP_HIT = np.dtype([("xyz", "f4", 3), ("count", "u4"), ("key", "i4", 3), ("flags", "u4"), ("d2", "f8")])  # wc_map_hit
assert MAP_HIT.itemsize == 40 and MAP_HIT.fields["d2"][1] == 32
MAP_MOMENTS = 1  # WC_MAP_MOMENTS
MAP_SURFEL = np.dtype(
    [("key", "i4", 3), ("count", "u4"), ("xyz", "f4", 3), ("flags", "u4"), ("cov", "f8", 6), ("ev", "f8", 3), ("normal", "f8", 3)]
)  # wc_map_surfel
assert MAP_SURFEL.itemsize == 128 and [MAP_SURFEL.fields[f][1] for f in ("count", "xyz", "flags", "cov", "ev", "normal")] == [12, 16, 28, 32, 80, 104]
# wc_map_voxel: one voxel of the map's exact state (the first 16 bytes as MAP_SURFEL's); the nine moment words travel as an (n, 9) int64 array
MAP_VOXEL = np.dtype([("key", "i4", 3), ("count", "u4"), ("sum", "i8", 3)])
assert MAP_VOXEL.itemsize == 40 and [MAP_VOXEL.fields[f][1] for f in ("key", "count", "sum")] == [0, 12, 16]
# wc_map_plane_hit: the fields of MAP_HIT (flags: bit 1 = the plane is valid), then the plane
MAP_PLANE_HIT = np.dtype(MAP_HIT.descr + [("normal", "f8", 3), ("sigma2", "f8"), ("dist", "f8")])
assert MAP_PLANE_HIT.itemsize == 80 and [MAP_PLANE_HIT.fields[f][1] for f in ("flags", "d2", "normal", "sigma2", "dist")] == [28, 32, 40, 64, 72]

# wc_map_linearize / wc_map_align: one point's row, the 240-byte normal equations
MAP_REG_ROW = np.dtype([("J", "f8", 6), ("d", "f8"), ("k", "f8")])  # wc_map_reg_row
MAP_NORMAL_EQ = np.dtype([("H", "f8", 21), ("g", "f8", 6), ("cost", "f8"), ("n_used", "u8"), ("n_found", "u8")])  # wc_map_normal_eq
assert MAP_REG_ROW.itemsize == 64 and MAP_NORMAL_EQ.itemsize == 240 and MAP_NORMAL_EQ.fields["cost"][1] == 216

# wc_map_linearize_ct / wc_map_align_ct: one point's row (J, d, k and the end pose's share s), the 640-byte normal equations of two poses
MAP_CT_ROW = np.dtype([("J", "f8", 6), ("d", "f8"), ("k", "f8"), ("s", "f8")])  # wc_map_ct_row
MAP_CT_NORMAL_EQ = np.dtype([("H00", "f8", 21), ("H01", "f8", 21), ("H11", "f8", 21), ("g0", "f8", 6), ("g1", "f8", 6), ("cost", "f8"),
                             ("n_used", "u8"), ("n_found", "u8"), ("n_outside", "u8"), ("reserved", "u8")])  # wc_map_ct_normal_eq
assert MAP_CT_ROW.itemsize == 72 and MAP_CT_NORMAL_EQ.itemsize == 640 and MAP_CT_NORMAL_EQ.fields["cost"][1] == 600

# wc_map_score: one pose hypothesis's counts (wc_map_score_batch)
MAP_SCORE = np.dtype([("n_hit", "u4"), ("n_in", "u4"), ("n_bad", "u4"), ("reserved", "u4")])
assert MAP_SCORE.itemsize == 16

# wc_map_ray_hit: the first 32 bytes as MAP_HIT's (flags: bit 0 = the ray was not cast), then the entering parameter and the walk's counts
MAP_RAY_HIT = np.dtype([("xyz", "f4", 3), ("count", "u4"), ("key", "i4", 3), ("flags", "u4"), ("t", "f8"), ("step", "u4"), ("tested", "u4")])
assert MAP_RAY_HIT.itemsize == 48 and [MAP_RAY_HIT.fields[f][1] for f in ("count", "key", "flags", "t", "step", "tested")] == [12, 16, 28, 32, 40, 44]

# wc_map_component: one connected component of the occupied voxels (wc_map_components, wc_map_label_keys)
MAP_COMPONENT = np.dtype([("first", "u4"), ("voxels", "u4"), ("points", "u8"), ("kmin", "i4", 3), ("kmax", "i4", 3)])
assert MAP_COMPONENT.itemsize == 40 and [MAP_COMPONENT.fields[f][1] for f in ("voxels", "points", "kmin", "kmax")] == [4, 8, 16, 28]
MAP_NO_COMPONENT = 0xFFFFFFFF  # WC_MAP_NO_COMPONENT
MAP_CC_DROP_SPARSE = 1  # WC_MAP_CC_DROP_SPARSE

assert SURFEL.itemsize == 144 and POSE.itemsize == 56 and IMU_STATE.itemsize == 112 and PAIR.itemsize == 8
assert SURFEL_ID.itemsize == 16 and POINT.itemsize == 48


class Points(C.Structure):
    """wc_points descriptor."""

    _fields_ = [
        ("xyz", C.c_void_p),
        ("time", C.c_void_p),
        ("xyz_stride", C.c_uint32),
        ("time_stride", C.c_uint32),
        ("n", C.c_uint64),
    ]


class Params(C.Structure):
    """wc_params."""

    _fields_ = [
        ("voxel_size", C.c_float),
        ("max_layer", C.c_int32),
        ("min_points", C.c_int32),
        ("planer_threshold", C.c_float),
        ("min_plane_likeness", C.c_double),
        ("view_point", C.c_double * 3),
        ("cluster_gap", C.c_double),
        ("cluster_min_points", C.c_int32),
        ("center_scale", C.c_double),
        ("angular_scale", C.c_double),
        ("surfel_dist_max", C.c_double),
        ("knn_k", C.c_int32),
        ("time_diff_min", C.c_double),
        ("surfel_sigma0", C.c_double),
        ("cauchy_a", C.c_double),
        ("w_gyr", C.c_double),
        ("w_acc", C.c_double),
        ("w_bg", C.c_double),
        ("w_ba", C.c_double),
        ("imu_dt", C.c_double),
        ("max_iterations", C.c_int32),
        ("reference_quirks", C.c_int32),
        ("exact_sums", C.c_int32),
    ]


class OdomConfig(C.Structure):
    """wc_odom_config (host/lio_config.h): LioConfig's reference fields; the oracle's wco_odom_config has the same layout."""

    _fields_ = [
        ("gyroscope_noise_density", C.c_double),
        ("accelerometer_noise_density", C.c_double),
        ("gyroscope_random_walk", C.c_double),
        ("accelerometer_random_walk", C.c_double),
        ("imu_factor_weight", C.c_double),
        ("max_range", C.c_double),
        ("min_range", C.c_double),
        ("blind_min", C.c_double * 3),
        ("blind_max", C.c_double * 3),
        ("ext_translation", C.c_double * 3),
        ("ext_rotation", C.c_double * 9),
        ("imu_rate", C.c_double),
        ("sample_dt", C.c_double),
        ("fixed_window_duration", C.c_double),
        ("sliding_window_duration", C.c_double),
        ("sweep_duration", C.c_double),
        ("gravity_norm", C.c_double),
        ("outer_iter_num_max", C.c_int32),
        ("inner_iter_num_max", C.c_int32),
    ]

    def to_dict(self):
        return dict((k, list(getattr(self, k)) if hasattr(getattr(self, k), "__len__") else getattr(self, k)) for k, _ in self._fields_)

    def update(self, **fields):
        """set the named fields (arrays from any sequence of the right length); an unknown name is a TypeError"""
        known = dict(self._fields_)
        for k, v in fields.items():
            if k not in known:
                raise TypeError("no configuration field %r" % k)
            if hasattr(getattr(self, k), "__len__"):
                v = [float(a) for a in np.asarray(v, np.float64).reshape(-1)]
                assert len(v) == len(getattr(self, k)), k
                setattr(self, k, known[k](*v))
            else:
                setattr(self, k, v)
        return self


COMM_ALLREDUCE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64)
COMM_ALLTOALLV = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint64))
COMM_ALLGATHERV = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64))


class Comm(C.Structure):
    """wc_comm."""

    _fields_ = [
        ("user", C.c_void_p),
        ("rank", C.c_int32),
        ("world", C.c_int32),
        ("allreduce_f64", COMM_ALLREDUCE),
        ("alltoallv", COMM_ALLTOALLV),
        ("allgatherv", COMM_ALLGATHERV),
        ("stream_ordered", C.c_int32),
    ]


class SolveSummary(C.Structure):
    """wc_solve_summary."""

    _fields_ = [
        ("initial_cost", C.c_double),
        ("final_cost", C.c_double),
        ("iterations", C.c_int32),
        ("successful_steps", C.c_int32),
        ("unsuccessful_steps", C.c_int32),
        ("termination", C.c_int32),
        ("n_linearizations", C.c_int32),
        ("n_cost_evaluations", C.c_int32),
        ("first_step", C.c_double * 16),
    ]


def points_from_aos(arr, base_ptr=None):
    """Descriptor for a POINT-dtype array (host array unless base_ptr, a device address, is given)."""
    assert arr.dtype == POINT
    base = arr.ctypes.data if base_ptr is None else base_ptr
    return Points(base, base + 24, 48, 48, len(arr))


class SweepJob(C.Structure):
    """wc_sweep_job (include/wc_types.h): one sweep of wc_extract_surfels_batch_*"""

    _fields_ = [("pts", Points), ("t_lo", C.c_double), ("t_hi", C.c_double), ("d_out", C.c_void_p), ("d_ids", C.c_void_p), ("cap", C.c_uint64)]


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class MapRegParams(C.Structure):
    """wc_map_reg_params"""

    _fields_ = [("max_dist", C.c_double), ("min_points", C.c_uint32), ("reserved", C.c_uint32), ("sigma0", C.c_double), ("cauchy_a", C.c_double)]


class MapScoreParams(C.Structure):
    """wc_map_score_params"""

    _fields_ = [("min_points", C.c_uint32), ("reserved", C.c_uint32)]


class MapCcParams(C.Structure):
    """wc_map_cc_params"""

    _fields_ = [("connectivity", C.c_uint32), ("min_points", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class MapAlignOpts(C.Structure):
    """wc_map_align_opts"""

    _fields_ = [
        ("reg", MapRegParams),
        ("max_iterations", C.c_uint32),
        ("min_used", C.c_uint32),
        ("tol_rot", C.c_double),
        ("tol_trans", C.c_double),
        ("min_pivot", C.c_double),
    ]


class MapAlignSummary(C.Structure):
    """wc_map_align_summary"""

    _fields_ = [
        ("initial_cost", C.c_double),
        ("final_cost", C.c_double),
        ("iterations", C.c_int32),
        ("termination", C.c_int32),
        ("n_used", C.c_uint64),
        ("n_found", C.c_uint64),
        ("last_step", C.c_double * 6),
    ]


class Pose(C.Structure):
    """wc_pose: pos, quat = (w, x, y, z)"""

    _fields_ = [("pos", C.c_double * 3), ("quat", C.c_double * 4)]


class MapCtAlignOpts(C.Structure):
    """wc_map_ct_align_opts"""

    _fields_ = [
        ("reg", MapRegParams),
        ("max_iterations", C.c_uint32),
        ("min_used", C.c_uint32),
        ("tol_rot", C.c_double),
        ("tol_trans", C.c_double),
        ("min_pivot", C.c_double),
        ("prior", C.c_double * 4),
    ]


class MapCtAlignSummary(C.Structure):
    """wc_map_ct_align_summary"""

    _fields_ = [
        ("initial_cost", C.c_double),
        ("final_cost", C.c_double),
        ("iterations", C.c_int32),
        ("termination", C.c_int32),
        ("n_used", C.c_uint64),
        ("n_found", C.c_uint64),
        ("n_outside", C.c_uint64),
        ("last_step", C.c_double * 12),
        ("prior_cost", C.c_double),
    ]


assert C.sizeof(Pose) == 56 and C.sizeof(MapCtAlignOpts) == 96 and C.sizeof(MapCtAlignSummary) == 152


class MapCarveParams(C.Structure):
    """wc_map_carve_params"""

    _fields_ = [
        ("min_range", C.c_double),
        ("max_range", C.c_double),
        ("shell", C.c_uint32),
        ("min_rays", C.c_uint32),
        ("max_steps", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class MapCarveResult(C.Structure):
    """wc_map_carve_result"""

    _fields_ = [
        ("rays_used", C.c_uint64),
        ("rays_skipped", C.c_uint64),
        ("steps", C.c_uint64),
        ("voxels_removed", C.c_uint64),
        ("points_removed", C.c_uint64),
    ]


class MapRaycastParams(C.Structure):
    """wc_map_raycast_params"""

    _fields_ = [
        ("min_range", C.c_double),
        ("max_range", C.c_double),
        ("first_step", C.c_uint32),
        ("end_shell", C.c_uint32),
        ("min_points", C.c_uint32),
        ("max_steps", C.c_uint32),
    ]


class MapRaycastResult(C.Structure):
    """wc_map_raycast_result"""

    _fields_ = [
        ("rays_cast", C.c_uint64),
        ("rays_skipped", C.c_uint64),
        ("hits", C.c_uint64),
        ("tested", C.c_uint64),
    ]


MAP_KNN_NOT_OWN = 1  # WC_MAP_KNN_NOT_OWN


class MapKnnParams(C.Structure):
    """wc_map_knn_params"""

    _fields_ = [("max_dist", C.c_double), ("k", C.c_uint32), ("reach", C.c_uint32), ("min_points", C.c_uint32), ("flags", C.c_uint32)]


assert C.sizeof(MapKnnParams) == 24
assert C.sizeof(MapCarveParams) == 32 and C.sizeof(MapCarveResult) == 40
assert C.sizeof(MapRaycastParams) == 32 and C.sizeof(MapRaycastResult) == 32
assert C.sizeof(MapRegParams) == 32 and C.sizeof(MapAlignOpts) == 64 and C.sizeof(MapAlignSummary) == 88
