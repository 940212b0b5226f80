"""The voxel map's coarser levels without a GPU (include/wildcat_hip.h: wc_map_coarsen, wc_map_align_pyramid): the re-basing
of map_coarsen_ref.py against a direct insert at the coarse size - dyadic voxel sizes with points on the faces, other sizes on random
clouds, the documented limit pinned with points placed on the faces -, its composition, the declared interface, and the basin of the
coarse-to-fine registration against the fine map alone, with map_register_ref's float64 loop."""
import ctypes as C
import os

import numpy as np
import pytest

import map_coarsen_ref as MC
import map_register_ref as G
import map_state_ref as MS
from helpers import xyz_of
from test_map_register_ref import P, scan_of
from wildcat_slam_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
V_F = float(np.float32(0.8)) / 4


def same_state(a, b):
    return a[0].tobytes() == b[0].tobytes() and ((a[1] is None and b[1] is None) or a[1].tobytes() == b[1].tobytes())


def check_against_direct_insert(xyz, v, factor):
    """coarsen_ref(state_of(xyz, v)) == state_of(xyz, (double)factor v) byte for byte, with moments and plain"""
    V = MC.coarse_voxel(v, factor)
    vox, mom = MS.state_of(xyz, v)
    want = MS.state_of(xyz, V)
    assert same_state(MC.coarsen_ref(vox, mom, v, factor), want)
    got, none = MC.coarsen_ref(vox, None, v, factor)
    assert none is None and got.tobytes() == want[0].tobytes()
    assert int(got["count"].sum()) == len(xyz) and len(got) < len(vox)


@pytest.mark.parametrize("v,factor", [(0.25, 2), (0.25, 3), (0.125, 4)])
def test_dyadic_voxel_equals_direct_insert_with_points_on_faces(v, factor):
    xyz = MC.face_cloud(4000, v, factor, seed=17 + factor)
    V = MC.coarse_voxel(v, factor)
    # the cloud does what it is for: points exactly on fine faces, on coarse faces, and negative coordinates
    p = xyz.astype(np.float64)
    assert np.any(p / v == np.rint(p / v), axis=1).sum() > 1000 and np.any(p / V == np.rint(p / V), axis=1).sum() > 500 and (p < 0).any()
    assert not MC.disagree(xyz, v, factor).any()
    check_against_direct_insert(xyz, v, factor)


@pytest.mark.parametrize("v,factor", [(0.1, 2), (0.1, 3), (0.2, 5), (V_F, 4), (0.05, 16)])
def test_other_voxel_sizes_equal_direct_insert_on_a_random_cloud(v, factor):
    xyz = np.random.default_rng(int(v * 1000) + factor).uniform(-6.0, 6.0, (17_000, 3)).astype(np.float32)
    assert MC.disagree(xyz, v, factor).sum() == 0  # (a condition of the equality, not a theorem: it held for these clouds)
    check_against_direct_insert(xyz, v, factor)


def test_points_on_faces_of_a_non_dyadic_grid_pin_the_limit():
    """v = 0.1, factor 3: a point on a face of the coarse grid to within rounding may go to the other side in one of the two divisions;
    such points exist, they are counted in the neighbouring coarse voxel, and without them the equality holds"""
    v, factor = 0.1, 3
    xyz = MC.face_cloud(3000, v, factor, seed=5, share=1.0)
    bad = MC.disagree(xyz, v, factor)
    print("v = 0.1, factor 3: points on faces that disagree:", int(bad.sum()), "of", len(xyz))
    assert 0 < bad.sum() < len(xyz)
    vox, mom = MS.state_of(xyz, v)
    got = MC.coarsen_ref(vox, mom, v, factor)
    assert not same_state(got, MS.state_of(xyz, MC.coarse_voxel(v, factor)))
    assert int(got[0]["count"].sum()) == len(xyz)  # (nothing is lost: the points are counted next door)
    check_against_direct_insert(xyz[~bad], v, factor)
    # ... while the same construction on v = 0.1, factor 2 and v = 0.2, factor 5 disagrees nowhere
    for v2, f2 in ((0.1, 2), (0.2, 5)):
        assert not MC.disagree(MC.face_cloud(3000, v2, f2, seed=5, share=1.0), v2, f2).any()


@pytest.mark.parametrize("v,a,b", [(0.25, 2, 3), (0.25, 3, 2), (0.25, 4, 4), (0.1, 2, 2), (V_F, 2, 2)])
def test_composition(v, a, b):
    """two levels in a row are the level of the product wherever the voxel sizes are bitwise equal: a dyadic v, or a = b = 2"""
    assert MC.coarse_voxel(MC.coarse_voxel(v, a), b) == MC.coarse_voxel(v, a * b)
    xyz = MC.face_cloud(3000, v, a, seed=a * 10 + b)
    vox, mom = MS.state_of(xyz, v)
    mid = MC.coarsen_ref(vox, mom, v, a)
    assert same_state(MC.coarsen_ref(mid[0], mid[1], MC.coarse_voxel(v, a), b), MC.coarsen_ref(vox, mom, v, a * b))


def test_factor_one_is_a_copy_and_negative_keys_round_down():
    xyz = MC.face_cloud(500, 0.25, 2, seed=1)
    vox, mom = MS.state_of(xyz, 0.25)
    assert same_state(MC.coarsen_ref(vox, mom, 0.25, 1), (vox, mom))
    K, D = MC.shifts(np.array([[-1, -3, -4], [0, 2, 3], [-7, 5, -6]]), 0.25, 3)
    assert K.tolist() == [[-1, -1, -2], [0, 0, 1], [-3, 1, -2]]
    # r(k, 0.25) = (k + 0.5) / 4 and r(K, 0.75) = (K + 0.5) 0.75 exactly: D = (k - 3 K - 1) 2^30
    assert D == [[(k - 3 * kk - 1) * 2**30 for k, kk in zip(row, Krow)] for row, Krow in zip([[-1, -3, -4], [0, 2, 3], [-7, 5, -6]], K.tolist())]


def test_header_and_library_declare_the_calls():
    from wildcat_slam_amd import lib

    declared, l = set(lib.declared_symbols()), lib.load()
    for s in ("wc_map_coarsen", "wc_map_align_pyramid"):
        assert s in declared and hasattr(l, s), s
    host = C.CDLL(os.path.join(HERE, "..", "wildcat-slam_amd", "host", "libwildcat_odometry.so"))
    assert hasattr(host, "wc_odom_map_relocalize")


def test_basin_pyramid_recovers_where_the_fine_map_is_lost():
    """DESIGN 8.9's experiment with the float64 restatement: the fine map alone (v = 0.2, 27 voxels around a point) ends lost, the levels
    1.6 -> 0.8 -> 0.4 -> 0.2, each from the pose of the one before, end within the bounds test_map_register_ref holds its recovery to.
    The finest level may run out its iterations (the IRLS behaviour of DESIGN 8.3): the pose errors are what is asserted"""
    T = MC.basin_pose()
    room = xyz_of(synth.g1_room(MC.BASIN_ROOM))
    scan = scan_of(MC.BASIN_SCAN, T)
    sizes = MC.basin_sizes()
    assert sizes == [0.2, 0.4, 0.8, 1.6]
    surf = {v: G.surfels_cpu(room, v) for v in sizes}
    T_fine, s_fine = MC.basin_ref(surf.get, scan, P, sizes[:1])
    T_pyr, s_pyr = MC.basin_ref(surf.get, scan, P, sizes[::-1])
    e_fine, e_pyr = G.pose_error(T_fine, T), G.pose_error(T_pyr, T)
    print("fine only: error", e_fine, "iterations", s_fine[0]["iterations"], "termination", s_fine[0]["termination"])
    print("pyramid: error", e_pyr, "iterations", [s["iterations"] for s in s_pyr], "termination", [s["termination"] for s in s_pyr])
    assert e_pyr[0] < np.deg2rad(0.1) and e_pyr[1] < 0.01  # (test_restated_alignment_recovers_the_pose's bounds)
    assert e_fine[0] > 10 * e_pyr[0] and e_fine[1] > 10 * e_pyr[1]
