"""Nearest-voxel queries and box cropping of the voxel map (include/wildcat_hip.h: wc_map_nearest, wc_map_crop) - the parts that need
no GPU: the entry points and the facade's wrappers are exported, argument checks, and the numpy restatements of map_query_ref.py
against a brute force over every centroid and on a hand-worked case."""
import ctypes as C
import os

import numpy as np
import pytest

import map_query_ref as Q
from helpers import xyz_of as _xyz
from test_map_cpu import downsample_voxel
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
WC_ERR_ARG = 11


def test_header_declares_and_library_exports_the_query_entry_points():
    from wildcat_slam_amd import lib

    declared = set(lib.declared_symbols())
    l = lib.load()
    for s in ("wc_map_nearest", "wc_map_crop"):
        assert s in declared, s
        assert hasattr(l, s), s


def test_odometry_library_exports_the_query_wrappers():
    from wildcat_slam_amd import lib

    lib.load()
    host = C.CDLL(os.path.join(HERE, "..", "wildcat-slam_amd", "host", "libwildcat_odometry.so"))
    for s in ("wc_odom_map_query", "wc_odom_map_crop", "wc_odom_set_map_keep_radius"):
        assert hasattr(host, s), s


def test_map_hit_record_matches_the_header():
    assert R.MAP_HIT.itemsize == 40
    assert [R.MAP_HIT.fields[f][1] for f in ("xyz", "count", "key", "flags", "d2")] == [0, 12, 16, 28, 32]
    txt = open(os.path.join(HERE, "..", "include", "wc_types.h")).read()
    body = txt[txt.index("typedef struct wc_map_hit") : txt.index("} wc_map_hit;")]
    order = [body.index(f) for f in ("float xyz[3]", "uint32_t count", "int32_t key[3]", "uint32_t flags", "double d2")]
    assert order == sorted(order)


def test_query_and_crop_refuse_bad_arguments():
    from wildcat_slam_amd import lib

    l = lib.load()
    desc = R.Points(0, 0, 12, 0, 0)
    n = C.c_uint64(0)
    lo, hi = (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(1, 1, 1)
    # NULL context or map
    assert l.wc_map_nearest(None, None, C.byref(desc), C.c_double(1.0), None, C.byref(n)) == WC_ERR_ARG
    assert l.wc_map_crop(None, None, lo, hi, C.byref(n)) == WC_ERR_ARG
    for d in (0.0, -1.0, float("nan")):
        assert l.wc_map_nearest(None, None, C.byref(desc), C.c_double(d), None, None) == WC_ERR_ARG, d
    bad_lo = (C.c_double * 3)(0, 2, 0)  # lo > hi
    assert l.wc_map_crop(None, None, bad_lo, hi, None) == WC_ERR_ARG
    nan_hi = (C.c_double * 3)(1, float("nan"), 1)
    assert l.wc_map_crop(None, None, lo, nan_hi, None) == WC_ERR_ARG


@pytest.fixture(scope="module")
def clouds():
    lat, _ = synth.g2_lattice(60, m=32)
    return dict(g1_room=_xyz(synth.g1_room(60_000)), g2_lattice=_xyz(lat))


@pytest.mark.parametrize("name", ["g1_room", "g2_lattice"])
def test_restatement_is_the_global_nearest_up_to_one_voxel(clouds, name):
    """for max_dist <= v the nearest of the 27 voxels is the nearest of ALL centroids within max_dist: idx and d2 identical for every
    query (queries: map points + N(0, (v / 2)^2) jitter)"""
    pts = clouds[name]
    rng = np.random.Generator(np.random.PCG64(11))
    for v in (0.05, 0.2, float(np.float32(0.8))):
        keys, cen, cnt, rej = downsample_voxel(pts, v)
        assert rej == 0
        q = (pts[rng.integers(0, len(pts), 2000)] + rng.normal(size=(2000, 3)) * (v / 2)).astype(np.float32)
        for max_dist in (v / 2, v):
            hits, idx = Q.nearest_voxel(keys, cen, cnt, q, v, max_dist)
            ref_idx, ref_d2 = Q.brute_force(cen, q, max_dist)
            assert np.array_equal(idx, ref_idx), (name, v, max_dist, int((idx != ref_idx).sum()))
            assert hits["d2"].tobytes() == ref_d2.tobytes(), (name, v, max_dist)
            assert 0 < (idx >= 0).sum() < len(q), "both hits and misses are exercised"
            assert np.array_equal(hits["count"][idx >= 0], cnt[idx[idx >= 0]]) and not hits["flags"].any()


def test_query_restatement_on_a_hand_worked_case():
    """v = 0.5, dyadic coordinates: a tie (the smaller key wins), queries on voxel faces, an empty own voxel with an occupied
    neighbour, d2 == max_dist^2 (accepted) and one ulp less (missed), a miss at max_dist = inf, NaN / inf / out-of-range queries"""
    keys, cen, cnt, rej = downsample_voxel(Q.HAND_POINTS, Q.HAND_V)
    assert rej == 0 and keys.tolist() == Q.HAND_KEYS and cnt.tolist() == Q.HAND_COUNTS
    assert np.array_equal(cen, np.array(Q.HAND_CENTROIDS, np.float32))
    for max_dist in Q.HAND_EXPECT:
        hits, idx = Q.nearest_voxel(keys, cen, cnt, Q.HAND_QUERIES, Q.HAND_V, max_dist)
        want, want_idx = Q.hand_expected_hits(max_dist)
        assert np.array_equal(idx, want_idx), max_dist
        assert hits.tobytes() == want.tobytes(), max_dist
    # an empty map: every searchable query misses
    hits, idx = Q.nearest_voxel(np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), Q.HAND_QUERIES, 0.5, np.inf)
    assert not hits["count"].any() and np.all(idx == -1) and hits["flags"].tolist() == Q.HAND_FLAGS and np.all(np.isinf(hits["d2"]))


def test_crop_keep_on_a_hand_worked_case():
    """boxes whose faces lie exactly on voxel faces, negative coordinates, infinite bounds; keys: D (-1, -1, -1), A (0, 0, 0),
    B (1, 0, 0), C (3, 0, 0)"""
    inf = np.inf
    keys = np.array(Q.HAND_KEYS, np.int32)
    cases = [
        ((0, 0, 0), (0.5, 0.5, 0.5), [0, 1, 1, 0]),  # hi on the face x = 0.5: voxel 1 intersects the box (floor(0.5 / 0.5) = 1)
        ((0, 0, 0), (0.499, 0.499, 0.499), [0, 1, 0, 0]),
        ((-0.5, -0.5, -0.5), (-0.25, -0.25, -0.25), [1, 0, 0, 0]),  # lo on the face -0.5: voxel -1
        ((-0.5, -0.5, -0.5), (0.0, 0.0, 0.0), [1, 1, 0, 0]),  # hi = 0 touches voxel 0
        ((-inf, -inf, -inf), (0.49, 0.49, 0.49), [1, 1, 0, 0]),
        ((1.5, 0, 0), (inf, inf, inf), [0, 0, 0, 1]),
        ((0.5, -inf, -inf), (1.0, inf, inf), [0, 0, 1, 0]),  # kx in [1, 2]
        ((-inf, -inf, -inf), (inf, inf, inf), [1, 1, 1, 1]),
        ((10, 10, 10), (11, 11, 11), [0, 0, 0, 0]),
    ]
    for lo, hi, want in cases:
        assert Q.crop_keep(keys, 0.5, lo, hi).tolist() == [bool(w) for w in want], (lo, hi)
    assert Q.pow2_at_least(0) == 1 and Q.pow2_at_least(2) == 2 and Q.pow2_at_least(3) == 4 and Q.pow2_at_least(1025) == 2048
