"""The numpy restatement of wc_map_knn (tests/map_knn_ref.py) against itself: it is wc_map_nearest's restatement at k = 1, reach = 1; it is
the brute-force answer for max_dist <= reach * v; ties go by key; max_dist is inclusive.  And the libraries export the entry points.
No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import map_knn_ref as K
import map_query_ref as Q
from wildcat_slam_amd import lib
from wildcat_slam_amd import records as R

HERE = os.path.dirname(os.path.abspath(__file__))
P = K.Params


def test_the_libraries_export_the_entry_points():
    declared = lib.declared_symbols()
    assert "wc_map_knn" in declared and hasattr(lib.load(), "wc_map_knn")
    host = C.CDLL(os.path.join(HERE, "..", "wildcat-slam_amd", "host", "libwildcat_odometry.so"))
    assert hasattr(host, "wc_odom_map_query_knn")
    assert C.sizeof(R.MapKnnParams) == 24 and R.MAP_KNN_NOT_OWN == 1
    assert hasattr(lib.PointMap, "knn") and hasattr(lib.Odometry, "map_query_knn")


def _random_map(seed, v=0.2, n=4000):
    rng = np.random.Generator(np.random.PCG64(seed))
    pts = (rng.random((n, 3)) * [3.0, 2.0, 1.0] - 0.7).astype(np.float32)
    kf = np.floor(pts.astype(np.float64) / v).astype(np.int64)
    uk, inv = np.unique(kf, axis=0, return_inverse=True)  # (rows sorted lexicographically: the export order)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv).astype(np.uint32)
    cen = np.stack([np.bincount(inv, pts[:, a].astype(np.float64)) for a in range(3)], -1) / cnt[:, None]
    q = np.concatenate([pts[::5] + rng.normal(size=(len(pts[::5]), 3)).astype(np.float32) * np.float32(v / 2), Q.HAND_QUERIES])
    return uk.astype(np.int32), cen.astype(np.float32), cnt, q.astype(np.float32)


@pytest.mark.parametrize("max_dist", list(Q.HAND_EXPECT))
def test_k1_reach1_is_nearest_voxel_on_the_hand_worked_case(max_dist):
    want, idx = Q.hand_expected_hits(max_dist)
    hits, within = K.knn_voxels(Q.HAND_KEYS, Q.HAND_CENTROIDS, Q.HAND_COUNTS, Q.HAND_QUERIES, Q.HAND_V, P(max_dist, 1, 1, 1, False))
    assert hits.shape == (len(want), 1) and hits[:, 0].tobytes() == want.tobytes()
    assert np.array_equal(within > 0, idx >= 0)


@pytest.mark.parametrize("max_dist", [0.1, 0.2, np.inf])
def test_k1_reach1_is_nearest_voxel_on_a_random_map(max_dist):
    keys, cen, cnt, q = _random_map(3)
    want, idx = Q.nearest_voxel(keys, cen, cnt, q, 0.2, max_dist)
    hits, within = K.knn_voxels(keys, cen, cnt, q, 0.2, P(max_dist, 1, 1, 1, False))
    assert 0 < (idx >= 0).sum() < len(q)
    assert hits[:, 0].tobytes() == want.tobytes() and np.array_equal(within > 0, idx >= 0)
    # and the first record of a longer answer is the same one
    hits4, within4 = K.knn_voxels(keys, cen, cnt, q, 0.2, P(max_dist, 4, 1, 1, False))
    assert hits4[:, 0].tobytes() == want.tobytes() and np.array_equal(within4, within)


@pytest.mark.parametrize("reach", [1, 2])
@pytest.mark.parametrize("min_points", [1, 2])
def test_equals_brute_force_within_reach_times_v(reach, min_points):
    """points and queries on a dyadic grid strictly inside their voxels: no centroid crosses a face, no case is excluded"""
    v = 0.25
    rng = np.random.Generator(np.random.PCG64(10 * reach + min_points))
    _, keys, cen, cnt = K.dyadic_map(rng, v, 600, 9)
    assert np.array_equal(np.floor(cen.astype(np.float64) / v).astype(np.int32), keys)
    q = K.dyadic_queries(rng, v, 400, 9)
    seen = []
    for max_dist in (reach * v, 0.6 * reach * v):
        for k in (1, 5, 16):
            p = P(max_dist, k, reach, min_points, False)
            got, got_within = K.knn_voxels(keys, cen, cnt, q, v, p)
            want, want_within = K.brute_knn(keys, cen, cnt, q, p)
            assert np.array_equal(got_within, want_within) and got.tobytes() == want.tobytes(), (max_dist, k)
            seen.append(((got_within == 0).any(), (got_within > k).any(), ((got_within > 0) & (got_within < k)).any()))
    assert all(np.any(seen, axis=0)), "queries with nothing, with more than k and with fewer than k neighbours all occur"


def _lattice(n=4, v=0.5):
    keys = np.array([[x, y, z] for x in range(n) for y in range(n) for z in range(n)], np.int32)
    return keys, ((keys + 0.5) * v).astype(np.float32), np.ones(len(keys), np.uint32)


def test_planted_exact_ties_are_ordered_by_key():
    v = 0.5
    keys, cen, cnt = _lattice()
    q = np.array([[1.0, 1.0, 1.0], [1.0, 1.25, 1.25], [1.25, 1.25, 1.25]], np.float32)  # a corner, a face centre, a voxel centre
    hits, within = K.knn_voxels(keys, cen, cnt, q, v, P(np.inf, 16, 1, 1, False))
    assert within.tolist() == [27, 27, 27]
    # the corner: the eight voxels around it at d2 = 3/16, in key order
    assert np.all(hits["d2"][0, :8] == 0.1875)
    assert hits["key"][0, :8].tolist() == [[x, y, z] for x in (1, 2) for y in (1, 2) for z in (1, 2)]
    # the face centre: two at 1/16, then eight at 5/16 (x in {1, 2}, one of y, z off by one)
    assert hits["d2"][1, :2].tolist() == [0.0625, 0.0625] and hits["key"][1, :2].tolist() == [[1, 2, 2], [2, 2, 2]]
    assert np.all(hits["d2"][1, 2:10] == 0.3125)
    k8 = hits["key"][1, 2:10]
    assert np.all(Q.pack(k8)[1:] > Q.pack(k8)[:-1])
    # the voxel centre: itself, then the six face neighbours in key order
    assert hits["d2"][2, 0] == 0.0 and np.all(hits["d2"][2, 1:7] == 0.25)
    assert hits["key"][2, 1:7].tolist() == [[1, 2, 2], [2, 1, 2], [2, 2, 1], [2, 2, 3], [2, 3, 2], [3, 2, 2]]
    # not_own takes the voxel itself out and nothing else
    own, own_within = K.knn_voxels(keys, cen, cnt, q[2:], v, P(np.inf, 16, 1, 1, True))
    assert own_within.tolist() == [26] and own[0, :15].tobytes() == hits[2, 1:16].tobytes()
    # every answer is sorted by (d2, key)
    for h in hits:
        d2, pk = h["d2"], Q.pack(h["key"])
        assert np.all((d2[1:] > d2[:-1]) | ((d2[1:] == d2[:-1]) & (pk[1:] > pk[:-1])))


def test_max_dist_is_inclusive_and_one_ulp_less_refuses():
    keys, cen, cnt = Q.HAND_KEYS, Q.HAND_CENTROIDS, Q.HAND_COUNTS
    q = Q.HAND_QUERIES[3:4]  # A at exactly 0.25, B at sqrt(0.25^2 + 0.5^2 ...) further
    hits, within = K.knn_voxels(keys, cen, cnt, q, Q.HAND_V, P(0.25, 2, 1, 1, False))
    assert within.tolist() == [1] and hits["d2"][0].tolist() == [0.0625, np.inf] and hits["count"][0].tolist() == [1, 0]
    hits, within = K.knn_voxels(keys, cen, cnt, q, Q.HAND_V, P(float(np.nextafter(0.25, 0)), 2, 1, 1, False))
    assert within.tolist() == [0] and not hits["count"].any() and np.all(np.isinf(hits["d2"])) and not hits["flags"].any()
    # min_points: C holds two points, B one
    hits, within = K.knn_voxels(keys, cen, cnt, Q.HAND_QUERIES[2:3], Q.HAND_V, P(np.inf, 2, 1, 2, False))
    assert within.tolist() == [1] and hits["key"][0, 0].tolist() == [3, 0, 0]
    # reach 2 sees C and D from query 0 (own voxel (1, 0, 0)): four candidates instead of two
    h1, w1 = K.knn_voxels(keys, cen, cnt, Q.HAND_QUERIES[:1], Q.HAND_V, P(np.inf, 4, 1, 1, False))
    h2, w2 = K.knn_voxels(keys, cen, cnt, Q.HAND_QUERIES[:1], Q.HAND_V, P(np.inf, 4, 2, 1, False))
    assert w1.tolist() == [2] and w2.tolist() == [4] and h2[0, :2].tobytes() == h1[0, :2].tobytes()
    # unsearchable queries: k flagged miss records
    hits, within = K.knn_voxels(keys, cen, cnt, Q.HAND_QUERIES[6:10], Q.HAND_V, P(np.inf, 3, 2, 1, False))
    assert not within.any() and np.all(hits["flags"] == 1) and np.all(np.isinf(hits["d2"])) and not hits["count"].any()
