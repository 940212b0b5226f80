"""Connected components of the voxel map without a GPU: the restatement of tests/map_components_ref.py against an independent
brute force and scipy.ndimage.label, the library's host labeller wc_map_label_keys against the restatement byte for byte, its refusals, the
declarations, and the planted shape that catches each deliberate fault of the restatement."""
import ctypes as C
import os

import numpy as np
import pytest

import map_components_ref as CC
from wildcat_slam_amd import lib
from wildcat_slam_amd import records as R

HERE = os.path.dirname(os.path.abspath(__file__))
WC_ERR_CAPACITY, WC_ERR_ARG = 1, 11
CONNS = (6, 18, 26)


@pytest.fixture(autouse=True)
def _the_labeller_exists():
    """every case here is about wc_map_label_keys or about the restatement it is held to: without the symbol none of them says anything"""
    assert hasattr(lib.load(), "wc_map_label_keys") and hasattr(R, "MAP_COMPONENT")


def _random_sets():
    """a few hundred random sparse key sets: 4 .. 60 voxels at fills from 5 to 50 percent"""
    rng = np.random.Generator(np.random.PCG64(17))
    return [CC.random_sparse(1000 + i, int(rng.integers(4, 61)), fill=float(rng.uniform(0.05, 0.5))) for i in range(300)]


def _bytes(labels, comps):
    return np.ascontiguousarray(labels, np.uint32).tobytes() + np.ascontiguousarray(comps).tobytes()


def test_the_record_is_the_headers():
    assert CC.COMPONENT == R.MAP_COMPONENT and CC.COMPONENT.itemsize == 40 and CC.NO_COMPONENT == R.MAP_NO_COMPONENT
    assert C.sizeof(R.MapCcParams) == 16 and [f for f, _ in R.MapCcParams._fields_] == ["connectivity", "min_points", "flags", "reserved"]
    assert [len(CC.offsets(c)) for c in CONNS] == [6, 18, 26]


def test_restatement_against_brute_force():
    for i, (keys, counts) in enumerate(_random_sets()):
        conn, mp = CONNS[i % 3], 1 + (i // 3) % 3
        labels, comps, out = CC.components(keys, counts, conn, mp)
        assert np.array_equal(labels, CC.brute(keys, counts, conn, mp)), i
        # the records restate the labels
        assert out["components"] == len(comps) and out["nodes"] == int(comps["voxels"].sum()) == int(np.sum(counts >= mp))
        for c, rec in enumerate(comps):
            mine = np.flatnonzero(labels == c)
            assert rec["first"] == mine[0] and rec["voxels"] == len(mine) and rec["points"] == counts[mine].sum()
            assert np.array_equal(rec["kmin"], keys[mine].min(0)) and np.array_equal(rec["kmax"], keys[mine].max(0))
        assert np.all(np.diff(comps["first"].astype(np.int64)) > 0)  # numbered in ascending order of the root


def test_pair_verdicts():
    for (kind, conn), joined in CC.PAIR_VERDICTS.items():
        assert CC.components(*CC.pair(kind), conn)[2]["components"] == (1 if joined else 2), (kind, conn)


def test_restatement_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    shapes = [s for s in _random_sets()[:90]] + [CC.planted()[n] for n in ("checker", "bridge", "comb", "block", "pair_edge", "pair_corner")]
    for i, (keys, counts) in enumerate(shapes):
        lo = keys.min(0)
        grid = np.zeros(tuple(keys.max(0) - lo + 1), bool)
        grid[tuple((keys - lo).T)] = True
        for rank, conn in enumerate(CONNS, 1):
            lab, n = ndimage.label(grid, structure=ndimage.generate_binary_structure(3, rank))
            labels, _, out = CC.components(keys, counts, conn)
            # (scipy numbers in C scan order of (x, y, z): ascending key order, the order of the roots)
            assert n == out["components"] and np.array_equal(lab[tuple((keys - lo).T)] - 1, labels.astype(np.int64)), (i, conn)


@pytest.mark.parametrize("conn", CONNS)
def test_label_keys_is_the_restatement(conn):
    shapes = list(CC.planted().items()) + [("random%d" % i, s) for i, s in enumerate(_random_sets())]
    shapes += [("sparse%d" % n, CC.random_sparse(n, n)) for n in (63, 64, 65, 255, 256, 257)]
    for name, (keys, counts) in shapes:
        for mp in (1, 2) if name in ("bridge", "sparse256") or name.startswith("random") else (1,):
            labels, comps, out = CC.components(keys, counts, conn, mp)
            got = lib.map_label_keys(keys, counts, conn, mp)
            assert got[2] == out, (name, mp)
            assert _bytes(got[0], got[1]) == _bytes(labels, comps), (name, mp)


def test_planted_figures():
    """the figures the shapes were planted for"""
    p = CC.planted()
    comp = lambda name, conn, mp=1: CC.components(*p[name], conn, mp)[2]
    assert [comp("snake", c)["components"] for c in CONNS] == [1, 1, 1] and comp("snake", 6)["largest"] == 3029
    assert [comp("comb", c)["components"] for c in CONNS] == [1, 1, 1]
    assert comp("block", 6) == dict(voxels=1728, nodes=1728, components=1, largest=1728)
    # no two voxels of the checkerboard share a face, every one shares an edge with twelve others: 2048 components under 6, ONE under 18 and 26
    assert [comp("checker", c)["components"] for c in CONNS] == [2048, 1, 1]
    assert [comp("bridge", c, 1)["components"] for c in CONNS] == [1, 1, 1] and [comp("bridge", c, 2)["components"] for c in CONNS] == [2, 2, 2]
    keys, counts, at = CC.bridge()
    assert CC.components(keys, counts, 26, 2)[0][at] == CC.NO_COMPONENT and tuple(keys[at]) == (3, 1, 1)
    # the ends of the range: per axis 2 alone and 2 face pairs (12), the face pair at the far corner (1), the corner pair at the near
    # corner (2 under 6 and 18, 1 under 26) and 4 that touch nothing
    assert [comp("range_ends", c)["components"] for c in CONNS] == [19, 19, 18]
    assert comp("empty", 26) == dict(voxels=0, nodes=0, components=0, largest=0)


# fault -> (the planted shape that catches it, connectivity, min_points)
CAUGHT_BY = {"wrap": ("range_ends", 6, 1), "upper_forgotten": ("pair_face", 6, 1), "gate_one_end": ("bridge", 26, 2), "first_seen": ("z_major_pair", 26, 1)}


def test_every_fault_is_caught_by_a_planted_shape():
    assert set(CAUGHT_BY) == set(CC.FAULTS)
    p = CC.planted()
    for fault, (name, conn, mp) in CAUGHT_BY.items():
        keys, counts = p[name]
        good, bad = CC.components(keys, counts, conn, mp), CC.components(keys, counts, conn, mp, fault=fault)
        assert _bytes(*good[:2]) != _bytes(*bad[:2]), fault
        got = lib.map_label_keys(keys, counts, conn, mp)
        assert _bytes(got[0], got[1]) == _bytes(*good[:2]), fault  # the library sides with the restatement
    # and what each fault does there
    assert CC.components(*p["range_ends"], 6, fault="wrap")[2]["components"] == 13  # per axis the two lone voxels join across the range's ends, and so do the two pairs
    assert CC.components(*p["pair_face"], 6, fault="upper_forgotten")[2]["components"] == 2
    assert CC.components(*p["bridge"], 26, 2, fault="gate_one_end")[2]["components"] == 1
    assert list(CC.components(*p["z_major_pair"], 26, fault="first_seen")[0]) == [1, 0]


def _raw(keys, counts, params, cap_comps=None, n=None):
    keys, counts = np.ascontiguousarray(keys, np.int32).reshape(-1, 3), np.ascontiguousarray(counts, np.uint32)
    n = len(keys) if n is None else n
    labels, comps, out = np.zeros(max(len(keys), 1), np.uint32), np.zeros(max(len(keys), 1), R.MAP_COMPONENT), (C.c_uint64 * 4)(9, 9, 9, 9)
    rc = lib.load().wc_map_label_keys(R.ptr(keys), R.ptr(counts), C.c_uint64(n), C.byref(params) if params is not None else None, R.ptr(labels),
                                      R.ptr(comps), C.c_uint64(len(keys) if cap_comps is None else cap_comps), out)
    return rc, [int(x) for x in out]


def test_label_keys_refusals():
    keys, counts = CC.random_sparse(5, 40)
    ok = lib.map_cc_params(26, 1)
    assert _raw(keys, counts, ok)[0] == 0
    swapped = keys.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    twice = keys.copy()
    twice[7] = twice[6]
    for bad_keys in (swapped, twice):
        assert _raw(bad_keys, counts, ok) == (WC_ERR_ARG, [9, 9, 9, 9])
    for axis in range(3):
        for k in (CC.KEY_LIM, -CC.KEY_LIM):
            far, _ = CC.sort_keys([(0, 0, 0), tuple(np.eye(3, dtype=np.int64)[axis] * k)])  # (ascending: only the range is wrong)
            assert _raw(far, [1, 1], ok) == (WC_ERR_ARG, [9, 9, 9, 9]), (axis, k)
            near, _ = CC.sort_keys([(0, 0, 0), tuple(np.eye(3, dtype=np.int64)[axis] * (k - np.sign(k)))])
            assert _raw(near, [1, 1], ok) == (0, [2, 2, 2, 1]), (axis, k)
    for bad in (lib.map_cc_params(7, 1), lib.map_cc_params(0, 1), lib.map_cc_params(26, 0), lib.map_cc_params(26, 1, reserved=1),
                R.MapCcParams(26, 1, 2, 0), None):
        assert _raw(keys, counts, bad) == (WC_ERR_ARG, [9, 9, 9, 9])
    assert _raw(keys, counts, R.MapCcParams(26, 1, R.MAP_CC_DROP_SPARSE, 0))[0] == 0  # (the one known flag)
    # a short cap_comps: WC_ERR_CAPACITY, h_out filled all the same
    want = CC.components(keys, counts, 26)[2]
    assert want["components"] > 1
    assert _raw(keys, counts, ok, cap_comps=want["components"] - 1) == (WC_ERR_CAPACITY, [want[k] for k in CC.OUT])
    assert _raw(keys, counts, ok, cap_comps=want["components"]) == (0, [want[k] for k in CC.OUT])
    with pytest.raises(lib.WildcatError) as e:
        lib.map_label_keys(keys, counts, 26, cap_comps=1)
    assert e.value.code == WC_ERR_CAPACITY and e.value.out == want
    # nothing at all: WC_OK and zeros
    assert _raw(np.zeros((0, 3), np.int32), np.zeros(0, np.uint32), ok) == (0, [0, 0, 0, 0])


def test_header_declares_the_calls_and_the_libraries_export_them():
    declared = set(lib.declared_symbols())
    l = lib.load()
    for s in ("wc_map_components", "wc_map_remove_small", "wc_map_label_keys"):
        assert s in declared and hasattr(l, s), s
    host = C.CDLL(os.path.join(HERE, "..", "wildcat-slam_amd", "host", "libwildcat_odometry.so"))
    for s in ("wc_odom_map_components", "wc_odom_map_remove_small"):
        assert hasattr(host, s), s
    with open(os.path.join(HERE, "..", "include", "wildcat_hip.h")) as f:
        text = f.read()
    with open(os.path.join(HERE, "..", "include", "wc_types.h")) as f:
        types = f.read()
    assert "WC_ERR_INTERNAL = 14" in text and "map_cc_groups" in text
    assert "#define WC_MAP_NO_COMPONENT 0xFFFFFFFFu" in types and "#define WC_MAP_CC_DROP_SPARSE 1u" in types
    for word in ("typedef struct wc_map_cc_params", "typedef struct wc_map_component", "uint32_t first;", "int32_t kmin[3];"):
        assert word in types, word
    for name in ("components", "components_device", "remove_small"):
        assert hasattr(lib.PointMap, name), name
    assert hasattr(lib.Odometry, "map_components") and hasattr(lib.Odometry, "map_remove_small")


def test_remove_small_restated():
    """the restatement of wc_map_remove_small: idempotent, thresholds of 0 switch a test off, the sparse voxels go only when asked"""
    keys, counts, at = CC.bridge()
    keep, out = CC.remove_small(keys, counts, 0, 0)
    assert keep.all() and out == dict(components=1, components_removed=0, voxels_removed=0, points_removed=0)
    keep, out = CC.remove_small(keys, counts, 28, 0, min_points=2)  # two blobs of 27: both go, the bridge stays
    assert list(np.flatnonzero(keep)) == [at] and out == dict(components=2, components_removed=2, voxels_removed=54, points_removed=162)
    keep, out = CC.remove_small(keys, counts, 0, 0, min_points=2, drop_sparse=True)
    assert list(np.flatnonzero(~keep)) == [at] and out == dict(components=2, components_removed=0, voxels_removed=1, points_removed=1)
    keys, counts = CC.random_sparse(9, 257)
    keep, out = CC.remove_small(keys, counts, 3, 6, 18)
    assert 0 < out["voxels_removed"] < 257
    keep2, out2 = CC.remove_small(keys[keep], counts[keep], 3, 6, 18)
    assert keep2.all() and out2["components"] == out["components"] - out["components_removed"] and out2["voxels_removed"] == 0
