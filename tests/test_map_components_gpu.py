"""Connected components of the voxel map on the device (csrc/map.hip: k_map_cc_index / _link / _flatten / _stats / _select / _erase;
DESIGN 8.14).

Every comparison is of bytes with the restatement of tests/map_components_ref.py run on export(): keys, labels, records and the four
counts of wc_map_components; fresh-map equivalence (as tests/test_map_remove_gpu.py has it) for wc_map_remove_small.  Shapes: at most a
few thousand voxels, every map built by ONE insert into a reserved table (v = 0.5, points that float32 holds exactly) or, for the room
scene, by one insert of 20 000 points."""
import ctypes as C
import functools

import numpy as np
import pytest

import map_carve_ref as CR
import map_components_ref as CC
import map_remove_ref as MR
from helpers import xyz_of as _xyz
from map_query_ref import pack
from test_map_gpu import _drive
from test_map_remove_gpu import _same
from wildcat_slam_amd import lib
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

pytestmark = pytest.mark.gpu

WC_ERR_CAPACITY, WC_ERR_ARG = 1, 11
V = MR.CLUSTER_V
CONNS = (6, 18, 26)
OFFS = (0.25, 0.125, 0.375, 0.0625)  # the points of one voxel: (k * v + off) on every axis, exact in float32
RM_OUT = ("components", "components_removed", "voxels_removed", "points_removed")


def _points(keys, counts):
    """counts[i] points in voxel keys[i] -> (n, 3) float32"""
    keys, counts = np.asarray(keys, np.int64).reshape(-1, 3), np.asarray(counts, np.int64).reshape(-1)
    assert counts.max(initial=1) <= len(OFFS)
    return np.concatenate([MR.centre_points(keys[counts > j], off) for j, off in enumerate(OFFS)]) if len(keys) else np.zeros((0, 3), np.float32)


def _map_of(gpu, keys, counts, moments=False, reserve=8192):
    m = gpu.map_create(V, reserve_voxels=reserve, moments=moments)
    pts = _points(keys, counts)
    if len(pts):
        assert m.insert(pts) == 0
    return m


@functools.lru_cache(maxsize=None)
def _shape(name):
    """a planted shape and a cache of its restatement per (connectivity, min_points): computed once, shared, left unchanged"""
    if name.startswith("sparse"):
        keys, counts = CC.random_sparse(int(name[6:]), int(name[6:]))
    else:
        keys, counts = CC.planted()[name]
    return keys, counts, {}


def _want(name, conn, mp=1):
    keys, counts, cache = _shape(name)
    if (conn, mp) not in cache:
        cache[conn, mp] = CC.components(keys, counts, conn, mp)
    return cache[conn, mp]


def _agrees(m, conn, mp=1, want=None):
    """wc_map_components of m against the restatement on m's own export -> the restatement's dict"""
    _, cnt, keys = m.export()
    labels, comps, out = want if want is not None else CC.components(keys, cnt, conn, mp)
    gk, gl, gc, res = m.components(conn, mp)
    assert res == out, (conn, mp, res, out)
    assert gk.tobytes() == np.ascontiguousarray(keys, np.int32).tobytes()
    assert gl.tobytes() == labels.tobytes() and gc.tobytes() == comps.tobytes(), (conn, mp)
    return out


# ---- smallest cases --------------------------------------------------------------------------------------------------------------
def test_empty_and_single(gpu):
    m = gpu.map_create(V, reserve_voxels=64)
    for conn in CONNS:
        keys, labels, comps, res = m.components(conn)
        assert len(keys) == len(labels) == len(comps) == 0 and res == dict(voxels=0, nodes=0, components=0, largest=0)
    assert m.remove_small(5) == dict(zip(RM_OUT, (0, 0, 0, 0)))
    m.insert(_points(*_shape("single")[:2]))
    for conn in CONNS:
        assert _agrees(m, conn, want=_want("single", conn)) == dict(voxels=1, nodes=1, components=1, largest=1)
    assert _agrees(m, 26, 2) == dict(voxels=1, nodes=0, components=0, largest=0)
    m.close()


@pytest.mark.parametrize("kind", list(CC.PAIRS))
def test_pairs(gpu, kind):
    """two voxels sharing a face, an edge, a corner, and two apart: the 12 verdicts"""
    keys, counts, _ = _shape("pair_" + kind)
    m = _map_of(gpu, keys, counts, reserve=64)
    for conn in CONNS:
        out = _agrees(m, conn, want=_want("pair_" + kind, conn))
        assert out["components"] == (1 if CC.PAIR_VERDICTS[kind, conn] else 2)
    m.close()


def test_key_range_ends(gpu):
    """voxels at k = 2^20 - 1 and k = -(2^20 - 1), the ends of the key range (k = -2^20 is no voxel index: the map refuses it), on each
    axis, with and without a partner one step inside: nothing joins across the range's ends or across axes"""
    keys, counts, _ = _shape("range_ends")
    m = _map_of(gpu, keys, counts, reserve=256)
    assert m.size() == (len(keys), len(keys))
    assert [_agrees(m, c, want=_want("range_ends", c))["components"] for c in CONNS] == [19, 19, 18]
    m.close()


# ---- long chains, late merges, contention -------------------------------------------------------------------------------------------
def test_snake_and_its_cut(gpu):
    """3029 voxels in one chain that folds back and forth; then cut in its middle by remove(): two components, the tombstone is no bridge"""
    keys, counts, chain = CC.snake()
    m = _map_of(gpu, keys, counts)
    for conn in CONNS:
        assert _agrees(m, conn, want=_want("snake", conn)) == dict(voxels=3029, nodes=3029, components=1, largest=3029)
    mid = len(chain) // 2
    assert m.remove(keys[chain[mid]][None]) == dict(voxels_removed=1, points_removed=1, keys_unused=0)
    for conn in CONNS:
        out = _agrees(m, conn)
        assert (out["voxels"], out["components"], out["largest"]) == (3028, 2, len(chain) - mid - 1)
    m.close()


@pytest.mark.parametrize("name, figures", [("comb", (1, 1, 1)), ("block", (1, 1, 1)), ("checker", (2048, 1, 1))])
def test_comb_block_checkerboard(gpu, name, figures):
    """comb: long teeth that grow from the small keys and meet only at their far end - large trees merge late; block: 12^3 voxels, every
    lane unites into one root; checkerboard: 2048 voxels of which no two share a face (2048 components under 6) and every one shares an
    edge with its neighbours (one component under 18 and 26)"""
    keys, counts, _ = _shape(name)
    m = _map_of(gpu, keys, counts)
    assert tuple(_agrees(m, c, want=_want(name, c))["components"] for c in CONNS) == figures
    m.close()


@pytest.mark.parametrize("moments", [False, True])
def test_node_gate(gpu, moments):
    """two blobs joined by a one-point voxel: one component at min_points = 1, two at min_points = 2 with the bridge unlabelled"""
    keys, counts, at = CC.bridge()
    m = _map_of(gpu, keys, counts, moments=moments, reserve=128)
    for conn in CONNS:
        assert _agrees(m, conn, 1, _want("bridge", conn, 1))["components"] == 1
        assert _agrees(m, conn, 2, _want("bridge", conn, 2)) == dict(voxels=55, nodes=54, components=2, largest=27)
    assert m.components(26, 2)[1][at] == R.MAP_NO_COMPONENT
    assert _agrees(m, 26, 4) == dict(voxels=55, nodes=0, components=0, largest=0)  # (no node at all: every label is the sentinel)
    m.close()


# ---- counts and table state ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_counts_at_wavefront_and_workgroup_ends(gpu, n):
    name = "sparse%d" % n
    keys, counts, _ = _shape(name)
    m = _map_of(gpu, keys, counts, reserve=512)
    for conn in CONNS:
        for mp in (1, 2, 3):
            _agrees(m, conn, mp, _want(name, conn, mp))
    m.close()


def test_collision_cluster_behind_tombstones(gpu):
    """a 64-key collision cluster and 2000 voxels at half fill in an 8192-slot table, every second key removed first: the probes of the
    link pass walk through tombstones, and a removed voxel joins nothing"""
    rng = np.random.Generator(np.random.PCG64(23))
    cluster = MR.cluster_keys(64, MR.CLUSTER_SLOTS - 1)
    rest = MR.distinct_keys(rng, 2000, -8, 8, avoid=cluster)
    keys, counts = CC.sort_keys(np.concatenate([cluster, rest]))
    m = _map_of(gpu, keys, counts, reserve=MR.CLUSTER_SLOTS // 2)
    assert m.info()["slots"] == MR.CLUSTER_SLOTS
    before = [_agrees(m, c)["components"] for c in CONNS]
    gone = keys[::2]
    assert m.remove(gone)["voxels_removed"] == len(gone) and m.tombstones() == (len(gone), 0)
    after = [_agrees(m, c) for c in CONNS]
    assert all(a["voxels"] == len(keys) - len(gone) for a in after) and [a["components"] for a in after] != before
    m.close()


@pytest.mark.parametrize("moments", [False, True])
def test_grid_sizes_and_repeated_calls(gpu, moments):
    """map_cc_groups 1, 7 and the default, each called twice in one context: the same bytes, and the map is what it was"""
    keys, counts = CC.random_sparse(77, 3000, fill=0.25)
    m = _map_of(gpu, keys, counts, moments=moments)
    state = [np.ascontiguousarray(a).tobytes() for a in m.state() if a is not None]
    outs = []
    try:
        for groups in (1, 1, 7, 7, 0, 0):
            gpu.set_dev_option("map_cc_groups", groups)
            for conn in CONNS:
                got = m.components(conn, 2)
                outs.append((conn, got[0].tobytes(), got[1].tobytes(), got[2].tobytes(), tuple(got[3].items())))
    finally:
        gpu.set_dev_option("map_cc_groups", 0)
    for conn in CONNS:
        mine = [o for o in outs if o[0] == conn]
        assert len(mine) == 6 and all(o == mine[0] for o in mine)
        _agrees(m, conn, 2)
    assert [np.ascontiguousarray(a).tobytes() for a in m.state() if a is not None] == state and m.tombstones() == (0, 0)
    m.close()


# ---- the room scene --------------------------------------------------------------------------------------------------------------
# v -> (voxels, {connectivity: (components, voxels of the largest)}) of 20 000 points of synth.g1_room, min_points = 1
ROOM_FIGURES = {
    0.2: (15336, {6: (4867, 2934), 18: (1882, 7299), 26: (1169, 7414)}),
    0.5: (6756, {6: (197, 4642), 18: (31, 6595), 26: (19, 6603)}),
}


@functools.lru_cache(maxsize=None)
def _room():
    return _xyz(synth.g1_room(20000))


@pytest.mark.parametrize("v", [0.2, 0.5])
def test_room_scene(gpu, v):
    m = gpu.map_create(v, reserve_voxels=20000, moments=True)
    assert m.insert(_room()) == 0
    n_vox, figures = ROOM_FIGURES[v]
    for conn in CONNS:
        out = _agrees(m, conn)
        assert (out["voxels"], (out["components"], out["largest"])) == (n_vox, figures[conn])
    _agrees(m, 26, 3)
    m.close()


# ---- wc_map_remove_small -----------------------------------------------------------------------------------------------------------
def _speckle(seed, v):
    """isolated points and short strands of two to four voxels hung in the free space of the room scene -> (n, 3) float32"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pts = []
    for _ in range(120):
        start = rng.uniform([-15.0, -10.0, 0.5], [15.0, 10.0, 4.0])
        step = np.eye(3)[int(rng.integers(0, 3))] * v
        pts += [start + j * step for j in range(int(rng.integers(1, 5)))]
    return np.array(pts, np.float32)


def _stays(points, v, keep_keys):
    """per point: its voxel is one of keep_keys"""
    return np.isin(pack(CR.point_keys(points, v)), pack(np.asarray(keep_keys, np.int64).reshape(-1, 3)))


def _removed_as_restated(gpu, m, points, call, rays, origin):
    """m.remove_small(**call) against the restatement on m's export, then fresh-map equivalence; a second call removes nothing -> dict"""
    _, cnt, keys = m.export()
    keep, want = CC.remove_small(keys, cnt, **call)
    tombs = m.tombstones()[0]
    got = m.remove_small(**call)
    assert got == want, (got, want)
    assert m.tombstones() == (tombs + want["voxels_removed"], 0)
    stays = _stays(points, m.voxel, keys[keep])
    left, gone_pts = points[stays], points[~stays]
    f = gpu.map_create(m.voxel, moments=m.moments)
    if len(left):
        assert f.insert(left) == 0
    assert m.size() == f.size() == (int(keep.sum()), int(cnt[keep].sum()))
    queries = np.concatenate([left[:: max(len(left) // 2500, 1)], gone_pts[:1500]])
    _same(m, f, queries, rays, origin, str(call))
    f.close()
    again = m.remove_small(**call)
    assert again == dict(components=want["components"] - want["components_removed"], components_removed=0, voxels_removed=0, points_removed=0)
    assert m.tombstones() == (tombs + want["voxels_removed"], 0)
    return want


@pytest.mark.parametrize("moments", [False, True])
def test_remove_small_on_the_room_with_speckle(gpu, moments):
    v = 0.5
    points = np.concatenate([_room(), _speckle(41, v)])
    m = gpu.map_create(v, reserve_voxels=32768, moments=moments)  # (room for every point of the insert: no growth)
    assert m.insert(points) == 0
    slots = m.info()["slots"]
    assert slots == 65536 and m.info()["growths"] == 0
    rays, origin = _room()[::20], np.array([0.25, -0.25, 1.25])
    first = _removed_as_restated(gpu, m, points, dict(min_voxels=5, min_comp_points=0, connectivity=26, min_points=1), rays, origin)
    assert first["components_removed"] >= 50 and first["voxels_removed"] >= 100  # (the speckle: most strands touch nothing)
    # what is left, under another rule: small in points, sparse voxels dropped
    left = points[_stays(points, v, m.export()[2])]
    second = _removed_as_restated(gpu, m, left, dict(min_voxels=0, min_comp_points=40, connectivity=6, min_points=2, drop_sparse=True), rays, origin)
    assert second["voxels_removed"] > 0
    # an insert afterwards: purge or growth as the room policy says (csrc/map_room.h, restated in map_remove_ref.room)
    live, tombs = m.size()[0], m.tombstones()[0]
    assert tombs == first["voxels_removed"] + second["voxels_removed"] and m.info()["slots"] == slots
    # as many new voxels as fit into half of the table beside the live ones, but not beside the tombstones as well: a purge
    n_new = slots // 2 - live - 10
    assert tombs > 10
    new = MR.centre_points(MR.distinct_keys(np.random.Generator(np.random.PCG64(3)), n_new, 200, 240))
    what, cap = MR.room(slots, live, tombs, len(new))
    assert (what, cap) == (MR.PURGE, slots)
    assert m.insert(new) == 0
    assert m.info()["slots"] == cap and m.info()["growths"] == (1 if what == MR.GROW else 0)
    assert m.tombstones() == ((tombs, 0) if what == MR.KEEP else (0, 1 if what == MR.PURGE else 0))
    assert m.size()[0] == live + n_new
    m.close()


@pytest.mark.parametrize("drop_sparse", [False, True])
def test_remove_small_on_the_bridge(gpu, drop_sparse):
    keys, counts, at = CC.bridge()
    extra = np.array([[20, 20, 20], [20, 20, 21]])  # a small component that goes either way
    keys, counts = CC.sort_keys(np.concatenate([keys, extra]), np.concatenate([counts, [2, 2]]))
    points = _points(keys, counts)
    m = gpu.map_create(V, reserve_voxels=128, moments=True)
    assert m.insert(points) == 0
    rays, origin = _points(keys, np.ones(len(keys), np.int64)) + np.float32(0.125), np.array([-3.3, 0.6, 0.7])
    want = _removed_as_restated(gpu, m, points, dict(min_voxels=3, min_comp_points=0, connectivity=26, min_points=2, drop_sparse=drop_sparse), rays, origin)
    assert want == dict(components=3, components_removed=1, voxels_removed=2 + drop_sparse, points_removed=4 + drop_sparse)
    assert (len(m.export()[1]) == 55) != drop_sparse
    # both thresholds 0: nothing goes, not even a tombstone
    assert m.remove_small(0, 0, min_points=2) == dict(components=2, components_removed=0, voxels_removed=0, points_removed=0)
    m.close()


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_map_unchanged(gpu):
    keys, counts = CC.random_sparse(5, 300)
    m = _map_of(gpu, keys, counts, moments=True, reserve=512)
    other = lib.Context(0)
    want = CC.components(keys, counts, 26)[2]
    snapshot = lambda: (m.size(), m.tombstones(), m.info(), [np.ascontiguousarray(a).tobytes() for a in m.state()])
    before = snapshot()
    out = (C.c_uint64 * 4)(9, 9, 9, 9)
    d_label, d_comps = gpu.alloc(4 * 300), gpu.alloc(40 * 300)
    ok = lib.map_cc_params(26, 1)
    bad_params = [lib.map_cc_params(7), lib.map_cc_params(26, 0), lib.map_cc_params(26, 1, reserved=1), R.MapCcParams(26, 1, 2, 0)]
    f, g = gpu.lib.wc_map_components, gpu.lib.wc_map_remove_small
    for p in bad_params:
        assert f(gpu.h, m.h, C.byref(p), None, C.c_void_p(d_label.ptr), C.c_uint64(300), None, C.c_uint64(0), out) == WC_ERR_ARG
        assert g(gpu.h, m.h, C.byref(p), C.c_uint32(1000), C.c_uint64(0), out) == WC_ERR_ARG
    assert f(gpu.h, m.h, None, None, C.c_void_p(d_label.ptr), C.c_uint64(300), None, C.c_uint64(0), out) == WC_ERR_ARG
    assert f(gpu.h, m.h, C.byref(ok), None, C.c_void_p(d_label.ptr), C.c_uint64(300), None, C.c_uint64(0), None) == WC_ERR_ARG
    assert f(gpu.h, m.h, C.byref(ok), None, None, C.c_uint64(300), None, C.c_uint64(0), out) == WC_ERR_ARG  # (room for labels, no labels)
    assert f(gpu.h, m.h, C.byref(ok), None, C.c_void_p(d_label.ptr + 2), C.c_uint64(300), None, C.c_uint64(0), out) == WC_ERR_ARG
    assert f(gpu.h, m.h, C.byref(ok), None, C.c_void_p(d_label.ptr), C.c_uint64(300), C.c_void_p(d_comps.ptr + 4), C.c_uint64(300), out) == WC_ERR_ARG
    assert f(other.h, m.h, C.byref(ok), None, C.c_void_p(d_label.ptr), C.c_uint64(300), None, C.c_uint64(0), out) == WC_ERR_ARG
    assert g(gpu.h, m.h, None, C.c_uint32(1000), C.c_uint64(0), out) == WC_ERR_ARG
    assert g(gpu.h, m.h, C.byref(ok), C.c_uint32(1000), C.c_uint64(0), None) == WC_ERR_ARG
    assert g(other.h, m.h, C.byref(ok), C.c_uint32(1000), C.c_uint64(0), out) == WC_ERR_ARG
    assert list(out) == [9, 9, 9, 9] and snapshot() == before
    # too little room: WC_ERR_CAPACITY with h_out filled, for the labels and for the records
    gpu.lib.wc_memset(gpu.h, C.c_void_p(d_label.ptr), C.c_int(0xEE), C.c_size_t(4 * 300))
    assert f(gpu.h, m.h, C.byref(ok), None, C.c_void_p(d_label.ptr), C.c_uint64(299), None, C.c_uint64(0), out) == WC_ERR_CAPACITY
    assert [int(x) for x in out] == [want[k] for k in CC.OUT]
    assert np.all(d_label.download(np.uint32, 300) == 0xEEEEEEEE)
    out[:] = [9, 9, 9, 9]
    assert want["components"] > 1
    assert f(gpu.h, m.h, C.byref(ok), None, C.c_void_p(d_label.ptr), C.c_uint64(300), C.c_void_p(d_comps.ptr), C.c_uint64(want["components"] - 1),
             out) == WC_ERR_CAPACITY
    assert [int(x) for x in out] == [want[k] for k in CC.OUT] and snapshot() == before
    # the device form with exactly enough room
    rc, res = m.components_device(ok, None, d_label, 300, d_comps, want["components"])
    labels, comps, _ = CC.components(keys, counts, 26)
    assert rc == 0 and res == want and d_label.download(np.uint32, 300).tobytes() == labels.tobytes()
    assert d_comps.download(R.MAP_COMPONENT, want["components"]).tobytes() == comps.tobytes()
    for b in (d_label, d_comps):
        b.free()
    other.close()
    m.close()


# ---- the facade --------------------------------------------------------------------------------------------------------------------
def test_facade(gpu):
    """Odometry.map_components / .map_remove_small on the map a few facade sweeps built are PointMap's on a map of the same points"""
    msgs, imu, _ = synth.raw_stream(1.7, pts_per_s=300_000, gyro_bias=(0.0, 0.0, 0.02), t_start=1000.0)
    v = 0.5
    odo = lib.Odometry(0)
    odo.set_fill_outputs(True)
    odo.set_map_voxel(v)
    scans = []
    _drive(odo, msgs, imu, lambda: scans.append(_xyz(odo.outputs()["scan"])))
    assert odo.sweeps() >= 2
    m = gpu.map_create(v)
    m.insert(np.concatenate(scans))
    samples = odo.samples().tobytes()
    for conn, mp in ((26, 1), (6, 2)):
        want, got = m.components(conn, mp), odo.map_components(conn, mp)
        assert got[3] == want[3] and want[3]["components"] >= 1
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], want[:3]))
    _agrees(m, 26)
    assert odo.map_components(7) is None and odo.map_remove_small(5, connectivity=5) is None and odo.map_remove_small(5, min_points=0) is None
    assert odo.samples().tobytes() == samples
    want = m.remove_small(4, 10, 18, 2, drop_sparse=True)
    assert odo.map_remove_small(4, 10, 18, 2, drop_sparse=True) == want and want["voxels_removed"] > 0
    xyz, cnt = odo.map_export()
    exported = m.export()
    assert exported[0].tobytes() == xyz.tobytes() and exported[1].tobytes() == cnt.tobytes() and odo.samples().tobytes() == samples
    odo.close()
    m.close()
    none = lib.Odometry(0)
    assert none.map_components() is None and none.map_remove_small(5) is None  # no map
    none.close()
