"""The voxel map's exact state on the device (include/wildcat_hip.h: wc_map_export_state, wc_map_absorb, wc_map_merge) and
its file through the facade, against the restatement of map_state_ref.py: the table's integer sums themselves, the round trip through
a state, merge = union, duplicates and the creation race, grid independence, rejection, flag combinations, argument errors, and
SaveMap / LoadMap.  Every case works on at most the 20 000 points of one room sweep."""
import ctypes as C

import numpy as np
import pytest

import map_query_ref as Q
import map_state_ref as MS
from helpers import xyz_of
from wildcat_slam_amd import lib as L
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

pytestmark = pytest.mark.gpu

VOXELS = (0.2, 0.05, float(np.float32(0.8)))
MIN_SHARED = {0.2: 1000, 0.05: 1, float(np.float32(0.8)): 1000}
WC_ERR_CAPACITY, WC_ERR_ARG = 1, 11
ORIGIN = np.array([0.3, -0.2, 1.1])


@pytest.fixture(scope="module")
def cloud():
    return xyz_of(synth.g1_room(20000, seed=3))


_states = {}


def ref_state(cloud, v, which="all"):
    """the restated state (with moments) of the cloud, its even-indexed or its odd-indexed points; computed once per (v, which)"""
    if (v, which) not in _states:
        pts = {"all": cloud, "even": cloud[0::2], "odd": cloud[1::2]}[which]
        _states[(v, which)] = MS.state_of(pts, v)
    return _states[(v, which)]


def new_map(gpu, v, moments, pts=None, **kw):
    m = gpu.map_create(v, moments=moments, **kw)
    if pts is not None:
        assert m.insert(pts) == 0
    return m


def state_bytes(m):
    vox, mom = m.state()
    return vox.tobytes() + (mom.tobytes() if mom is not None else b"")


def want_bytes(state, moments):
    return state[0].tobytes() + (state[1].tobytes() if moments else b"")


def summary_bytes(s):
    """every field of align's summary, exactly"""
    return np.array([s["initial_cost"], s["final_cost"]]).tobytes() + s["last_step"].tobytes() + repr(
        (s["iterations"], s["termination"], s["n_used"], s["n_found"])).encode()


class Shifted:
    """a device buffer's address moved by a few bytes: a misaligned pointer"""

    def __init__(self, buf, by):
        self.ptr = buf.ptr + by


@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("v", VOXELS)
def test_state_is_the_tables_integer_sums(gpu, cloud, v, moments):
    want = ref_state(cloud, v)
    m = new_map(gpu, v, moments, cloud)
    vox, mom = m.state()
    assert len(vox) == len(want[0])
    for f in ("key", "count", "sum"):
        assert np.array_equal(vox[f], want[0][f]), f
    if moments:
        assert mom.dtype == np.int64 and np.array_equal(mom, want[1])
        surf = m.surfels()
        assert vox.view(np.uint8).reshape(-1, 40)[:, :16].tobytes() == surf.view(np.uint8).reshape(-1, 128)[:, :16].tobytes()
    else:
        assert mom is None
    xyz, cnt, keys = m.export()
    assert np.array_equal(keys, vox["key"]) and np.array_equal(cnt, vox["count"])
    m.close()


@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("v", VOXELS)
def test_round_trip_through_a_state(gpu, cloud, v, moments):
    a = new_map(gpu, v, moments, cloud)
    vox, mom = a.state()
    b = new_map(gpu, v, moments, reserve_voxels=1)
    assert b.absorb(vox, mom) == 0
    assert b.info()["growths"] > 0 and b.info()["rejected"] == 0
    assert b.size() == a.size() == (len(vox), len(cloud))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.export(), b.export()))
    assert state_bytes(a) == state_bytes(b) == want_bytes(ref_state(cloud, v), moments)
    if moments:
        assert a.surfels().tobytes() == b.surfels().tobytes()
        rng = np.random.Generator(np.random.PCG64(5))
        q = (cloud[rng.integers(0, len(cloud), 4096)] + rng.normal(size=(4096, 3)) * (v / 2)).astype(np.float32)
        assert a.nearest_plane(q, np.inf).tobytes() == b.nearest_plane(q, np.inf).tobytes()
        scan, T = cloud[::4], np.eye(3, 4)
        T[:, 3] = [0.01, -0.02, 0.005]
        ne_a, ne_b = a.linearize(scan, T, max_dist=2 * v), b.linearize(scan, T, max_dist=2 * v)
        assert ne_a.tobytes() == ne_b.tobytes() and len(ne_a.tobytes()) == 240
        (Ta, sa), (Tb, sb) = (m.align(scan, T, params=L.map_reg_params(2 * v), max_iterations=3) for m in (a, b))
        assert Ta.tobytes() == Tb.tobytes() and summary_bytes(sa) == summary_bytes(sb)
        if v > 0.5:  # (voxels of 0.8 m hold planes enough for a step; the smaller ones mostly hold one or two points of this sweep)
            assert ne_a["n_used"] > 100 and sa["iterations"] >= 1
    else:
        q = cloud[::5]
        assert a.nearest(q, np.inf).tobytes() == b.nearest(q, np.inf).tobytes()
    a.close(), b.close()


@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("v", VOXELS)
def test_merge_is_the_union(gpu, cloud, v, moments):
    even, odd, whole = ref_state(cloud, v, "even"), ref_state(cloud, v, "odd"), ref_state(cloud, v)
    ka, kb = Q.pack(even[0]["key"].astype(np.int64)), Q.pack(odd[0]["key"].astype(np.int64))
    shared = len(np.intersect1d(ka, kb))
    assert shared >= MIN_SHARED[v] and shared < len(ka) and shared < len(kb), (shared, len(ka), len(kb))
    want = want_bytes(whole, moments)
    A, B = new_map(gpu, v, moments, cloud[0::2]), new_map(gpu, v, moments, cloud[1::2])
    b_before, b_size = state_bytes(B), B.size()
    A.merge(B)
    assert state_bytes(A) == want and A.size() == (len(whole[0]), len(cloud))
    assert state_bytes(B) == b_before == want_bytes(odd, moments) and B.size() == b_size
    A2 = new_map(gpu, v, moments, cloud[0::2])
    assert A2.absorb(*B.state()) == 0
    assert state_bytes(A2) == want and A2.size() == A.size()
    W = new_map(gpu, v, moments, cloud)
    for m in (A, A2):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(m.export(), W.export()))
    A.close(), A2.close(), B.close(), W.close()


@pytest.mark.parametrize("moments", [False, True])
def test_duplicate_keys_and_the_creation_race(gpu, cloud, moments):
    v = 0.2
    even, odd = ref_state(cloud, v, "even"), ref_state(cloud, v, "odd")
    vox, mom = np.concatenate([even[0], odd[0]]), np.concatenate([even[1], odd[1]])
    perm = np.random.Generator(np.random.PCG64(9)).permutation(len(vox))
    m = new_map(gpu, v, moments)
    assert m.absorb(vox[perm], mom[perm]) == 0
    assert state_bytes(m) == want_bytes(ref_state(cloud, v), moments) and m.size()[1] == len(cloud)
    m.close()
    # 4 096 records over 8 new keys in one call: every lane of a wavefront creates or finds one of them at the same time
    rng = np.random.Generator(np.random.PCG64(10))
    keys = np.array([[0, 0, 0], [0, 0, 1], [-7, 3, 2], [2**20 - 1, 0, 0], [-(2**20) + 1, 5, 5], [100, -100, 100], [1, 1, 1], [1, 1, 2]], np.int32)
    few = np.zeros(4096, R.MAP_VOXEL)
    few["key"] = keys[rng.integers(0, 8, 4096)]
    few["count"] = rng.integers(1, 1000, 4096)
    few["sum"] = rng.integers(-(2**40), 2**40, (4096, 3))
    few_mom = rng.integers(-(2**45), 2**45, (4096, 9))
    w_vox, w_mom, w_rej = MS.absorb_ref([(few, few_mom)], moments)
    m = new_map(gpu, v, moments)
    assert m.absorb(few, few_mom) == w_rej == 0
    assert state_bytes(m) == want_bytes((w_vox, w_mom), moments) and m.size() == (8, int(few["count"].sum()))
    m.close()


def test_record_counts_around_a_wavefront_and_a_workgroup(gpu, cloud):
    vox, mom = ref_state(cloud, 0.2)
    for n in (1, 63, 64, 65, 255, 256, 257):
        m = new_map(gpu, 0.2, True)
        assert m.absorb(vox[:n], mom[:n]) == 0
        assert state_bytes(m) == want_bytes((vox[:n], mom[:n]), True) and m.size() == (n, int(vox["count"][:n].sum()))
        m.close()


@pytest.mark.parametrize("moments", [False, True])
def test_grid_size_and_repetition_change_no_byte(gpu, cloud, moments):
    vox, mom = ref_state(cloud, 0.2)
    got = []
    try:
        for groups in (1, 7, 0, 0):
            gpu.set_dev_option("map_absorb_groups", groups)
            m = new_map(gpu, 0.2, moments)
            assert m.absorb(vox, mom) == 0
            got.append(state_bytes(m))
            m.close()
    finally:
        gpu.set_dev_option("map_absorb_groups", 0)
    assert all(g == want_bytes((vox, mom), moments) for g in got)


@pytest.mark.parametrize("moments", [False, True])
def test_rejected_records_are_counted_and_not_applied(gpu, cloud, moments):
    vox, mom = (x[:500].copy() for x in ref_state(cloud, 0.2))
    bad = {3: ("key", 0, 2**20), 77: ("key", 1, -(2**20)), 130: ("key", 2, 2**20), 131: ("count", None, 0), 400: ("count", None, 2**30 + 1)}
    for i, (f, axis, val) in bad.items():
        if axis is None:
            vox[f][i] = val
        else:
            vox[f][i][axis] = val
    vox["count"][401] = 2**30  # (the largest count a record may carry)
    w_vox, w_mom, w_rej = MS.absorb_ref([(vox, mom)], moments)
    assert w_rej == len(bad) and len(w_vox) == 500 - len(bad)
    m = new_map(gpu, 0.2, moments)
    assert m.insert(np.array([[np.nan, 0, 0]], np.float32)) == 1 and m.info()["rejected"] == 1  # (a rejected POINT: another counter)
    assert m.absorb(vox, mom) == w_rej
    assert m.info()["rejected"] == 1
    assert state_bytes(m) == want_bytes((w_vox, w_mom), moments)
    assert m.size() == (len(w_vox), int(w_vox["count"].astype(np.int64).sum()))
    assert m.absorb(vox[:3], mom[:3]) == 0 and m.absorb(vox[3:4], mom[3:4]) == 1  # (this call's count, not a running one)
    m.close()


def test_flag_combinations(gpu, cloud):
    v = 0.2
    vox, mom = ref_state(cloud, v)
    plain, full = new_map(gpu, v, False), new_map(gpu, v, True)
    assert plain.absorb(vox, mom) == 0  # a moments state into a plain map: the moments are ignored
    assert state_bytes(plain) == vox.tobytes()
    inserted = new_map(gpu, v, False, cloud)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(plain.export(), inserted.export()))
    assert full.absorb(vox, mom) == 0
    dst = new_map(gpu, v, False)
    dst.merge(full)  # a moments src into a plain dst
    assert state_bytes(dst) == vox.tobytes() and state_bytes(full) == want_bytes((vox, mom), True)
    with pytest.raises(L.WildcatError) as e:
        full.merge(plain)  # a moments dst needs moments
    assert e.value.code == WC_ERR_ARG
    with pytest.raises(L.WildcatError) as e:
        full.absorb(vox, None)
    assert e.value.code == WC_ERR_ARG
    assert state_bytes(full) == want_bytes((vox, mom), True)  # (the refused calls changed nothing)
    d_vox, d_mom = gpu.alloc(40 * len(vox)), gpu.alloc(72 * len(vox))
    assert plain.state_device(d_vox, d_mom, len(vox))[0] == WC_ERR_ARG
    assert plain.state_device(d_vox, None, len(vox)) == (0, len(vox))
    assert full.state_device(d_vox, None, len(vox)) == (0, len(vox))  # (the moments are optional on a moments map)
    assert d_vox.download(R.MAP_VOXEL, len(vox)).tobytes() == vox.tobytes()
    for b in (d_vox, d_mom):
        b.free()
    for m in (plain, full, dst, inserted):
        m.close()


def test_argument_errors(gpu, cloud):
    v = 0.2
    vox, mom = ref_state(cloud, v)
    n = len(vox)
    m = new_map(gpu, v, True, cloud)
    before = state_bytes(m)
    d_vox, d_mom = gpu.alloc(40 * n + 8), gpu.alloc(72 * n + 8)
    assert m.state_device(Shifted(d_vox, 4), d_mom, n)[0] == WC_ERR_ARG
    assert m.state_device(d_vox, Shifted(d_mom, 4), n)[0] == WC_ERR_ARG
    assert m.state_device(d_vox, d_mom, n - 1) == (WC_ERR_CAPACITY, n)
    assert m.state_device(None, None, 0) == (WC_ERR_CAPACITY, n)
    assert m.state_device(None, None, n)[0] == WC_ERR_ARG
    assert m.state_device(Shifted(d_vox, 8), Shifted(d_mom, 8), n) == (0, n)
    d_vox.upload(vox), d_mom.upload(mom)
    for args in ((Shifted(d_vox, 4), d_mom), (d_vox, Shifted(d_mom, 4)), (None, d_mom)):
        with pytest.raises(L.WildcatError) as e:
            m.absorb_device(*args, n)
        assert e.value.code == WC_ERR_ARG
    with pytest.raises(L.WildcatError) as e:
        m.merge(m)
    assert e.value.code == WC_ERR_ARG
    other_v = new_map(gpu, 0.25, True, cloud[:100])
    with pytest.raises(L.WildcatError) as e:
        m.merge(other_v)
    assert e.value.code == WC_ERR_ARG
    ctx2 = L.Context(0)
    foreign = ctx2.map_create(v, moments=True)
    try:
        for dst, src in ((m, foreign), (foreign, m)):
            assert gpu.lib.wc_map_merge(gpu.h, dst.h, src.h) == WC_ERR_ARG
        n_out = C.c_uint64(0)
        assert gpu.lib.wc_map_absorb(gpu.h, foreign.h, None, None, C.c_uint64(0), None) == WC_ERR_ARG
        assert gpu.lib.wc_map_export_state(gpu.h, foreign.h, None, None, C.c_uint64(0), C.byref(n_out)) == WC_ERR_ARG
        assert foreign.state_device(None, None, 0) == (0, 0)  # (through its own context)
    finally:
        foreign.close()
        ctx2.close()
    assert state_bytes(m) == before and m.size() == (n, len(cloud))
    # nothing to do is no error: n = 0 (no pointer is looked at), an empty map as either side of a merge, the state of an empty map
    empty = new_map(gpu, v, True)
    assert m.absorb_device(None, None, 0) == 0 and m.absorb(vox[:0], mom[:0]) == 0
    e_vox, e_mom = empty.state()
    assert len(e_vox) == 0 and e_mom.shape == (0, 9) and empty.state_device(None, None, 0) == (0, 0)
    m.merge(empty)
    assert state_bytes(m) == before
    empty.merge(m)
    assert state_bytes(empty) == before and empty.size() == m.size()
    for b in (d_vox, d_mom):
        b.free()
    for x in (m, other_v, empty):
        x.close()


@pytest.mark.parametrize("moments", [False, True])
def test_an_absorbed_map_is_an_ordinary_map(gpu, cloud, moments):
    v = 0.2
    first, rest = cloud[:12000], cloud[12000:]
    a = new_map(gpu, v, moments, reserve_voxels=1)
    vox, mom = MS.state_of(first, v)
    assert a.absorb(vox, mom) == 0 and a.insert(rest) == 0
    b = new_map(gpu, v, moments, cloud)
    assert state_bytes(a) == state_bytes(b) == want_bytes(ref_state(cloud, v), moments) and a.size() == b.size()
    sweep = cloud[:5000]
    res = a.carve(sweep, ORIGIN, np.inf, shell=1, min_rays=1)
    assert res == b.carve(sweep, ORIGIN, np.inf, shell=1, min_rays=1) and res["rays_used"] > 0 and res["steps"] > 0
    (hits_a, res_a), (hits_b, res_b) = (m.raycast(sweep, ORIGIN, np.inf, end_shell=1) for m in (a, b))
    assert hits_a.tobytes() == hits_b.tobytes() and res_a == res_b and res_a["hits"] > 0
    # ... and a merged one: more points after the merge
    c, d = new_map(gpu, v, moments, cloud[:6000]), new_map(gpu, v, moments, cloud[6000:12000])
    c.merge(d)
    assert c.insert(rest) == 0 and state_bytes(c) == state_bytes(b) and c.size() == b.size()
    for m in (a, b, c, d):
        m.close()


def test_facade_saves_and_loads_the_canonical_file(gpu, cloud, tmp_path):
    v = 0.2
    vox, mom = ref_state(cloud, v)
    canonical = MS.encode_ref(v, vox, mom)
    path = lambda name: str(tmp_path / name)  # noqa: E731

    def write(name, data):
        open(path(name), "wb").write(data)
        return path(name)

    def facade(surfels=True):
        odo = L.Odometry(0)
        odo.set_map_voxel(v)
        odo.set_map_surfels(surfels)
        return odo

    no_map = L.Odometry(0)
    assert not no_map.map_save(path("none.bin")) and not no_map.map_load(write("whole.bin", canonical))
    no_map.close()
    a = facade()
    assert a.map_load(path("whole.bin")) and a.map_size() == (len(vox), len(cloud), 0)
    ref = gpu.map_create(v, moments=True)
    assert ref.insert(cloud) == 0
    xyz, cnt, _ = ref.export()
    assert a.map_export()[0].tobytes() == xyz.tobytes() and a.map_export()[1].tobytes() == cnt.tobytes()
    assert a.map_surfels().tobytes() == ref.surfels().tobytes()
    ref.close()
    assert a.map_save(path("saved.bin")) and open(path("saved.bin"), "rb").read() == canonical
    b = facade()  # a fresh facade with the same settings
    assert b.map_load(path("saved.bin"))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.map_export(), b.map_export()))
    assert a.map_surfels().tobytes() == b.map_surfels().tobytes() and len(b.map_surfels()) == len(vox)
    # the same sweeps in another order: the same file
    sweeps = [write("sweep%d.bin" % j, MS.encode_ref(v, *MS.state_of(cloud[j::3], v))) for j in range(3)]
    for odo, order, out in ((a, (0, 1, 2), "order_a.bin"), (b, (2, 0, 1), "order_b.bin")):
        for j, s in enumerate(order):
            assert odo.map_load(sweeps[s], merge=j > 0)
        assert odo.map_save(path(out))
    assert open(path("order_a.bin"), "rb").read() == open(path("order_b.bin"), "rb").read() == canonical
    # merge = True on top of the same map doubles every count and sum
    assert b.map_load(path("saved.bin"), merge=True) and b.map_save(path("double.bin"))
    code, v2, flags, vox2, mom2 = MS.decode_ref(open(path("double.bin"), "rb").read())
    assert code == MS.OK and v2 == v and flags == 1 and np.array_equal(vox2["key"], vox["key"])
    assert np.array_equal(vox2["count"], 2 * vox["count"]) and np.array_equal(vox2["sum"], 2 * vox["sum"]) and np.array_equal(mom2, 2 * mom)
    # refused files leave the map as it is
    before = [x.tobytes() for x in b.map_export()] + [b.map_surfels().tobytes()]
    corrupt = bytearray(canonical)
    corrupt[64 + 40 * 17 + 20] ^= 4
    for name, data in (("other_voxel.bin", MS.encode_ref(0.25, vox, mom)), ("plain.bin", MS.encode_ref(v, vox, None)),
                       ("corrupt.bin", bytes(corrupt)), ("short.bin", canonical[:-1])):
        for merge in (False, True):
            assert not b.map_load(write(name, data), merge=merge), (name, merge)
    assert not b.map_load(path("missing.bin"))
    assert [x.tobytes() for x in b.map_export()] + [b.map_surfels().tobytes()] == before
    # a facade without map_surfels takes either kind of file (the moments are dropped) and writes a plain one
    a.set_map_surfels(False)
    for name in ("saved.bin", "plain.bin"):
        assert a.map_load(path(name)) and a.map_export()[0].tobytes() == xyz.tobytes() and a.map_export()[1].tobytes() == cnt.tobytes()
        assert a.map_save(path("plain_out.bin")) and open(path("plain_out.bin"), "rb").read() == MS.encode_ref(v, vox, None)
    a.close(), b.close()
