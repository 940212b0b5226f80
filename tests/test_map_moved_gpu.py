"""A map built in another frame merged under a rigid pose, on the device (include/wildcat_hip.h: wc_map_merge_moved; csrc/map.hip:
k_map_merge_moved): the destination's state byte for byte against map_moved_ref.py and against wc_map_absorb of
wc_map_move_state's output - source sizes at the table's and the workgroup's edges, empty, overlapping and growing destinations, a turn
that sends several voxels into one, the flag combinations, tombstones on either side, the four counts, rejected keys, repetition and slot
order -, the moved map in use, every refusal, and the facade's MergeMapFile against the direct calls."""
import ctypes as C

import numpy as np
import pytest

import map_moved_ref as MM
import map_register_ref as G
import map_state_ref as MS
import map_surfel_ref as S
from helpers import xyz_of
from test_map_register_ref import true_pose
from wildcat_slam_amd import lib as L
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

pytestmark = pytest.mark.gpu

V = 0.2
VS = float(np.float32(0.8))
WC_ERR_ARG = 11


def pose10():
    return MM.pose_of(10.0, (1.0, 2.0, 3.0), (0.37, -1.2, 0.05))


def turn45():
    return MM.pose_of(45.0, (0.0, 0.0, 1.0), (0.1, 0.0, 0.0))


@pytest.fixture(scope="module")
def cloud():
    return xyz_of(synth.g1_room(20000, seed=3))


@pytest.fixture(scope="module")
def state(cloud):
    """the restated state of the cloud at v = 0.2, with moments: about 8300 voxels in ascending key order"""
    return MS.state_of(cloud, V)


def part(state, n, start=0):
    return state[0][start:start + n].copy(), state[1][start:start + n].copy()


def map_of(gpu, st, v=V, moments=True, reserve=0, order=None):
    """a map that holds the state st (absorbed; order: a permutation of its records)"""
    m = gpu.map_create(v, moments=moments, reserve_voxels=reserve)
    vox, mom = st
    if order is not None:
        vox, mom = vox[order], (None if mom is None else mom[order])
    if len(vox):
        assert m.absorb(vox, mom if moments else None) == 0
    return m


def state_bytes(m):
    vox, mom = m.state()
    return vox.tobytes() + (mom.tobytes() if mom is not None else b"")


def want_bytes(vox, mom):
    return vox.tobytes() + (mom.tobytes() if mom is not None else b"")


def check_merge(gpu, dst_st, src_st, T, v=V, dst_moments=True, src_moments=True, reserve=0, want_counts=True):
    """wc_map_merge_moved of map(src_st) into map(dst_st) == the restatement == wc_map_absorb of wc_map_move_state's records; the four
    counts; src byte-equal before and after; dst's voxel and point counts -> (the merged state, the counts)"""
    plain = lambda st: (st[0], None)  # noqa: E731
    dst_st, src_st = (dst_st if dst_moments else plain(dst_st)), (src_st if src_moments else plain(src_st))
    want_vox, want_mom, want_n = MM.merge_moved_ref(dst_st, src_st, v, T, moments=dst_moments)
    dst, src = map_of(gpu, dst_st, v, dst_moments, reserve), map_of(gpu, src_st, v, src_moments)
    src_before = state_bytes(src)
    got_n = dst.merge_moved(src, T, want_counts=want_counts)
    assert got_n == (want_n if want_counts else None)
    assert state_bytes(dst) == want_bytes(want_vox, want_mom)
    assert dst.size() == (len(want_vox), int(want_vox["count"].astype(np.int64).sum()))
    assert state_bytes(src) == src_before
    # the host route: the moved records, absorbed
    via = map_of(gpu, dst_st, v, dst_moments, reserve)
    mv, mm, n_rej = L.map_move_state(src_st[0], src_st[1] if dst_moments else None, v, T)
    assert n_rej == want_n[2] and via.absorb(mv, mm) == n_rej
    assert state_bytes(via) == want_bytes(want_vox, want_mom) and via.size() == dst.size()
    for m in (dst, src, via):
        m.close()
    return (want_vox, want_mom), want_n


EMPTY = (np.zeros(0, R.MAP_VOXEL), np.zeros((0, 9), np.int64))


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 3000])
def test_into_an_empty_map(gpu, state, n):
    """source tables of 2 .. 8192 slots: one workgroup and several"""
    (vox, _), counts = check_merge(gpu, EMPTY, part(state, n, 2000), pose10())
    assert counts == [n, int(state[0]["count"][2000:2000 + n].sum()), 0, 0] and len(vox) <= n and (n == 0 or len(vox) > n // 2)


def test_into_a_map_that_holds_overlapping_voxels(gpu, state, cloud):
    """dst: the map of the moved POINTS of the same part of the room, so most moved voxels meet a voxel that exists"""
    src = part(state, 3000, 2000)
    T = pose10()
    keys = {tuple(k) for k in src[0]["key"]}
    pts = cloud[[tuple(k) in keys for k in np.floor(cloud.astype(np.float64) / V).astype(np.int64)]]
    dst = MS.state_of(G.transform(pts, T), V)
    (vox, _), counts = check_merge(gpu, dst, src, T)
    assert counts[0] == 3000 and len(vox) < len(dst[0]) + 3000 // 2  # (more than half of the moved voxels found their voxel there)


def test_into_a_map_that_must_grow(gpu, state):
    dst = part(state, 40, 0)
    m = map_of(gpu, dst, reserve=1)
    cap0, growths0 = m.info()["slots"], m.info()["growths"]
    src = map_of(gpu, part(state, 3000, 2000))
    assert m.merge_moved(src, pose10())[0] == 3000
    assert m.info()["slots"] >= 2 * 3000 > cap0 and m.info()["growths"] > growths0
    m.close(), src.close()
    check_merge(gpu, dst, part(state, 3000, 2000), pose10(), reserve=1)


def test_a_turn_sends_several_voxels_into_one(gpu, state):
    src = part(state, 3000, 2000)
    (vox, _), counts = check_merge(gpu, EMPTY, src, turn45())
    assert counts[0] == 3000 and len(vox) < 3000 - 100  # (asserted: hundreds of source voxels share a destination voxel)
    assert int(vox["count"].sum()) == int(src[0]["count"].sum())


@pytest.mark.parametrize("dst_moments,src_moments", [(True, True), (False, True), (False, False)])
def test_flag_combinations_that_pass(gpu, state, dst_moments, src_moments):
    check_merge(gpu, part(state, 300, 2100), part(state, 600, 2000), pose10(), dst_moments=dst_moments, src_moments=src_moments)


def test_tombstones_on_either_side(gpu, state):
    T = pose10()
    src_st, dst_st = part(state, 600, 2000), part(state, 300, 2100)
    gone_src, gone_dst = np.arange(0, 600, 3), np.arange(0, 300, 2)
    keep = lambda st, gone: tuple(np.delete(x, gone, axis=0) for x in st)  # noqa: E731
    want_vox, want_mom, want_n = MM.merge_moved_ref(keep(dst_st, gone_dst), keep(src_st, gone_src), V, T)
    src, dst = map_of(gpu, src_st), map_of(gpu, dst_st)
    assert src.remove(src_st[0]["key"][gone_src])["voxels_removed"] == len(gone_src) and src.tombstones()[0] == len(gone_src)
    assert dst.remove(dst_st[0]["key"][gone_dst])["voxels_removed"] == len(gone_dst) and dst.tombstones()[0] == len(gone_dst)
    src_before = state_bytes(src)
    assert dst.merge_moved(src, T) == want_n and want_n[0] == 400
    assert state_bytes(dst) == want_bytes(want_vox, want_mom) and state_bytes(src) == src_before
    src.close(), dst.close()


def test_the_null_form_returns_no_counts(gpu, state):
    check_merge(gpu, part(state, 300, 2100), part(state, 600, 2000), pose10(), want_counts=False)


@pytest.mark.parametrize("sign", [1, -1])
def test_keys_beyond_the_range_are_counted_and_not_applied(gpu, state, sign):
    src = part(state, 600, 2000)
    ky = src[0]["key"][:, 1].astype(np.int64)  # (600 consecutive records share k_x; k_y takes some 37 values)
    mid = int(np.median(ky))
    T = np.eye(3, 4)
    T[1, 3] = (sign * 2**20 - mid) * V  # (the voxels at and beyond the median land at |K_y| >= 2^20, or - for the negative end - under it)
    (vox, _), counts = check_merge(gpu, part(state, 10, 0), src, T)
    assert counts[0] > 50 and counts[2] > 50 and counts[0] + counts[2] == 600
    assert counts[1] + counts[3] == int(src[0]["count"].sum()) and np.abs(vox["key"]).max() == 2**20 - 1


def test_repetition_and_slot_order_change_no_byte(gpu, state):
    src_st, dst_st, T = part(state, 3000, 2000), part(state, 300, 2100), turn45()
    rng = np.random.default_rng(11)
    results = []
    for order, reserve in ((None, 0), (None, 0), (rng.permutation(3000), 0), (rng.permutation(3000), 20000)):
        src, dst = map_of(gpu, src_st, reserve=reserve, order=order), map_of(gpu, dst_st)
        results.append((dst.merge_moved(src, T), state_bytes(dst), src.info()["slots"]))
        src.close(), dst.close()
    assert all(r[:2] == results[0][:2] for r in results) and results[3][2] > results[0][2]  # (another table size: other slots)


def test_the_moved_map_in_use(gpu, state, cloud):
    """PointMap.moved(T) + nearest_plane against the restatement's records: the voxel found, its count, centroid and distance exactly,
    the plane's variance within the export's own bounds"""
    src_st, T = part(state, 3000, 2000), pose10()
    src = map_of(gpu, src_st)
    moved = src.moved(T)
    assert moved.voxel == V and moved.moments
    want_vox, want_mom, _ = MM.merge_moved_ref(EMPTY, src_st, V, T)
    assert state_bytes(moved) == want_bytes(want_vox, want_mom)
    surf = MM.surfels_of_state(want_vox, want_mom, V)
    q = surf["xyz"][::5] + np.random.default_rng(5).normal(0, 0.03, (len(surf[::5]), 3)).astype(np.float32)
    want, idx = S.plane_hits(surf, q, V, 0.3, 3)
    got = moved.nearest_plane(q, 0.3, 3)
    for f in ("xyz", "count", "key", "flags", "d2"):
        assert got[f].tobytes() == want[f].tobytes(), f
    planes = (got["flags"] & 2) != 0
    assert planes.sum() > 100
    # sigma2: the export's eigenvalue bound, 32 x 2^-53 of the scale, plus its covariance's 2 ulp per entry against the restatement's
    # correctly rounded one: |dC|_F <= 3 x 4 x 2^-53 max |C_ab| <= 12 x 2^-53 ev[2]
    scale = surf["ev"][np.maximum(idx, 0)][:, 2]
    assert (np.abs(got["sigma2"] - want["sigma2"])[planes] <= 44 * 2.0**-53 * scale[planes]).all()
    plain = map_of(gpu, (src_st[0], None), moments=False).moved(T)
    assert not plain.moments and state_bytes(plain) == want_vox.tobytes()
    for m in (src, moved, plain):
        m.close()


def test_every_refusal_leaves_dst_and_h_out_untouched(gpu, state):
    src_st, dst_st = part(state, 300, 2000), part(state, 100, 2100)
    dst, src = map_of(gpu, dst_st), map_of(gpu, src_st)
    plain_src, other_v = map_of(gpu, (src_st[0], None), moments=False), map_of(gpu, EMPTY, v=0.25)
    ctx2 = L.Context(0)
    foreign = ctx2.map_create(V, moments=True)
    before = state_bytes(dst)
    good = np.ascontiguousarray(pose10().reshape(-1))

    def bad_T(k, x):
        T = good.copy()
        T[k] = x
        return T

    scaled = good.copy()
    scaled[[0, 1, 2, 4, 5, 6, 8, 9, 10]] *= 1.0 + 1e-8
    cases = [(dst, dst, good), (dst, foreign, good), (foreign, src, good), (dst, other_v, good), (dst, plain_src, good), (dst, src, None),
             (dst, src, bad_T(3, float("nan"))), (dst, src, bad_T(5, float("inf"))), (dst, src, bad_T(1, good[1] + 1e-8)), (dst, src, scaled),
             (dst, src, np.zeros(12))]
    try:
        for d, s, T in cases:
            for with_out in (True, False):
                out = (C.c_uint64 * 4)(71, 72, 73, 74)
                rc = gpu.lib.wc_map_merge_moved(gpu.h, d.h, s.h, None if T is None else R.ptr(T), out if with_out else None)
                assert rc == WC_ERR_ARG and list(out) == [71, 72, 73, 74]
        with pytest.raises(L.WildcatError) as e:
            dst.merge_moved(plain_src, good)
        assert e.value.code == WC_ERR_ARG
        with pytest.raises(L.WildcatError):
            src.moved(scaled)
        assert state_bytes(dst) == before and dst.size() == (100, int(dst_st[0]["count"].sum()))
        # an empty source is no error: four zeros, nothing changes
        empty = map_of(gpu, EMPTY)
        assert dst.merge_moved(empty, good) == [0, 0, 0, 0] and state_bytes(dst) == before
        empty.close()
    finally:
        foreign.close()
        ctx2.close()
    for m in (dst, src, plain_src, other_v):
        m.close()


# ---- the facade -------------------------------------------------------------------------------------------------------------------
def summary_bytes(s):
    return np.array([s["initial_cost"], s["final_cost"]]).tobytes() + s["last_step"].tobytes() + repr(
        (s["iterations"], s["termination"], s["n_used"], s["n_found"])).encode()


def facade(v, path=None, surfels=True):
    odo = L.Odometry(0)
    odo.set_map_voxel(v)
    odo.set_map_surfels(surfels)
    if path is not None:
        assert odo.map_load(path)
    return odo


def facade_state(odo, path):
    assert odo.map_save(path)
    return open(path, "rb").read()


def test_facade_merges_a_file_of_another_frame(gpu, tmp_path):
    """the room in frame A is the facade's map; the same room saved in frame B, 2 degrees and 6 cm away; MergeMapFile from identity"""
    path = lambda name: str(tmp_path / name)  # noqa: E731
    T_ab = true_pose()  # B -> A
    room_a = xyz_of(synth.g1_room(60_000))
    room_b = ((room_a.astype(np.float64) - T_ab[:, 3]) @ T_ab[:, :3]).astype(np.float32)
    st_a, st_b = MS.state_of(room_a, VS), MS.state_of(room_b, VS)
    open(path("a.bin"), "wb").write(MS.encode_ref(VS, *st_a))
    open(path("b.bin"), "wb").write(MS.encode_ref(VS, *st_b))
    factor, n_levels = 2, 2
    finest = L.map_align_opts(L.map_reg_params(VS, 3), max_iterations=20, tol_rot=G.TOL_ROT, tol_trans=G.TOL_TRANS)
    odo = facade(VS, path("a.bin"))
    res = odo.map_merge_file(path("b.bin"), np.eye(3, 4), factor, n_levels, finest)
    assert res is not None and odo.map_ms() > 0.0
    T_odo, s_odo = res
    # the direct calls: the file's centroids through the same levels, then wc_map_merge_moved with that pose
    map_a, map_b = map_of(gpu, st_a, VS), map_of(gpu, st_b, VS)
    xyz_b = map_b.export()[0]
    levels = map_a.pyramid(factor, n_levels)[::-1]
    opts = [L.map_align_opts(L.map_reg_params(VS * float(factor) ** l, 3), max_iterations=20, tol_rot=G.TOL_ROT, tol_trans=G.TOL_TRANS)
            for l in range(n_levels)][::-1]
    T_ref, s_ref = L.map_align_pyramid(levels, xyz_b, np.eye(3, 4), opts)
    for m in levels[:-1]:
        m.close()
    assert T_odo.tobytes() == T_ref.tobytes() and [summary_bytes(s) for s in s_odo] == [summary_bytes(s) for s in s_ref]
    assert s_odo[-1]["termination"] in (0, 1) and s_odo[-1]["n_used"] > 1000
    e_rot, e_tr = G.pose_error(T_odo, T_ab)
    print("facade: pose error", e_rot, e_tr, "iterations", [s["iterations"] for s in s_odo])
    assert e_rot < np.deg2rad(0.1) and e_tr < 0.02  # (from 2 degrees and 6 cm: found, not merely returned)
    counts = map_a.merge_moved(map_b, T_ref)
    assert counts == [len(st_b[0]), 60_000, 0, 0]
    assert facade_state(odo, path("merged.bin")) == MS.encode_ref(VS, *map_a.state())
    assert odo.map_size()[:2] == map_a.size() and map_a.size()[1] == 120_000
    merged = facade_state(odo, path("merged.bin"))
    # false returns: each leaves the map and the pose as they were
    open(path("other_voxel.bin"), "wb").write(MS.encode_ref(0.25, *MS.state_of(room_b[:2000], 0.25)))
    open(path("plain.bin"), "wb").write(MS.encode_ref(VS, st_b[0], None))
    for name, f, nl in (("missing.bin", factor, n_levels), ("other_voxel.bin", factor, n_levels), ("plain.bin", factor, n_levels),
                        ("b.bin", factor, 0), ("b.bin", factor, 9), ("b.bin", 0, 2), ("b.bin", 3, 3)):
        assert odo.map_merge_file(path(name), np.eye(3, 4), f, nl, finest) is None, name
    assert facade_state(odo, path("after.bin")) == merged
    odo.set_map_surfels(False)
    assert odo.map_merge_file(path("b.bin"), np.eye(3, 4), factor, n_levels, finest) is None
    odo.close()
    map_a.close(), map_b.close()


def test_facade_refuses_a_single_wall(gpu, tmp_path):
    """a wall alone leaves three pose directions free: the alignment ends with termination 2 and nothing is merged"""
    path = lambda name: str(tmp_path / name)  # noqa: E731
    v = G.HAND_V
    off = (0.125, 0.25, 0.375)
    wall = np.array([[i * v + a, j * v + b, G.HAND_FACE] for i in range(1, 9) for j in range(1, 9) for a in off for b in off], np.float32)
    shifted = (wall.astype(np.float64) - np.array([0.0, 0.0, 1 / 64])).astype(np.float32)
    open(path("wall.bin"), "wb").write(MS.encode_ref(v, *MS.state_of(wall, v)))
    open(path("shifted.bin"), "wb").write(MS.encode_ref(v, *MS.state_of(shifted, v)))
    opts = L.map_align_opts(L.map_reg_params(v, 3, sigma0=2.0**-4))
    m, other = map_of(gpu, MS.state_of(wall, v), v), map_of(gpu, MS.state_of(shifted, v), v)
    _, summ = m.align(other.export()[0], np.eye(3, 4), opts)
    assert summ["termination"] == 2 and summ["n_used"] == 64  # (the direct call: enough points, no unique pose)
    m.close(), other.close()
    odo = facade(v, path("wall.bin"))
    before = facade_state(odo, path("before.bin"))
    assert odo.map_merge_file(path("shifted.bin"), np.eye(3, 4), 2, 1, opts) is None
    assert facade_state(odo, path("after.bin")) == before
    odo.close()
