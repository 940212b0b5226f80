"""The occupancy score of pose hypotheses on the device (include/wildcat_hip.h: wc_map_score_batch; csrc/map.hip: k_map_score_batch;
DESIGN 8.11): every record byte for byte against the numpy restatement of map_score_ref.py - which takes nothing from the library but the
map's exported keys and counts -, a crowded table with removed voxels, planted cases with known counts, the refusals, and the scene of
tests/test_map_score_ref.py through the facade."""
import ctypes as C

import numpy as np
import pytest

import map_coarsen_ref as MC
import map_register_ref as G
import map_score_ref as SC
import map_search_ref as MS
import map_state_ref
from helpers import point_records
from helpers import xyz_of as _xyz
from test_map_coarsen_gpu import new_map, summary_bytes
from wildcat_slam_amd import lib as L
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

pytestmark = pytest.mark.gpu

WC_ERR_CAPACITY, WC_ERR_ARG = 1, 11
BLOCK = 32  # csrc/map.hip: kScoreBlock, the hypotheses one work item walks with its tile


def eye(t=(0.0, 0.0, 0.0)):
    return np.concatenate([np.eye(3), np.array(t, np.float64).reshape(3, 1)], 1)


def test_records_equal_the_restatement_byte_for_byte(gpu):
    """ONE map; n = 1 .. 8193 (33 tiles: several workgroups add to one counter) and K = 1 .. 1025 - the kernel's hypothesis block and its
    neighbours among them - in an order in which both grow and shrink; strides 12 and 48; map_score_groups 0, 1, 7; min_points 1 and 3;
    the first configuration once again at the end"""
    m = new_map(gpu, SC.EQ_V, False, SC.eq_cloud())
    _, counts, keys = m.export()
    assert len(keys) == len(SC.voxels_of(SC.eq_cloud(), SC.EQ_V)[0])
    scan, Ts = SC.eq_scan(), SC.eq_poses()
    want = {mp: SC.flags(keys, counts, SC.EQ_V, scan, Ts, mp) for mp in (1, 3)}
    full = SC.records_of(want[1], SC.EQ_N, SC.EQ_K)
    assert full["n_bad"][SC.EQ_BAD] == SC.EQ_N - 2 and full["n_in"][SC.EQ_OUT] == 0 and full["n_in"][0] == SC.EQ_N - 2
    assert full["n_hit"][SC.EQ_FLOAT] < full["n_hit"][0] > SC.records_of(want[3], SC.EQ_N, 1)["n_hit"][0] > 0
    bufs = [gpu.to_device(scan), gpu.to_device(point_records(scan))]
    order = [(257, 33), (8193, 1025), (1, 1), (256, BLOCK), (63, 2), (8193, BLOCK + 1), (64, 1025), (255, BLOCK - 1), (65, 33), (8193, 1), (1, 1025)]
    try:
        for groups in (0, 1, 7):
            gpu.set_dev_option("map_score_groups", groups)
            for b, stride in zip(bufs, (12, 48)):
                for j, (n, K) in enumerate(order):
                    mp = (1, 3)[(j + groups) % 2]
                    got = m.score_batch_device(R.Points(b.ptr, 0, stride, 0, n), Ts[:K], mp)
                    assert got.dtype == R.MAP_SCORE and got.tobytes() == SC.records_of(want[mp], n, K).tobytes(), (groups, stride, n, K, mp)
        gpu.set_dev_option("map_score_groups", 0)
        n, K = order[0]
        again = m.score_batch_device(R.Points(bufs[0].ptr, 0, 12, 0, n), Ts[:K], 1)
        assert again.tobytes() == SC.records_of(want[1], n, K).tobytes()
        assert m.score_batch(scan[:300], Ts[:5], 3).tobytes() == SC.records_of(want[3], 300, 5).tobytes()  # (the uploading form)
    finally:
        gpu.set_dev_option("map_score_groups", 0)
        for b in bufs:
            b.free()
        m.close()


def test_a_crowded_table_with_removed_voxels(gpu):
    """2048 voxels in 4096 slots - the fullest a table gets before it grows -, every third removed in place: the removed ones stop
    counting, and the voxels whose probe chain passes a tombstone still count (tests/test_map_score_ref.py: a chain that ended there
    would lose 150 of the 1365 in a table of this content)"""
    ck = SC.crowd_keys()
    pts, poses = SC.centres(ck, SC.CROWD_V), SC.crowd_poses()
    m = gpu.map_create(SC.CROWD_V, reserve_voxels=SC.CROWD_M)
    assert m.insert(pts) == 0 and m.info()["slots"] == 2 * SC.CROWD_M and m.info()["growths"] == 0 and m.size()[0] == SC.CROWD_M
    before = m.score_batch(pts, poses)
    assert before["n_hit"][0] == SC.CROWD_M
    assert before.tobytes() == SC.score_fast(ck, np.ones(SC.CROWD_M), SC.CROWD_V, pts, poses).tobytes()
    gone = ck[::3]
    assert m.remove(gone)["voxels_removed"] == len(gone) and m.tombstones()[0] == len(gone) and m.info()["slots"] == 2 * SC.CROWD_M
    _, counts, keys = m.export()
    got = m.score_batch(pts, poses)
    assert got.tobytes() == SC.score_fast(keys, counts, SC.CROWD_V, pts, poses).tobytes()
    assert got["n_hit"][0] == SC.CROWD_M - len(gone) and np.all(got["n_in"] == SC.CROWD_M)
    only_gone = m.score_batch(SC.centres(gone, SC.CROWD_V), poses[:1])
    assert only_gone["n_hit"][0] == 0 and only_gone["n_in"][0] == len(gone)
    m.close()


def test_planted_cases_with_known_counts(gpu):
    v, n = 0.5, 300
    rng = np.random.default_rng(31)
    flat = rng.permutation(20**3)[:n]
    ck = np.stack([flat // 400, (flat // 20) % 20, flat % 20], 1) * 2 - 20  # (even indices: every odd voxel is empty)
    pts = SC.centres(ck, v)
    maps = [new_map(gpu, v, moments, pts) for moments in (False, True)]
    far = eye((1e39, 0.0, 0.0))
    poses = np.stack([eye(), eye((v, 0.0, 0.0)), far, eye((0.0, 0.0, -v)), eye()])
    got = [m.score_batch(pts, poses) for m in maps]
    assert got[0].tobytes() == got[1].tobytes()  # (a plain map and a moments map)
    assert got[0]["n_hit"].tolist() == [n, 0, 0, 0, n] and got[0]["n_in"].tolist() == [n, n, 0, n, n]
    assert got[0]["n_bad"].tolist() == [0, 0, n, 0, 0] and not got[0]["reserved"].any()
    # min_points: every voxel holds one point
    assert maps[0].score_batch(pts, poses[:1], 2)["n_hit"][0] == 0
    # the key range: a translation that puts every index at +-2^20 exactly, and one voxel inside
    # (every coordinate 4.75; the sums below are exact in double and in float: q = 524288.25, -524288, 524287.75, -524287.5 on every axis,
    # index 2^20, -2^20, 2^20 - 1, -(2^20 - 1))
    one = np.full((n, 3), 4.75, np.float32)
    out = maps[0].score_batch(one, [eye((524283.5,) * 3), eye((-524292.75,) * 3), eye((524283.0,) * 3), eye((-524292.25,) * 3)])
    assert out["n_in"].tolist() == [0, 0, n, n] and not out["n_bad"].any() and not out["n_hit"].any()
    # NaN and inf coordinates count nowhere
    odd = pts.copy()
    odd[3, 0], odd[70, 2], odd[299, 1] = np.nan, np.inf, -np.inf
    out = maps[0].score_batch(odd, poses)
    assert out["n_hit"].tolist() == [n - 3, 0, 0, 0, n - 3] and out["n_in"].tolist() == [n - 3, n - 3, 0, n - 3, n - 3]
    assert out["n_bad"].tolist() == [0, 0, n - 3, 0, 0]
    # an empty map
    empty = gpu.map_create(v)
    out = empty.score_batch(odd, poses)
    assert not out["n_hit"].any() and out["n_in"].tolist() == [n - 3, n - 3, 0, n - 3, n - 3] and out["n_bad"].tolist() == [0, 0, n - 3, 0, 0]
    for m in maps + [empty]:
        m.close()


def test_refusals_leave_the_output_untouched_and_the_edge_calls(gpu):
    lib = gpu.lib
    m = new_map(gpu, 0.5, False, SC.eq_cloud()[:2000])
    n = 1000
    d = gpu.to_device(SC.eq_scan()[:n])
    desc = R.Points(d.ptr, 0, 12, 0, n)
    good = np.ascontiguousarray(np.tile(np.eye(3, 4).reshape(-1), (16, 1)))
    out = np.zeros(16, R.MAP_SCORE)
    prm = R.MapScoreParams(1, 0)

    def fill():
        out.view(np.uint8)[:] = 0x5A

    def untouched():
        return np.all(out.view(np.uint8) == 0x5A)

    def rc(ctx=gpu, mp=m, pts=desc, T=good, K=4, p=prm, o=out):
        return lib.wc_map_score_batch(ctx.h, mp.h if mp else None, C.byref(pts) if pts is not None else None, R.ptr(T) if T is not None else None,
                                      C.c_uint32(K), C.byref(p) if p is not None else None, R.ptr(o) if o is not None else None)

    nan_T, inf_T = good[:4].copy(), good[:4].copy()
    nan_T[3, 7], inf_T[0, 0] = np.nan, np.inf
    other = L.Context(0)
    fill()
    cases = [dict(T=nan_T), dict(T=inf_T), dict(ctx=other), dict(mp=None), dict(pts=None), dict(T=None), dict(p=None), dict(o=None),
             dict(p=R.MapScoreParams(0, 0)), dict(p=R.MapScoreParams(1, 1)), dict(pts=R.Points(d.ptr, 0, 8, 0, 10)), dict(pts=R.Points(d.ptr + 2, 0, 12, 0, 10)),
             dict(pts=R.Points(0, 0, 12, 0, 10)), dict(pts=R.Points(d.ptr, 0, 12, 0, 2**31)), dict(K=2**20 + 1)]
    for kw in cases:
        assert rc(**kw) == WC_ERR_ARG and untouched(), kw
    other.close()
    # the capacity cap, reached by K n alone - 9 (2^31 - 1) > 2^34 with n and K each within their own caps: nothing of the points is read
    # before the check (K = 8 would be 2^34 - 8, a call the library accepts: a descriptor has to be true then)
    assert 9 * (2**31 - 1) > 2**34 >= 8 * (2**31 - 1)
    assert rc(K=9, pts=R.Points(d.ptr, 0, 12, 0, 2**31 - 1)) == WC_ERR_CAPACITY and untouched()
    assert rc(K=9, pts=R.Points(d.ptr, 0, 12, 0, 2**31 + 5)) == WC_ERR_ARG and untouched()
    # K = 0: nothing is touched; n = 0: zero records
    assert rc(K=0) == 0 and rc(K=0, T=None, o=None) == 0 and untouched()
    assert rc(K=4, pts=R.Points(0, 0, 12, 0, 0)) == 0
    assert out[:4].tobytes() == bytes(64) and np.all(out[4:].view(np.uint8) == 0x5A)
    assert rc(K=4) == 0 and out["n_in"][:4].tolist() == [n - 2] * 4 and np.all(out[4:].view(np.uint8) == 0x5A)
    d.free(), m.close()


@pytest.fixture(scope="module")
def room(gpu):
    """the room of DESIGN 8.9 at v = 0.2, its state as the canonical file's bytes, and its coarsest level (v = 1.6)"""
    fine = new_map(gpu, MC.BASIN_V, True, _xyz(synth.g1_room(MC.BASIN_ROOM)))
    levels = fine.pyramid(MC.BASIN_FACTOR, MC.BASIN_LEVELS)
    vox, mom = fine.state()
    yield dict(coarse=levels[-1], file=map_state_ref.encode_ref(MC.BASIN_V, vox, mom))
    for m in levels:
        m.close()


def test_scene_scores_of_the_whole_grid_equal_the_restatement(gpu, room):
    """all 7056 poses of the scene's grid on the coarsest level"""
    coarse, scan = room["coarse"], MS.search_scan()
    assert coarse.voxel == MS.search_sizes()[0]
    grid = L.pose_grid(SC.scene_start(), SC.SCENE_YAW, SC.SCENE_N, SC.SCENE_STEP)
    assert len(grid) == 7056
    got = coarse.score_batch(scan, grid)
    _, counts, keys = coarse.export()
    want = SC.score_fast(keys, counts, coarse.voxel, scan, grid)
    assert got.tobytes() == want.tobytes() and got["n_hit"].max() > len(scan) // 2 and not got["n_bad"].any()
    top = L.map_score_top(got, 16, 6)
    assert top.tolist() == SC.top_ref(want, 16, 6)[0]


def test_scene_through_the_facade(gpu, room, tmp_path):
    """Odometry.map_relocalize_global from the start, grid and top_m tests/test_map_score_ref.py fixed ends within 0.1 degree and 1 cm of
    the truth - with top_m = 16 as well -; map_relocalize_search, 16 headings from the same start, does not; the degenerate grid is
    map_relocalize byte for byte; the cases that return None"""
    path = str(tmp_path / "room.bin")
    open(path, "wb").write(room["file"])
    odo = L.Odometry(0)
    odo.set_map_voxel(MC.BASIN_V)
    odo.set_map_surfels(True)
    assert odo.map_load(path)
    scan, start, T_true = MS.search_scan(), SC.scene_start(), MS.search_pose()
    finest = L.map_align_opts(L.map_reg_params(MC.BASIN_V), max_iterations=SC.SCENE_ITERS, tol_rot=G.TOL_ROT, tol_trans=G.TOL_TRANS)
    args = (SC.SCENE_YAW, SC.SCENE_N, SC.SCENE_STEP)
    size_before = odo.map_size()
    for top_m in (SC.SCENE_TOP_M, 16):
        T, summ, best = odo.map_relocalize_global(scan, start, *args, top_m, MC.BASIN_FACTOR, MC.BASIN_LEVELS, finest)
        e = G.pose_error(T, T_true)
        print("global (device): top_m", top_m, "winner's rank", best, "n_used", summ[-1][best]["n_used"], "ends", e)
        assert e[0] < np.deg2rad(0.1) and e[1] < 0.01
        assert len(summ) == MC.BASIN_LEVELS and all(len(row) == top_m for row in summ) and 0 <= best < top_m
    assert odo.map_size() == size_before
    T_yaw = odo.map_relocalize_search(scan, start, SC.SCENE_YAW, MC.BASIN_FACTOR, MC.BASIN_LEVELS, finest)
    e_yaw = G.pose_error(T_yaw[0], T_true) if T_yaw is not None else (np.inf, np.inf)
    print("global (device): the yaw search alone ends", e_yaw)
    assert e_yaw[0] > 1.0 or e_yaw[1] > 1.0
    # the degenerate grid from a start the pyramid recovers from: map_relocalize, byte for byte
    near = MC.basin_pose()
    q = ((_xyz(synth.g1_room(MC.BASIN_SCAN, seed=synth.SEED + 7)).astype(np.float64) - near[:, 3]) @ near[:, :3]).astype(np.float32)
    T_rel, s_rel = odo.map_relocalize(q, np.eye(3, 4), MC.BASIN_FACTOR, MC.BASIN_LEVELS, finest)
    T_one, s_one, best = odo.map_relocalize_global(q, np.eye(3, 4), 1, (1, 1, 1), (0.0, 0.0, 0.0), 1, MC.BASIN_FACTOR, MC.BASIN_LEVELS, finest)
    assert best == 0 and T_one.tobytes() == T_rel.tobytes() and T_one.tobytes() != np.eye(3, 4).tobytes()
    assert [summary_bytes(row[0]) for row in s_one] == [summary_bytes(s) for s in s_rel]
    # fewer candidates than top_m: the summaries keep top_m records per level, the missing ones zero
    T_two, s_two, best = odo.map_relocalize_global(q, np.eye(3, 4), 1, (2, 1, 1), (0.4, 0.0, 0.0), 4, MC.BASIN_FACTOR, MC.BASIN_LEVELS, finest)
    zero = summary_bytes(L._summary_dict(R.MapAlignSummary()))
    assert best in (0, 1) and all(len(row) == 4 for row in s_two) and G.pose_error(T_two, near)[1] < 0.01
    assert all(summary_bytes(row[r]) == zero for row in s_two for r in (2, 3)) and all(summary_bytes(row[r]) != zero for row in s_two for r in (0, 1))
    # refused: nothing computed, nothing touched, no abort
    f, lv = MC.BASIN_FACTOR, MC.BASIN_LEVELS
    assert odo.map_relocalize_global(scan, start, *args, 0, f, lv, finest) is None and odo.map_relocalize_global(scan, start, *args, 1025, f, lv, finest) is None
    assert odo.map_relocalize_global(scan, start, 0, SC.SCENE_N, SC.SCENE_STEP, 4, f, lv, finest) is None
    assert odo.map_relocalize_global(scan, start, 16, (21, 0, 1), SC.SCENE_STEP, 4, f, lv, finest) is None
    assert odo.map_relocalize_global(scan, start, 16, SC.SCENE_N, (0.8, -0.8, 0.0), 4, f, lv, finest) is None
    assert odo.map_relocalize_global(scan, start, 1024, (1025, 1, 1), SC.SCENE_STEP, 4, f, lv, finest) is None
    assert odo.map_relocalize_global(scan, start, *args, 4, f, 9, finest) is None and odo.map_relocalize_global(scan, start, *args, 4, 7, 3, finest) is None
    assert odo.map_relocalize_global(scan, eye((500.0, 0.0, 0.0)), 2, (2, 2, 1), SC.SCENE_STEP, 4, f, lv, finest) is None  # (no candidate: nothing near)
    Tio, sentinel = np.ascontiguousarray(start.reshape(-1)).copy(), C.c_int32(77)
    n3, s3 = np.array(SC.SCENE_N, np.uint32), np.array(SC.SCENE_STEP, np.float64)
    for top_m in (0, 1025):
        assert odo.lib.wc_odom_map_relocalize_global(odo.h, R.ptr(scan), C.c_uint64(len(scan)), R.ptr(Tio), C.c_uint32(16), R.ptr(n3), R.ptr(s3),
                                                     C.c_uint32(top_m), C.c_uint32(f), C.c_uint32(lv), C.byref(finest), None, C.byref(sentinel)) == 0
        assert Tio.tobytes() == start.tobytes() and sentinel.value == 77
    odo.set_map_surfels(False)
    assert odo.map_relocalize_global(scan, start, *args, 4, f, lv, finest) is None
    odo.close()
