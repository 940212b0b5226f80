"""The occupancy score of pose hypotheses (include/wildcat_hip.h: wc_map_score_batch, wc_pose_grid, wc_map_score_top) - the
parts that need no GPU: the two host functions against the restatements of map_score_ref.py, the scene on which the GPU test rests worked
through in numpy, and the proof that the GPU test's inputs tell three wrong forms of the score from the right one."""
import ctypes as C

import numpy as np
import pytest

import map_register_ref as G
import map_score_ref as SC
import map_search_ref as MS
from extract_ref import LD
from helpers import xyz_of as _xyz
from test_map_register_ref import P
from wildcat_slam_amd import lib as L
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

WC_ERR_ARG = 11


def _some_pose(seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([G.rodrigues(rng.normal(size=3)), rng.normal(size=(3, 1)) * 10.0], 1)


GRIDS = [(1, (1, 1, 1), (0.0, 0.0, 0.0)), (1, (1, 1, 1), (0.3, 0.7, 0.1)), (3, (2, 1, 4), (0.8, 0.0, 0.3)), (4, (5, 3, 1), (0.1, 1e-3, 7.0)),
         (16, (3, 2, 2), (0.8, 0.8, 0.25)), (2, (6, 7, 1), (1.0 / 3.0, 0.7, 0.0))]


@pytest.mark.parametrize("n_yaw,n,step", GRIDS)
def test_pose_grid_against_the_restatements(n_yaw, n, step):
    """rotations bitwise wc_pose_yaw_grid's and within 8 x 2^-53 of the longdouble grid (test_map_search_ref.py has the bound);
    translations bitwise the two-rounding formula and within 2^-53 (|offset| + |t|) of the longdouble one: half an ulp of the product,
    half an ulp of the sum; the index order; n_a = 1 leaves t0_a"""
    for seed in (1, 2):
        T0 = _some_pose(seed)
        got = L.pose_grid(T0, n_yaw, n, step)
        K = n_yaw * n[0] * n[1] * n[2]
        assert got.shape == (K, 3, 4)
        rot = L.pose_yaw_grid(T0, n_yaw)
        want = SC.pose_grid_bits(rot, T0, n, step)
        assert got.tobytes() == want.tobytes()
        ref = SC.pose_grid_ref(T0, n_yaw, n, step)
        assert np.abs(got[:, :, :3].astype(LD) - ref[:, :, :3]).max() <= 8 * G.EPS
        off = np.abs(ref[:, :, 3] - T0[:, 3].astype(LD))
        assert np.all(np.abs(got[:, :, 3].astype(LD) - ref[:, :, 3]) <= LD(G.EPS) * (off + np.abs(ref[:, :, 3])) * LD(1.0 + 2.0**-40))
        # the index order, and what the lattice is: symmetric about t0, spaced by step
        for k, i in ((0, (0, 0, 0)), (n_yaw - 1, (n[0] - 1, 0, n[2] - 1)), (n_yaw // 2, (n[0] // 2, n[1] - 1, 0))):
            T = got[SC.grid_index(k, i, n)]
            assert T[:, :3].tobytes() == rot[k][:, :3].tobytes()
            assert np.allclose(T[:, 3], T0[:, 3] + (np.array(i) - (np.array(n) - 1) / 2.0) * np.array(step), rtol=0, atol=1e-12)
        for a in range(3):
            if n[a] == 1:
                assert np.all(got[:, a, 3] == T0[a, 3])
            if n[a] % 2 == 1:  # (odd: the centre is t0 itself)
                i = [0, 0, 0]
                i[a] = n[a] // 2
                assert got[SC.grid_index(0, i, n)][a, 3] == T0[a, 3]


def test_pose_grid_minus_zero_and_refusals():
    T0 = np.concatenate([np.eye(3), [[-0.0], [2.0], [-0.0]]], 1)
    got = L.pose_grid(T0, 1, (1, 1, 1), (0.5, 0.5, 0.0))
    assert got.shape == (1, 3, 4) and not np.signbit(got[0, :, 3]).any() and np.all(got[0, :, 3] == [0.0, 2.0, 0.0])
    assert got[0, :, :3].tobytes() == T0[:, :3].tobytes()
    lib = L.load()
    T0 = np.ascontiguousarray(MS.search_start().reshape(-1))
    out = np.full(4 * 12, 7.0)

    def rc(T=T0, n_yaw=2, n=(2, 1, 1), step=(0.5, 0.5, 0.5), o=out):
        n, step = np.array(n, np.uint32) if n is not None else None, np.array(step, np.float64) if step is not None else None
        return lib.wc_pose_grid(R.ptr(T) if T is not None else None, C.c_uint32(n_yaw), R.ptr(n) if n is not None else None,
                                R.ptr(step) if step is not None else None, R.ptr(o) if o is not None else None)

    nan_T, inf_T = T0.copy(), T0.copy()
    nan_T[3], inf_T[0] = np.nan, np.inf
    cases = [dict(T=None), dict(n=None), dict(step=None), dict(o=None), dict(n_yaw=0), dict(n=(2, 0, 1)), dict(n=(0, 1, 1)), dict(n=(1, 1, 0)),
             dict(n_yaw=1024, n=(1025, 1, 1)), dict(n_yaw=2**20, n=(2, 1, 1)), dict(n_yaw=2**31, n=(2**31, 4, 1)), dict(n=(2**16, 2**16, 2**16)),
             dict(step=(0.5, -0.1, 0.5)), dict(step=(np.nan, 0.5, 0.5)), dict(step=(0.5, 0.5, np.inf)), dict(T=nan_T), dict(T=inf_T)]
    for kw in cases:
        assert rc(**kw) == WC_ERR_ARG and np.all(out == 7.0), kw
    assert rc() == 0 and not np.any(out == 7.0)
    with pytest.raises(L.WildcatError):
        L.pose_grid(T0, 0, (1, 1, 1), (0.1, 0.1, 0.1))
    assert L.pose_grid(T0, 2**10, (2**10, 1, 1), (0.0, 0.0, 0.0)).shape == (2**20, 3, 4)  # (the cap itself)


def rec(n_hit, n_bad=0, n_in=0):
    return (n_hit, n_in, n_bad, 0)


TOP_CASES = {
    "an ineligible record of each kind": ([rec(900, 1), rec(5), rec(40), rec(2**31, 2**31), rec(6)], 3, 6, [2, 4, -1], 2),
    "ties on n_hit broken by index": ([rec(7), rec(9), rec(9), rec(8), rec(9)], 4, 0, [1, 2, 4, 3], 4),
    "M larger than the eligible count": ([rec(3), rec(1), rec(2, 1)], 5, 1, [0, 1, -1, -1, -1], 2),
    "min_hit is inclusive": ([rec(9), rec(10)], 2, 10, [1, -1], 1),
    "M = 0": ([rec(9), rec(10)], 0, 0, [], 0),
    "K = 0": ([], 3, 0, [-1, -1, -1], 0),
}


def _top(scores, M, min_hit):
    """the C call itself: (idx_out with its fill, n_out)"""
    scores = np.array(scores, SC.SCORE).reshape(-1)
    idx, cnt = np.full(M, 77, np.int32), C.c_uint32(99)
    assert L.load().wc_map_score_top(R.ptr(scores) if len(scores) else None, C.c_uint32(len(scores)), C.c_uint32(M), C.c_uint32(min_hit),
                                     R.ptr(idx) if M else None, C.byref(cnt)) == 0
    return idx.tolist(), cnt.value


@pytest.mark.parametrize("name", list(TOP_CASES))
def test_score_top_planted(name):
    scores, M, min_hit, want, want_n = TOP_CASES[name]
    assert SC.top_ref(np.array(scores, SC.SCORE).reshape(-1), M, min_hit) == (want, want_n)  # (the restatement, against the hand-made answer)
    assert _top(scores, M, min_hit) == (want, want_n)
    assert L.map_score_top(np.array(scores, SC.SCORE).reshape(-1), M, min_hit).tolist() == want[:want_n]


def test_score_top_random_and_refusals():
    rng = np.random.default_rng(6)
    for _ in range(200):
        K, M = int(rng.integers(0, 40)), int(rng.integers(0, 12))
        scores = np.zeros(K, SC.SCORE)
        scores["n_hit"], scores["n_bad"] = rng.integers(0, 6, K), rng.choice([0, 0, 0, 1], K)
        min_hit = int(rng.integers(0, 4))
        assert _top(scores, M, min_hit) == SC.top_ref(scores, M, min_hit)
    lib, one, idx, cnt = L.load(), np.zeros(1, SC.SCORE), np.full(2, 77, np.int32), C.c_uint32(99)
    assert lib.wc_map_score_top(None, 1, 2, 0, R.ptr(idx), C.byref(cnt)) == WC_ERR_ARG
    assert lib.wc_map_score_top(R.ptr(one), 1, 2, 0, None, C.byref(cnt)) == WC_ERR_ARG
    assert lib.wc_map_score_top(R.ptr(one), 1, 2, 0, R.ptr(idx), None) == WC_ERR_ARG
    assert idx.tolist() == [77, 77] and cnt.value == 99


def test_the_fast_lookup_equals_the_dict():
    """score_fast and flags - what the GPU test compares with - against the dict form, on a slice of the GPU test's inputs"""
    keys, counts = SC.voxels_of(SC.eq_cloud(), SC.EQ_V)
    scan, Ts = SC.eq_scan()[:700], SC.eq_poses()[:12]
    for min_points in (1, 3):
        want = SC.score_ref(keys, counts, SC.EQ_V, scan, Ts, min_points)
        assert SC.score_fast(keys, counts, SC.EQ_V, scan, Ts, min_points).tobytes() == want.tobytes()
        assert SC.records_of(SC.flags(keys, counts, SC.EQ_V, scan, Ts, min_points), 700, 12).tobytes() == want.tobytes()
    assert want["n_bad"][SC.EQ_BAD] == 698 and want["n_in"][SC.EQ_OUT] == 0 and want["n_bad"][SC.EQ_OUT] == 0 and want["n_in"][0] == 698
    assert 0 < want["n_hit"][0] < SC.score_ref(keys, counts, SC.EQ_V, scan, Ts[:1], 1)["n_hit"][0] < 698


def test_the_gpu_tests_inputs_tell_the_wrong_forms_apart():
    """a score that drops one tile, one that forms P in float arithmetic and one whose probe chain ends at a tombstone each change at
    least one record of the inputs tests/test_map_score_gpu.py compares byte for byte"""
    keys, counts = SC.voxels_of(SC.eq_cloud(), SC.EQ_V)
    scan, Ts = SC.eq_scan(), SC.eq_poses()
    right = SC.score_fast(keys, counts, SC.EQ_V, scan, Ts[:1])
    # one tile dropped: every one of the 33 tiles holds a point that counts for the identity
    for tile in (0, 17, 32):
        wrong = SC.score_ref(keys, counts, SC.EQ_V, scan, Ts[:1], drop_tile=tile)
        assert wrong["n_in"][0] < right["n_in"][0]
    # P in float arithmetic
    right = SC.score_fast(keys, counts, SC.EQ_V, scan, Ts)
    wrong = SC.score_fast(keys, counts, SC.EQ_V, scan, Ts, float_P=True)
    n_rec = int(np.sum(wrong != right))
    print("float P: records changed", n_rec, "of", SC.EQ_K)
    assert n_rec >= 1 and wrong["n_hit"][SC.EQ_FLOAT] != right["n_hit"][SC.EQ_FLOAT]
    at = slice(SC.EQ_FLOAT_AT, SC.EQ_FLOAT_AT + 1)
    one_r = SC.score_ref(keys, counts, SC.EQ_V, scan[at], Ts[SC.EQ_FLOAT:SC.EQ_FLOAT + 1])
    one_w = SC.score_ref(keys, counts, SC.EQ_V, scan[at], Ts[SC.EQ_FLOAT:SC.EQ_FLOAT + 1], float_P=True)
    assert (one_r["n_hit"][0], one_w["n_hit"][0]) == (0, 1)  # (the planted point: voxel (3, 2, 2) is empty, (4, 2, 2) is not)
    # a tombstone as the end of a chain, in a table the device can have built
    ck = SC.crowd_keys()
    gone, pts, poses = ck[::3], SC.centres(ck, SC.CROWD_V), SC.crowd_poses()
    slots = SC.table_remove(SC.table_ref(ck, 2 * SC.CROWD_M), gone)
    live = np.delete(ck, np.arange(0, SC.CROWD_M, 3), 0)
    want = SC.score_fast(live, np.ones(len(live)), SC.CROWD_V, pts, poses)["n_hit"]
    assert SC.score_table(slots, SC.CROWD_V, pts, poses).tolist() == want.tolist() and want[0] == SC.CROWD_M - len(gone)
    cut = SC.score_table(slots, SC.CROWD_V, pts, poses, tomb_ends=True)
    print("tombstone ends the chain: n_hit", cut.tolist(), "instead of", want.tolist())
    assert cut[0] < want[0]


@pytest.fixture(scope="module")
def scene():
    """DESIGN 8.11's scene in numpy: the room's levels, the grid around the start scored on the coarsest level, the SCENE_TOP_M best
    aligned through the levels; and DESIGN 8.10's yaw search from the same start"""
    room = _xyz(synth.g1_room(60_000))
    surf = {}

    def surfels_of(v):
        if v not in surf:
            surf[v] = G.surfels_cpu(room, v)
        return surf[v]

    sizes, T_true, scan, start = MS.search_sizes(), MS.search_pose(), MS.search_scan(), SC.scene_start()
    grid = L.pose_grid(start, SC.SCENE_YAW, SC.SCENE_N, SC.SCENE_STEP)
    coarse = surfels_of(sizes[0])
    scores = SC.score_fast(coarse["key"], coarse["count"], sizes[0], scan, grid, 1)
    top, cnt = SC.top_ref(scores, SC.SCENE_TOP_M, 6)
    Ts, summ = MS.search_ref(surfels_of, scan, grid[top[:cnt]], sizes, P, iters=SC.SCENE_ITERS)
    for r, h in enumerate(top[:cnt]):
        e0, e1 = G.pose_error(grid[h], T_true), G.pose_error(Ts[r], T_true)
        print("global (restatement): rank", r, "pose", h, "n_hit", scores["n_hit"][h], "start off", e0, "n_used", summ[-1][r]["n_used"], "ends", e1)
    Ty, sy = MS.search_ref(surfels_of, scan, MS.yaw_grid_ref(start, SC.SCENE_YAW).astype(np.float64), sizes, P, iters=SC.SCENE_ITERS)
    return dict(grid=grid, scores=scores, top=top[:cnt], Ts=Ts, summ=summ, T_true=T_true, Ty=Ty, sy=sy)


def test_scene_the_score_finds_the_neighbourhood_the_winner_the_pose_and_the_yaw_search_is_lost(scene):
    """the conditions that make the GPU test meaningful, from the start (I | c + (6.5, -7.5, 0)), 9.9 m off: (1) a hypothesis within one
    grid step per axis and one heading step of the truth is among the SCENE_TOP_M best scores; (2) the aligned winner ends within 0.1
    degree and 1 cm; (3) DESIGN 8.10's yaw search alone, 16 headings from the same start, ends more than 1 m or 1 rad off.  From the
    issue's start (I | c + (5, -4, 0)) the yaw search is NOT lost - the 1.6 m level pulls it in from 6.4 m -, so the start was moved.
    SCENE_TOP_M = 1 is the smallest power of two at which (1) and (2) hold; DESIGN 8.11 has the table of the 16 best"""
    T_true, grid = scene["T_true"], scene["grid"]
    near = [h for h in scene["top"] if G.pose_error(grid[h], T_true)[0] <= 2 * np.pi / SC.SCENE_YAW
            and np.all(np.abs(grid[h][:2, 3] - T_true[:2, 3]) <= SC.SCENE_STEP[0])]
    assert near
    win = MS.best_ref(scene["summ"][-1], [0] * len(scene["top"]), 6)
    assert win >= 0
    e = G.pose_error(scene["Ts"][win], T_true)
    assert e[0] < np.deg2rad(0.1) and e[1] < 0.01
    wy = MS.best_ref(scene["sy"][-1], [0] * SC.SCENE_YAW, 6)
    ey = G.pose_error(scene["Ty"][wy], T_true) if wy >= 0 else (np.inf, np.inf)
    print("global (restatement): winner ends", e, "; the yaw search alone ends", ey)
    assert ey[0] > 1.0 or ey[1] > 1.0
