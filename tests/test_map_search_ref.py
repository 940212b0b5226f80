"""The search over pose hypotheses (include/wildcat_hip.h: wc_map_align_best, wc_pose_yaw_grid) - the parts that need no GPU:
the two host functions against the restatements of map_search_ref.py, and the scene on which the GPU test rests, worked through with the
float64 restatement of the registration."""
import numpy as np
import pytest

import map_register_ref as G
import map_search_ref as MS
from extract_ref import LD
from helpers import xyz_of as _xyz
from test_map_register_ref import P
from wildcat_slam_amd import lib as L
from wildcat_slam_amd import synth

WC_ERR_ARG = 11


def S(n_used, final_cost, termination=0):
    return dict(n_used=n_used, final_cost=final_cost, termination=termination)


BEST_CASES = {
    "an ineligible hypothesis of each kind": ([S(900, 1.0), S(900, 1.0, 2), S(5, 1.0), S(900, np.inf), S(900, np.nan), S(100, 50.0, 1)],
                                              [WC_ERR_ARG, 0, 0, 0, 0, 0], 6),
    "more inliers beat a lower cost": ([S(100, 1.0), S(101, 1e9), S(99, 0.0)], [0, 0, 0], 6),
    "ties on n_used broken by cost": ([S(500, 3.0), S(500, 2.0), S(500, 2.5), S(499, 0.1)], [0, 0, 0, 0], 6),
    "full ties broken by index": ([S(7, 4.0), S(8, 2.0), S(8, 2.0), S(8, 2.0)], [0, 0, 0, 0], 6),
    "min_used is inclusive": ([S(9, 1.0), S(10, 5.0)], [0, 0], 10),
    "none eligible": ([S(900, 1.0, 2), S(3, 1.0), S(900, -np.inf)], [0, 0, 0], 6),
    "every status an error": ([S(900, 1.0), S(800, 1.0)], [WC_ERR_ARG, 1], 6),
    "K = 0": ([], [], 6),
}
BEST_WANT = {"an ineligible hypothesis of each kind": 5, "more inliers beat a lower cost": 1, "ties on n_used broken by cost": 1,
             "full ties broken by index": 1, "min_used is inclusive": 1, "none eligible": -1, "every status an error": -1, "K = 0": -1}


@pytest.mark.parametrize("name", list(BEST_CASES))
def test_align_best_equals_the_restatement(name):
    summ, status, min_used = BEST_CASES[name]
    want = MS.best_ref(summ, status, min_used)
    assert want == BEST_WANT[name]  # (the restatement itself, against the answer worked out by hand)
    assert L.map_align_best(summ, status, min_used) == want


def test_align_best_on_random_summaries():
    rng = np.random.default_rng(5)
    for _ in range(200):
        K = int(rng.integers(1, 12))
        summ = [S(int(rng.integers(0, 6)), float(rng.choice([1.0, 2.0, 3.0, np.inf, np.nan])), int(rng.integers(0, 3))) for _ in range(K)]
        status = rng.choice([0, 0, 0, WC_ERR_ARG], K)
        min_used = int(rng.integers(0, 4))
        assert L.map_align_best(summ, status, min_used) == MS.best_ref(summ, status, min_used)


def _some_pose(seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([G.rodrigues(rng.normal(size=3)), rng.normal(size=(3, 1)) * 10.0], 1)


@pytest.mark.parametrize("K", [1, 2, 8, 1024])
def test_yaw_grid_against_longdouble(K):
    """every entry within 8 x 2^-53 of the longdouble grid for an orthonormal R0: an entry is c r - s r' or s r + c r' with sine and cosine
    within 1 ulp (2 x 2^-53 below 1), two rounded products and one rounded sum, and |c r| + |s r'| <= sqrt(2):
    2 sqrt(2) + sqrt(2) + 1 = 5.3 units of 2^-53"""
    for seed in (1, 2):
        T0 = _some_pose(seed)
        got, want = L.pose_yaw_grid(T0, K), MS.yaw_grid_ref(T0, K)
        assert got.shape == (K, 3, 4)
        err = np.abs(got.astype(LD) - want).max()
        print("yaw grid K", K, "largest error", float(err / LD(G.EPS)), "x 2^-53")
        assert err <= 8 * G.EPS
        assert got[0].tobytes() == T0.tobytes()
        assert all(got[k, :, 3].tobytes() == T0[:, 3].tobytes() and got[k, 2].tobytes() == T0[2].tobytes() for k in range(K))
    if K >= 2:  # what the grid is: half a turn about z at k = K / 2, the scan turned about the sensor's position
        T0 = MS.search_start()
        half = L.pose_yaw_grid(T0, K)[K // 2]
        assert np.abs(half - np.concatenate([np.diag([-1.0, -1.0, 1.0]), MS.SEARCH_C[:, None]], 1)).max() <= 2 * G.EPS


def test_yaw_grid_refusals_and_empty():
    lib = L.load()
    T0 = np.ascontiguousarray(MS.search_start().reshape(-1))
    out = np.full(24, 7.0)
    from wildcat_slam_amd import records as R

    assert lib.wc_pose_yaw_grid(None, 2, R.ptr(out)) == WC_ERR_ARG and lib.wc_pose_yaw_grid(R.ptr(T0), 2, None) == WC_ERR_ARG
    assert lib.wc_pose_yaw_grid(R.ptr(T0), 0, None) == 0 and np.all(out == 7.0)
    assert L.pose_yaw_grid(T0, 0).shape == (0, 3, 4)
    assert lib.wc_map_align_best(None, None, 0, 6, None) == WC_ERR_ARG


@pytest.fixture(scope="module")
def scene():
    """DESIGN 8.10's table: K = 8 yaw hypotheses through the four levels, by the float64 restatement"""
    room = _xyz(synth.g1_room(60_000))
    surf = {}

    def surfels_of(v):
        if v not in surf:
            surf[v] = G.surfels_cpu(room, v)
        return surf[v]

    T_true, scan = MS.search_pose(), MS.search_scan()
    starts = MS.yaw_grid_ref(MS.search_start(), MS.SEARCH_K).astype(np.float64)
    Ts, summ = MS.search_ref(surfels_of, scan, starts, MS.search_sizes(), P)
    table = MS.report(Ts, summ[-1], T_true)
    for k, row in enumerate(table):
        print("search (restatement): k", k, "n_used", row[0], "final_cost", row[1], "termination", row[2], "error", row[3], row[4])
    return dict(Ts=Ts, summ=summ, table=table, T_true=T_true)


def test_scene_the_winner_is_at_the_truth_and_the_start_alone_is_lost(scene):
    """the condition that makes the GPU test meaningful: the winner ends within 0.1 degree and 1 cm; hypothesis 0 - what the pyramid alone
    does from this start - ends more than 1 rad off; the best hypothesis more than 1 rad from the truth holds at most 0.8 of the winner's
    inliers.  (No assertion on the winner's index: the two neighbours of the true heading tie on n_used.)"""
    table, finest = scene["table"], scene["summ"][-1]
    win = MS.best_ref(finest, [0] * MS.SEARCH_K, 6)
    assert win >= 0
    assert table[win][3] < np.deg2rad(0.1) and table[win][4] < 0.01
    assert table[0][3] > 1.0
    wrong = [row[0] for row in table if row[3] > 1.0]
    assert wrong and max(wrong) <= 0.8 * table[win][0]
