"""Removal in place without a GPU: the room policy of csrc/map_room.h through its g++ instantiation in the facade library
(wc_host_map_room), the declared and exported entry points, the carve restatement's figures on the room scene of map_carve_ref.py when
its selection is removed, and the table model of map_remove_ref.py: each of its named faults is caught by a comparison that
test_map_remove_gpu.py makes on the cluster scenario, and the faultless model passes them all."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import map_carve_ref as CR
import map_remove_ref as MR
from map_query_ref import pack
from wildcat_slam_amd import records as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def host():
    from wildcat_slam_amd import lib

    lib.load()
    return C.CDLL(os.path.join(HERE, "..", "wildcat-slam_amd", "host", "libwildcat_odometry.so"))


def cxx_room(host, cap, bound, tombs, n):
    new_cap = C.c_uint64(0)
    rc = host.wc_host_map_room(C.c_uint64(cap), C.c_uint64(bound), C.c_uint64(tombs), C.c_uint64(n), C.byref(new_cap))
    return int(rc), int(new_cap.value)


def test_room_without_tombstones_is_the_growth_policy_as_it_was(host):
    caps = [2, 8, 8192, 2**20, 2**31, 2**32]
    bounds = [0, 1, 3, 4, 4095, 4096, 4097, 2**19, 2**30 - 1, 2**30, 2**31 - 1, 2**31, 2**31 + 1, 2**33]
    ns = [0, 1, 2, 5, 4096, 2**20, 2**30, 2**31, 2**31 + 1, 2**32]
    seen = set()
    for cap, bound, n in itertools.product(caps, bounds, ns):
        want = MR.room_before(cap, bound, n)
        assert cxx_room(host, cap, bound, 0, n) == want == MR.room(cap, bound, 0, n), (cap, bound, n)
        assert want[0] != MR.PURGE
        seen.add(want[0])
    assert seen == {MR.KEEP, MR.GROW, MR.FULL}
    assert cxx_room(host, 2**32, 2**30, 0, 2**30) == (MR.KEEP, 2**32) and cxx_room(host, 2**32, 2**30, 0, 2**30 + 1) == (MR.FULL, 2**32)


def test_room_with_tombstones(host):
    # the worked cases of test_map_remove_gpu.py: 8192 slots, 3000 voxels, 2500 of them removed
    assert cxx_room(host, 8192, 500, 2500, 1200) == (MR.PURGE, 8192)  # 2 (500 + 2500 + 1200) = 8400 > 8192, 2 (500 + 1200) <= 8192
    assert cxx_room(host, 8192, 500, 2500, 5000) == (MR.GROW, 16384)
    assert cxx_room(host, 8192, 500, 2500, 1096) == (MR.KEEP, 8192)  # 2 * 4096 = 8192: exactly half
    assert cxx_room(host, 8192, 500, 2500, 1097) == (MR.PURGE, 8192)
    assert cxx_room(host, 8192, 500, 2500, 3596) == (MR.PURGE, 8192) and cxx_room(host, 8192, 500, 2500, 3597) == (MR.GROW, 16384)
    assert cxx_room(host, 8192, 0, 4096, 0) == (MR.KEEP, 8192) and cxx_room(host, 8192, 0, 4097, 0) == (MR.PURGE, 8192)
    assert cxx_room(host, 2**32, 2**30, 2**30, 2**30) == (MR.PURGE, 2**32) and cxx_room(host, 2**32, 2**31, 5, 1)[0] == MR.FULL
    rng = np.random.Generator(np.random.PCG64(4))
    for _ in range(3000):
        cap = 1 << int(rng.integers(1, 33))
        bound, tombs, n = (int(rng.integers(0, 2 * cap + 2)) >> int(rng.integers(0, 20)) for _ in range(3))
        what, new_cap = cxx_room(host, cap, bound, tombs, n)
        assert (what, new_cap) == MR.room(cap, bound, tombs, n), (cap, bound, tombs, n)
        assert new_cap >= cap and (new_cap == cap) == (what != MR.GROW)  # never smaller; equal unless it grows
        if what in (MR.GROW, MR.PURGE):  # a replacement drops the tombstones: the call then fits into half of the table
            assert 2 * (bound + n) <= new_cap and new_cap <= 2**32 and (what == MR.PURGE or new_cap < 4 * (bound + n))


def test_header_declares_the_removal_calls_and_the_libraries_export_them(host):
    from wildcat_slam_amd import lib

    declared = set(lib.declared_symbols())
    l = lib.load()
    for s in ("wc_map_carve_remove", "wc_map_remove_keys", "wc_map_tombstones"):
        assert s in declared and hasattr(l, s), s
    for s in ("wc_odom_map_carve_remove", "wc_odom_map_remove_keys", "wc_odom_set_map_carve", "wc_host_map_room"):
        assert hasattr(host, s), s
    # the calls take the carve's records and plain arrays: nothing new in records.py, and what they take is laid out as the header says
    assert C.sizeof(R.MapCarveParams) == 32 and C.sizeof(R.MapCarveResult) == 40 and C.sizeof(R.Points) == 32
    assert [f for f, _ in R.MapCarveResult._fields_] == list(CR.RESULT_FIELDS)
    assert C.sizeof(C.c_uint64 * 3) == 24 and np.dtype(np.int32).itemsize * 3 == 12
    with open(os.path.join(HERE, "..", "include", "wildcat_hip.h")) as f:
        text = f.read()
    assert "const int32_t *d_keys, uint64_t n, uint64_t h_out[3]" in text and "wc_map_tombstones(wc_ctx *ctx, wc_map *m, uint64_t h_out[2])" in text
    assert "map_remove_groups" in text


# (shell, min_rays) -> voxels / points the room scene's sweep removes from the map of sweep + phantom, origin ROOM_ORIGIN, infinite range
ROOM_FIGURES = {
    0.5: (811, 48, {(0, 1): (46, 652), (0, 2): (44, 650), (1, 1): (28, 452), (1, 2): (26, 450), (2, 1): (15, 357), (2, 2): (14, 356)}),
    0.3: (1983, 148, {(0, 1): (144, 650), (0, 2): (144, 650), (1, 1): (89, 450), (1, 2): (89, 450), (2, 1): (47, 332), (2, 2): (38, 306)}),
}


@pytest.mark.parametrize("v", [0.5, 0.3])
def test_room_scene_figures(v):
    sweep, phantom = CR.room_scene()
    assert len(sweep) == 6401 and len(phantom) == 654
    n_vox, n_phantom, figures = ROOM_FIGURES[v]
    phantom_keys = np.unique(pack(CR.point_keys(phantom, v)))
    assert len(phantom_keys) == n_phantom
    for (shell, min_rays), (vox, pts) in figures.items():
        s = MR.Survivors(v)
        s.insert(np.concatenate([sweep, phantom]))
        assert len(s.voxels()[0]) == n_vox
        res, gone = s.carve_remove(sweep, CR.ROOM_ORIGIN, np.inf, shell=shell, min_rays=min_rays)
        assert (res["voxels_removed"], res["points_removed"]) == (vox, pts), (v, shell, min_rays, res)
        assert np.isin(pack(gone), phantom_keys).all()
        assert len(s.voxels()[0]) == n_vox - vox and len(s.points) == len(sweep) + len(phantom) - pts
        again, gone2 = s.carve_remove(sweep, CR.ROOM_ORIGIN, np.inf, shell=shell, min_rays=min_rays)
        assert again["voxels_removed"] == 0 and again["points_removed"] == 0 and len(gone2) == 0
        assert all(again[k] == res[k] for k in ("rays_used", "rays_skipped", "steps"))


def test_cluster_keys_share_a_home_slot():
    keys = MR.cluster_keys(64, 8191)
    assert len(np.unique(pack(keys))) == 64 and len({MR.map_hash(int(k)) & 8191 for k in pack(keys)}) == 1
    assert np.array_equal(MR.map_hash_np(pack(keys)), np.array([MR.map_hash(int(k)) for k in pack(keys)], np.uint64))
    assert MR.map_hash(0) == 0 and MR.map_hash(2**64 - 1) != MR.map_hash(2**64 - 2)


def run_cluster_scenario(fault):
    """the cluster scenario on the table model -> the list of the comparisons of test_map_remove_gpu.py's cluster test that fail"""
    sc = MR.cluster_scenario()
    t, ref = MR.Table(MR.CLUSTER_SLOTS, fault), MR.Survivors(MR.CLUSTER_V)
    first = np.concatenate([sc["cluster"], sc["rest"]])
    failed = []

    def compare(tag, tombs):
        keys, cnt = ref.voxels()
        if t.export() != (pack(keys).tolist(), cnt.tolist()):
            failed.append(tag + ": export")
        if t.size() != (len(cnt), int(cnt.sum())):
            failed.append(tag + ": size")
        live = set(pack(keys).tolist())
        if any((t.find(int(k)) >= 0) != (int(k) in live) for k in pack(np.concatenate([first, sc["fresh"]]))):
            failed.append(tag + ": nearest")
        if t.tombstones() != tombs or t.cap != MR.CLUSTER_SLOTS:
            failed.append(tag + ": tombstones, slots")

    t.insert(pack(first))
    ref.insert(MR.centre_points(first))
    compare("inserted", (0, 0))
    want = ref.remove(sc["remove_list"])
    assert want == dict(voxels_removed=len(sc["removed"]), points_removed=len(sc["removed"]), keys_unused=len(sc["remove_list"]) - len(sc["removed"]))
    if t.remove(sc["remove_list"]) != want:
        failed.append("removed: the three counts")
    compare("removed", (len(sc["removed"]), 0))
    more = np.concatenate([sc["again"], sc["fresh"]])
    t.insert(pack(more))
    ref.insert(MR.centre_points(more, 0.125))
    compare("inserted again", (0, 1))  # (live + tombstones + the new points exceed half of the table, live + new points do not: a purge)
    return failed


def test_the_faultless_model_passes_every_comparison():
    assert run_cluster_scenario(None) == []


@pytest.mark.parametrize("fault", MR.FAULTS)
def test_the_gpu_tests_comparisons_catch_each_fault(fault):
    failed = run_cluster_scenario(fault)
    print(fault, "caught by", failed)
    assert failed, fault


def test_reinserted_voxel_starts_from_zero():
    t = MR.Table(64)
    t.insert([5, 6], [3, 4])
    key = np.array([[0, 0, 0]])
    k = int(pack(key)[0])
    t.insert([k], [7])
    assert t.remove(key) == dict(voxels_removed=1, points_removed=7, keys_unused=0) and t.size() == (2, 7)
    t.insert([k], [2])
    assert t.export() == ([5, 6, k], [3, 4, 2]) and t.size() == (3, 9) and t.tombstones() == (1, 0)
