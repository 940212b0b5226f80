"""Nearest-voxel queries and box cropping of the device-resident voxel map (wc_map_nearest, wc_map_crop, csrc/map.hip) and their facade
surface (QueryMap, CropMap, LioConfig::map_keep_radius) against the numpy restatements of map_query_ref.py.  Every comparison is over
all queries of its test."""
import ctypes as C

import numpy as np
import pytest

import map_query_ref as Q
from helpers import check_unreadable_points_refused, point_records as _records, xyz_of as _xyz
from test_map_cpu import centroids_close, downsample_voxel
from test_map_gpu import _drive
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

pytestmark = pytest.mark.gpu

VOXELS = (0.05, 0.2, float(np.float32(0.8)))
WC_ERR_ARG = 11
BAD = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [3e38, 0, 0], [1, -3e38, 1]], np.float32)


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _queries(xyz, v, seed):
    """the inserted points themselves, jittered points, a block translated 1 km away (all misses), the bad queries, and queries at the
    ends of the key range"""
    rng = np.random.Generator(np.random.PCG64(seed))
    jit = (xyz[rng.integers(0, len(xyz), 200_000)] + rng.normal(size=(200_000, 3)) * (v / 2)).astype(np.float32)
    far = xyz[:10_000] + np.float32(1000.0)
    edge = np.array([[2.0**20 * v * 1.5, 1, 1], [1, -(2.0**20) * v * 1.5, 1]], np.float32)
    return np.concatenate([xyz, jit, far, BAD, edge]), len(xyz) + len(jit), len(far)


def _assert_hits_equal(got, want, what):
    for f in ("key", "count", "flags"):
        assert np.array_equal(got[f], want[f]), (what, f, int((got[f] != want[f]).sum()))
    assert got["xyz"].tobytes() == want["xyz"].tobytes(), (what, "xyz")
    assert got["d2"].tobytes() == want["d2"].tobytes(), (what, "d2")


@pytest.fixture(scope="module")
def clouds():
    lat, _ = synth.g2_lattice(200, m=32)
    return dict(g2_lattice=_xyz(lat), g1_room=_xyz(synth.g1_room(1_000_000)))


@pytest.mark.parametrize("name", ["g2_lattice", "g1_room"])
def test_query_agrees_with_the_export_bitwise(gpu, clouds, name):
    """query and export describe the same map: the restatement on the map's own export() gives key, count, flags, and xyz and d2 as
    bytes, and the found count; through the 12-byte and the 48-byte query layouts"""
    xyz = clouds[name]
    for v in VOXELS:
        m = gpu.map_create(v)
        assert m.insert(xyz) == 0
        cen, cnt, keys = m.export()
        q, n_near, n_far = _queries(xyz, v, 11)
        found = Q.search(keys, cen, q, v)
        d_q12, d_q48 = gpu.to_device(q), gpu.to_device(_records(q))
        d_hits = gpu.alloc(R.MAP_HIT.itemsize * len(q))
        for max_dist in (v / 2, v, np.inf):
            want, idx = Q.accept(keys, cen, cnt, found, max_dist)
            assert not np.any(idx[n_near : n_near + n_far] >= 0) and np.all(want["flags"][n_near + n_far : n_near + n_far + len(BAD) + 2] == 1)
            assert 0 < (idx >= 0).sum() < len(q)
            for what, desc in (("xyz12", R.Points(d_q12.ptr, 0, 12, 0, len(q))), ("point48", R.Points(d_q48.ptr, d_q48.ptr + 24, 48, 48, len(q)))):
                d_hits.upload(np.full(len(q) * 10, 0xA5A5A5A5, np.uint32))
                n_found = m.nearest_device(desc, max_dist, d_hits)
                got = d_hits.download(R.MAP_HIT, len(q))
                _assert_hits_equal(got, want, (name, v, max_dist, what))
                assert n_found == int((idx >= 0).sum()), (name, v, max_dist, what)
            # the host convenience, and the call that does not wait
            if max_dist == v:
                _assert_hits_equal(m.nearest(q[-50_000:], max_dist), want[-50_000:], (name, v, "nearest()"))
                d_hits.upload(np.zeros(len(q) * 10, np.uint32))
                assert m.nearest_device(R.Points(d_q12.ptr, 0, 12, 0, len(q)), max_dist, d_hits, want_count=False) is None
                _assert_hits_equal(d_hits.download(R.MAP_HIT, len(q)), want, (name, v, "no wait"))
        for b in (d_q12, d_q48, d_hits):
            b.free()
        m.close()


@pytest.mark.parametrize("name", ["g2_lattice", "g1_room"])
def test_query_against_centroids_formed_independently(gpu, clouds, name):
    """max_dist = inf against the restatement run on downsample_voxel's float64-sum centroids: the hit / miss pattern is identical (the
    keys are exact), hit.count is the reference count of hit.key, and |sqrt(d2) - sqrt(d2_ref)| <= delta with
    delta = sqrt(3) * (2 float32 ulps of the largest |coordinate| + 1e-9 m): centroids_close lets every centroid coordinate move by
    that much, and the minimum of distances is 1-Lipschitz in the centroids.  delta is derived, not measured."""
    xyz = clouds[name]
    for v in VOXELS:
        keys, cen, cnt, rej = downsample_voxel(xyz, v)
        assert rej == 0
        q, _, _ = _queries(xyz, v, 12)
        ref, ref_idx = Q.nearest_voxel(keys, cen, cnt, q, v, np.inf)
        m = gpu.map_create(v)
        m.insert(xyz)
        got = m.nearest(q, np.inf)
        m.close()
        hit = got["count"] > 0
        assert np.array_equal(hit, ref_idx >= 0), (name, v)
        assert np.array_equal(got["flags"], ref["flags"])
        # (the nearest KEY may differ from the reference's where two centroids are within delta of a tie: the count is looked up by hit.key)
        row = np.searchsorted(Q.pack(keys), Q.pack(got["key"][hit]))
        assert np.array_equal(Q.pack(keys)[row], Q.pack(got["key"][hit])) and np.array_equal(got["count"][hit], cnt[row]), (name, v)
        delta = np.sqrt(3.0) * (2.0 * float(np.spacing(np.float32(np.abs(cen).max()))) + 1e-9)
        err = np.abs(np.sqrt(got["d2"][hit]) - np.sqrt(ref["d2"][hit]))
        print(name, v, "max |sqrt(d2) - sqrt(d2_ref)| =", float(err.max()), "delta =", delta)
        assert np.all(err <= delta), (name, v, float(err.max()), delta)
        assert np.all(np.isinf(got["d2"][~hit]))


def test_hand_worked_case_on_the_gpu(gpu):
    m = gpu.map_create(Q.HAND_V)
    assert m.insert(Q.HAND_POINTS) == 0
    cen, cnt, keys = m.export()
    assert keys.tolist() == Q.HAND_KEYS and cnt.tolist() == Q.HAND_COUNTS and np.array_equal(cen, np.array(Q.HAND_CENTROIDS, np.float32))
    for max_dist in Q.HAND_EXPECT:
        want, idx = Q.hand_expected_hits(max_dist)
        d_q = gpu.to_device(Q.HAND_QUERIES)
        d_hits = gpu.alloc(40 * len(want))
        n = m.nearest_device(R.Points(d_q.ptr, 0, 12, 0, len(want)), max_dist, d_hits)
        got = d_hits.download(R.MAP_HIT, len(want))
        assert got.tobytes() == want.tobytes(), (max_dist, got, want)
        assert n == int((idx >= 0).sum())
    # the crop of the hand-worked keys: [0, 0.5]^3 keeps A and B (the face x = 0.5 belongs to voxel 1)
    assert m.crop((0, 0, 0), (0.5, 0.5, 0.5)) == 2
    assert m.export()[2].tolist() == [[0, 0, 0], [1, 0, 0]] and m.size() == (2, 2) and m.info()["slots"] == 4
    m.close()


def test_queries_change_nothing(gpu, clouds):
    xyz = clouds["g1_room"][:300_000]
    m = gpu.map_create(0.2)
    m.insert(np.concatenate([xyz, BAD]))
    before, size, info = m.export(), m.size(), m.info()
    q, _, _ = _queries(xyz, 0.2, 5)
    for max_dist in (0.1, np.inf):
        m.nearest(q, max_dist)
        m.nearest(_records(q[:1000]), max_dist)
    assert _same(before, m.export()) and m.size() == size and m.info() == info
    m.close()


def _grown_map(gpu):
    m = gpu.map_create(0.05, reserve_voxels=16)
    sweeps = [synth.g1_room(150_000, seed=100 + i, t_start=1000.0 + 0.5 * i) for i in range(20)]
    for s in sweeps:
        assert m.insert(s) == 0
    return m, np.concatenate([_xyz(s) for s in sweeps])


def test_query_after_growth_and_after_a_crop(gpu):
    m, union = _grown_map(gpu)
    assert m.info()["growths"] > 1
    v = 0.05
    q = _queries(union[::7], v, 9)[0]
    for step in ("grown", "cropped"):
        cen, cnt, keys = m.export()
        for max_dist in (v, np.inf):
            want, idx = Q.nearest_voxel(keys, cen, cnt, q, v, max_dist)
            assert 0 < (idx >= 0).sum() < len(q)
            _assert_hits_equal(m.nearest(q, max_dist), want, (step, max_dist))
        if step == "grown":
            assert m.crop((-3.0, -np.inf, -1.0), (4.0, 2.5, np.inf)) > 0
    m.close()


def test_shrink_to_fit_keeps_the_map_and_gives_memory_back(gpu):
    m, union = _grown_map(gpu)
    before, size, info = m.export(), m.size(), m.info()
    inf3 = (np.inf,) * 3
    assert m.crop(tuple(-x for x in inf3), inf3) == 0
    after = m.info()
    assert _same(before, m.export()) and m.size() == size
    assert after["slots"] == Q.pow2_at_least(2 * size[0]) and after["slots"] < info["slots"] and after["bytes"] < info["bytes"]
    assert after["rejected"] == info["rejected"] and after["growths"] == info["growths"]
    # a second one changes nothing; an insert afterwards grows the table again and finds every voxel
    assert m.crop(tuple(-x for x in inf3), inf3) == 0 and m.info() == after
    extra = _xyz(synth.g1_room(150_000, seed=77, t_start=2000.0))
    assert m.insert(extra) == 0
    ref = gpu.map_create(0.05)
    ref.insert(np.concatenate([union, extra]))
    assert _same(m.export(), ref.export()) and m.info()["slots"] >= 2 * m.size()[0]
    m.close()
    ref.close()


@pytest.mark.parametrize("v", [0.2, 0.5])
def test_crop_is_the_map_of_the_kept_points(gpu, clouds, v):
    """for every box: export() byte-equal to a fresh map of only the points whose voxel is kept, size(), the return value, the table
    size, `rejected` unchanged; then more sweeps go in and the map is that of (kept points u new points)"""
    xyz = clouds["g1_room"][:400_000]
    lo_all, hi_all = xyz.min(0).astype(np.float64), xyz.max(0).astype(np.float64)
    mid, ext = 0.5 * (lo_all + hi_all), hi_all - lo_all
    inf = np.inf
    on_faces_lo, on_faces_hi = np.floor((mid - 0.25 * ext) / v) * v, np.floor((mid + 0.25 * ext) / v) * v  # bounds on voxel faces
    boxes = [
        (mid - 0.2 * ext, mid + 0.3 * ext),  # interior
        (on_faces_lo, on_faces_hi),  # touching faces
        ((-inf, mid[1], -inf), (inf, inf, inf)),  # half-infinite
        ((-inf, -inf, -inf), (mid[0], inf, mid[2])),
        ((-inf, -inf, -inf), (inf, inf, inf)),  # all-infinite
        (hi_all + 100.0, hi_all + 200.0),  # disjoint from the map
        ((-inf, -inf, 5e6), (inf, inf, inf)),  # beyond the key range
    ]
    extra = _xyz(synth.g1_room(200_000, seed=31, t_start=3000.0))
    for lo, hi in boxes:
        m = gpu.map_create(v)
        assert m.insert(np.concatenate([xyz, BAD])) == len(BAD)
        voxels_before = m.size()[0]
        keep = Q.crop_keep(Q.point_keys(xyz, v), v, lo, hi)
        ref = gpu.map_create(v)
        ref.insert(xyz[keep])
        want = ref.export()
        kept = len(want[1])
        assert np.array_equal(Q.crop_keep(m.export()[2], v, lo, hi).sum(), kept)
        removed = m.crop(lo, hi)
        assert _same(m.export(), want), (lo, hi)
        assert m.size() == (kept, int(keep.sum())) and removed == voxels_before - kept, (lo, hi)
        info = m.info()
        assert info["slots"] == Q.pow2_at_least(2 * max(kept, 1)) and info["rejected"] == len(BAD), (lo, hi, info)
        # more sweeps after the crop
        for part in np.split(extra, 2):
            assert m.insert(part) == 0
            ref.insert(part)
        assert _same(m.export(), ref.export()) and m.size() == ref.size(), (lo, hi)
        assert m.info()["slots"] >= 2 * m.size()[0]
        m.close()
        ref.close()


def test_query_and_crop_api_edges(gpu, clouds):
    lib = gpu.lib
    pts = clouds["g1_room"][:100_000]
    a, b = gpu.map_create(0.2), gpu.map_create(0.05)
    a.insert(pts)
    b.insert(pts[:500])
    b_before = b.export()
    d_q = gpu.to_device(pts[:1000])
    d_hits = gpu.alloc(40 * 1000)
    desc = R.Points(d_q.ptr, 0, 12, 0, 1000)
    n = C.c_uint64(7)
    for d in (0.0, -1.0, float("nan")):
        assert lib.wc_map_nearest(gpu.h, a.h, C.byref(desc), C.c_double(d), C.c_void_p(d_hits.ptr), C.byref(n)) == WC_ERR_ARG
    assert lib.wc_map_nearest(gpu.h, None, C.byref(desc), C.c_double(1.0), C.c_void_p(d_hits.ptr), C.byref(n)) == WC_ERR_ARG
    assert lib.wc_map_nearest(gpu.h, a.h, C.byref(desc), C.c_double(1.0), None, C.byref(n)) == WC_ERR_ARG  # NULL d_hits, n > 0
    check_unreadable_points_refused(gpu, lambda bad: lib.wc_map_nearest(gpu.h, a.h, C.byref(bad), C.c_double(1.0), C.c_void_p(d_hits.ptr), C.byref(n)))
    empty = R.Points(0, 0, 12, 0, 0)
    assert lib.wc_map_nearest(gpu.h, a.h, C.byref(empty), C.c_double(1.0), None, C.byref(n)) == 0 and n.value == 0
    assert len(a.nearest(np.zeros((0, 3), np.float32))) == 0
    lo, hi = (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(1, 1, 1)
    assert lib.wc_map_crop(gpu.h, None, lo, hi, None) == WC_ERR_ARG
    assert lib.wc_map_crop(gpu.h, a.h, (C.c_double * 3)(0, 2, 0), hi, None) == WC_ERR_ARG
    assert lib.wc_map_crop(gpu.h, a.h, lo, (C.c_double * 3)(1, float("nan"), 1), None) == WC_ERR_ARG
    assert lib.wc_map_crop(gpu.h, a.h, None, hi, None) == WC_ERR_ARG
    # an empty map: queries miss, a crop removes nothing
    e = gpu.map_create(0.2)
    hits = e.nearest(pts[:100])
    assert not hits["count"].any() and np.all(np.isinf(hits["d2"])) and e.crop((-1, -1, -1), (1, 1, 1)) == 0 and e.size() == (0, 0)
    e.close()
    # NULL h_removed_voxels; the second map of the context stays untouched by the first one's queries and crop
    a.nearest(pts[:1000], 0.3)
    assert lib.wc_map_crop(gpu.h, a.h, lo, hi, None) == 0
    keys, cen, cnt, _ = downsample_voxel(pts, 0.2)
    assert a.size()[0] == int(Q.crop_keep(keys, 0.2, (0, 0, 0), (1, 1, 1)).sum())
    assert _same(b_before, b.export())
    for x in (d_q, d_hits):
        x.free()
    a.close()
    b.close()


def test_facade_keep_radius_query_and_crop(gpu):
    """the stream of test_facade_map_is_every_published_sweep_and_leaves_the_odometry_alone with map_keep_radius: the map is the numpy
    replay (after every sweep: append the published scan, keep the points whose voxel intersects the cube around the published tf
    origin); map_query is the restatement on the export; the odometry is the same with the radius on, off and with no map"""
    from wildcat_slam_amd import lib

    msgs, imu, _ = synth.raw_stream(1.7, pts_per_s=300_000, gyro_bias=(0.0, 0.0, 0.02), t_start=1000.0)
    v = 0.1
    radius = 10.0  # the room is 40 m x 30 m around the sensor (synth._room_hits): its far walls lie outside the cube on every sweep
    runs = []
    for mode in ("radius", "map", "none"):
        odo = lib.Odometry(0)
        odo.set_fill_outputs(True)
        if mode != "none":
            odo.set_map_voxel(v)
        if mode == "radius":
            with pytest.raises(lib.WildcatError):
                odo.set_map_keep_radius(-1.0)
            with pytest.raises(lib.WildcatError):
                odo.set_map_keep_radius(float("nan"))
            odo.set_map_keep_radius(radius)
        kept, dropped, states, last_scan = [np.zeros((0, 3), np.float32)], [], [], []

        def on_sweep():
            if mode == "radius":
                out = odo.outputs()
                scan = _xyz(out["scan"])
                c = np.asarray(out["tf"][1:4], np.float64)
                pts = np.concatenate([kept[0], scan])
                keep = Q.crop_keep(Q.point_keys(pts, v), v, c - radius, c + radius)
                dropped.append(len(np.unique(Q.point_keys(pts[~keep], v), axis=0)))
                kept[0] = pts[keep]
                last_scan[:] = [scan]
            st = odo.stats()
            states.append((odo.samples().tobytes(), st["binary"], st["unary"]))

        _drive(odo, msgs, imu, on_sweep)
        assert odo.sweeps() >= 2
        if mode == "radius":
            assert max(dropped) > 0, "the replay itself drops voxels"
            xyz, cnt = odo.map_export()
            keys, cen, ref_cnt, rej = downsample_voxel(kept[0], v)
            assert rej == 0 and odo.map_size() == (len(cnt), len(kept[0]), 0)
            assert np.array_equal(cnt, ref_cnt) and centroids_close(xyz, cen)
            assert odo.map_ms() > 0
            # the query of a published scan (the keys of the export are the replay's: exact)
            q = np.concatenate([last_scan[0], BAD])
            want, idx = Q.nearest_voxel(keys, xyz, cnt, q, v, v)
            assert 0 < (idx >= 0).sum() < len(q)
            _assert_hits_equal(odo.map_query(q, v), want, "facade")
            # CropMap
            inside = Q.crop_keep(keys, v, (-5, -5, -5), (5, 5, 5))
            assert odo.map_crop((-5, -5, -5), (5, 5, 5)) == int((~inside).sum())
            xyz2, cnt2 = odo.map_export()
            assert xyz2.tobytes() == xyz[inside].tobytes() and np.array_equal(cnt2, cnt[inside])
        elif mode == "none":
            hits = odo.map_query(BAD, 1.0)
            assert not hits["count"].any() and np.all(np.isinf(hits["d2"])) and odo.map_crop((0, 0, 0), (1, 1, 1)) == 0
        runs.append(states)
        odo.close()
    assert runs[0] == runs[1] == runs[2]
