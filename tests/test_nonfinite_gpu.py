"""The extraction's rule for non-finite points on the GPU (include/wildcat_hip.h): a point with a NaN or infinite x, y or z
contributes to nothing - no node's count, sums, time bins or clusters, no status flag whatever its stamp, not the key origin, and by
itself no reason to leave the default path.  So the surfels of a cloud are the surfels of the same cloud with those points removed, and
every test here compares a call on a dirty cloud (tests/nonfinite.py: points INSERTED into a clean one) with the call on the clean cloud:
count and ids equal, the surfels byte for byte whenever the two calls ended in the same arithmetic, and within the suite's bar between the
two arithmetics (helpers.check_surfels, 1e-6 / 1e-4 s) where they did not.  tests/test_nonfinite_ref.py shows on the CPU that the oracle
gives the clean cloud's surfels for every case and that the wrong rule (NaN -> voxel 0, inf saturates) fails every one."""
import contextlib

import numpy as np
import pytest

import helpers
import nonfinite as NF
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

pytestmark = pytest.mark.gpu

INT32_MIN = -(2**31)


def _hint(name):
    c = NF.cloud(name)
    return float(c["time"][0]), float(c["time"][-1])


def _same_or_close(got, got_fast, ref, ref_fast, what):
    """count and ids equal; bytes when the two calls ended in the same arithmetic, the bar between the two arithmetics otherwise"""
    (s, ids), (s0, ids0) = got, ref
    assert len(s) == len(s0), (what, len(s), len(s0))
    if got_fast == ref_fast:
        assert ids.tobytes() == ids0.tobytes(), what
        assert s.tobytes() == s0.tobytes(), what
    else:
        helpers.check_surfels(s, ids, s0, ids0, tol=1e-6, t_tol=1e-4)


@contextlib.contextmanager
def _mode(ctx, exact, split=-1):
    ctx.set_exact_sums(bool(exact))
    ctx.set_dev_option("fx_split", split)
    try:
        yield ctx
    finally:
        ctx.set_dev_option("fx_split", -1)
        ctx.set_exact_sums(False)


@contextlib.contextmanager
def _context(gpu, fresh):
    """fresh: a context of its own - which path a sweep takes depends on what a context remembers of earlier sweeps, and the tests
    that state the path must not depend on the tests that ran before them"""
    if not fresh:
        yield gpu
        return
    from wildcat_slam_amd import lib

    ctx = lib.Context(0)
    try:
        yield ctx
    finally:
        ctx.close()


MODES = [(1, -1), (0, 0), (0, 1)]  # (exact_sums, fx_split): the reference's summation order; the default arithmetic in both forms of its node stage


@pytest.mark.parametrize("exact,split", MODES, ids=["exact", "default-fused", "default-split"])
@pytest.mark.parametrize("case", NF.cases(), ids=lambda c: "%s-%s" % c)
def test_extraction_ignores_nonfinite_points(gpu, case, exact, split):
    name, pattern = case
    clean, dirty, removed = NF.case(name, pattern)
    pinned = name in ("lattice0", "far")
    with _context(gpu, pinned) as ctx, _mode(ctx, exact, split):
        ref = ctx.extract_surfels(clean, hint=_hint(name))
        info0 = ctx.extract_path_info()
        got = ctx.extract_surfels(dirty, hint=_hint(name))  # (rc 0: a return code raises)
        info1 = ctx.extract_path_info()
    print("\n%s / %s, exact %d, fx_split %d: %d + %d points, %d surfels; clean %s, dirty %s"
          % (name, pattern, exact, split, len(clean), len(removed), len(ref[0]), info0, info1))
    assert len(ref[0]) == 0 if pattern == "all" else len(ref[0]) > 0
    _same_or_close(got, info1["fast"], ref, info0["fast"], case)
    if pinned:  # a NaN return must not cost a sweep the default path, nor a second pipeline
        if not exact and pattern != "all":
            assert info0["fast"] and info0["runs"] == 1, info0  # (or the condition below would say nothing)
        if pattern == "all":
            assert info1["runs"] == 1, info1
        elif info0["fast"] and info0["runs"] == 1:
            assert info1["fast"] and info1["runs"] == 1, (info0, info1)


@pytest.mark.parametrize("exact", [0, 1], ids=["default", "exact"])
@pytest.mark.parametrize("name", NF.GATES)
def test_count_gates(gpu, oracle, name, exact):
    """five points (NaN, y, z) next to a patch of exactly min_points (cluster_min_points - 1) points, in a root whose x index is 0, must
    not push it over the gate; next to a patch of one point more they must not change its surfel"""
    c = NF.gate(name)
    s_orc, id_orc, _ = oracle.extract_surfels(c["clean"])
    with _mode(gpu, exact):
        ref = gpu.extract_surfels(c["clean"])
        info0 = gpu.extract_path_info()
        got = gpu.extract_surfels(c["dirty"])
        info1 = gpu.extract_path_info()
    print("\n%s, exact %d: %d surfels (oracle %d); clean %s, dirty %s" % (name, exact, len(got[0]), len(s_orc), info0, info1))
    assert len(ref[0]) == len(s_orc) and helpers.id_tuples(ref[1]) == helpers.id_tuples(id_orc)
    _same_or_close(got, info1["fast"], ref, info0["fast"], name)
    site = (got[1]["kx"] == NF.GATE_K[0]) & (got[1]["ky"] == NF.GATE_K[1]) & (got[1]["kz"] == NF.GATE_K[2])
    assert int(site.sum()) == (1 if c["emits"] else 0) + (1 if c["site"] == "l1" else 0)


def _enqueue(gpu, pts, layout, hint):
    """one sweep through wc_extract_surfels_enqueue / _finish in a point layout: the 48-byte record, or xyz | time arrays with an xyz
    stride of 12 (packed: the default path reads it directly) or 16 bytes"""
    n = len(pts)
    cap = max(1024, (3 * n) // 20 + 1)
    d_out, d_ids = gpu.alloc(cap * 144), gpu.alloc(cap * 16)
    if layout == "aos":
        d_p = gpu.to_device(pts)
        desc = gpu.points_desc(d_p, n)
    else:
        stride = int(layout[3:])
        xyz = np.zeros((n, stride // 4), np.float32)
        xyz[:, 0], xyz[:, 1], xyz[:, 2] = pts["x"], pts["y"], pts["z"]
        d_p, d_t = gpu.to_device(xyz), gpu.to_device(np.ascontiguousarray(pts["time"], np.float64))
        desc = R.Points(d_p.ptr, d_t.ptr, stride, 8, n)
        # soa12: what the default path reads directly, without staging (csrc/extract.hip, enqueue: xyz stride 12, time stride 8, both
        # arrays 16-byte aligned; k_fx_acc takes every FULL tile of such a sweep that way) - the caller asserts that path completed it
        assert stride != 12 or (d_p.ptr % 16 == 0 and d_t.ptr % 16 == 0 and n >= NF.KTILE)
    gpu.extract_enqueue(desc, d_out, d_ids, cap, *hint)
    m = gpu.extract_finish()
    return (d_out.download(R.SURFEL, m), d_ids.download(R.SURFEL_ID, m)), gpu.extract_path_info()


@pytest.mark.parametrize("layout", ["aos", "soa12", "soa16"])
@pytest.mark.parametrize("pattern", ["scatter", "runs"])
def test_layouts(gpu, pattern, layout):
    clean, dirty, _ = NF.case("lattice0", pattern)
    with _mode(gpu, 0):
        ref, info0 = _enqueue(gpu, clean, layout, _hint("lattice0"))
        got, info1 = _enqueue(gpu, dirty, layout, _hint("lattice0"))
    print("\n%s / %s: clean %s, dirty %s" % (pattern, layout, info0, info1))
    assert len(ref[0]) == 480
    assert info0["fast"] and info1["fast"], (info0, info1)  # the default path itself: for soa12 the packed direct loads of k_fx_acc
    _same_or_close(got, info1["fast"], ref, info0["fast"], (pattern, layout))


def test_batch(gpu):
    """one batch of five sweeps - a dirty lattice, a clean room, an empty sweep, a sweep without one finite point, a dirty room -
    run twice: every sweep of it is the single call on the same cloud byte for byte, and the clean cloud's surfels"""
    from wildcat_slam_amd import lib

    lat, room = NF.case("lattice0", "scatter"), NF.case("room_firing", "runs")
    sweeps = [("lattice0", lat[1], lat[0]), ("room_firing", room[0], room[0]), ("lattice0", lat[0][:0], lat[0][:0]),
              ("lattice0", NF.case("lattice0", "all")[1], lat[0][:0]), ("room_firing", room[1], room[0])]
    single, clean = [], []
    with _mode(gpu, 0):
        for name, pts, cl in sweeps:
            single.append((gpu.extract_surfels(pts, hint=_hint(name)), gpu.extract_path_info()["fast"]))
            clean.append((gpu.extract_surfels(cl, hint=_hint(name)), gpu.extract_path_info()["fast"]))
    for k in range(len(sweeps)):
        _same_or_close(single[k][0], single[k][1], clean[k][0], clean[k][1], ("single", k))
    ctx = lib.Context(0)
    try:
        jobs, keep = [], []
        for name, pts, _ in sweeps:
            n = len(pts)
            cap = max(1024, (3 * n) // 20 + 1)
            d_p, d_o, d_i = (ctx.to_device(pts) if n else ctx.alloc(48)), ctx.alloc(144 * cap), ctx.alloc(16 * cap)
            keep.append((d_p, d_o, d_i))
            jobs.append((ctx.points_desc(d_p, n), d_o, d_i, cap) + _hint(name))
        enq, fin = ctx.extract_batch_prepare(jobs)
        for rnd in range(2):
            enq()
            counts = fin()
            for k in range(len(sweeps)):
                s, ids = keep[k][1].download(R.SURFEL, counts[k]), keep[k][2].download(R.SURFEL_ID, counts[k])
                assert s.tobytes() == single[k][0][0].tobytes() and ids.tobytes() == single[k][0][1].tobytes(), (rnd, k)
    finally:
        ctx.close()
    assert [len(c[0][0]) for c in clean][2:4] == [0, 0]


@pytest.mark.parametrize("world,exact", [(2, 1), (3, 1), (2, 0), (3, 0)])
def test_sharded(gpu, world, exact):
    """the routed call: every dirty point has ONE defined owner (whose extraction drops it), the ranks' owned points add up to the dirty
    cloud, and the gathered + merged list is the unsharded CLEAN call's"""
    from test_route_gpu import _run_ranks

    a, b = NF.case("lattice0", "scatter"), NF.case("room_firing", "scatter")
    shift = float(a[0]["time"][-1]) + 1e-3 - float(b[0]["time"][0])
    parts = []
    for pts in (a[0], a[1], b[0], b[1]):
        parts.append(pts.copy())
    for pts in parts[2:]:
        pts["time"] += shift
    clean, dirty = synth.concat_points(parts[0], parts[2]), synth.concat_points(parts[1], parts[3])
    assert NF.same_records(dirty[NF.finite_rows(dirty)], clean)
    with _mode(gpu, exact):
        s_ref, i_ref = gpu.extract_surfels(clean)
        ref_fast = gpu.extract_path_info()["fast"]
    out = _run_ranks(world, dirty, exact=bool(exact))
    assert sum(o[0][2] for o in out) == len(dirty)
    assert sum(len(o[0][0]) for o in out) == len(s_ref) > 480  # (480: the lattice's own, by construction)
    same_arithmetic = exact or (ref_fast and all(o[0][3] for o in out))
    for r in range(world):
        ms, mi = out[r][1]
        if same_arithmetic:
            assert mi.tobytes() == i_ref.tobytes() and ms.tobytes() == s_ref.tobytes()
        else:
            assert len(ms) == len(s_ref)
            helpers.check_surfels(ms, mi, s_ref, i_ref, tol=1e-6, t_tol=1e-4)


def test_voxel_keys(gpu, oracle):
    """wc_voxel_keys: the oracle's index for every finite coordinate, INT32_MIN on an axis whose coordinate is not finite"""
    for name in ("lattice0", "room_firing"):
        _, dirty, removed = NF.case(name, "scatter")
        got, ref = gpu.voxel_keys(dirty), oracle.voxel_keys(dirty)
        fin = np.isfinite(NF.xyz(dirty))
        assert np.array_equal(got[fin], ref[fin])
        assert np.array_equal(got[fin.all(axis=1)], NF.voxels(dirty[fin.all(axis=1)]))
        assert (~fin).sum() >= len(removed) and np.all(got[~fin] == INT32_MIN)
        assert np.array_equal(got, ref)
    # beyond int32 (finite): the same value, as the reference's cast gives it
    far = helpers.point_records(np.array([[3e9, -3e9, 1.0], [np.float32(3.4e38), 0.0, -np.float32(3.4e38)]], np.float32))
    assert gpu.voxel_keys(far).tolist() == [[INT32_MIN, INT32_MIN, 1], [INT32_MIN, 0, INT32_MIN]] == oracle.voxel_keys(far).tolist()


def _ext_quat():
    return synth.mat_to_quat(synth.EXT_R[None])[0]


def test_undistort_passes_them_on(gpu):
    """the stages in front of the extraction keep their rule: the pre-filter keeps a NaN point (every comparison is false), the
    undistortion leaves every point that came in non-finite non-finite and every other point untouched - and the extraction at the
    end of that chain gives the clean message's surfels"""
    msg = synth.g1_room(40_000, t_start=1000.0)
    imu, _ = synth.imu_states(1000.0 - 0.0031, 1000.51, t_origin=1000.0)
    dirty, removed = NF.dirty(msg, "scatter")
    fin = NF.finite_rows(dirty)
    rec0, (xyz0, t0) = gpu.undistort_sweep(msg, imu), gpu.undistort_sweep_packed(msg, imu)
    rec1, (xyz1, t1) = gpu.undistort_sweep(dirty, imu), gpu.undistort_sweep_packed(dirty, imu)
    assert not NF.finite_rows(rec1)[~fin].any() and not np.isfinite(xyz1[~fin]).all(axis=1).any()
    assert NF.same_records(rec1[fin], rec0)
    assert xyz1[fin].tobytes() == xyz0.tobytes() and t1[fin].tobytes() == t0.tobytes() and np.array_equal(t1, dirty["time"])
    # pre-filter -> undistort_sweep_packed -> extraction (the packed arrays stay on the device)
    args = (_ext_quat(), synth.EXT_T, 0.3, 120.0, np.array([-0.8, -0.5, -0.4]), np.array([0.3, 0.5, 0.4]))
    res = []
    for pts in (msg, dirty):
        kept = gpu.prefilter_points(pts, *args)
        n = len(kept)
        d_xyz, d_t = gpu.undistort_sweep_packed(kept, imu, keep_on_device=True)
        cap = max(1024, (3 * n) // 20 + 1)
        d_out, d_ids = gpu.alloc(cap * 144), gpu.alloc(cap * 16)
        gpu.extract_enqueue(R.Points(d_xyz.ptr, d_t.ptr, 12, 8, n), d_out, d_ids, cap, 1000.0, 1000.51)
        m = gpu.extract_finish()
        res.append((kept, (d_out.download(R.SURFEL, m), d_ids.download(R.SURFEL_ID, m)), gpu.extract_path_info()["fast"]))
    k0, k1 = res[0][0], res[1][0]
    assert 0 < (~NF.finite_rows(k1)).sum() <= len(removed)  # the NaN points pass the pre-filter: every comparison is false
    assert NF.same_records(k1[NF.finite_rows(k1)], k0)
    assert len(res[0][1][0]) > 100
    _same_or_close(res[1][1], res[1][2], res[0][1], res[0][2], "chain")


def _drive(odo, msgs, imu, on_sweep):
    k = 0
    for msg in msgs:
        if len(msg) == 0:
            continue
        t_end = msg["time"][-1]
        while k < len(imu["t"]) and imu["t"][k] <= t_end + 0.02:
            odo.add_imu(imu["t"][k], imu["acc"][k], imu["gyr"][k])
            k += 1
        before = odo.sweeps()
        odo.add_scan(msg)
        if odo.sweeps() != before:
            on_sweep()


@pytest.mark.parametrize("exact", [1, 0], ids=["exact-sums", "default-arithmetic"])
def test_facade(gpu, exact):
    """a raw stream with 1 % NaN returns ("no return" of a lidar driver) through the facade: the odometry is the clean stream's - per
    published sweep the sample states and pair counts in the exact arithmetic, the pair counts in the default one - and the map
    rejects exactly the NaN points of the published sweeps"""
    from wildcat_slam_amd import lib

    msgs, imu, _ = synth.raw_stream(1.7, pts_per_s=300_000, gyro_bias=(0.0, 0.0, 0.02), t_start=1000.0)
    rng = np.random.default_rng(3)
    noisy = []
    for m in msgs:
        k = len(m) // 100
        at = np.sort(rng.integers(0, len(m) + 1, k)) if len(m) else np.zeros(0, np.int64)
        noisy.append(NF.insert(m, at, np.full((k, 3), np.nan, np.float32))[0] if k else m)
    runs = []
    for stream in (msgs, noisy):
        odo = lib.Odometry(0)
        odo.set_exact_sums(bool(exact))
        odo.set_fill_outputs(True)
        odo.set_map_voxel(0.1)
        states, bad, good = [], [], []

        def on_sweep():
            st = odo.stats()
            states.append((odo.samples().tobytes(), st["binary"], st["unary"]))
            f = NF.finite_rows(odo.outputs()["scan"])
            bad.append(int((~f).sum())), good.append(int(f.sum()))

        _drive(odo, stream, imu, on_sweep)
        assert odo.sweeps() >= 2
        size = odo.map_size()
        assert size[1] == sum(good) and size[2] == sum(bad), (size, good, bad)
        runs.append((states, bad, good))
        odo.close()
    (s0, bad0, good0), (s1, bad1, good1) = runs
    assert sum(bad0) == 0 and sum(bad1) > 1000 and good0 == good1
    assert len(s0) == len(s1)
    if exact:
        assert s0 == s1
    else:
        assert [s[1:] for s in s0] == [s[1:] for s in s1]
