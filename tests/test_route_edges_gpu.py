"""The routed cloud (csrc/route.hip) at its edges, on one GPU, against tests/route_ref.py - a restatement that owes nothing to the
library (Python-integer hash, numpy voxel index, sorted()): the partition kernels at every size that ends inside a wavefront, a
256-lane iteration or a 2048-point tile, for 1 ... 64 owners, with prescribed owner sequences, voxel-rule edge points, strided layouts,
a context reused with smaller clouds, and the refusals; the k-way surfel merge on crafted lists whose order its tie rules alone decide;
the sharded call and the gather with ranks that own nothing, empty slices, a zero total and a short buffer.  Every comparison is byte
equality.  The inputs are tests/route_cases.py; tests/test_route_ref.py asserts without a GPU that each is what it claims."""
import ctypes as C
import threading

import numpy as np
import pytest

import route_cases as RC
import route_ref as RR
from wildcat_slam_amd import dist as wdist
from wildcat_slam_amd import lib
from wildcat_slam_amd import records as R

pytestmark = pytest.mark.gpu

WC_OK, WC_ERR_CAPACITY, WC_ERR_ARG = 0, 1, 11
FILL = 0xA5  # what the outputs hold before a call: a record the call leaves unwritten shows
_HASHES = {}


def _hashes(name, pts, voxel):
    """the Python hashes of a cloud's voxels, once per cloud (the owner is hash % world)"""
    key = (name, float(voxel))
    if key not in _HASHES:
        _HASHES[key] = RR.hashes_of(RR.route_voxel(RR.xyz_of(pts), voxel))
    return _HASHES[key]


def _first_diff(got, want):
    g, w = np.frombuffer(got.tobytes(), np.uint8).reshape(-1, got.dtype.itemsize), np.frombuffer(want.tobytes(), np.uint8).reshape(-1, want.dtype.itemsize)
    bad = np.flatnonzero((g != w).any(1))
    return "%d records differ, the first at %d: got %s, want %s" % (len(bad), bad[0], got[bad[0]], want[bad[0]]) if len(bad) else "equal"


def _check_partition(ctx, pts, world, hashes, desc=None, keep=None):
    """one wc_route_partition call against partition_ref: the counts, their sum, and every byte of the 24-byte records (x, y, z, t as
    bit patterns, src == 0) -> the records"""
    n = len(pts)
    d_pts = (ctx.to_device(pts) if n else ctx.alloc(48)) if desc is None else None
    d_send, counts = ctx.route_partition(d_pts, n, world, desc=desc, fill=FILL)
    got = d_send.download(R.ROUTE_POINT, n)
    want, want_counts = RC.expected(pts, RR.partition_ref(pts, None, world, hashes))
    assert [int(c) for c in counts] == want_counts and int(counts.sum()) == n, (n, world)
    assert got.tobytes() == want.tobytes(), (n, world, _first_diff(got, want))
    assert not got["src"].any()
    for b in (d_pts, d_send):
        if b:
            b.free()
    return got


# ---- the partition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", RC.NS)
def test_partition_sizes_and_worlds(gpu, n):
    """a random cloud cut to every size that ends inside a wavefront, a 256-lane iteration or a 2048-point tile, for 1 ... 64 owners"""
    cloud = RC.random_cloud(RC.N_MAX)
    hashes = _hashes("random", cloud, RC.V_DEFAULT)
    for world in RC.WORLDS:
        _check_partition(gpu, cloud[:n], world, hashes[:n])


@pytest.mark.parametrize("world", RC.SEQ_WORLDS)
@pytest.mark.parametrize("name", sorted(RC.SEQS))
def test_partition_prescribed_owner_sequences(gpu, name, world):
    """one owner throughout; all owners cycling lane by lane (64 distinct owners in one wavefront at world 64); the owner changing exactly
    at 64, 256 and 2048; a random sequence - stamps strictly ascending, so an unstable partition shows"""
    seq = RC.SEQS[name](RC.N_MAX, world)
    pts = RC.owner_cloud(world, seq)
    got = _check_partition(gpu, pts, world, _hashes(("seq", name, world), pts, RC.V_DEFAULT))
    o = 0
    for r in range(world):  # what the restatement says, said once more from the prescription itself
        mine = pts["time"][seq == r]
        assert np.array_equal(got["t"][o : o + len(mine)], mine)
        o += len(mine)


@pytest.mark.parametrize("voxel", [0.8, 0.2, 0.5])
def test_partition_voxel_rule_edges(gpu, oracle, voxel):
    """faces and their float neighbours, negatives, -0.0 and subnormals, quotients next to and beyond int32, NaN and +-inf, mixed into a
    random cloud: the owner follows floor(p / voxel) in float64 with INT32_MIN for what does not fit - at the default voxel size and,
    through set_params, at 0.2f and 0.5f"""
    v32 = np.float32(voxel)
    P = oracle.default_params()
    P.voxel_size = float(v32)
    pts = RC.edge_cloud(v32)
    try:
        gpu.set_params(P)
        for world in (2, 3, 64):
            _check_partition(gpu, pts, world, _hashes("edge", pts, v32))
    finally:
        gpu.set_params(oracle.default_params())


def test_partition_layouts(gpu):
    """the same cloud as 48-byte records, as packed xyz (stride 12) with a separate array of doubles, with stride 16, and as 24-byte
    routed records: byte-equal results"""
    pts = RC.random_cloud(4097, seed=5)
    n, world = len(pts), 7
    hashes = _hashes("layouts", pts, RC.V_DEFAULT)
    ref = _check_partition(gpu, pts, world, hashes)
    xyz, t = RR.xyz_of(pts), np.ascontiguousarray(pts["time"])
    d_t = gpu.to_device(t)
    d_xyz = gpu.to_device(xyz)
    got = _check_partition(gpu, pts, world, hashes, desc=R.Points(d_xyz.ptr, d_t.ptr, 12, 8, n))
    assert got.tobytes() == ref.tobytes()
    xyzw = np.full((n, 4), np.float32(np.nan))
    xyzw[:, :3] = xyz
    d_xyzw = gpu.to_device(xyzw)
    got = _check_partition(gpu, pts, world, hashes, desc=R.Points(d_xyzw.ptr, d_t.ptr, 16, 8, n))
    assert got.tobytes() == ref.tobytes()
    rp = np.zeros(n, R.ROUTE_POINT)
    rp["x"], rp["y"], rp["z"], rp["t"], rp["src"] = pts["x"], pts["y"], pts["z"], pts["time"], 0xDEADBEEF
    d_rp = gpu.to_device(rp)
    got = _check_partition(gpu, pts, world, hashes, desc=gpu.route_desc(d_rp, n))
    assert got.tobytes() == ref.tobytes()


def test_partition_one_context_in_sequence():
    """the scratch and the total cell are reused: a large call, then smaller ones, then none, each right on its own"""
    ctx = lib.Context(0)
    try:
        cloud = RC.random_cloud(RC.N_MAX)
        hashes = _hashes("random", cloud, RC.V_DEFAULT)
        for n, world in ((6143, 64), (1, 1), (2049, 3)):
            _check_partition(ctx, cloud[:n], world, hashes[:n])
        d_send, counts = ctx.route_partition(ctx.alloc(48), 0, 5, fill=FILL)
        assert counts.tolist() == [0] * 5 and (d_send.download(np.uint8, 24) == FILL).all()
        counts = (C.c_uint64 * 3)(7, 7, 7)
        desc = R.Points(0, 0, 48, 48, 0)
        assert ctx.lib.wc_route_partition(ctx.h, C.byref(desc), C.c_int(3), None, counts) == WC_OK and list(counts) == [0, 0, 0]
        _check_partition(ctx, cloud[:257], 8, hashes[:257])
    finally:
        ctx.close()


def test_partition_refusals():
    ctx = lib.Context(0)
    try:
        cloud = RC.random_cloud(300, seed=9)
        hashes = RR.hashes_of(RR.route_voxel(RR.xyz_of(cloud), RC.V_DEFAULT))
        d_pts, d_send = ctx.to_device(cloud), ctx.alloc(24 * 300)
        desc = ctx.points_desc(d_pts, 300)
        counts = (C.c_uint64 * 65)()
        f = ctx.lib.wc_route_partition
        for world, out, cnt in ((0, d_send.ptr, counts), (65, d_send.ptr, counts), (3, d_send.ptr, None), (3, 0, counts)):
            assert f(ctx.h, C.byref(desc), C.c_int(world), C.c_void_p(out), cnt) == WC_ERR_ARG, (world, out, cnt is None)
            _check_partition(ctx, cloud, 3, hashes)
    finally:
        ctx.close()


# ---- the k-way merge -----------------------------------------------------------------------------------------------------------------
def _check_merge(ctx, c, want_ids=True):
    lists, ids = c["lists"], c["ids"]
    order = RR.merge_ref(lists, ids)
    ms, mi = ctx.merge_surfels(lists, ids, want_ids=want_ids, fill=FILL)
    want = RR.take(lists, order, R.SURFEL)
    assert ms.tobytes() == want.tobytes(), _first_diff(ms, want)
    if ids is not None and want_ids:
        want_i = RR.take(ids, order, R.SURFEL_ID)
        assert mi.tobytes() == want_i.tobytes(), _first_diff(mi, want_i)
    else:
        assert mi is None


@pytest.mark.parametrize("name", sorted(RC.merge_cases()))
def test_merge_crafted_lists(gpu, name):
    """k = 1 and 64, empty lists, one long list among singletons, totals around a workgroup, lists wholly in front and behind, equal stamps
    (ids alone order: negative indices, node ids across 2^31), the same (t, id) in 2, 3 and 64 lists, no ids at all: equal keys from a list
    in front go first, then position"""
    _check_merge(gpu, RC.merge_cases()[name])


@pytest.mark.parametrize("name", ["equal_stamps", "dups", "big_and_singletons"])
def test_merge_ids_in_and_no_id_output(gpu, name):
    """the ids steer the merge, only the surfels are written"""
    _check_merge(gpu, RC.merge_cases()[name], want_ids=False)


def test_merge_refusals(gpu):
    c = RC.merge_cases()["total_257"]
    s, i = np.concatenate(c["lists"]), np.concatenate(c["ids"])
    d_in, d_ids, d_out, d_oid = gpu.to_device(s), gpu.to_device(i), gpu.alloc(144 * 257), gpu.alloc(16 * 257)
    counts = (C.c_uint64 * 65)(*[len(a) for a in c["lists"]])
    f = gpu.lib.wc_merge_surfels
    for k, out, cnt in ((0, d_out.ptr, counts), (65, d_out.ptr, counts), (3, d_in.ptr, counts), (3, d_out.ptr, None)):
        assert f(gpu.h, C.c_void_p(d_in.ptr), C.c_void_p(d_ids.ptr), cnt, C.c_int(k), C.c_void_p(out), C.c_void_p(d_oid.ptr)) == WC_ERR_ARG, (k, cnt is None)
        _check_merge(gpu, c)
    zeros = (C.c_uint64 * 64)()
    for k in (1, 64):  # all counts zero, null buffers
        assert f(gpu.h, None, None, zeros, C.c_int(k), None, None) == WC_OK


# ---- the sharded call and the gather ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    """eight contexts (with the session's: nine alive), in the reference's summation order: a rank's surfels are then the unsharded call's
    bit for bit whichever arithmetic the unsharded call would have ended in"""
    ctxs = [lib.Context(0) for _ in range(8)]
    for c in ctxs:
        c.set_exact_sums(True)
    yield ctxs
    for c in ctxs:
        c.close()


def _ranks(ctxs, fn, timeout=120):
    """fn(rank, ctx, shared) on one thread per context, a dist.ThreadComm between them; a rank that raises aborts the barrier, so no
    other is left waiting -> the ranks' results"""
    world = len(ctxs)
    shared = wdist.ThreadComm.shared(world)
    out, errors = [None] * world, []

    def run(r):
        try:
            ctxs[r].set_comm(wdist.ThreadComm(shared, r, ctxs[r]))
            out[r] = fn(r, ctxs[r], shared)
        except Exception as e:  # pragma: no cover
            errors.append((r, repr(e)))
            shared["bar"].abort()

    th = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=timeout)
    assert not any(t.is_alive() for t in th), "a rank did not return"
    for c in ctxs:
        c.set_comm(None)
    assert not errors, errors
    return out, shared


def _unsharded(gpu, pts):
    gpu.set_exact_sums(True)
    try:
        return gpu.extract_surfels(pts)
    finally:
        gpu.set_exact_sums(False)


def _sharded(ctx, r, world, pts):
    """this rank's time-contiguous slice through wc_extract_surfels_sharded -> (d_surfels, d_ids, surfels, points owned)"""
    lo, cnt = wdist.shard_range(len(pts), r, world)
    d_slice = ctx.to_device(pts[lo : lo + cnt]) if cnt else ctx.alloc(48)
    return ctx.extract_surfels_sharded(d_slice, cnt, float(pts["time"][0]), float(pts["time"][-1]), cap=2048)


def _local(d_s, d_i, m):
    return d_s.download(R.SURFEL, m), d_i.download(R.SURFEL_ID, m)


def test_sharded_one_root_voxel_two_ranks_own_nothing(gpu, pool):
    pts, info = RC.one_root_cloud()
    s_ref, i_ref = _unsharded(gpu, pts)
    assert len(s_ref) == 8
    owner = RR.route_owner(*[int(k) for k in info["root_keys"][0]], 3)

    def fn(r, ctx, shared):
        d_s, d_i, m, owned = _sharded(ctx, r, 3, pts)
        return m, owned, ctx.gather_surfels(d_s, d_i, m, cap=8)

    out, _ = _ranks(pool[:3], fn)
    for r, (m, owned, (ms, mi)) in enumerate(out):
        assert (m, owned) == ((8, 256) if r == owner else (0, 0)), r  # the extraction of nothing returns nothing
        assert ms.tobytes() == s_ref.tobytes() and mi.tobytes() == i_ref.tobytes(), r


@pytest.mark.parametrize("world", [2, 3, 5, 8])
def test_sharded_lattice_equals_unsharded(gpu, pool, world):
    pts, info = RC.lattice12()
    s_ref, i_ref = _unsharded(gpu, pts)
    assert len(s_ref) == 96
    owners = RC.owners_of_roots(info, world)

    def fn(r, ctx, shared):
        d_s, d_i, m, owned = _sharded(ctx, r, world, pts)
        return m, owned, _local(d_s, d_i, m), ctx.gather_surfels(d_s, d_i, m, cap=96)

    out, shared = _ranks(pool[:world], fn)
    assert sum(o[1] for o in out) == len(pts)
    for r, (m, owned, (ls, li), (ms, mi)) in enumerate(out):
        assert owned == 256 * owners.count(r) and m == 8 * owners.count(r), r  # by the Python hash
        assert set(RR.route_owner(int(a), int(b), int(c), world) for a, b, c in zip(li["kx"], li["ky"], li["kz"])) <= {r}
        assert ms.tobytes() == s_ref.tobytes() and mi.tobytes() == i_ref.tobytes(), r
    if world == 8:
        assert any(o[0] == 0 and o[1] == 0 for o in out)  # a rank that owns no voxel
    assert wdist.ThreadComm.counts(shared, "alltoallv") == [2] * world and wdist.ThreadComm.counts(shared, "allgatherv") == [3] * world


def test_sharded_two_points_three_ranks_total_zero(pool):
    pts = RC.random_cloud(2, seed=21)

    def fn(r, ctx, shared):
        d_s, d_i, m, owned = _sharded(ctx, r, 3, pts)
        d_out, d_oid = ctx.alloc(144), ctx.alloc(16)
        return m, owned, ctx.gather_surfels_device(d_s, d_i, m, d_out, d_oid, 0, want_rc=True)

    out, _ = _ranks(pool[:3], fn)
    assert [o[0] for o in out] == [0, 0, 0] and sum(o[1] for o in out) == 2
    assert [o[1] for o in out] == [len(s) for s in RR.partition_ref(pts, RC.V_DEFAULT, 3)]
    assert all(o[2] == (WC_OK, 0) for o in out)


def test_gather_capacity(gpu, pool):
    """cap equal to the total is fine; one less is WC_ERR_CAPACITY on every rank with the total in *h_n_out; the next sharded call and
    gather on the same contexts are right"""
    pts, _ = RC.lattice12()
    s_ref, i_ref = _unsharded(gpu, pts)
    total = len(s_ref)

    def fn(r, ctx, shared):
        d_s, d_i, m, _ = _sharded(ctx, r, 3, pts)
        d_out, d_oid = ctx.alloc(144 * total), ctx.alloc(16 * total)
        res = []
        for cap in (total, total - 1):
            d_out.upload(np.full(144 * total, FILL, np.uint8))
            rc, n = ctx.gather_surfels_device(d_s, d_i, m, d_out, d_oid, cap, want_rc=True)
            res.append((rc, n, d_out.download(R.SURFEL, total), d_oid.download(R.SURFEL_ID, total)))
        d_s, d_i, m, _ = _sharded(ctx, r, 3, pts)
        return res, ctx.gather_surfels(d_s, d_i, m, cap=total)

    out, _ = _ranks(pool[:3], fn)
    for r, (res, (ms, mi)) in enumerate(out):
        assert res[0][:2] == (WC_OK, total) and res[0][2].tobytes() == s_ref.tobytes() and res[0][3].tobytes() == i_ref.tobytes(), r
        assert res[1][:2] == (WC_ERR_CAPACITY, total), r
        assert ms.tobytes() == s_ref.tobytes() and mi.tobytes() == i_ref.tobytes(), r


def test_gather_null_ids(gpu, pool):
    """no ids in and none out: the lists merge by their stamps, ties in rank order; ids in and none out: the unsharded surfels"""
    pts, _ = RC.lattice12()
    s_ref, _ = _unsharded(gpu, pts)

    def fn(r, ctx, shared):
        d_s, d_i, m, _ = _sharded(ctx, r, 5, pts)
        return _local(d_s, d_i, m), ctx.gather_surfels(d_s, None, m, cap=96), ctx.gather_surfels(d_s, d_i, m, cap=96, want_ids=False)

    out, _ = _ranks(pool[:5], fn)
    lists = [o[0][0] for o in out]
    want = RR.take(lists, RR.merge_ref(lists), R.SURFEL)
    for r, (_, (ms, mi), (ms2, mi2)) in enumerate(out):
        assert mi is None and mi2 is None
        assert ms.tobytes() == want.tobytes() and ms2.tobytes() == s_ref.tobytes(), r


def test_sharded_refusals_enter_no_collective(pool):
    ctx = pool[0]
    pts, _ = RC.one_root_cloud()
    d_pts = ctx.to_device(pts)
    d_s, d_i = ctx.alloc(144 * 64), ctx.alloc(16 * 64)
    t_lo, t_hi = float(pts["time"][0]), float(pts["time"][-1])
    # no communicator installed
    with pytest.raises(lib.WildcatError) as e:
        ctx.extract_surfels_sharded(d_pts, len(pts), t_lo, t_hi, out=(d_s, d_i, 64))
    assert e.value.code == WC_ERR_ARG
    assert ctx.gather_surfels_device(d_s, d_i, 0, d_s, d_i, 64, want_rc=True)[0] == WC_ERR_ARG
    # t_lo > t_hi, on one rank of two: it returns without waiting for the other
    shared = wdist.ThreadComm.shared(2)
    ctx.set_comm(wdist.ThreadComm(shared, 0, ctx))
    try:
        with pytest.raises(lib.WildcatError) as e:
            ctx.extract_surfels_sharded(d_pts, len(pts), t_hi, t_lo, out=(d_s, d_i, 64))
        assert e.value.code == WC_ERR_ARG
        assert all(wdist.ThreadComm.counts(shared, k) == [0, 0] for k in (None, "allreduce", "alltoallv", "allgatherv"))
    finally:
        ctx.set_comm(None)
