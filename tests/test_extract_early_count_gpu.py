"""The early count of the default extraction path: k_slot_emit's last workgroup stores the sweep's surfel count, layer-2 queue length
and bin-overflow flag to the pinned mailbox as it starts (two 64-bit words under the sweep's ticket, csrc/extract_plan.h: ex_mail_*),
and wc_extract_surfels_finish returns on them - while the kernel may still be copying surfels.  The surfels are complete in the order
of the context's stream, which is where every download below reads them.  What must hold: the host never sees another sweep's count
or flags, no store of a sweep's k_slot_emit lands in the mailbox the host has cleared for the next sweep, and every byte equals what
the full stream wait (development option ex_sync = 1) gives."""
import ctypes as C
import time

import numpy as np
import pytest

import helpers
from wildcat_slam_amd import lib
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

pytestmark = pytest.mark.gpu

FX, WIDE, RUN_SORT, BIN_ORDER = 1, 2, 4, 8  # extract_path_info()["path"]: bits of csrc/extract_plan.h's ExPath


class Cloud:
    """a cloud resident on a context, with its hint"""

    def __init__(self, ctx, pts):
        self.pts, self.n = pts, len(pts)
        self.d = ctx.to_device(pts) if self.n else ctx.alloc(48)
        self.desc = ctx.points_desc(self.d, self.n)
        self.hint = (float(pts["time"][0]), float(pts["time"][-1])) if self.n else (1.0, 0.0)
        self.cap = max(1024, (3 * self.n) // 20 + 1)


class Out:
    def __init__(self, ctx, cap):
        self.cap = cap
        self.d_out, self.d_ids = ctx.alloc(cap * 144), ctx.alloc(cap * 16)

    def get(self, m):
        """(count, surfel bytes, id bytes): a download on the context's stream"""
        return m, self.d_out.download(R.SURFEL, m).tobytes(), self.d_ids.download(R.SURFEL_ID, m).tobytes()


def sweep(ctx, cloud, out, hint=None, cap=None):
    """the split form, nothing in between: -> surfel count"""
    t_lo, t_hi = hint or cloud.hint
    ctx.extract_enqueue(cloud.desc, out.d_out, out.d_ids, out.cap if cap is None else cap, t_lo, t_hi)
    return ctx.extract_finish()


def recorded(ctx, cloud, out):
    """the sweep's (count, bytes, bytes) under the full stream wait"""
    ctx.set_dev_option("ex_sync", 1)
    try:
        return out.get(sweep(ctx, cloud, out))
    finally:
        ctx.set_dev_option("ex_sync", 0)


@pytest.fixture(scope="module")
def small_clouds():
    return [synth.g2_lattice(300, m=32)[0], synth.g2_lattice(77, m=24)[0], synth.g1_room(60_000, seed=5)]


@pytest.fixture(scope="module")
def on_gpu(gpu, small_clouds):
    """the three small clouds on the shared context, and what ex_sync = 1 gives for each (recorded once, never changed)"""
    gpu.set_exact_sums(False)
    clouds = [Cloud(gpu, p) for p in small_clouds]
    cap = max(c.cap for c in clouds)
    bufs = [Out(gpu, cap), Out(gpu, cap)]
    want = [recorded(gpu, c, bufs[0]) for c in clouds]
    assert len({w[0] for w in want}) == len(clouds) and all(w[0] > 0 for w in want)  # (a foreign count would show)
    return clouds, bufs, want


@pytest.fixture
def fresh_gpu():
    ctx = lib.Context(0)
    yield ctx
    ctx.close()


def _pairs(reps):
    """(X, Y) of every alternation: the walk over the three clouds steps by one or by two, so pairs occur in both directions and no
    cloud runs twice in a row (a sweep the default path hands to the exact path twice running would send the NEXT sweep there
    directly - extract_plan.h's back-off - and the exact path's bytes are not the default path's)"""
    seq, cur = [], 0
    for k in range(2 * reps):
        seq.append(cur)
        cur = (cur + 1 + (k // 5) % 2) % 3
    return list(zip(seq[0::2], seq[1::2]))


def test_back_to_back_into_different_buffers(gpu, on_gpu):
    """X -> A, finish; at once Y -> B, finish; only then A and B are read: the second sweep's kernels queue behind the first one's
    k_slot_emit, and the host has cleared the mailbox for Y while X's copy may still be running"""
    clouds, (A, B), want = on_gpu
    for rep, (i, j) in enumerate(_pairs(60)):
        nx = sweep(gpu, clouds[i], A)
        ny = sweep(gpu, clouds[j], B)
        assert (nx, ny) == (want[i][0], want[j][0]), (rep, i, j, nx, ny)
        assert A.get(nx) == want[i], (rep, i)
        assert B.get(ny) == want[j], (rep, j)


def test_back_to_back_into_one_buffer(gpu, on_gpu):
    """the same with one output buffer, read between the sweeps: the download is ordered behind k_slot_emit on the stream"""
    clouds, (A, _), want = on_gpu
    for rep, (i, j) in enumerate(_pairs(60)):
        assert A.get(sweep(gpu, clouds[i], A)) == want[i], (rep, i)
        assert A.get(sweep(gpu, clouds[j], A)) == want[j], (rep, j)


def test_bin_overflow_is_reported_and_stays_out_of_the_next_mailbox(fresh_gpu, oracle, small_clouds):
    """the wide-hint sweep of test_extract_gpu.py: every surfel in one time bin.  The flag travels in word B; the workgroups that meet
    the overfull bin must not touch the mailbox, which belongs to the next sweep once finish() has returned"""
    ctx = fresh_gpu
    pts = small_clouds[0]
    s_ref, id_ref, _ = oracle.extract_surfels(pts)
    c = Cloud(ctx, pts)
    A, B = Out(ctx, c.cap), Out(ctx, c.cap)
    t0, t1 = c.hint
    n_wide = sweep(ctx, c, A, hint=(t0 - 1.0, t1 + 2000.0))
    info = ctx.extract_path_info()
    assert info["runs"] == 2 and info["fallbacks"] == 1 and info["flags"] == 16 and not info["fast"], info
    n_reg = sweep(ctx, c, B)  # immediately after
    info = ctx.extract_path_info()
    assert info["runs"] == 1 and info["fast"] and info["path"] == FX | BIN_ORDER and info["flags"] == 0 and info["fallbacks"] == 1, info
    assert n_wide == n_reg == len(s_ref)
    for out in (A, B):
        helpers.check_surfels(out.d_out.download(R.SURFEL, n_reg), out.d_ids.download(R.SURFEL_ID, n_reg), s_ref, id_ref, tol=1e-6, t_tol=1e-5)


ROOM_L2 = 155_000  # the smallest g1_room, in steps of 5 000 points, that reaches octree layer 2 (150 000: nodes_tested[2] == 0)


def test_late_layer2_pass(fresh_gpu, oracle, small_clouds):
    """a regular sweep queues nothing for layer 2, so the room that follows starts without the layer-2 launches: finish() learns the
    queue length from word B, runs the pass and a second k_slot_emit under a fresh ticket, and the next regular sweep is as ever"""
    ctx = fresh_gpu
    room = synth.g1_room(ROOM_L2)
    s_ref, id_ref, st = oracle.extract_surfels(room)
    assert st.nodes_tested[2] > 0
    reg_ref = oracle.extract_surfels(small_clouds[0])
    regular, big = Cloud(ctx, small_clouds[0]), Cloud(ctx, room)
    out = Out(ctx, big.cap)
    want_reg, want_room = recorded(ctx, regular, out), recorded(ctx, big, out)
    assert want_room[0] == len(s_ref) and want_reg[0] == len(reg_ref[0])
    assert out.get(sweep(ctx, regular, out)) == want_reg  # (leaves last_splits == 0: the room's layer-2 pair is not launched)
    got = out.get(sweep(ctx, big, out))
    ids = np.frombuffer(got[2], R.SURFEL_ID)
    assert set(helpers.id_tuples(ids)) == set(helpers.id_tuples(id_ref)) and len(ids) == len(id_ref)
    assert got == want_room
    assert ctx.extract_path_info()["fast"]
    assert out.get(sweep(ctx, regular, out)) == want_reg


def test_capacity_error_reports_the_count(gpu, on_gpu):
    clouds, (A, _), want = on_gpu
    n = C.c_uint64(0)
    gpu.extract_enqueue(clouds[0].desc, A.d_out, A.d_ids, 10, *clouds[0].hint)
    rc = gpu.lib.wc_extract_surfels_finish(gpu.h, C.byref(n))
    assert rc == lib.WC_ERR_CAPACITY and int(n.value) == want[0][0]
    with pytest.raises(lib.WildcatError) as e:
        sweep(gpu, clouds[1], A, cap=want[1][0] - 1)
    assert e.value.code == lib.WC_ERR_CAPACITY
    for i in (1, 0):  # the next sweeps are unaffected
        assert A.get(sweep(gpu, clouds[i], A)) == want[i]


def test_zero_results_do_not_wait_out_the_timeout(gpu, on_gpu):
    """no surfel at all: the words still arrive (count 0 under the sweep's ticket) - finish() must not sit out its 20 ms fallback"""
    clouds, (A, _), want = on_gpu
    tiny = Cloud(gpu, synth.g2_lattice(1, m=5)[0][:10])
    empty = Cloud(gpu, np.zeros(0, R.POINT))
    for c in (tiny, empty):
        assert sweep(gpu, c, A) == 0  # (the first call on a size may allocate)
        t0 = time.perf_counter()
        m = sweep(gpu, c, A)
        dt = time.perf_counter() - t0
        assert m == 0 and dt < 5e-3, (c.n, m, dt)
    assert A.get(sweep(gpu, clouds[0], A)) == want[0]


def test_forms_without_a_ticket_agree(gpu, on_gpu):
    """stage events (every stage, or the bracket only) and ex_sync = 1 run k_slot_emit without a ticket: plain mailbox words, stream wait"""
    clouds, (A, _), want = on_gpu
    keys = {"init", "point_sort", "roots_stream", "roots_emit", "slot_order"}
    try:
        for mode in (True, 2):
            gpu.extract_profile(mode)
            for i in range(3):
                assert A.get(sweep(gpu, clouds[i], A)) == want[i], (mode, i)
                assert set(gpu.extract_stage_ms()) == keys
    finally:
        gpu.extract_profile(False)
    gpu.set_dev_option("ex_sync", 1)
    try:
        for i in range(3):
            assert A.get(sweep(gpu, clouds[i], A)) == want[i], i
    finally:
        gpu.set_dev_option("ex_sync", 0)
    for i in range(3):  # and with the ticket again
        assert A.get(sweep(gpu, clouds[i], A)) == want[i], i


def test_two_contexts_keep_their_own_counts(gpu, on_gpu, small_clouds):
    """each context has its own mailbox and its own ticket sequence: sweeps of two contexts in flight together"""
    clouds, (A, _), want = on_gpu
    other = lib.Context(0)
    try:
        o_clouds = [Cloud(other, p) for p in small_clouds]
        B = Out(other, A.cap)
        for rep in range(40):
            i, j = rep % 3, (rep + 1 + rep // 3) % 3
            gpu.extract_enqueue(clouds[i].desc, A.d_out, A.d_ids, A.cap, *clouds[i].hint)
            other.extract_enqueue(o_clouds[j].desc, B.d_out, B.d_ids, B.cap, *o_clouds[j].hint)
            first, second = (gpu, other) if rep % 2 else (other, gpu)
            got = {first: first.extract_finish()}
            got[second] = second.extract_finish()
            assert (got[gpu], got[other]) == (want[i][0], want[j][0]), (rep, i, j, got[gpu], got[other])
            assert A.get(got[gpu]) == want[i] and B.get(got[other]) == want[j], (rep, i, j)
    finally:
        other.close()
