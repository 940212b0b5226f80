"""wc_match_sharded at its edges, on one GPU (threads, one context per rank, dist.ThreadComm): the 4095 / 4096-query switch, share
boundaries that are no multiple of the eight queries a wavefront serves, 3 ... 8 ranks, k other than 10, the refusal at nine ranks and
wc_match_pair_sharded.  A synth.surfel_window is cut to exactly the wanted number of queries; the unsharded wc_match gives the expected
pairs and every rank's pairs must equal them byte for byte, for the same-set search and for the fixed-window search."""
import threading

import numpy as np
import pytest

import route_cases as RC
from wildcat_slam_amd import dist as wdist
from wildcat_slam_amd import lib
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

pytestmark = pytest.mark.gpu

WC_ERR_ARG = 11
_W, _REF = {}, {}


def _window(nq):
    """the first nq surfels (time order) of one window of 4 400, and its 1 500 fixed-window surfels"""
    if not _W:
        _W.update(synth.surfel_window(4, 1100, seed=17, fixed_patches=1500))
        assert len(_W["surf"]) == 4400 and np.all(np.diff(_W["surf"]["t"]) >= 0)
    return _W["surf"][:nq].copy(), _W["pose"][:nq].copy(), _W["fix_surf"], _W["fix_pose"]


def _params(k):
    P = lib.default_params()
    P.knn_k = k
    return P


def _reference(gpu, nq, k):
    """the unsharded call's pairs of both searches, once per (nq, k)"""
    if (nq, k) not in _REF:
        s, p, fs, fp = _window(nq)
        gpu.set_params(_params(k))
        try:
            _REF[(nq, k)] = (gpu.match(s, p, s, p, True), gpu.match(s, p, fs, fp, False))
        finally:
            gpu.set_params(lib.default_params())
        assert len(_REF[(nq, k)][0]) > nq // 4 and len(_REF[(nq, k)][1]) > nq // 20  # (both lists are worth comparing)
    return _REF[(nq, k)]


@pytest.fixture(scope="module")
def pool():
    ctxs = [lib.Context(0) for _ in range(8)]  # with the session's context: nine alive
    yield ctxs
    for c in ctxs:
        c.close()


def _ranks(ctxs, fn, timeout=120):
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


@pytest.mark.parametrize("nq,world,k", RC.MATCH_CASES)
def test_sharded_match_equals_unsharded(gpu, pool, nq, world, k):
    """below 4 096 queries the call does not shard (no all-gather); from 4 096 on it does, one all-gather per call; at 4 099 queries
    shares begin inside a wavefront's eight queries and end in a wavefront that is not full (tests/test_route_ref.py asserts it)"""
    ref_b, ref_u = _reference(gpu, nq, k)
    s, p, fs, fp = _window(nq)
    ctxs = pool[:world]
    for c in ctxs:
        c.set_params(_params(k))

    def fn(r, ctx, shared):
        b = ctx.match(s, p, s, p, True, sharded=True)
        n1 = wdist.ThreadComm.counts(shared, "allgatherv")[r]
        u = ctx.match(s, p, fs, fp, False, sharded=True)
        return b, u, n1, wdist.ThreadComm.counts(shared, "allgatherv")[r]

    try:
        out, shared = _ranks(ctxs, fn)
    finally:
        for c in ctxs:
            c.set_params(lib.default_params())
    per_call = 1 if nq >= RC.MATCH_SHARD_FROM else 0
    for r, (b, u, n1, n2) in enumerate(out):
        assert (n1, n2) == (per_call, 2 * per_call), r
        assert b.dtype == R.PAIR and b.tobytes() == ref_b.tobytes() and u.tobytes() == ref_u.tobytes(), r
    assert wdist.ThreadComm.counts(shared) == [2 * per_call] * world  # and no other collective


def test_nine_ranks_are_refused_without_a_collective(gpu, pool):
    """more than eight ranks: WC_ERR_ARG on every rank, no collective entered; a plain wc_match on rank 0 afterwards is right"""
    nq = 4099
    ref_b, ref_u = _reference(gpu, nq, 10)
    s, p, fs, fp = _window(nq)

    def fn(r, ctx, shared):
        codes = []
        for same in (True, False):
            with pytest.raises(lib.WildcatError) as e:
                ctx.match(s, p, s if same else fs, p if same else fp, same, sharded=True)
            codes.append(e.value.code)
        plain = (ctx.match(s, p, s, p, True), ctx.match(s, p, fs, fp, False)) if r == 0 else None
        return codes, plain

    out, shared = _ranks([gpu] + pool, fn)
    assert all(o[0] == [WC_ERR_ARG, WC_ERR_ARG] for o in out)
    assert all(wdist.ThreadComm.counts(shared, kind) == [0] * 9 for kind in (None, "allreduce", "alltoallv", "allgatherv"))
    assert out[0][1][0].tobytes() == ref_b.tobytes() and out[0][1][1].tobytes() == ref_u.tobytes()
    # (below 4 096 queries nothing is sharded, so nine ranks are no obstacle)
    s, p, fs, fp = _window(4095)
    ref_b, _ = _reference(gpu, 4095, 10)
    out, shared = _ranks([gpu] + pool, lambda r, ctx, shared: ctx.match(s, p, s, p, True, sharded=True))
    assert all(o.tobytes() == ref_b.tobytes() for o in out) and wdist.ThreadComm.counts(shared) == [0] * 9


def test_match_pair_sharded_equals_the_two_searches(gpu, pool):
    nq, world = 4099, 3
    ref_b, ref_u = _reference(gpu, nq, 10)
    s, p, fs, fp = _window(nq)

    def fn(r, ctx, shared):
        d_s, d_p, d_fs, d_fp = ctx.to_device(s), ctx.to_device(p), ctx.to_device(fs), ctx.to_device(fp)
        d_b, d_u = ctx.alloc(8 * nq), ctx.alloc(8 * nq)
        nb, nu = ctx.match_pair_device(d_s, d_p, nq, d_fs, d_fp, len(fs), d_b, nq, d_u, nq, sharded=True)
        return d_b.download(R.PAIR, nb), d_u.download(R.PAIR, nu)

    out, shared = _ranks(pool[:world], fn)
    for r, (b, u) in enumerate(out):
        assert b.tobytes() == ref_b.tobytes() and u.tobytes() == ref_u.tobytes(), r
    assert wdist.ThreadComm.counts(shared, "allgatherv") == [2] * world
