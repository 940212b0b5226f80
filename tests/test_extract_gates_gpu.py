"""The default extraction path's gates AT their thresholds (tests/extract_gates.py builds the clouds, tests/test_extract_gates_ref.py holds
what is assumed of them).  The path promises that counts and ids stay the reference's because every decision it cannot trust raises
kFlagFxFallback and the sweep is repeated on the exact path; tests/test_extract_precision_gpu.py matches surfels by id first, so it
rests on that promise.  Here one gate of one node or cluster sits a prescribed distance from its threshold, and per class:

  always   ids and counts byte-equal to the oracle's (in the oracle's order once both are sorted by id), helpers.check_surfels at the
           tolerances of the fall-back tests of tests/test_extract_gpu.py
  decide   (margin in [4, 64] x (band + the path's own bound), or further) the default path completes the sweep itself: fast, one run, no
           fall-back counted; and check_precision of tests/test_extract_precision_gpu.py holds
  fall     (margin + bound <= band) two runs, not fast, flag 64, and `why` names exactly the call site the case was built for: bit 13 a
           child's test, 14 the root's, 15 a job's (+ in the two-kernel form 17 + FxPca::which), the form's FxWhy::gap for a stamp gap -
           the bits of every other gate site clear
  grey     (between the two) the "always" clause alone: whichever side decides, it decides as the reference does

under both forms of the node stage (fx_split 0: k_fx_nodes, 1: k_fx_walk + k_fx_test).  Every sweep is preceded by set_exact_sums(False):
the back-off of an earlier fall-back never hides the default path.  One case per sweep, so `why` is attributable.  pytest -s prints, per
case, its margin / band and which path completed it; DESIGN.md 4.3 records the worst margin / band at which the path decided itself."""
import numpy as np
import pytest

import extract_gates as G
import helpers
import test_extract_precision_gpu as PG

pytestmark = pytest.mark.gpu

# fx_fallback's codes at the gate sites, per form of the node stage: kFxWhyNodes (csrc/extract_fast.inc) and kFxWhySplit
# (csrc/extract_split.inc) for the gap and job_which entries, the literals of fx_test_children / fx_test_root / fx_run_job for the rest
WHY = {0: dict(child=13, root=14, job=15, job_which=None, gap=7), 1: dict(child=13, root=14, job=15, job_which=17, gap=17)}
GATE_BITS = sum(1 << b for b in (7, 13, 14, 15, 17, 18, 19))


def expected_why(split, gate, site):
    w = WHY[split]
    if gate == "gap":
        return 1 << w["gap"]
    if site == "job":
        return (1 << w["job"]) | ((1 << (w["job_which"] + {"lam0": 0, "like": 1}[gate])) if w["job_which"] is not None else 0)
    return 1 << (w["root"] if site == "root" else w["child"])


@pytest.fixture(scope="module")
def ctx():
    """a context of this file's own: the fall-backs provoked here leave no back-off or table state to any other test"""
    from wildcat_slam_amd import lib

    c = lib.Context(0)
    yield c
    c.close()


_ORACLE = {}


def _truth(oracle, name, pts, params):
    if name not in _ORACLE:
        s, ids, _ = oracle.extract_surfels(pts, params)
        _ORACLE[name] = (s, ids)
    return _ORACLE[name]


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("name", G.CASES)
def test_gate_at_its_threshold(ctx, oracle, name, split):
    c = G.case(name)
    pts, cls = c["points"], c["cls"]
    params = oracle.default_params()
    for k_, v in c["over"].items():
        setattr(params, k_, v)
    s_orc, id_orc = _truth(oracle, name, pts, params)
    try:
        ctx.params = params
        ctx.set_dev_option("fx_split", split)
        ctx.set_exact_sums(False)  # (sets the parameters: the choice between the paths starts afresh)
        before = ctx.extract_path_info()["fallbacks"]
        s, ids = ctx.extract_surfels(pts)
        info = ctx.extract_path_info()
    finally:
        ctx.set_dev_option("fx_split", -1)
    what = ("%d ticks" % c["ticks"]) if c["gate"] == "gap" else "margin %+.3e = %.2f bands" % (c["margin"], abs(c["margin"]) / c["band"])
    print("\n%s, fx_split %d: %s, class %s -> %s, runs %d, flags %#x, why %#x, %d surfels (oracle %d)"
          % (name, split, what, cls, "default path" if info["fast"] else "exact path", info["runs"], info["flags"], info["why"], len(ids), len(id_orc)))
    # always
    assert len(ids) == len(id_orc) == len(s)
    by_id = lambda a: a[np.lexsort((a["node"], a["kz"], a["ky"], a["kx"]))].tobytes()
    assert by_id(ids) == by_id(id_orc), (helpers.id_tuples(ids), helpers.id_tuples(id_orc))
    helpers.check_surfels(s, ids, s_orc, id_orc, tol=1e-6, t_tol=1e-5)
    if cls in ("decide", "far"):
        assert info["fast"] and info["runs"] == 1 and info["fallbacks"] == before, info
        if len(ids):
            PG.check_precision("%s, fx_split %d" % (name, split), pts, params, c["ref"], s, ids, s_orc, id_orc)
    elif cls == "fall":
        assert info["runs"] == 2 and not info["fast"] and info["fallbacks"] == before + 1 and info["flags"] & 64, info
        assert info["why"] & GATE_BITS == expected_why(split, c["gate"], c["site"]), (hex(info["why"]), hex(expected_why(split, c["gate"], c["site"])))
    else:
        assert cls == "grey"
