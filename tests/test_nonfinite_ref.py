"""The non-finite cases of tests/nonfinite.py on the CPU: the builder does what it says, the oracle drops the points (as the reference
does, without saying so), every case is LIVE - the voxel a NaN -> 0 / saturating conversion would send a point to is one that matters -
and the wrong rule, restated as data (nonfinite.fault_model), makes every case fail.  The GPU tests (tests/test_nonfinite_gpu.py) then
only have to compare a dirty call with the clean call."""
import numpy as np
import pytest

import extract_gates as G
import extract_ref as X
import helpers
import nonfinite as NF

CASES = NF.cases()
_ORACLE = {}


def _ids(c):
    return "%s-%s" % c


def _clean_result(oracle, name, pattern=""):
    name = "empty" if pattern == "all" else name
    if name not in _ORACLE:
        s, ids, _ = oracle.extract_surfels(NF.cloud(name) if name != "empty" else NF.cloud("lattice0")[:0])
        _ORACLE[name] = (s, ids)
    return _ORACLE[name]


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def _faulty_voxels(pts, removed):
    """the voxel a NaN -> 0, saturating float -> int conversion gives each removed point"""
    p = NF.xyz(pts)[removed].astype(np.float64)
    with np.errstate(invalid="ignore"):
        k = np.floor(p / NF.VS)
    k = np.where(np.isnan(k), 0.0, np.clip(k, -2.0**31, 2.0**31 - 1))
    return k.astype(np.int64)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_builder(case):
    clean, dirty, removed = NF.case(*case)
    fin = NF.finite_rows(dirty)
    assert NF.same_records(dirty[fin], clean)
    assert np.array_equal(np.flatnonzero(~fin), removed) and len(removed) > 0
    if case[1] == "all":
        assert len(removed) == len(dirty)
    elif case[1] != "stamps":  # the stamp rule: the stamp of the clean point behind it (of the last one at the very end)
        nxt = np.searchsorted(np.flatnonzero(fin), removed)
        assert np.array_equal(dirty["time"][removed], clean["time"][np.minimum(nxt, len(clean) - 1)])
        assert np.all(np.diff(dirty["time"]) >= 0)
    else:
        lo, hi = clean["time"][0], clean["time"][-1]
        t = dirty["time"][removed]
        assert np.isnan(t).any() and (t < lo).any() and (t > hi).any() and not ((t >= lo) & (t <= hi)).any()
    if case[1].startswith("ends"):
        assert removed.tolist() == [0, len(dirty) - 1]
    if case[1] == "scatter":  # about 1 %, every kind of value on every axis and on all three
        p = NF.xyz(dirty)[removed]
        assert 0.005 * len(clean) <= len(removed) <= max(24, 0.02 * len(clean))
        for test in (np.isnan, np.isposinf, np.isneginf):
            bad = test(p)
            assert all(((bad[:, a]) & (bad.sum(axis=1) == 1)).any() for a in range(3)) and bad.all(axis=1).any()


def test_lattice0_occupies_the_origin_voxel(oracle):
    _, ids = _clean_result(oracle, "lattice0")
    assert ((ids["kx"] == 0) & (ids["ky"] == 0) & (ids["kz"] == 0)).any()
    k = NF.voxels(NF.cloud("lattice0"))
    for a in range(3):  # roots on each plane k = 0
        assert (k[:, a] == 0).any()
    assert NF.key_extent(NF.cloud("far")) <= 511  # far: the relative keys fit the narrow range around the cloud's own points ...
    assert abs(NF.voxels(NF.cloud("far"))[:, 0]).max() > 512  # ... and not around voxel 0
    # shuffled: no run structure (consecutive points share a voxel in fewer than 1 % of the places)
    ks = NF.voxels(NF.cloud("shuffled"))
    assert (ks[1:] == ks[:-1]).all(axis=1).mean() < 0.05


@pytest.mark.parametrize("case", [c for c in CASES if c[1] in ("scatter", "stamps", "runs")], ids=_ids)
def test_case_is_live(oracle, case):
    """at least one dirty point would be counted into a voxel that emits a surfel in the clean cloud"""
    clean, dirty, removed = NF.case(*case)
    _, ids = _clean_result(oracle, case[0])
    emitting = {(int(a), int(b), int(c)) for a, b, c in zip(ids["kx"], ids["ky"], ids["kz"])}
    hit = [tuple(k) in emitting for k in _faulty_voxels(dirty, removed).tolist()]
    assert any(hit), case


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_oracle_drops_the_points(oracle, case):
    clean, dirty, _ = NF.case(*case)
    ref = _clean_result(oracle, *case)
    s, ids, _ = oracle.extract_surfels(dirty)
    assert _same((s, ids), ref)
    assert len(s) == 0 if case[1] == "all" else len(s) > 0


def _fault_outcome(oracle, pts):
    """the faulty library's answer: "error" (a key beyond the wide range), or (surfels, ids, the keys fit the narrow range)"""
    ext = NF.key_extent(pts)
    if ext >= 2**20:
        return "error"
    s, ids, _ = oracle.extract_surfels(pts)
    return s, ids, ext <= 511


@pytest.mark.parametrize("case", [c for c in CASES if c[1] != "all"], ids=_ids)
def test_fault_model_fails_the_case(oracle, case):
    """The wrong rule as data: NaN -> the centre of voxel 0 on that axis, +-inf -> +-(2^20 vs); the oracle on the result.  It must differ
    from the clean cloud's - an error (an extent beyond 2^20 root voxels is WC_ERR_ARG) counts as differing, and so does, for the ends,
    a key origin that no longer lets the cloud fit the narrow keys (the condition of the GPU test: the default path must be kept).  Where
    a case has NaN points, those ALONE must make it differ: the infinite ones give the error whatever else the case does."""
    clean, dirty, removed = NF.case(*case)
    ref = _clean_result(oracle, case[0])
    narrow = NF.key_extent(clean) <= 511
    p = NF.xyz(dirty)[removed]
    if np.isinf(p).any():
        assert _fault_outcome(oracle, NF.fault_model(dirty)) == "error"
    if np.isnan(p).any():
        out = _fault_outcome(oracle, NF.fault_model(dirty, only_nan=True))
        assert out != "error"
        differs = not _same(out[:2], ref)
        if case[1].startswith("ends"):
            differs = differs or out[2] != narrow
        assert differs, case


@pytest.mark.parametrize("name", NF.GATES)
def test_count_gates(oracle, name):
    """20 finite points in a root stay untested, 21 give the root's surfel; a cluster of 19 is dropped, one of 20 kept - with five points
    (NaN, y, z) next to them that would make it 25 / 26 / 24 / 25.  The oracle ignores them; the fault model does not."""
    c = NF.gate(name)
    ref = oracle.extract_surfels(c["clean"])[:2]
    got = oracle.extract_surfels(c["dirty"])[:2]
    assert _same(got, ref)
    ids = ref[1]
    layer_code = 0 if c["site"] == "root" else 1
    site = (ids["kx"] == NF.GATE_K[0]) & (ids["ky"] == NF.GATE_K[1]) & (ids["kz"] == NF.GATE_K[2]) & ((ids["node"] & 3) == layer_code)
    # (the layer-1 node's second cluster, 40 points 0.1 s later, is always there)
    assert int(site.sum()) == (1 if c["emits"] else 0) + (1 if c["site"] == "l1" else 0), (name, ids)
    # live: the five points would be counted into the site's root, and the fault model's answer differs
    assert (_faulty_voxels(c["dirty"], c["removed"]) == np.array(NF.GATE_K)).all()
    bad = oracle.extract_surfels(NF.fault_model(c["dirty"]))[:2]
    assert not _same(bad, ref), name
    if not c["emits"]:  # ... by the very surfel the gate holds back
        assert len(bad[0]) == len(ref[0]) + 1


def test_extract_ref_drops_the_points(oracle):
    """tests/extract_ref.py states the rule explicitly, and agrees with the oracle on a dirty cloud"""
    clean, dirty, removed = NF.case("lattice0", "scatter")
    P = G._Params()
    ref = X.extract(dirty, P)
    s, ids = _clean_result(oracle, "lattice0")
    assert ref["ids"].tobytes() == ids.tobytes()
    helpers.check_surfels(ref["surfels"], ref["ids"], s, ids, tol=1e-6, t_tol=1e-5)
    fin = NF.finite_rows(dirty)
    assert all(fin[m].all() for m in ref["members"])
    assert X.extract(clean, P)["surfels"].tobytes() == ref["surfels"].tobytes()
