"""The forms of k_fx_acc (development option fx_acc_form: bit 0 - pass A per load round, under the loads; bit 1 - records linked
before their sums exist; 0 - neither; -1 - the library's own) write THE SAME BYTES: the moments are integers and the record indices
do not depend on the form, so surfels and ids are compared byte for byte between the forms, and one form with the CPU oracle
(tolerances of tests/test_extract_gpu.py).  Every form runs every sweep twice: the second run equals the first only if the kernels
left their tables zero at rest."""
import numpy as np
import pytest

import helpers
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

pytestmark = pytest.mark.gpu

FORMS = (0, 1, 2, -1)
MIN_FAST = 64  # sweeps of fewer points never reach the default path (csrc/extract.hip: fx_applicable): no form of k_fx_acc runs for them
KTILE = 1024  # kFxTile (csrc/extract_plan.h): the points of one k_fx_acc workgroup, 256 lanes, four load rounds
ROUND_EDGES = (0, 255, 256, 511, 512, 767, 768, 1023)  # first and last lane of every load round of a tile


@pytest.fixture(scope="module")
def ctx():
    """a context of its own: the option is the context's, and the fall-back count is counted from its creation"""
    from wildcat_slam_amd import lib

    c = lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lattice():
    return synth.g2_lattice(300, m=32)[0]


def _upload(ctx, pts, layout):
    """-> (descriptor, buffers to keep alive).  rec48: the 48-byte records; stride16: xyz at a stride of 16 bytes and the stamps in an
    array of their own (element-wise loads); packed: 12-byte xyz + 8-byte stamps, 16-byte aligned (the direct path)"""
    n = len(pts)
    if layout == "rec48":
        d = ctx.to_device(pts) if n else ctx.alloc(48)
        return ctx.points_desc(d, n), (d,)
    xyz = np.zeros((max(n, 1), 4 if layout == "stride16" else 3), np.float32)
    xyz[:n, 0], xyz[:n, 1], xyz[:n, 2] = pts["x"], pts["y"], pts["z"]
    d_xyz = ctx.to_device(xyz.reshape(-1))
    d_t = ctx.to_device(np.ascontiguousarray(pts["time"], np.float64) if n else np.zeros(1))
    return R.Points(d_xyz.ptr, d_t.ptr, 4 * xyz.shape[1], 8, n), (d_xyz, d_t)


def _hint(pts):
    return float(pts["time"][0]), float(pts["time"][-1])


def _once(ctx, desc, n, hint):
    cap = max(1024, (3 * n) // 20 + 1)
    d_out, d_ids = ctx.alloc(cap * 144), ctx.alloc(cap * 16)
    ctx.extract_enqueue(desc, d_out, d_ids, cap, hint[0], hint[1])
    m = ctx.extract_finish()
    return d_out.download(R.SURFEL, m), d_ids.download(R.SURFEL_ID, m)


def _forms(ctx, pts, layout="rec48", hint=None, forms=FORMS):
    """every form twice on the same device-resident points -> {form: (surfels, ids)}; asserts what every case asserts"""
    desc, keep = _upload(ctx, pts, layout)
    hint = hint or _hint(pts)
    out, fell = {}, {}
    try:
        for f in forms:
            ctx.set_dev_option("fx_acc_form", f)
            before = ctx.extract_path_info()["fallbacks"]
            runs = []
            for rep in range(2):
                s, i = _once(ctx, desc, len(pts), hint)
                info = ctx.extract_path_info()
                assert info["fast"] == (len(pts) >= MIN_FAST), (f, rep, info)
                runs.append((s.tobytes(), i.tobytes()))
            assert runs[0] == runs[1], "form %d: the second run differs from the first" % f
            fell[f] = ctx.extract_path_info()["fallbacks"] - before
            out[f] = (s, i)
    finally:
        ctx.set_dev_option("fx_acc_form", -1)
    del keep
    assert len(set(fell.values())) == 1, fell
    for f in forms[1:]:
        assert out[f][0].tobytes() == out[forms[0]][0].tobytes(), "surfels of form %d differ from form %d's" % (f, forms[0])
        assert out[f][1].tobytes() == out[forms[0]][1].tobytes(), "ids of form %d differ from form %d's" % (f, forms[0])
    return out


def _against_oracle(oracle, pts, got, params=None):
    s_ref, i_ref, _ = oracle.extract_surfels(pts, params)
    s, i = got
    assert len(s) == len(s_ref)
    if len(s_ref):
        helpers.check_surfels(s, i, s_ref, i_ref, tol=1e-6, t_tol=1e-5)
    return len(s_ref)


@pytest.mark.parametrize("kw", [dict(m=32), dict(m=30), dict(m=16), dict(m=12), dict(m=48, patches_per_root=1)],
                         ids=["m32", "m30-in-lane", "m16-direct-limit", "m12-lds-hash", "m48-one-patch"])
def test_run_structured_lattices(ctx, oracle, kw):
    """m = 30: cell boundaries inside lanes (classes 0 - 2); m = 16: 16 tails per wavefront, exactly kFxDirect; m = 12: more than 16,
    the LDS-hash route; one patch per root.  A patch of 20 points or fewer is no surfel under the default thresholds (n > min_points,
    n >= cluster_min_points): the library and the oracle run the two small-patch lattices with both thresholds at 8, so that the
    forms are compared on real bytes at the direct limit and on the lattice's LDS-hash route"""
    pts = synth.g2_lattice(300, **kw)[0]
    params = None
    if kw["m"] <= 20:
        params = oracle.default_params()
        params.min_points = params.cluster_min_points = 8
        ctx.set_params(params)
    try:
        out = _forms(ctx, pts)
        n_ref = _against_oracle(oracle, pts, out[-1], params)
    finally:
        if params is not None:
            ctx.set_params(oracle.default_params())
    assert n_ref > 0  # (count, ids and geometry are the oracle's: _against_oracle)


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 255, 257, 1023, 1025, 4099])
def test_partial_tiles(ctx, oracle, lattice, n):
    """partial load rounds, the partial tile behind full ones, a single lane (below MIN_FAST points the library takes the exact path by
    rule: the forms must agree there too, and `fast` must say so)"""
    pts = lattice[:n].copy()
    out = _forms(ctx, pts)
    _against_oracle(oracle, pts, out[-1])


def test_firing_order(ctx, oracle):
    """no run structure: LDS hash, spill pool, layer 2"""
    pts = synth.g1_room(60_000)
    out = _forms(ctx, pts)
    assert _against_oracle(oracle, pts, out[-1]) > 0


@pytest.mark.parametrize("layout", ["rec48", "packed"])
def test_library_choice_above_the_resident_bound(ctx, layout):
    """above 2 M points (more than one round of workgroups) the library's own choice is another instantiation on the staged path
    (csrc/extract_fast.inc: fx_acc_form_of): the smallest such sweep, in both layouts, against forms 0 and 3"""
    pts = synth.g2_lattice(7820, m=32)[0]
    assert len(pts) > 2_000_000
    _forms(ctx, pts, layout, forms=(0, 3, -1))


@pytest.mark.parametrize("kind", ["nan", "pinf", "face"])
def test_point_rules_at_the_round_edges(ctx, oracle, lattice, kind):
    """the first and last lane of every load round of a tile hold a NaN, +inf, or a coordinate exactly on a voxel face"""
    pts = lattice.copy()
    at = 3 * KTILE + np.array(ROUND_EDGES)
    if kind == "face":
        vs = synth.VS
        pts["x"][at] = (np.floor(pts["x"][at].astype(np.float64) / vs) * vs).astype(np.float32)
        pts["y"][at[::2]] = ((np.floor(pts["y"][at[::2]].astype(np.float64) / vs) + 1.0) * vs).astype(np.float32)
    else:
        val = np.nan if kind == "nan" else np.inf
        pts["x"][at[0::3]] = val
        pts["y"][at[1::3]] = val
        pts["z"][at[2::3]] = val
    out = _forms(ctx, pts)
    assert _against_oracle(oracle, pts, out[-1]) > 0


@pytest.mark.parametrize("val", [np.nan, -np.inf])
def test_non_finite_origin(ctx, oracle, lattice, val):
    """point 0 is not finite: the key origin is the first finite point"""
    pts = lattice.copy()
    pts["y"][0] = val
    pts["x"][1] = val
    out = _forms(ctx, pts)
    assert _against_oracle(oracle, pts, out[-1]) > 0


@pytest.mark.parametrize("layout", ["rec48", "stride16", "packed"])
def test_layouts(ctx, oracle, lattice, layout):
    """48-byte records, element-wise loads, packed 12 + 8 bytes; with a partial last tile"""
    pts = lattice[: 20 * KTILE + 77].copy()
    out = _forms(ctx, pts, layout)
    assert _against_oracle(oracle, pts, out[-1]) > 0


def _outcome(ctx, desc, n, hint):
    from wildcat_slam_amd import lib

    try:
        s, i = _once(ctx, desc, n, hint)
    except lib.WildcatError as e:
        return ("error", e.code)
    info = ctx.extract_path_info()
    return ("ok", info["fast"], info["flags"], s.tobytes(), i.tobytes())


@pytest.mark.parametrize("case", ["stamp-outside", "wider-than-1024-roots"])
def test_error_paths(ctx, lattice, case):
    """a stamp outside [t_lo, t_hi], a cloud wider than 1024 root voxels: the same outcome - error code, or flags and bytes - in every form"""
    pts = lattice.copy()
    hint = _hint(pts)
    if case == "stamp-outside":
        pts["time"][2 * KTILE + 300] = hint[1] + 10.0
    else:
        pts["x"][2 * KTILE + 300] += np.float32(1100 * synth.VS)
    desc, keep = _upload(ctx, pts, "rec48")
    got = {}
    try:
        for f in FORMS:
            ctx.set_dev_option("fx_acc_form", f)
            got[f] = [_outcome(ctx, desc, len(pts), hint) for rep in range(2)]
    finally:
        ctx.set_dev_option("fx_acc_form", -1)
    del keep
    print(case, {f: v[0][:3] for f, v in got.items()})
    for f in FORMS:
        assert got[f][0] == got[f][1], f
        assert got[f][0] == got[FORMS[0]][0], f
    assert got[0][0][0] == "error" or not got[0][0][1], "the default path cannot complete this sweep"
    # the tables are zero at rest behind the failed sweeps: a clean sweep on the same context
    _forms(ctx, lattice, forms=(0, -1))


def test_batch_of_two_equals_single_calls(ctx, lattice):
    """wc_extract_surfels_batch_* under the library's own form: two sweeps in one launch chain = the two single calls"""
    a, b = lattice[: 30 * KTILE + 5].copy(), synth.g2_lattice(150, m=30, seed=synth.SEED + 1)[0]
    single = [_forms(ctx, p, forms=(-1,))[-1] for p in (a, b)]
    jobs, keep = [], []
    for p in (a, b):
        desc, k = _upload(ctx, p, "rec48")
        cap = max(1024, (3 * len(p)) // 20 + 1)
        d_out, d_ids = ctx.alloc(cap * 144), ctx.alloc(cap * 16)
        keep.append((k, d_out, d_ids))
        jobs.append((desc, d_out, d_ids, cap) + _hint(p))
    enqueue, finish = ctx.extract_batch_prepare(jobs)
    for rep in range(2):
        enqueue()
        counts = finish()
        for k in range(2):
            s, i = keep[k][1].download(R.SURFEL, counts[k]), keep[k][2].download(R.SURFEL_ID, counts[k])
            assert s.tobytes() == single[k][0].tobytes() and i.tobytes() == single[k][1].tobytes(), (rep, k)
