"""tests/route_ref.py held to the library's host side (wc_route_owner, dist.route_partition_host, dist.merge_surfels_host) and to the
oracle's voxel index, and every planted case of tests/route_cases.py asserted to be what its name claims - all without a GPU."""
import numpy as np
import pytest

import route_cases as RC
import route_ref as RR
from wildcat_slam_amd import dist as wdist
from wildcat_slam_amd import lib
from wildcat_slam_amd import records as R

I32 = (RR.INT32_MIN, RR.INT32_MAX)


def test_hash_known_answers():
    assert [RR.route_hash(*k) for k in RR.KNOWN_KEYS[:3]] == RR.KNOWN_HASHES
    assert [RR.route_owner(*k, 64) for k in RR.KNOWN_KEYS] == RR.KNOWN_OWNERS_64
    assert all(0 <= RR.route_hash(*k) <= RR.M32 for k in RR.KNOWN_KEYS)


def test_hash_and_owner_equal_the_library():
    f = lib.load().wc_route_owner
    rng = np.random.default_rng(1)
    corners = [(a, b, c) for a in I32 + (0, -1) for b in I32 + (0, 1) for c in I32 + (0, -1)]
    rand = [tuple(int(x) for x in k) for k in rng.integers(RR.INT32_MIN, RR.INT32_MAX, size=(1000, 3), endpoint=True)]
    rand += [tuple(int(x) for x in k) for k in rng.integers(-300, 300, size=(1000, 3))]
    keys = RR.KNOWN_KEYS + corners + rand
    hashes = [RR.route_hash(*k) for k in keys]
    for world in range(1, 65):
        assert [h % world for h in hashes] == [f(k[0], k[1], k[2], world) for k in keys], world
    assert f(1, 2, 3, 0) == -1 and f(1, 2, 3, -5) == -1  # the library's refusal; the restatement has no such case


def _oracle_keys(oracle, pts, voxel):
    P = oracle.default_params()
    P.voxel_size = float(np.float32(voxel))
    return oracle.voxel_keys(pts, P)


@pytest.mark.parametrize("voxel", [0.2, 0.5, 0.1, 0.8])
def test_route_voxel_equals_the_oracle(oracle, voxel):
    v32 = np.float32(voxel)
    rng = np.random.default_rng(2)
    inside = RC.make_points(rng.uniform(-60, 60, size=(4000, 3)))
    assert np.array_equal(RR.route_voxel(RR.xyz_of(inside), v32), _oracle_keys(oracle, inside, v32))
    # faces float32(k v) and their two float neighbours (k negative and positive), -0.0, subnormals, the int32 range's ends, non-finite
    edge = RC.edge_cloud(v32)
    got = RR.route_voxel(RR.xyz_of(edge), v32)
    assert np.array_equal(got, _oracle_keys(oracle, edge, v32))
    assert (got == RR.INT32_MIN).any() and (np.abs(got.astype(np.int64)) > 2147483000).sum() > (got == RR.INT32_MIN).sum()
    # what the planted values claim
    for k, (lo, f, hi) in zip(RC.FACE_KS, RC.face_values(v32)):
        tri = RR.route_voxel(np.array([[lo, f, hi]], np.float32), v32)[0]
        assert lo < f < hi and tri[0] == k - 1 and tri[2] == k and tri[1] in (k - 1, k), (k, tri)  # the face lies between the neighbours
    z = RR.route_voxel(np.array([[-0.0, 0.0, 1e-45], [-1e-45, 1e-39, -1e-39]], np.float32), v32)
    assert z.tolist() == [[0, 0, 0], [-1, 0, -1]]
    v = np.float64(v32)
    out = RR.route_voxel(np.array([[np.nan, np.inf, -np.inf], [3e9 * v, -3e9 * v, np.finfo(np.float32).max]], np.float32), v32)
    assert (out == RR.INT32_MIN).all()
    vals = RC.edge_values(v32)
    kv = RR.route_voxel(np.stack([vals, vals, vals], 1), v32)[:, 0]
    fin = np.isfinite(vals)
    assert (~fin).sum() == 3 and (kv[~fin] == RR.INT32_MIN).all()
    with np.errstate(all="ignore"):
        q = np.floor(vals.astype(np.float64) / v)
    beyond = fin & ((q < -2147483648.0) | (q > 2147483647.0))
    near = fin & ~beyond & (np.abs(q) > 2147483000.0)
    assert beyond.sum() >= 6 and near.sum() >= 2  # quotients beyond the int32 range, and the last ones inside it
    assert (kv[beyond] == RR.INT32_MIN).all() and (kv[near] == q[near].astype(np.int64)).all()
    assert ((vals < 0) & fin).sum() > 20 and np.signbit(vals[vals == 0]).any()


@pytest.mark.parametrize("world", [1, 2, 3, 8, 64])
def test_partition_ref_equals_the_host_restatement(oracle, world):
    for pts in (RC.random_cloud(3000), RC.edge_cloud(RC.V_DEFAULT)):
        segs = RR.partition_ref(pts, RC.V_DEFAULT, world)
        host = wdist.route_partition_host(pts, oracle.voxel_keys(pts), world)
        assert len(segs) == world and sum(len(s) for s in segs) == len(pts)
        for s, h in zip(segs, host):
            assert np.all(np.diff(s) > 0) and len(s) == len(h)
            for f in ("x", "y", "z", "intensity", "time", "ring"):  # (field by field: the 48-byte record has padding)
                assert pts[f][s].tobytes() == h[f].tobytes(), f
        want, counts = RC.expected(pts, segs)
        assert counts == [len(h) for h in host] and want["src"].max(initial=0) == 0
        assert want["t"].tobytes() == np.concatenate([h["time"] for h in host]).tobytes()


def test_partition_sizes_end_where_they_claim():
    assert RC.N_MAX == max(RC.NS) == 3 * 2048 - 1
    for unit in (64, 256, 2048):  # a wavefront, a 256-lane iteration, a 2048-point tile: one below, on and one above each
        assert {unit - 1, unit, unit + 1} <= set(RC.NS)
    assert {1, 2, 4097} <= set(RC.NS) and set(RC.WORLDS) == {1, 2, 3, 7, 8, 63, 64}
    # the random cloud spreads over every rank of the largest world inside its first tile
    assert len(set(RR.owners_of(RR.xyz_of(RC.random_cloud(2048)), RC.V_DEFAULT, 64).tolist())) == 64


@pytest.mark.parametrize("world", RC.SEQ_WORLDS)
def test_owner_sequences_are_what_they_prescribe(world):
    keys = RR.keys_owned_by(world)
    assert [RR.route_owner(*k, world) for k in keys.tolist()] == list(range(world)) and len(set(map(tuple, keys.tolist()))) == world
    n = RC.N_MAX
    for name, fn in RC.SEQS.items():
        seq = fn(n, world)
        pts = RC.owner_cloud(world, seq)
        assert np.array_equal(RR.owners_of(RR.xyz_of(pts), RC.V_DEFAULT, world), seq), name
        assert np.all(np.diff(pts["time"]) > 0)  # strictly ascending stamps: stability shows
    assert set(RC.seq_one(n, world).tolist()) == {world - 1}
    cyc = RC.seq_cycle(n, world)
    for w0 in (0, 64, 2048 - 64):  # every owner sits in one wavefront (all 64 of them at world 64)
        assert len(set(cyc[w0 : w0 + 64].tolist())) == min(world, 64)
    st = RC.seq_steps(n, world)
    assert (np.flatnonzero(np.diff(st)) + 1).tolist() == list(RC.SEQ_BOUNDS)  # the owner changes exactly at 64, 256 and 2048
    rnd = RC.seq_random(n, world)
    assert len(set(rnd.tolist())) == world and len(set(rnd[:64].tolist())) > 1


def _is_sorted(rows):
    ks = [RC.canon(r) for r in rows]
    return all(a <= b for a, b in zip(ks, ks[1:]))


def test_merge_ref_equals_the_host_restatement():
    cases = RC.merge_cases()
    for name, c in cases.items():
        assert all(_is_sorted(rows) for rows in c["rows"]), name  # what the merge expects of its inputs
        order = RR.merge_ref(c["lists"], c["ids"])
        assert sorted(order) == [(j, p) for j, s in enumerate(c["lists"]) for p in range(len(s))]
        ms = RR.take(c["lists"], order, R.SURFEL)
        assert [(int(a), int(b)) for a, b in ms["center"][:, :2]] == order  # every record carries its (list, position)
        if c["ids"] is None:
            continue
        hs, hi = wdist.merge_surfels_host(c["lists"], c["ids"])  # a stable sort of the concatenation: ties in list order, then position
        assert ms.tobytes() == hs.tobytes() and RR.take(c["ids"], order, R.SURFEL_ID).tobytes() == hi.tobytes(), name
    # distinct keys: the order owes nothing to the tie rules
    c = cases["front_behind"]
    allk = [RC.canon(r) for rows in c["rows"] for r in rows]
    assert len(set(allk)) == len(allk)
    assert [j for j, _ in RR.merge_ref(c["lists"], c["ids"])] == [2] * 100 + [0] * 100 + [1] * 100


def _keys_by_list(c):
    return [[RC.canon(r) for r in rows] for rows in c["rows"]]


def test_merge_cases_are_what_they_claim():
    cases = RC.merge_cases()
    n = {name: [len(s) for s in c["lists"]] for name, c in cases.items()}
    assert n["k1"] == [300]
    assert len(n["k64_small"]) == 64 and set(n["k64_small"]) == {0, 1, 2, 3}
    assert n["empties"] == [0, 0, 40, 0, 0, 37, 0]  # empty lists first, last and adjacent
    assert sorted(n["big_and_singletons"]) == [1] * 63 + [1000] and n["big_and_singletons"][RC.BIG_LIST] == 1000
    for t in (255, 256, 257):
        assert sum(n["total_%d" % t]) == t and len(n["total_%d" % t]) == 3 and min(n["total_%d" % t]) > 0
    # ties across lists, of stamps alone and of whole keys, in the cases that are about them
    for name in ("k64_small", "total_255", "total_256", "total_257"):
        kl = _keys_by_list(cases[name])
        shared = [k for j, ks in enumerate(kl) for k in ks if any(k in other for i, other in enumerate(kl) if i != j)]
        assert len(shared) >= 4, name
    # the long list: singletons equal to one of its records in lists in front of it and behind it, others between its records and beyond its ends
    kl = _keys_by_list(cases["big_and_singletons"])
    big = set(kl[RC.BIG_LIST])
    eq = [j for j in range(64) if j != RC.BIG_LIST and kl[j][0] in big]
    assert min(eq) < RC.BIG_LIST < max(eq) and len(eq) >= 10
    ts = sorted(k[0] for k in big)
    singles = [kl[j][0] for j in range(64) if j != RC.BIG_LIST]
    assert any(k[0] < ts[0] for k in singles) and any(k[0] > ts[-1] for k in singles)
    assert any(k not in big and ts[0] < k[0] < ts[-1] and k[0] not in ts for k in singles)
    assert any(k not in big and k[0] in ts for k in singles)  # a record's stamp and voxel with another node id
    # every stamp equal: negative indices, and node ids whose signed and unsigned orders differ, in DIFFERENT lists of one voxel
    c = cases["equal_stamps"]
    assert {float(t) for s in c["lists"] for t in s["t"]} == {5.0} and sum(len(s) for s in c["lists"]) == 400
    kl = _keys_by_list(c)
    assert any(k[1] < 0 for ks in kl for k in ks) and any(k[2] < 0 for ks in kl for k in ks) and any(k[3] < 0 for ks in kl for k in ks)
    found = 0
    for a in range(5):
        for b in range(5):
            if a != b:
                found += sum(1 for x in kl[a] for y in kl[b] if x[:4] == y[:4] and x[4] < 2**31 <= y[4])
    assert found >= 5
    order = RR.merge_ref(c["lists"], c["ids"])
    merged = [kl[j][p] for j, p in order]
    assert merged == sorted(merged) and len(set(merged)) == 400
    # the same (t, id) in 64, 3 and 2 lists, and twice in one
    kl = _keys_by_list(cases["dups"])
    where = {}
    for j, ks in enumerate(kl):
        for k in ks:
            where.setdefault(k, []).append(j)
    assert sorted(len(set(v)) for v in where.values() if len(v) > 1) == [2, 2, 3, 64]
    assert any(3 in v and 7 in v and len(v) == 2 for v in where.values())  # list 3 and list 7 share a (t, id)
    assert any(v == [7, 7, 9] for v in where.values())
    order = RR.merge_ref(cases["dups"]["lists"], cases["dups"]["ids"])
    assert order[:64] == [(j, 0) for j in range(64)]  # equal keys: list order
    assert cases["no_ids"]["ids"] is None and len(cases["no_ids"]["lists"]) == 6
    tl = [set(s["t"].tolist()) for s in cases["no_ids"]["lists"]]
    assert all(tl[a] & tl[b] for a in range(6) for b in range(a))  # every two lists share a stamp
    o = RR.merge_ref(cases["no_ids"]["lists"])
    tt = [float(cases["no_ids"]["lists"][j]["t"][p]) for j, p in o]
    assert all((ta, ja, pa) < (tb, jb, pb) for (ta, (ja, pa)), (tb, (jb, pb)) in zip(zip(tt, o), zip(tt[1:], o[1:])))


def test_match_shares_are_what_they_claim():
    g = RC.MATCH_GROUP
    assert RC.MATCH_SHARD_FROM == 4096 and RC.MATCH_MAX_WORLD == 8
    cases = {(nq, w) for nq, w, _ in RC.MATCH_CASES}
    assert {(4095, 3), (4096, 3), (4104, 8)} <= cases and {(4099, w) for w in (3, 5, 7, 8)} <= cases
    assert {k for nq, w, k in RC.MATCH_CASES if (nq, w) == (4099, 5)} == {3, 10, 16}
    for nq, w, _ in RC.MATCH_CASES:
        sh = RC.match_shares(nq, w)
        assert sh[0][0] == 0 and sh[-1][1] == nq and all(a[1] == b[0] for a, b in zip(sh, sh[1:])) and w <= RC.MATCH_MAX_WORLD
        if nq == 4099:  # shares that begin inside a wavefront's eight queries, and shares whose last wavefront is not full
            assert any(b % g for b, _ in sh[1:]) and any((e - b) % g for b, e in sh)
    assert all((e - b) == 513 for b, e in RC.match_shares(4104, 8))  # equal shares, each one query past a full wavefront


def test_sharded_clouds_are_what_they_claim():
    pts, info = RC.one_root_cloud()
    keys = RR.route_voxel(RR.xyz_of(pts), RC.V_DEFAULT)
    assert len(pts) == 256 and len(set(map(tuple, keys.tolist()))) == 1 and keys[0].tolist() == info["root_keys"][0].tolist()
    assert len(set(RR.owners_of(RR.xyz_of(pts), RC.V_DEFAULT, 3).tolist())) == 1  # two of three ranks own nothing
    pts, info = RC.lattice12()
    keys = RR.route_voxel(RR.xyz_of(pts), RC.V_DEFAULT)
    assert len(pts) == 12 * 256 and set(map(tuple, keys.tolist())) == set(map(tuple, info["root_keys"].tolist()))
    for world in (2, 3, 5):
        assert len(set(RC.owners_of_roots(info, world))) > 1
    assert len(set(RC.owners_of_roots(info, 8))) < 8  # at world 8 at least one rank owns no voxel
    assert wdist.shard_range(2, 0, 3)[1] == 0  # two points on three ranks: rank 0's slice is empty
