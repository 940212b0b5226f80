"""Per-voxel plane surfels of the device-resident voxel map (WC_MAP_MOMENTS: wc_map_create_ex, wc_map_export_surfels,
wc_map_nearest_plane, csrc/map.hip) and their facade surface against the restatement of map_surfel_ref.py: exact integer moments,
the covariance within 2 ulp of the rational, eigenpairs against the longdouble Jacobi iteration, order independence, growth / crop /
clear, the plane query byte for byte on the exports."""
import ctypes as C

import numpy as np
import pytest

import map_query_ref as Q
import map_surfel_ref as S
from extract_ref import LD
from helpers import point_records as _records, xyz_of as _xyz
from test_map_gpu import _drive
from test_map_query_gpu import BAD, _queries
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

pytestmark = pytest.mark.gpu

VOXELS = (0.05, 0.2, float(np.float32(0.8)))
WC_ERR_CAPACITY, WC_ERR_ARG = 1, 11
EPS = 2.0**-53
FRACTION_VOXELS = 50_000  # above this many voxels the integer / longdouble steps run on a seeded subset


def _map(gpu, xyz, v, **kw):
    m = gpu.map_create(v, moments=True, **kw)
    assert m.insert(xyz) == 0
    return m


def _surfels_of(gpu, xyz, v, **kw):
    m = _map(gpu, xyz, v, **kw)
    s = m.surfels()
    m.close()
    return s


def _centroid(sums, v):
    """map_centroid restated: (float)(r + (double)sum / (count * 2^32)) per axis"""
    c = sums["count"].astype(np.float64)[:, None]
    return (S.map_ref(sums["keys"], v) + sums["Q"].astype(np.float64) / (c * S.UNIT_Q)).astype(np.float32)


def _check_sums(surf, sums, v, what, rows=None):
    """key, count and centroid of EVERY voxel; the covariance of the voxels `rows` (all by default) within 2 ulp of N / (n^2 2^32);
    -> the restated covariance of those voxels, correctly rounded (Python's int / int)"""
    assert len(surf) == len(sums["count"]), (what, len(surf), len(sums["count"]))
    assert np.array_equal(surf["key"], sums["keys"]) and np.array_equal(surf["count"], sums["count"]), what
    assert surf["xyz"].tobytes() == _centroid(sums, v).tobytes(), what
    rows = range(len(surf)) if rows is None else rows
    cov_ref = np.zeros((len(rows), 6))
    for j, i in enumerate(rows):
        n = int(sums["count"][i])
        D = n * n * 2**32
        for e, N in enumerate(S.numerators(n, sums["U"][i], sums["M"][i])):
            assert S.within_ulps(surf["cov"][i, e], N, D), (what, surf["key"][i], e, surf["cov"][i, e], N, n)
            cov_ref[j, e] = N / D
    return cov_ref


def _check_eigen(surf, cov_ref, what):
    """ev, normal and the plane bit of the records against the longdouble Jacobi iteration on the restated covariance cov_ref (the
    records' own is within 2 ulp of it, _check_sums)"""
    ev_ref, n_ref = S.eigen_ref(cov_ref)
    ev, nrm = surf["ev"], surf["normal"]
    assert np.all(ev[:, 0] <= ev[:, 1]) and np.all(ev[:, 1] <= ev[:, 2]), what
    scale = np.abs(ev_ref).max(axis=1)
    err_ev = np.abs(ev.astype(LD) - ev_ref).max(axis=1)
    assert np.all(err_ev <= 32 * EPS * scale), (what, float((err_ev / np.maximum(scale, LD(1e-300))).max()) / (32 * EPS))
    nl = nrm.astype(LD)
    unit = np.abs(np.sqrt((nl * nl).sum(axis=1)) - 1)
    assert np.all(unit <= 8 * EPS), (what, float(unit.max()) / (8 * EPS))
    assert nrm.tobytes() == S.sign_rule(nrm).tobytes(), (what, "the sign rule on the record's own normal")
    lam = ev_ref.astype(np.float64)
    gap = lam[:, 1] - lam[:, 0]
    sep = gap > 1e-6 * lam[:, 2]
    bound = (32 * EPS * lam[:, 2] + 1e-12 * (np.abs(lam[:, 0]) + lam[:, 2])) / np.where(sep, gap, 1.0)
    raw_ref = n_ref  # (sign rule applied)
    d = np.minimum(np.sqrt(((nl - raw_ref) ** 2).sum(axis=1)), np.sqrt(((nl + raw_ref) ** 2).sum(axis=1))).astype(np.float64)
    assert np.all(d[sep] <= bound[sep]), (what, float((d[sep] / bound[sep]).max()))
    # where the reference's leading component stands out by more than the bound, the sign is the reference's
    mag = np.sort(np.abs(raw_ref.astype(np.float64)), axis=1)
    clear = sep & (mag[:, 2] - mag[:, 1] > bound)
    assert np.all((nl[clear] * raw_ref[clear]).sum(axis=1) > 0), (what, "sign")
    assert np.array_equal(surf["flags"], ((surf["count"] >= 3) & (ev[:, 2] > 0)).astype(np.uint32)), what
    return int(sep.sum()), int(clear.sum())


@pytest.fixture(scope="module")
def clouds():
    lat, _ = synth.g2_lattice(200, m=32)
    return dict(g2_lattice=_xyz(lat), g1_room=_xyz(synth.g1_room(200_000)))


# the hand map (v = 0.5): dyadic coordinates on the 2^-16 m grid, so every moment and every covariance below is exact in any arithmetic
HAND_V = 0.5
HAND = dict(
    one=[[0.25, 0.25, 0.25]],  # voxel (0, 0, 0)
    two=[[0.625, 0.125, 0.125], [0.875, 0.375, 0.375]],  # (1, 0, 0)
    coincident=[[1.75, 0.125, 0.375]] * 3,  # (3, 0, 0)
    plane_z=[[0.125, 1.125, 0.125], [0.375, 1.125, 0.125], [0.125, 1.25, 0.125], [0.375, 1.25, 0.125]],  # (0, 2, 0): a rectangle in z = 1/8
    negative=[[-0.25, -0.375, -0.125], [-0.125, -0.25, -0.375], [-0.375, -0.125, -0.25], [-0.3125, -0.4375, -0.0625]],  # (-1, -1, -1)
    last_pos=[[524287.75, 0.125, 0.25], [524287.875, 0.375, 0.125], [524287.96875, 0.25, 0.4375]],  # kx = 2^20 - 1
    last_neg=[[-524287.25, 0.125, 0.25], [-524287.375, 0.375, 0.125], [-524287.46875, 0.25, 0.4375]],  # kx = -(2^20 - 1): mirrored in x
)
HAND_KEYS = dict(one=(0, 0, 0), two=(1, 0, 0), coincident=(3, 0, 0), plane_z=(0, 2, 0), negative=(-1, -1, -1),
                 last_pos=(2**20 - 1, 0, 0), last_neg=(-(2**20) + 1, 0, 0))


def test_hand_map(gpu):
    """one point, two points, three coincident points (covariance and ev exactly 0, no plane), four points on the grid plane z = 1/8 (an
    axis-aligned rectangle: the covariance is diagonal with an exactly zero z row, so ev[0] == 0 and the normal is (0, 0, 1) exactly),
    negative indices, and the two ends of the key range"""
    xyz = np.array(sum(HAND.values(), []), np.float32)
    sums = S.voxel_sums(xyz, HAND_V)
    surf = _surfels_of(gpu, xyz, HAND_V)
    _check_eigen(surf, _check_sums(surf, sums, HAND_V, "hand"), "hand")
    row = {name: int(np.flatnonzero(np.all(surf["key"] == np.array(k), axis=1))[0]) for name, k in HAND_KEYS.items()}
    for name, k in HAND_KEYS.items():
        assert surf["count"][row[name]] == len(HAND[name]), name
        # dyadic inputs: the covariance is the exact rational, not merely within 2 ulp of it
        i = row[name]
        exact = [float(c) for c in S.covariance_exact(sums["count"][i], sums["U"][i], sums["M"][i])]
        assert surf["cov"][i].tolist() == exact, name
    for name in ("one", "coincident"):
        s = surf[row[name]]
        assert not s["cov"].any() and not s["ev"].any() and s["flags"] == 0, name
    assert surf["flags"][row["two"]] == 0 and surf["ev"][row["two"]][2] > 0  # (two points: a line, and too few)
    s = surf[row["plane_z"]]
    assert s["cov"].tolist() == [0.015625, 0.0, 0.0, 0.00390625, 0.0, 0.0]
    assert s["ev"].tolist() == [0.0, 0.00390625, 0.015625] and s["normal"].tolist() == [0.0, 0.0, 1.0] and s["flags"] == 1
    assert s["xyz"].tolist() == [0.25, 1.1875, 0.125]
    for name in ("negative", "last_pos", "last_neg"):
        assert surf["flags"][row[name]] == 1 and surf["ev"][row[name]][0] >= -32 * EPS * surf["ev"][row[name]][2], name
    assert np.array_equal(surf["cov"][row["last_pos"]][[0, 3, 4, 5]], surf["cov"][row["last_neg"]][[0, 3, 4, 5]])


@pytest.mark.parametrize("name", ["g2_lattice", "g1_room"])
def test_centroids_untouched(gpu, clouds, name):
    """export(), nearest() and size() of a moments map are byte-equal to a plain map's; a plain map still holds 40 bytes per slot"""
    xyz = clouds[name]
    for v in VOXELS:
        plain, mom = gpu.map_create(v), gpu.map_create(v, moments=True)
        assert plain.insert(xyz) == 0 and mom.insert(xyz) == 0
        a, b = plain.export(), mom.export()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), (name, v)
        assert plain.size() == mom.size()
        q = _queries(xyz[::20], v, 3)[0][::7]
        assert plain.nearest(q, v).tobytes() == mom.nearest(q, v).tobytes()
        pi, mi = plain.info(), mom.info()
        assert pi["bytes"] == 40 * pi["slots"] and mi["bytes"] == 112 * mi["slots"] and pi["slots"] == mi["slots"]
        surf = mom.surfels()
        assert np.array_equal(surf["key"], a[2]) and np.array_equal(surf["count"], a[1]) and surf["xyz"].tobytes() == a[0].tobytes()
        plain.close()
        mom.close()


@pytest.mark.parametrize("v", VOXELS)
@pytest.mark.parametrize("name", ["g2_lattice", "g1_room"])
def test_covariance_and_eigenpairs(gpu, clouds, name, v):
    """every voxel's key, count and centroid; every covariance entry within 2 ulp of the Fraction value N / (n^2 2^32) (compared with
    integers); ev ascending and within 32 x 2^-53 max|ev_ref| of the longdouble Jacobi's; the normal unit to 8 x 2^-53 and, where
    lambda_1 - lambda_0 > 1e-6 lambda_2, within fx_eig3's own bound of the reference's up to sign; the sign rule"""
    xyz = clouds[name]
    sums = S.voxel_sums(xyz, v)
    surf = _surfels_of(gpu, xyz, v)
    rows = None
    if len(surf) > FRACTION_VOXELS:
        rows = np.sort(np.random.Generator(np.random.PCG64(17)).choice(len(surf), FRACTION_VOXELS // 2, replace=False))
    cov_ref = _check_sums(surf, sums, v, (name, v), rows)
    sub = surf if rows is None else surf[rows]
    n_sep, n_clear = _check_eigen(sub, cov_ref, (name, v))
    print(name, v, "voxels", len(surf), "checked", len(sub), "planes", int((surf["flags"] & 1).sum()), "vector checks", n_sep, "sign checks", n_clear)
    assert n_sep > 0 and n_clear > 0


def test_order_independence(gpu, clouds):
    """the same cloud whole, in 7 unequal pieces, and permuted: the surfels() bytes are equal"""
    xyz = clouds["g1_room"]
    rng = np.random.Generator(np.random.PCG64(3))
    for v in (0.05, 0.2):
        whole = _surfels_of(gpu, xyz, v).tobytes()
        m = gpu.map_create(v, moments=True)
        cuts = np.sort(rng.choice(np.arange(1, len(xyz)), 6, replace=False))
        for part in np.split(xyz, cuts):
            assert m.insert(part) == 0
        assert m.surfels().tobytes() == whole, (v, "pieces")
        m.close()
        assert _surfels_of(gpu, xyz[rng.permutation(len(xyz))], v).tobytes() == whole, (v, "permuted")


@pytest.mark.parametrize("pts_per_lane", [1, 2])
def test_tile_edges(gpu, clouds, pts_per_lane):
    """inserts around the tile sizes of both forms of the moments insert (256 and 512 points per workgroup) against the restatement's
    integer sums, through the count and the covariance; a tile of 512 points in 512 distinct voxels (the LDS hash at half full); 2^20
    copies of one corner point of a v = 4.0 voxel (n M ~ 2^74: the 128-bit numerator), whose covariance is exactly 0"""
    gpu.set_dev_option("map_mom_pts", pts_per_lane)
    try:
        v = 0.2
        for n in (1, 255, 256, 257, 511, 512, 513, 1025):
            xyz = clouds["g1_room"][:n]
            _check_sums(_surfels_of(gpu, xyz, v), S.voxel_sums(xyz, v), v, ("edge", n))
        # (two inserts into one map: the second tile starts on a dirty table)
        xyz = clouds["g1_room"][:1025]
        m = _map(gpu, xyz[:513], v)
        assert m.insert(xyz[513:]) == 0
        _check_sums(m.surfels(), S.voxel_sums(xyz, v), v, "edge 513 + 512")
        m.close()
        i = np.arange(512)
        spread = np.stack([(i + 0.5) * v, 0.3 + 0.0 * i, -0.1 + 0.0 * i], -1).astype(np.float32)
        surf = _surfels_of(gpu, spread, v)
        assert len(surf) == 512 and np.all(surf["count"] == 1) and not surf["cov"].any()
        _check_sums(surf, S.voxel_sums(spread, v), v, "512 voxels")
        corner = np.nextafter(np.float32(8.0), np.float32(0.0))
        many = np.full((2**20, 3), corner, np.float32)
        surf = _surfels_of(gpu, many, 4.0)
        assert len(surf) == 1 and surf["count"][0] == 2**20 and surf["key"][0].tolist() == [1, 1, 1]
        assert not surf["cov"].any() and not surf["ev"].any() and surf["flags"][0] == 0
        u = int(S.quantise(many[:1], 4.0)[2][0, 0])
        assert 2**20 * (2**20 * u * u) > 2**73  # (the case does reach past 64 bits)
        # ... and with one more, distinct point the numerator is a small difference of two ~2^74 products
        more = np.concatenate([many, np.array([[4.0, 4.0, 4.0]], np.float32)])
        _check_sums(_surfels_of(gpu, more, 4.0), S.voxel_sums(more, 4.0), 4.0, "2^20 + 1")
    finally:
        gpu.set_dev_option("map_mom_pts", 1)


def test_growth_crop_and_clear_carry_the_moments(gpu, clouds):
    xyz = clouds["g1_room"]
    v = 0.2
    want = _surfels_of(gpu, xyz, v, reserve_voxels=1 << 18)
    m = gpu.map_create(v, reserve_voxels=8, moments=True)
    for part in np.array_split(xyz, 5):
        assert m.insert(part) == 0
    assert m.info()["growths"] > 1
    assert m.surfels().tobytes() == want.tobytes()
    # crop: byte-equal to a fresh map of exactly the points whose voxel is kept
    lo_all, hi_all = xyz.min(0).astype(np.float64), xyz.max(0).astype(np.float64)
    mid, ext = 0.5 * (lo_all + hi_all), hi_all - lo_all
    lo, hi = mid - 0.2 * ext, mid + 0.3 * ext
    keep = Q.crop_keep(Q.point_keys(xyz, v), v, lo, hi)
    assert 0 < keep.sum() < len(xyz)
    removed = m.crop(lo, hi)
    kept = _surfels_of(gpu, xyz[keep], v)
    assert removed == len(want) - len(kept) > 0 and m.surfels().tobytes() == kept.tobytes()
    assert m.info()["bytes"] == 112 * m.info()["slots"]
    # clear and reinsert
    m.clear()
    assert len(m.surfels()) == 0 and m.size() == (0, 0)
    assert m.insert(xyz) == 0
    assert m.surfels().tobytes() == want.tobytes()
    m.close()


@pytest.mark.parametrize("name", ["g2_lattice", "g1_room"])
def test_plane_query(gpu, clouds, name):
    """Against nearest() and surfels() of the same map.  The first 40 bytes of a record are nearest()'s record byte for byte, except
    bit 1 of flags, which the header defines as "the plane is valid" (the 80-byte record has no other flags word): the bytes are compared
    with that bit cleared, and flags itself - like dist - against the restatement on the exports.  normal and sigma2 are the chosen
    voxel's surfel record.  min_points 3 and 10, the 12-byte and the 48-byte query layouts, the found count."""
    xyz = clouds[name]
    planes = {3: 0, 10: 0}
    for v in VOXELS:
        m = _map(gpu, xyz, v)
        surf = m.surfels()
        q = _queries(xyz[::4], v, 11)[0][::3]
        found = Q.search(surf["key"], surf["xyz"], q, v)
        d_q12, d_q48 = gpu.to_device(q), gpu.to_device(_records(q))
        d_near, d_hits = gpu.alloc(R.MAP_HIT.itemsize * len(q)), gpu.alloc(R.MAP_PLANE_HIT.itemsize * len(q))
        for max_dist in (v, np.inf):
            n_near = m.nearest_device(R.Points(d_q12.ptr, 0, 12, 0, len(q)), max_dist, d_near)
            near = d_near.download(R.MAP_HIT, len(q))
            assert 0 < n_near < len(q)
            for min_points in (3, 10):
                want, idx = S.plane_hits(surf, q, v, max_dist, min_points, found)
                valid = (want["flags"] & 2) != 0
                planes[min_points] += int(valid.sum())
                for what, desc in (("xyz12", R.Points(d_q12.ptr, 0, 12, 0, len(q))), ("point48", R.Points(d_q48.ptr, d_q48.ptr + 24, 48, 48, len(q)))):
                    d_hits.upload(np.full(len(q) * 20, 0xA5A5A5A5, np.uint32))
                    n_found = m.nearest_plane_device(desc, max_dist, min_points, d_hits)
                    got = d_hits.download(R.MAP_PLANE_HIT, len(q))
                    tag = (name, v, max_dist, min_points, what)
                    assert n_found == n_near, tag
                    head = got.copy()
                    head["flags"] &= ~np.uint32(2)
                    assert np.ascontiguousarray(head.view(np.uint8).reshape(-1, 80)[:, :40]).tobytes() == near.tobytes(), tag
                    assert np.array_equal(got["flags"], want["flags"]), tag
                    at = np.maximum(idx, 0)
                    assert got["normal"][valid].tobytes() == surf["normal"][at][valid].tobytes(), tag
                    assert got["sigma2"][valid].tobytes() == np.ascontiguousarray(surf["ev"][at][valid][:, 0]).tobytes(), tag
                    assert not got["normal"][~valid].any() and not got["sigma2"][~valid].any() and not got["dist"][~valid].any(), tag
                    assert got["dist"].tobytes() == want["dist"].tobytes(), tag
                    assert got.tobytes() == want.tobytes(), tag
        # the host convenience
        want, _ = S.plane_hits(surf, q[:5000], v, v, 3)
        assert m.nearest_plane(q[:5000], v).tobytes() == want.tobytes()
        for b in (d_q12, d_q48, d_near, d_hits):
            b.free()
        m.close()
    assert planes[3] > planes[10] > 0, planes


def test_surfel_api_edges(gpu, clouds):
    lib = gpu.lib
    pts = clouds["g1_room"][:50_000]
    plain, mom = gpu.map_create(0.2), gpu.map_create(0.2, moments=True)
    plain.insert(pts)
    mom.insert(pts)
    n_vox = mom.size()[0]
    d_q = gpu.to_device(pts[:1000])
    d_hits = gpu.alloc(80 * 1000)
    d_out = gpu.alloc(128 * n_vox)
    desc = R.Points(d_q.ptr, 0, 12, 0, 1000)
    n = C.c_uint64(7)
    h = C.c_void_p(0)
    # unknown flag bits
    for flags in (2, 3, 0x80000000):
        assert lib.wc_map_create_ex(gpu.h, C.c_double(0.2), C.c_uint64(0), C.c_uint32(flags), C.byref(h)) == WC_ERR_ARG and not h.value
    assert lib.wc_map_create_ex(gpu.h, C.c_double(0.2), C.c_uint64(0), C.c_uint32(0), C.byref(h)) == 0  # flags = 0: wc_map_create
    assert lib.wc_map_export_surfels(gpu.h, h, C.c_void_p(d_out.ptr), C.c_uint64(n_vox), C.byref(n)) == WC_ERR_ARG
    assert lib.wc_map_destroy(gpu.h, h) == 0
    # the surfel and the plane call on a plain map
    assert lib.wc_map_export_surfels(gpu.h, plain.h, C.c_void_p(d_out.ptr), C.c_uint64(n_vox), C.byref(n)) == WC_ERR_ARG
    args = (C.byref(desc), C.c_double(1.0), C.c_uint32(3), C.c_void_p(d_hits.ptr), C.byref(n))
    assert lib.wc_map_nearest_plane(gpu.h, plain.h, *args) == WC_ERR_ARG
    with pytest.raises(Exception):
        plain.surfels()
    # min_points < 3, max_dist as wc_map_nearest, NULL map, NULL hits
    for mp in (0, 1, 2):
        assert lib.wc_map_nearest_plane(gpu.h, mom.h, C.byref(desc), C.c_double(1.0), C.c_uint32(mp), C.c_void_p(d_hits.ptr), C.byref(n)) == WC_ERR_ARG
    for d in (0.0, -1.0, float("nan")):
        assert lib.wc_map_nearest_plane(gpu.h, mom.h, C.byref(desc), C.c_double(d), C.c_uint32(3), C.c_void_p(d_hits.ptr), C.byref(n)) == WC_ERR_ARG
    assert lib.wc_map_nearest_plane(gpu.h, None, *args) == WC_ERR_ARG
    assert lib.wc_map_nearest_plane(gpu.h, mom.h, C.byref(desc), C.c_double(1.0), C.c_uint32(3), None, C.byref(n)) == WC_ERR_ARG
    assert lib.wc_map_export_surfels(gpu.h, None, C.c_void_p(d_out.ptr), C.c_uint64(n_vox), C.byref(n)) == WC_ERR_ARG
    assert lib.wc_map_export_surfels(gpu.h, mom.h, C.c_void_p(d_out.ptr), C.c_uint64(n_vox), None) == WC_ERR_ARG
    empty = R.Points(0, 0, 12, 0, 0)
    assert lib.wc_map_nearest_plane(gpu.h, mom.h, C.byref(empty), C.c_double(1.0), C.c_uint32(3), None, C.byref(n)) == 0 and n.value == 0
    assert len(mom.nearest_plane(np.zeros((0, 3), np.float32))) == 0
    # a map of another context
    from wildcat_slam_amd import lib as L

    other = L.Context(0)
    assert lib.wc_map_export_surfels(other.h, mom.h, C.c_void_p(d_out.ptr), C.c_uint64(n_vox), C.byref(n)) == WC_ERR_ARG
    assert lib.wc_map_nearest_plane(other.h, mom.h, *args) == WC_ERR_ARG
    other.close()
    # capacity
    rc, need = mom.surfels_device(d_out, n_vox - 1)
    assert rc == WC_ERR_CAPACITY and need == n_vox
    rc, need = mom.surfels_device(None, 0)
    assert rc == WC_ERR_CAPACITY and need == n_vox
    rc, got = mom.surfels_device(d_out, n_vox)
    assert rc == 0 and got == n_vox and d_out.download(R.MAP_SURFEL, n_vox).tobytes() == mom.surfels().tobytes()
    # an empty map
    e = gpu.map_create(0.2, moments=True)
    assert len(e.surfels()) == 0 and e.surfels_device(None, 0) == (0, 0)
    hits = e.nearest_plane(np.concatenate([pts[:100], BAD]))
    assert not hits["count"].any() and np.all(np.isinf(hits["d2"])) and not hits["normal"].any() and np.all(hits["flags"][:100] == 0)
    assert np.all(hits["flags"][100:] == 1)
    e.close()
    for x in (d_q, d_hits, d_out):
        x.free()
    plain.close()
    mom.close()


def test_facade_map_surfels(gpu):
    """the short stream of test_map_gpu with map_surfels on and off: the odometry and the map's export are byte-equal between the two;
    with it on, map_surfels() is a stand-alone moments map fed the same published sweeps, and map_query_planes is its nearest_plane"""
    from wildcat_slam_amd import lib

    msgs, imu, _ = synth.raw_stream(1.7, pts_per_s=300_000, gyro_bias=(0.0, 0.0, 0.02), t_start=1000.0)
    v = 0.1
    runs, exports = [], []
    for surfels_on in (True, False):
        odo = lib.Odometry(0)
        odo.set_fill_outputs(True)
        odo.set_map_voxel(v)
        if surfels_on:
            odo.set_map_surfels(True)
        scans, states = [], []

        def on_sweep():
            scans.append(_xyz(odo.outputs()["scan"]))
            st = odo.stats()
            states.append((odo.samples().tobytes(), st["binary"], st["unary"]))

        _drive(odo, msgs, imu, on_sweep)
        assert odo.sweeps() >= 2
        xyz, cnt = odo.map_export()
        exports.append((xyz.tobytes(), cnt.tobytes(), odo.map_size()))
        q = np.concatenate([scans[-1][::3], BAD])
        if surfels_on:
            ref = gpu.map_create(v, moments=True)
            for s in scans:
                assert ref.insert(s) == 0
            surf = odo.map_surfels()
            assert len(surf) == len(cnt) and surf.tobytes() == ref.surfels().tobytes()
            for min_points in (3, 10):
                got = odo.map_query_planes(q, v, min_points)
                assert got.tobytes() == ref.nearest_plane(q, v, min_points).tobytes()
                assert 0 < ((got["flags"] & 2) != 0).sum() < len(q)
            with pytest.raises(lib.WildcatError):
                odo.map_query_planes(q, v, 2)
            ref.close()
            # switching it off re-creates the map empty
            odo.set_map_surfels(False)
            assert odo.map_size() == (0, 0, 0) and len(odo.map_surfels()) == 0
        else:
            assert len(odo.map_surfels()) == 0
            hits = odo.map_query_planes(q, v, 3)
            assert not hits["count"].any() and np.all(np.isinf(hits["d2"])) and not hits["normal"].any()
        runs.append(states)
        odo.close()
    assert runs[0] == runs[1] and exports[0] == exports[1]
