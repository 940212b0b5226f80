"""The voxel map's surfels (include/wildcat_hip.h: "map surfels") - the parts that need no GPU: the restatement of map_surfel_ref.py
against the longdouble covariance of the raw points, the word sizes of the worst case, the new entry points and the two records."""
import ctypes as C
import os

import numpy as np
import pytest

import map_surfel_ref as S
from extract_ref import LD
from helpers import xyz_of as _xyz
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("name,v", [("g1_room", 0.2), ("g1_room", float(np.float32(0.8))), ("g2_lattice", 0.05), ("g2_lattice", 0.2)])
def test_restated_covariance_against_the_raw_points(name, v):
    """The restatement's covariance is that of the points moved onto the 2^-16 m grid.  Per coordinate the moved point differs from
    the raw one by d with |d| <= delta = 2^-17 + 2^-33 m (half a unit of u, plus the half unit of q that u is rounded from).  With
    x' = x + d:  cov'_ab - cov_ab = cov(x_a, d_b) + cov(d_a, x_b) + cov(d_a, d_b); by Cauchy-Schwarz |cov(x_a, d_b)| <=
    sqrt(cov_aa var d_b) <= delta sqrt(cov_aa) (var d <= E d^2 <= delta^2) and |cov(d_a, d_b)| <= delta^2, so
        |cov'_ab - cov_ab| <= delta (sqrt(cov_aa) + sqrt(cov_bb)) + delta^2.
    Held on every entry of every voxel; the raw covariance is formed in longdouble about the voxel's reference point."""
    xyz = _xyz(synth.g1_room(200_000)) if name == "g1_room" else _xyz(synth.g2_lattice(200, m=32)[0])
    sums = S.voxel_sums(xyz, v)
    delta = LD(2.0**-17 + 2.0**-33)
    p = xyz.astype(np.float64)
    worst = 0.0
    for i, rows in enumerate(sums["rows"]):
        n = int(sums["count"][i])
        assert n == len(rows)
        x = (p[rows] - S.map_ref(sums["keys"][i], v)).astype(LD)  # (|x| <= 2.0005: the shift is exact in longdouble)
        mean = x.sum(0) / LD(n)
        xc = x - mean
        raw = np.array([(xc[:, a] * xc[:, b]).sum() / LD(n) for a, b in S.PAIRS], LD)
        got = np.array([LD(float(c)) for c in S.covariance_exact(n, sums["U"][i], sums["M"][i])], LD)
        var = np.sqrt(np.maximum(raw[[0, 3, 5]], 0))
        bound = np.array([delta * (var[a] + var[b]) + delta * delta for a, b in S.PAIRS], LD)
        err = np.abs(got - raw)
        assert np.all(err <= bound), (name, v, sums["keys"][i], err, bound)
        worst = max(worst, float(np.max(err / bound)))
    print(name, v, "voxels", len(sums["rows"]), "max |dcov| / bound =", worst)


def test_worst_case_magnitudes_fit_their_words():
    """|u| at a voxel corner for v = 4.0 and N for 2^28 such points, in Python integers"""
    v = 4.0
    # a point just inside the far corner of a voxel whose reference point was rounded down, and the analytic limit |p - r| <= v / 2 + 2^-11
    corner = np.nextafter(np.float32(8.0), np.float32(0.0))
    keys, q, u = S.quantise(np.array([[corner, corner, corner], [4.0, 4.0, 4.0]], np.float32), v)
    assert keys.tolist() == [[1, 1, 1], [1, 1, 1]] and abs(int(u[0, 0])) <= 2**17 and int(u[1, 0]) == -(2**17)
    q_lim = int((v / 2 + 2.0**-11) * 2**32) + 1
    u_lim = (q_lim + 2**15) >> 16
    assert u_lim < 2**17.001 and u_lim * u_lim < 2**34.01
    n = 2**28
    assert n * u_lim * u_lim < 2**63  # a second-moment word after 2^28 such points
    assert n * u_lim < 2**63
    # N_aa = n sum u^2 - (sum u)^2 lies in [0, n sum u^2]; |N_ab| = n^2 |cov_ab| <= n^2 sqrt(cov_aa cov_bb) <= n^2 u_lim^2 as well.  Both
    # products n M and U U stay below the same limit, so the difference never leaves the signed 128-bit range on the way
    N_lim = n * (n * u_lim * u_lim)
    assert (n * u_lim) ** 2 <= N_lim < 2**91 and 2 * N_lim < 2**127
    assert n * n < 2**63  # n^2 as an unsigned 64-bit word (the count itself stays below 2^30: n^2 < 2^60)
    # the restatement on 3 copies of the corner point: covariance exactly zero although n M ~ 2^36
    s = S.voxel_sums(np.repeat(np.array([[corner, corner, corner]], np.float32), 3, 0), v)
    assert S.numerators(s["count"][0], s["U"][0], s["M"][0]) == [0] * 6


def test_header_declares_and_libraries_export_the_surfel_entry_points():
    from wildcat_slam_amd import lib

    declared = set(lib.declared_symbols())
    l = lib.load()
    for s in ("wc_map_create_ex", "wc_map_export_surfels", "wc_map_nearest_plane"):
        assert s in declared, s
        assert hasattr(l, s), s
    host = C.CDLL(os.path.join(HERE, "..", "wildcat-slam_amd", "host", "libwildcat_odometry.so"))
    for s in ("wc_odom_set_map_surfels", "wc_odom_map_surfels_on", "wc_odom_map_surfels", "wc_odom_map_query_planes"):
        assert hasattr(host, s), s


def _c_fields(name):
    """(declaration, ...) of a typedef struct in include/wc_types.h, comments stripped"""
    import re

    txt = open(os.path.join(HERE, "..", "include", "wc_types.h")).read()
    body = txt[txt.index("typedef struct %s {" % name) + len("typedef struct %s {" % name) : txt.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [" ".join(d.split()) for d in body.split(";") if d.strip()]


def test_map_surfel_and_plane_hit_records_match_the_header():
    assert R.MAP_MOMENTS == 1 and "#define WC_MAP_MOMENTS 1u" in open(os.path.join(HERE, "..", "include", "wc_types.h")).read()
    assert _c_fields("wc_map_surfel") == ["int32_t key[3]", "uint32_t count", "float xyz[3]", "uint32_t flags", "double cov[6]",
                                          "double ev[3]", "double normal[3]"]
    s = R.MAP_SURFEL
    assert s.itemsize == 128 and s.names == ("key", "count", "xyz", "flags", "cov", "ev", "normal")
    assert [s.fields[f][1] for f in s.names] == [0, 12, 16, 28, 32, 80, 104]
    assert [s.fields[f][0].base for f in s.names] == [np.dtype(x) for x in ("i4", "u4", "f4", "u4", "f8", "f8", "f8")]
    assert _c_fields("wc_map_plane_hit") == ["wc_map_hit hit", "double normal[3]", "double sigma2", "double dist"]
    h = R.MAP_PLANE_HIT
    assert h.itemsize == 80 and h.names == R.MAP_HIT.names + ("normal", "sigma2", "dist")
    assert [h.fields[f][1] for f in R.MAP_HIT.names] == [R.MAP_HIT.fields[f][1] for f in R.MAP_HIT.names]
    assert [h.fields[f][1] for f in ("normal", "sigma2", "dist")] == [40, 64, 72]
