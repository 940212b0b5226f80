"""Restatement, without a GPU, of a voxel map's state under a rigid pose (include/wildcat_hip.h: wc_map_merge_moved, wc_map_move_state;
DESIGN 8.13): every word a Python integer wrapped to 64 bits, every fp64 operation of steps 1 - 4 a single IEEE operation on Python
floats in the header's order (CPython never fuses a multiply and an add; int -> float and round() are correctly rounded, ties to even),
the deposit map_state_ref.absorb_ref's integer additions by key; and the surfels of a state, as map_register_ref.surfels_cpu makes them
from points."""
import math

import numpy as np

import map_query_ref as Q
import map_state_ref as MS
import map_surfel_ref as S
from wildcat_slam_amd import records as R

MASK64 = 2**64 - 1
UNIT = 4294967296.0  # 2^32
RIGID_TOL = 1e-9  # |(R^T R - I)_ij|: the header's design threshold
BIG_V, BIG_COUNT = 2.0, 2**26  # the count cap: with v > 2 a source voxel of more than 2^26 points is rejected


def _wrap(x):
    return ((x + 2**63) & MASK64) - 2**63


def pose12(T):
    """(3, 4) or 12 numbers -> list of 12 Python floats, row-major (R | t)"""
    return [float(x) for x in np.asarray(T, np.float64).reshape(-1)[:12]]


def rigid_ok(T):
    """the pose the move accepts: finite, and |(R^T R - I)_ij| <= 1e-9 with (R^T R)_ij = (R_0i R_0j + R_1i R_1j) + R_2i R_2j"""
    if T is None:
        return False
    T = pose12(T)
    if not all(math.isfinite(x) for x in T):
        return False
    for i in range(3):
        for j in range(3):
            g = (T[i] * T[j] + T[4 + i] * T[4 + j]) + T[8 + i] * T[8 + j]
            if not abs(g - (1.0 if i == j else 0.0)) <= RIGID_TOL:
                return False
    return True


def _ref(k, v):
    return float(S.map_ref(int(k), v))


def move_one(key, n, sums, mom, v, T, variant=None):
    """one voxel through steps 1 - 4 -> None when it is rejected, else dict(K, S: three ints, words: nine ints or None, Cr: the six
    llrint(C'_ab), c: the moved centroid).  variant (for the proof that the geometry bar bites): "transposed" forms R^T C R, "float32"
    rounds C' to float before llrint"""
    T = pose12(T)
    v, n = float(v), int(n)
    dn = float(n)
    c = [_ref(key[a], v) + (float(int(sums[a])) / dn) * (1.0 / UNIT) for a in range(3)]
    p = [((T[4 * a] * c[0] + T[4 * a + 1] * c[1]) + T[4 * a + 2] * c[2]) + T[4 * a + 3] for a in range(3)]
    if not all(math.isfinite(x) for x in p):
        return None
    f = [math.floor(x / v) for x in p]
    if any(abs(x) >= Q.KEY_LIM for x in f):
        return None
    if v > BIG_V and n > BIG_COUNT:
        return None
    K = [int(x) for x in f]
    m = [round((p[a] - _ref(K[a], v)) * UNIT) for a in range(3)]
    out = dict(K=K, S=[_wrap(n * m[a]) for a in range(3)], words=None, Cr=None, c=p)
    if mom is not None:
        Rm = [[T[4 * i + j] for j in range(3)] for i in range(3)]
        if variant == "transposed":
            Rm = [[Rm[j][i] for j in range(3)] for i in range(3)]
        c6 = []
        for N in S.numerators(n, mom[:3], mom[3:]):
            mag = float(abs(N))  # (one rounding of the magnitude, ties to even)
            c6.append((-mag if N < 0 else mag) / dn)
        Cm = [[c6[0], c6[1], c6[2]], [c6[1], c6[3], c6[4]], [c6[2], c6[4], c6[5]]]
        B = [[(Rm[i][0] * Cm[0][j] + Rm[i][1] * Cm[1][j]) + Rm[i][2] * Cm[2][j] for j in range(3)] for i in range(3)]
        e = [(m[a] + 2**15) >> 16 for a in range(3)]
        Cr = []
        for i, j in S.PAIRS:
            cp = (B[i][0] * Rm[j][0] + B[i][1] * Rm[j][1]) + B[i][2] * Rm[j][2]
            if variant == "float32":
                cp = float(np.float32(cp))
            Cr.append(round(cp))
        out["Cr"] = Cr
        out["words"] = [_wrap(n * e[a]) for a in range(3)] + [_wrap(Cr[x] + n * e[i] * e[j]) for x, (i, j) in enumerate(S.PAIRS)]
    return out


def moved_ref(vox, mom, v, T, variant=None):
    """wc_map_move_state restated -> (out_vox, out_mom or None, records rejected, details: per record move_one's dict or None).  A
    rejected record - by the move, or one wc_map_absorb would reject - is all zeros"""
    assert rigid_ok(T) and 0.01 <= float(v) <= 4.0
    vox = np.ascontiguousarray(vox, R.MAP_VOXEL)
    bad = MS.rejected(vox)
    out = np.zeros(len(vox), R.MAP_VOXEL)
    out_mom = None if mom is None else np.zeros((len(vox), 9), np.int64)
    details, n_rej = [], 0
    for i in range(len(vox)):
        d = None if bad[i] else move_one(vox["key"][i], vox["count"][i], vox["sum"][i], None if mom is None else [int(x) for x in mom[i]], v,
                                         T, variant)
        details.append(d)
        if d is None:
            n_rej += 1
            continue
        out["key"][i], out["count"][i], out["sum"][i] = d["K"], vox["count"][i], d["S"]
        if mom is not None:
            out_mom[i] = d["words"]
    return out, out_mom, n_rej, details


def merge_moved_ref(dst_state, src_state, v, T, moments=True):
    """wc_map_merge_moved restated on two states ((vox, mom or None) each) -> (vox, mom or None, [voxels applied, points applied,
    voxels rejected, points rejected]); moments: dst holds them (then src must)"""
    svox, smom = src_state
    mv, mm, n_rej, det = moved_ref(svox, smom if moments else None, v, T)
    ok = np.array([d is not None for d in det], bool)
    cnt = svox["count"].astype(np.int64)
    out, out_mom, rej2 = MS.absorb_ref([(dst_state[0], dst_state[1] if moments else None), (mv, mm)], moments=moments)
    assert rej2 == n_rej
    return out, out_mom, [int(ok.sum()), int(cnt[ok].sum()), int((~ok).sum()), int(cnt[~ok].sum())]


def surfels_of_state(vox, mom, v):
    """the MAP_SURFEL records of a state, as map_register_ref.surfels_cpu makes them from points: the correctly rounded covariance of the
    integer numerators, eigenpairs by the longdouble Jacobi iteration"""
    m = len(vox)
    out = np.zeros(m, R.MAP_SURFEL)
    out["key"], out["count"] = vox["key"], vox["count"]
    c = vox["count"].astype(np.float64)[:, None]
    out["xyz"] = (S.map_ref(vox["key"], v) + vox["sum"].astype(np.float64) / (c * S.UNIT_Q)).astype(np.float32)
    for i in range(m):
        n = int(vox["count"][i])
        out["cov"][i] = [N / (n * n * 2**32) for N in S.numerators(n, mom[i][:3], mom[i][3:])]
    ev, nrm = S.eigen_ref(out["cov"])
    out["ev"], out["normal"] = ev.astype(np.float64), nrm.astype(np.float64)
    out["flags"] = ((out["count"] >= 3) & (out["ev"][:, 2] > 0)).astype(np.uint32)
    return out


def pose_of(deg, axis, t):
    """`deg` degrees about axis / |axis| and the translation t -> (3, 4)"""
    import map_register_ref as G

    axis = np.asarray(axis, np.float64)
    return np.concatenate([G.rodrigues(np.deg2rad(deg) * axis / np.linalg.norm(axis)), np.asarray(t, np.float64).reshape(3, 1)], 1)


def quarter_turn(v, shift=(3, -2, 1)):
    """90 degrees about z, exactly, plus a translation of whole voxels -> (3, 4)"""
    return np.array([[0.0, -1.0, 0.0, shift[0] * float(v)], [1.0, 0.0, 0.0, shift[1] * float(v)], [0.0, 0.0, 1.0, shift[2] * float(v)]])


def compose(A, B):
    """A after B, both (3, 4) -> (3, 4)"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return np.concatenate([A[:, :3] @ B[:, :3], (A[:, :3] @ B[:, 3] + A[:, 3])[:, None]], 1)
