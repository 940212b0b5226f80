"""A plain numpy longdouble restatement of the per-point and per-surfel stages in front of the hot path - the point pre-filter
(lidar_odometry.cc:489-496), UndistortSweep (:143-158), UpdateSurfelPoses (:160-170, surfel.h:48-58) and the reversed copy of
ShrinkToFit - and the seeded inputs tests/test_sweep_ref.py and tests/test_sweep_precision_gpu.py hold them on.  Nothing here
imports the library or the oracle: the record layouts are restated too (the CPU test compares them with records.py).

Conventions: quaternions are (w, x, y, z); LD arrays carry the exact values of the fp32 / fp64 inputs, every operation after
that is longdouble (64-bit mantissa on x86: about 2^-11 of the fp64 roundings the bounds are made of).
"""
import numpy as np

LD = np.longdouble
U = 2.0**-53  # fp64 unit roundoff
ONE_EPS = LD(1) - LD(2.220446049250313e-16)  # Eigen's slerp threshold 1 - epsilon (dmath.h::qslerp)
TIE_CAP = 2  # coordinates per cloud that may fall under the tie clause

POINT = np.dtype({"names": ["x", "y", "z", "intensity", "time", "ring"], "formats": ["f4", "f4", "f4", "f4", "f8", "u2"],
                  "offsets": [0, 4, 8, 16, 24, 32], "itemsize": 48})
SURFEL = np.dtype([("t", "f8"), ("center", "f8", 3), ("cov", "f8", 9), ("normal", "f8", 3), ("resolution", "f8"), ("sigma", "f8")])
POSE = np.dtype([("pos", "f8", 3), ("quat", "f8", 4)])
IMU_STATE = np.dtype([("t", "f8"), ("pos", "f8", 3), ("quat", "f8", 4), ("acc", "f8", 3), ("gyr", "f8", 3)])
assert POINT.itemsize == 48 and SURFEL.itemsize == 144 and POSE.itemsize == 56 and IMU_STATE.itemsize == 112


# ---- quaternion algebra in longdouble ------------------------------------------------------------------------------------------
def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def qrot(q, v):
    """v + 2w(u x v) + 2 u x (u x v): Eigen's quaternion * vector, NOT normalised"""
    w, u = q[..., 0:1], q[..., 1:4]
    uv = cross(u, v)
    return v + 2 * w * uv + 2 * cross(u, uv)


def qconj(q):
    return q * np.array([1, -1, -1, -1], LD)


def qmul(a, b):
    aw, ax, ay, az = (a[..., i] for i in range(4))
    bw, bx, by, bz = (b[..., i] for i in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx], -1)


def qmat(q):
    """Eigen's toRotationMatrix: the polynomial in the components, not normalised"""
    w, x, y, z = (q[..., i] for i in range(4))
    r = np.empty(q.shape[:-1] + (3, 3), LD)
    r[..., 0, 0], r[..., 0, 1], r[..., 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    r[..., 1, 0], r[..., 1, 1], r[..., 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    r[..., 2, 0], r[..., 2, 1], r[..., 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    return r


def qslerp(a, f, b):
    """Eigen's slerp as dmath.h::qslerp states it: not normalised, linear when |d| >= 1 - eps, b negated when d < 0.  -> (q, d)"""
    d = (a * b).sum(-1)
    ad = np.abs(d)
    lin = ad >= ONE_EPS
    th = np.arccos(np.minimum(ad, LD(1)))
    st = np.where(lin, LD(1), np.sin(th))
    s0 = np.where(lin, 1 - f, np.sin((1 - f) * th) / st)
    s1 = np.where(lin, f, np.sin(f * th) / st)
    s1 = np.where(d < 0, -s1, s1)
    return s0[..., None] * a + s1[..., None] * b, d


def interpolate(imu, t):
    """lower_bound over the states' stamps, fac, lerp, slerp.  ok: the reference's CHECK(idx >= 1 && idx < size) holds"""
    it = np.ascontiguousarray(imu["t"])
    lo = np.searchsorted(it, t, "left")
    ok = (lo >= 1) & (lo < len(it))
    lo_c = np.clip(lo, 1, max(len(it) - 1, 1))
    a, b = imu[lo_c - 1], imu[lo_c]
    fac = (t.astype(LD) - a["t"].astype(LD)) / (b["t"].astype(LD) - a["t"].astype(LD))
    pos = a["pos"].astype(LD) * (1 - fac)[:, None] + b["pos"].astype(LD) * fac[:, None]
    rot, d = qslerp(a["quat"].astype(LD), fac, b["quat"].astype(LD))
    pmax = np.maximum(np.abs(a["pos"]), np.abs(b["pos"]))  # per coordinate
    return dict(lo=lo, ok=ok, fac=fac, pos=pos, rot=rot, d=d, pmax=pmax)


# ---- fp32 rounding boundaries ----------------------------------------------------------------------------------------------------
def f32_round(w):
    """-> (float32(w), distance of w from the nearest fp32 rounding boundary, the float on the other side of that boundary)"""
    with np.errstate(invalid="ignore", over="ignore"):
        f = w.astype(np.float32)
        up, dn = np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))
        du = np.abs((f.astype(LD) + up.astype(LD)) / 2 - w)
        dd = np.abs(w - (f.astype(LD) + dn.astype(LD)) / 2)
    return f, np.minimum(du, dd), np.where(du <= dd, up, dn)


def check_f32(got, w, bound):
    """the kernel's float must equal float32(w); where w lies within `bound` of a rounding boundary the float on the other side of
    that boundary is allowed too.  -> (mask of wrong entries, number of entries under the tie clause - from the reference alone)"""
    f, dist, other = f32_round(w)
    tie = dist.astype(np.float64) <= bound
    ok = (got == f) | (tie & (got == other)) | (np.isnan(got) & np.isnan(f))
    return ~ok, int(tie.sum())


def records_at(a, index):
    """a[index] with every byte of the records (numpy's own indexing copies a padded record field by field and drops the rest)"""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(len(a), a.dtype.itemsize)
    return np.ascontiguousarray(raw[index]).view(a.dtype).reshape(-1)


# ---- the stages ------------------------------------------------------------------------------------------------------------------
def xyz_of(points):
    return np.stack([points["x"], points["y"], points["z"]], -1)


def prefilter(points, ext_quat, ext_t, min_range, max_range, blind_min, blind_max):
    """the extrinsic in longdouble, cast to fp32; the decisions are fp32 BY DEFINITION in the reference (Eigen's float norm:
    x*x + y*y + z*z in that order, correctly rounded sqrt), the comparisons double, the blind box inclusive"""
    v = xyz_of(points)
    p = qrot(np.asarray(ext_quat, np.float64).astype(LD), v.astype(LD)) + np.asarray(ext_t, np.float64).astype(LD)
    f, dist, _ = f32_round(p)
    x, y, z = f[:, 0], f[:, 1], f[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        nrm = np.sqrt(x * x + y * y + z * z)
        assert nrm.dtype == np.float32
        nd, fd = nrm.astype(np.float64), f.astype(np.float64)
        blind = ((fd >= np.asarray(blind_min, np.float64)) & (fd <= np.asarray(blind_max, np.float64))).all(axis=1)
        keep = ~((nd < min_range) | (nd > max_range) | blind)
    out = records_at(points, keep)
    out["x"], out["y"], out["z"] = x[keep], y[keep], z[keep]
    # the same count as B_w: ~10 rounded fp64 operations on terms <= |v|, one addition of t.  With a zero vector part and a zero t every
    # operation is exact (v + 1 * 0 + 0 + 0): no coordinate is a tie then, whatever it is
    q64, t64 = np.asarray(ext_quat, np.float64), np.asarray(ext_t, np.float64)
    exact = not q64[1:].any() and not t64.any()
    bound = (0.0 if exact else 16 * U) * (np.linalg.norm(v.astype(np.float64), axis=1) + np.abs(t64).max())
    return dict(keep=keep, out=out, p=p, xyz=f, nrm=nrm, blind=blind, dist=dist, bound=bound)


def monotonic(times, keep, prev_time):
    """CHECK(points_buff_.empty() || pt.time >= points_buff_.back().time): every incoming point against the last KEPT point before
    it, or prev_time (-inf: nothing buffered) when there is none.  -> (held, indices of the violating points)"""
    n = len(times)
    last = np.maximum.accumulate(np.where(keep, np.arange(n), -1))
    before = np.concatenate([[-1], last[:-1]]).astype(np.int64)
    prev = np.where(before >= 0, times[np.maximum(before, 0)], prev_time)
    bad = np.flatnonzero(~(times >= prev))
    return len(bad) == 0, bad


def undistort(points, imu):
    I = interpolate(imu, np.ascontiguousarray(points["time"]))
    v = xyz_of(points)
    I["w"] = qrot(I["rot"], v.astype(LD)) + I["pos"]
    I["bound"] = 16 * U * (np.linalg.norm(v.astype(np.float64), axis=1) + I["pmax"].max(axis=1))  # B_w
    return I


def update_poses(imu, surf, flags):
    I = interpolate(imu, np.ascontiguousarray(surf["t"]))
    rc = qconj(I["rot"])
    c0 = surf["center"].astype(LD)
    I["center"] = qrot(rc, c0 - I["pos"])
    I["normal"] = qrot(rc, surf["normal"].astype(LD))
    Rm = qmat(I["rot"])
    C = surf["cov"].astype(LD).reshape(-1, 3, 3)
    I["cov"] = np.matmul(np.matmul(np.swapaxes(Rm, 1, 2), C), Rm)
    I["fresh"] = np.asarray(flags) == 0
    I["b_pos"] = 4 * U * I["pmax"]
    I["b_quat"] = 8 * U
    I["b_center"] = 16 * U * (np.linalg.norm((c0 - I["pos"]).astype(np.float64), axis=1) + np.abs(I["pos"]).max(axis=1).astype(np.float64))
    I["b_normal"] = 16 * U
    I["b_cov"] = K_COV * U * np.abs(surf["cov"]).max(axis=1)
    return I


# (R^T C) R with R = qmat(rot), per entry, first order.  rot carries eps_q = 8 U per component (the bound asserted on it).  An entry of
# R is 1 or 0 plus two terms 2 q_a q_b: its perturbation is <= 2 eps_q (|q_a| + |q_b|) per term, i.e. <= 4 sqrt(2) eps_q < 6 eps_q on the
# diagonal and <= 2 eps_q (|w| + |x| + |y| + |z|) <= 4 eps_q off it, plus the 3 roundings of its own evaluation: eps_R = (6 * 8 + 3) U.
# M = R^T C is three products and two additions per entry: |dM| <= 3 eps_R |C|max + 3 U sum_k |R_ki| |C|max, with sum_k |R_ki| <= sqrt 3.
# Cb = M R the same again on |M| <= sqrt 3 |C|max:  |dCb| <= sqrt 3 |dM| + 3 sqrt 3 |C|max eps_R + 3 U * 3 |C|max
#    = (6 sqrt 3 eps_R / U + 18) U |C|max = (6 * 1.7321 * 51 + 18) U |C|max < 549 U |C|max
K_COV = 549


def reverse_copy(surf, pose):
    rev = np.arange(len(surf))[::-1]
    return records_at(surf, rev), records_at(pose, rev)


# ---- the comparisons the CPU and the GPU tests share --------------------------------------------------------------------------
def compare_poses(ref, surf_in, flags_in, s, pose, fl):
    """the assertions of the pose update, shared with the GPU test -> worst error / bound per field"""
    n = len(s)
    fresh = ref["fresh"]
    assert fl.all() and len(fl) == n
    for f in ("t", "sigma", "resolution"):
        assert s[f].tobytes() == surf_in[f].tobytes()
    assert s[~fresh].tobytes() == surf_in[~fresh].tobytes()  # already in the body frame: only the pose is new
    r = {}
    r["pos"] = float((np.abs(pose["pos"].astype(LD) - ref["pos"]).astype(np.float64) / ref["b_pos"]).max())
    r["quat"] = float(np.abs(pose["quat"].astype(LD) - ref["rot"]).max() / ref["b_quat"])
    if fresh.any():
        g = s[fresh]
        r["center"] = float((np.abs(g["center"].astype(LD) - ref["center"][fresh]).max(axis=1).astype(np.float64) / ref["b_center"][fresh]).max())
        r["normal"] = float(np.abs(g["normal"].astype(LD) - ref["normal"][fresh]).max() / ref["b_normal"])
        dc = np.abs(g["cov"].reshape(-1, 3, 3).astype(LD) - ref["cov"][fresh]).max(axis=(1, 2)).astype(np.float64)
        r["cov"] = float((dc / ref["b_cov"][fresh]).max())
    return r


def compare_survivors(out, ref, padding=True):
    """survivors against the cast reference, bit for bit up to the tie clause, everything else of the record byte for byte (padding=False:
    the named fields only, for records that went through a numpy copy, which drops the bytes between the fields)"""
    want = ref["out"]
    assert len(out) == len(want)
    got = np.stack([out["x"], out["y"], out["z"]], -1)
    bad, _ = check_f32(got, ref["p"][ref["keep"]], ref["bound"][ref["keep"]][:, None])
    assert not bad.any()
    a, b = out.view(np.uint8).reshape(-1, 48), want.view(np.uint8).reshape(-1, 48)
    for lo, hi in ((12, 48),) if padding else ((16, 20), (24, 34)):
        assert np.array_equal(a[:, lo:hi], b[:, lo:hi])


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
SEED = 0x53575031
KINDS = ("smooth", "epoch", "steps", "signs", "tiny")
SIZES = (37, 2, 5001)
LENGTHS = (1, 255, 256, 257, 1000)
LONG_LENGTHS = (20001, 70001)
POS0 = np.array([800.0, -300.0, 20.0])
# planted pairs of consecutive states (index of the first): equal quaternions, dot = 1 - 2^-53 (linear side), dot = 1 - 2^-51
# (slerp side), a near half-turn (|d| ~ 1e-3)
PLANT = {"equal": 5, "lin": 9, "slerp": 13, "half": 17}


def _qexp(r):
    th = np.linalg.norm(r, axis=-1, keepdims=True)
    a = r / np.maximum(th, 1e-300)
    return np.concatenate([np.cos(th / 2), np.sin(th / 2) * a], -1)


def _qmul64(a, b):
    return qmul(np.asarray(a, np.float64), np.asarray(b, np.float64)).astype(np.float64)


def imu_table(kind, size):
    """`size` states with uneven 2-20 ms spacing, positions near (800, -300, 20) m"""
    rng = np.random.default_rng([SEED, KINDS.index(kind), size])
    t0 = 1.6e9 if kind == "epoch" else 1000.0
    s = np.cumsum(rng.uniform(0.002, 0.020, size))
    imu = np.zeros(size, IMU_STATE)
    imu["t"] = t0 + s
    assert np.all(np.diff(imu["t"]) > 0)
    imu["pos"] = POS0 + np.stack([0.5 * s, 0.3 * np.sin(0.4 * s), 0.1 * np.sin(0.7 * s)], -1)
    smooth = _qexp(np.stack([0.05 * np.sin(0.5 * s), 0.04 * np.sin(0.3 * s), 0.2 * s], -1))
    if kind in ("smooth", "epoch"):
        q = smooth
    elif kind == "signs":
        q = smooth * np.where(np.arange(size) % 2 == 1, -1.0, 1.0)[:, None]
    else:
        ang = 1.2 if kind == "steps" else 1e-9
        ax = rng.normal(size=(size, 3))
        ax /= np.linalg.norm(ax, axis=1, keepdims=True)
        q = np.empty((size, 4))
        q[0] = smooth[0]
        for i in range(1, size):
            q[i] = _qmul64(q[i - 1], _qexp(ang * ax[i]))
            q[i] /= np.linalg.norm(q[i])
    if size > PLANT["half"] + 1:
        i = PLANT["equal"]
        q[i + 1] = q[i]
        for name, e in (("lin", 2.0**-53), ("slerp", 2.0**-51)):
            i = PLANT[name]
            c = 1.0 - e
            q[i], q[i + 1] = (1.0, 0.0, 0.0, 0.0), (c, np.sqrt(1.0 - c * c), 0.0, 0.0)
        i = PLANT["half"]
        q[i + 1] = _qmul64(q[i], _qexp(np.array([0.6, -0.64, 0.48]) * (np.pi - 2e-3)))
    imu["quat"] = q
    imu["acc"], imu["gyr"] = rng.normal(size=(size, 3)), rng.normal(size=(size, 3))
    return imu


def stamps(imu, n, rng):
    """n stamps inside the table: 30 exactly on interior states and one on the last state (as far as n allows), the rest inside
    intervals drawn from the planted pairs and from the whole table.  Not sorted: neither stage needs it"""
    size = len(imu)
    it = imu["t"]
    pool = np.arange(1, size)  # interval k lies between state k - 1 and state k
    if size > 64:
        pool = np.concatenate([np.array(sorted(PLANT.values())) + 1, rng.choice(pool, 200, replace=False), [1, size - 1]])
    k = pool[rng.integers(0, len(pool), n)]
    f = rng.uniform(0.0, 1.0, n)
    t = it[k - 1] + f * (it[k] - it[k - 1])
    t = np.where(t <= it[k - 1], it[k], np.minimum(t, it[k]))
    exact = []
    if size > 2:
        exact = list(rng.choice(np.arange(1, size - 1), min(30, size - 2), replace=False))
    exact = [size - 1] + exact  # the last state is a valid stamp
    slots = rng.permutation(n)[: min(len(exact), max(n // 2, 1))]
    for s_, e in zip(slots, exact):
        t[s_] = it[e]
    return t


def cloud(kind, size, n):
    """-> (points, imu): radii log-uniform in 1e-3 ... 120 m"""
    imu = imu_table(kind, size)
    rng = np.random.default_rng([SEED, 7, KINDS.index(kind), size, n])
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.exp(rng.uniform(np.log(1e-3), np.log(120.0), n))
    pts = np.zeros(n, POINT)
    xyz = (d * r[:, None]).astype(np.float32)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["time"] = stamps(imu, n, rng)
    pts["intensity"] = rng.uniform(0, 255, n).astype(np.float32)
    pts["ring"] = rng.integers(0, 64, n)
    raw = pts.view(np.uint8).reshape(n, 48)  # the padding bytes carry something too: they must pass through
    for lo, hi in ((12, 16), (20, 24), (34, 48)):
        raw[:, lo:hi] = rng.integers(0, 256, (n, hi - lo), dtype=np.uint8)
    return pts, imu


def undistort_cases():
    """(kind, states, points): every table at n = 1000, the block-tail lengths on one of them, one case at each long length"""
    c = [(k, s, 1000) for k in KINDS for s in SIZES]
    c += [("signs", 37, n) for n in LENGTHS if n != 1000]
    c += [("steps", 37, LONG_LENGTHS[0]), ("epoch", 37, LONG_LENGTHS[1])]
    return c


def pose_cases():
    c = [(k, s, 1000) for k in KINDS for s in SIZES]
    c += [("signs", 37, n) for n in LENGTHS if n != 1000]
    return c


def surfels(kind, size, n):
    """-> (surfels, flags, imu): R.SURFEL records built directly; centres up to 1 km from the origin, anisotropic covariances with
    eigenvalues in 1e-6 ... 1 m^2, random flags"""
    imu = imu_table(kind, size)
    rng = np.random.default_rng([SEED, 11, KINDS.index(kind), size, n])
    s = np.zeros(n, SURFEL)
    s["t"] = stamps(imu, n, rng)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    s["center"] = d * np.exp(rng.uniform(0.0, np.log(1000.0), n))[:, None]
    nn = rng.normal(size=(n, 3))
    s["normal"] = nn / np.linalg.norm(nn, axis=1, keepdims=True)
    Q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    lam = np.exp(rng.uniform(np.log(1e-6), 0.0, (n, 3)))
    C = np.einsum("nij,nj,nkj->nik", Q, lam, Q)
    s["cov"] = (0.5 * (C + np.swapaxes(C, 1, 2))).reshape(n, 9)
    s["resolution"], s["sigma"] = rng.uniform(0.1, 0.8, n), rng.uniform(1e-3, 0.1, n)
    flags = rng.integers(0, 2, n).astype(np.uint8)
    if n > 1:
        flags[:2] = (0, 1)
    return s, flags, imu


# ---- pre-filter inputs -----------------------------------------------------------------------------------------------------------
EXTS = ("identity", "lidar2imu")
EXT_T = np.array([-0.001, -0.00855, 0.055])  # lio_config.h:23-28, as synth.EXT_T (compared in the CPU test)
MIN_RANGE, MAX_RANGE = 0.3, 120.0
BOX = (np.array([-0.8, -0.5, -0.4]), np.array([0.3, 0.5, 0.4]))
BOX_EXACT = (np.array([-0.5, -0.25, -0.5]), np.array([0.25, 0.5, 0.25]))  # float-representable faces
BOX_AWAY = (np.array([10.0, 10.0, 10.0]), np.array([10.5, 10.5, 10.5]))
PATTERNS = ("none", "all", "alternate", "runs")
RUN = 9000  # longer than a tile of the device scan


def ext(name):
    """-> (quat, t).  The lidar -> imu rotation is a half-turn about (1, -1, 0) / sqrt 2 up to its 5e-8 entries: the quaternion
    synth.mat_to_quat gives for it (compared in the CPU test)"""
    if name == "identity":
        return np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3)
    return np.array([0.0, np.sqrt(0.5), -np.sqrt(0.5), 0.0]), EXT_T.copy()


def _to_input(name, targets):
    """fp32 lidar-frame points whose image under the extrinsic is near `targets` (imu frame)"""
    q, t = ext(name)
    return qrot(qconj(q.astype(LD)), (np.asarray(targets, np.float64) - t).astype(LD)).astype(np.float32)


def _scan(name, target, axis, k=8):
    """2k + 1 inputs that differ by one ulp each in the input coordinate that moves output coordinate `axis`"""
    q, _ = ext(name)
    j = int(np.argmax(np.abs(qmat(q.astype(LD)).astype(np.float64)[axis])))
    p = np.repeat(_to_input(name, [target]), 2 * k + 1, axis=0)
    for step in range(k):
        p[k + 1 + step:, j] = np.nextafter(p[k + 1 + step:, j], np.float32(np.inf))
        p[: k - step, j] = np.nextafter(p[: k - step, j], np.float32(-np.inf))
    return p


def _points(xyz, rng):
    n = len(xyz)
    pts = np.zeros(n, POINT)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["time"] = 1000.0 + 1e-5 * np.arange(n)
    pts["intensity"] = rng.uniform(0, 255, n).astype(np.float32)
    pts["ring"] = rng.integers(0, 64, n)
    raw = pts.view(np.uint8).reshape(n, 48)
    for lo, hi in ((12, 16), (20, 24), (34, 48)):
        raw[:, lo:hi] = rng.integers(0, 256, (n, hi - lo), dtype=np.uint8)
    return pts


def norm_variants(f):
    """fp32 norm as the reference computes it, with the sum fused (fma(z, z, fma(y, y, x * x))), and in fp64"""
    x, y, z = (f[:, i] for i in range(3))
    xd, yd, zd = (f[:, i].astype(np.float64) for i in range(3))
    plain = np.sqrt(x * x + y * y + z * z)
    s = (xd * xd).astype(np.float32)
    s = (yd * yd + s.astype(np.float64)).astype(np.float32)
    s = (zd * zd + s.astype(np.float64)).astype(np.float32)
    return plain, np.sqrt(s), np.sqrt(xd * xd + yd * yd + zd * zd)


def _in_range(nrm):
    nd = nrm.astype(np.float64)
    return ~((nd < MIN_RANGE) | (nd > MAX_RANGE))


def range_edges(name):
    """points on the axes whose fp32 norm is float32(limit) and its neighbours, and diagonal points at the limits chosen - from
    the reference's own values - so that the fused sum, or an fp64 norm, decides differently from the fp32 norm.  The blind box
    is far away.  -> (points, args, dict of index arrays)"""
    rng = np.random.default_rng([SEED, 21, EXTS.index(name)])
    q, t = ext(name)
    parts, groups, o = [], {}, 0
    for lim in (MIN_RANGE, MAX_RANGE):
        l32 = np.float32(lim)
        # on the axes of the LIDAR frame: t + s e_a with |t + s e_a| = limit (a target with zero coordinates in the imu frame would
        # come out of a cancellation against t, where an absolute error of B covers many fp32 spacings: all of them ties)
        ax = []
        for a in range(3):
            root = np.sqrt(t[a] ** 2 - (t @ t - float(l32) ** 2))
            ax += [_scan(name, t + s_ * np.eye(3)[a], a) for s_ in (-t[a] + root, -t[a] - root)]
        ax = np.concatenate(ax)
        groups["axis%g" % lim] = np.arange(o, o + len(ax))
        parts.append(ax)
        o += len(ax)
        d = rng.normal(size=(40000, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        cand = _to_input(name, d * (float(l32) * (1 + rng.uniform(-3, 3, (40000, 1)) * 2.0**-24)))
        f = f32_round(qrot(q.astype(LD), cand.astype(LD)) + t.astype(LD))[0]
        plain, fused, dbl = norm_variants(f)
        kp = _in_range(plain)
        sel_f = np.flatnonzero(kp != _in_range(fused))[:16]
        sel_d = np.flatnonzero(kp != _in_range(dbl))[:16]
        for key, sel in (("fused%g" % lim, sel_f), ("dbl%g" % lim, sel_d), ("diag%g" % lim, np.arange(16))):
            groups[key] = np.arange(o, o + len(sel))
            parts.append(cand[sel])
            o += len(sel)
    return _points(np.concatenate(parts), rng), (q, t, MIN_RANGE, MAX_RANGE) + BOX_AWAY, groups


def blind_edges(name):
    """coordinates exactly on each face of a float-representable blind box and ulps either side of it, the other two coordinates
    inside the box and the norm in range; NaN coordinates.  -> (points, args, dict face -> index array)"""
    rng = np.random.default_rng([SEED, 22, EXTS.index(name)])
    q, t = ext(name)
    parts, groups, o = [], {}, 0
    for a in range(3):
        for side in (0, 1):
            tgt = np.full(3, 0.2)
            tgt[a] = BOX_EXACT[side][a]
            sc = _scan(name, tgt, a)
            groups[(a, side)] = np.arange(o, o + len(sc))
            parts.append(sc)
            o += len(sc)
    nan = np.full((6, 3), 1.0, np.float32)
    nan[0, 0] = nan[1, 1] = nan[2, 2] = nan[3] = np.nan
    nan[4], nan[5] = (0.1, np.nan, 0.1), (np.nan, 500.0, 0.0)
    groups["nan"] = np.arange(o, o + len(nan))
    parts.append(nan)
    return _points(np.concatenate(parts), rng), (q, t, MIN_RANGE, MAX_RANGE) + BOX_EXACT, groups


def random_cloud(name, n, pattern=None):
    """radii log-uniform in 0.05 ... 400 m (dropped, kept, dropped), some points inside the blind box; with a pattern the keep
    decision is forced by the radius: nothing kept, everything kept, alternating, runs of RUN"""
    rng = np.random.default_rng([SEED, 23, EXTS.index(name), n, PATTERNS.index(pattern) if pattern else 99])
    q, t = ext(name)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    if pattern is None:
        r = np.exp(rng.uniform(np.log(0.05), np.log(400.0), n))
        tg = d * r[:, None]
        inside = rng.uniform(size=n) < 0.1
        tg[inside] = rng.uniform(BOX[0], BOX[1], (int(inside.sum()), 3))
    else:
        i = np.arange(n)
        want = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "alternate": i % 2 == 0, "runs": (i // RUN) % 2 == 0}[pattern]
        r = np.where(want, rng.uniform(2.0, 100.0, n), np.where(i % 3 == 0, rng.uniform(0.01, 0.2, n), rng.uniform(130.0, 400.0, n)))
        tg = d * r[:, None]
    return _points(_to_input(name, tg), rng), (q, t, MIN_RANGE, MAX_RANGE) + BOX


def prefilter_cases():
    """name -> builder of (points, args)"""
    c = {}
    for e in EXTS:
        c["range_edges-" + e] = lambda e=e: range_edges(e)[:2]
        c["blind_edges-" + e] = lambda e=e: blind_edges(e)[:2]
        for n in LENGTHS + LONG_LENGTHS:
            c["random%d-%s" % (n, e)] = lambda e=e, n=n: random_cloud(e, n)
        for p in PATTERNS:
            c["%s-%s" % (p, e)] = lambda e=e, p=p: random_cloud(e, LONG_LENGTHS[1], p)
    return c


_CACHE = {}


def cached(key, fn):
    """a reference is computed once and shared; nobody writes into it"""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]
