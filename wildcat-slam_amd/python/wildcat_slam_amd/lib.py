"""ctypes binding of libwildcat_hip.so (include/wildcat_hip.h).

There is NO CPU fallback: if the HIP library is missing or no gfx950 device is visible, every compute entry
point raises.  (`load()` alone works without a GPU so that the CPU test-suite can check the exported symbols.)
"""
import contextlib
import ctypes as C
import os
import re
import weakref

import numpy as np

from . import records as R

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "csrc")
_SO = os.path.join(_CSRC, "libwildcat_hip.so")
_INCLUDE = os.path.join(os.path.dirname(os.path.dirname(_CSRC)), "include")
_LIB = None

WC_OK, WC_ERR_CAPACITY = 0, 1
WC_ERR_ARG = 11


class WildcatError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"wildcat_hip error {code}: {msg}")
        self.code = code


def so_path():
    return _SO


def load():
    """Load libwildcat_hip.so; raises if it has not been built (see __graft_entry__.build())."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            raise FileNotFoundError(f"{_SO} not built — run `python -c 'import __graft_entry__ as g; g.build()'`")
        _LIB = C.CDLL(_SO)
        _LIB.wc_version.restype = C.c_char_p
        _LIB.wc_last_error.restype = C.c_char_p
    return _LIB


def declared_symbols():
    """Every function name declared in include/wildcat_hip.h."""
    txt = open(os.path.join(_INCLUDE, "wildcat_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(wc_[a-z0-9_]+)\s*\(", txt)))


def default_params():
    p = R.Params()
    load().wc_params_default(C.byref(p))
    return p


def params_check(params):
    """wc_params_check (host only, no context) -> (return code, name of the first refused field or None)"""
    field = C.c_char_p()
    rc = load().wc_params_check(C.byref(params), C.byref(field))
    return rc, field.value.decode() if field.value else None


def _odom_lib():
    load()
    return C.CDLL(os.path.join(os.path.dirname(_CSRC), "host", "libwildcat_odometry.so"))


def default_config():
    """the default LioConfig's reference fields (records.OdomConfig); needs no GPU"""
    c = R.OdomConfig()
    _odom_lib().wc_host_default_config(C.byref(c))
    return c


def host_params_from_config(config=None):
    """the wc_params the facade derives from a configuration (records.OdomConfig, None = the default), without a context ->
    (Params, wc_params_check's return code)"""
    p = R.Params()
    rc = _odom_lib().wc_host_params_from_config(C.byref(config) if config is not None else None, C.byref(p))
    return p, rc


def rccl_unique_id():
    """128 opaque bytes from ncclGetUniqueId (rank 0 creates them, the launcher distributes them)"""
    buf = C.create_string_buffer(128)
    rc = load().wc_comm_rccl_unique_id(buf)
    if rc != WC_OK:
        raise WildcatError(rc, "wc_comm_rccl_unique_id failed (librccl.so not loadable?)")
    return bytes(buf.raw)


def route_owner(keys_xyz, world):
    """owner rank of every root voxel index (n x 3 int32) - wc_route_owner, needs no GPU"""
    keys_xyz = np.asarray(keys_xyz, np.int64).reshape(-1, 3)
    uniq, inv = np.unique(keys_xyz, axis=0, return_inverse=True)
    f = load().wc_route_owner
    own = np.array([f(int(k[0]), int(k[1]), int(k[2]), int(world)) for k in uniq], np.int32)
    return own[inv.reshape(-1)]


class DeviceBuffer:
    """A block of HBM owned through the C-ABI (wc_dev_alloc / wc_dev_free)."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p(0)
        ctx._ck(ctx.lib.wc_dev_alloc(ctx.h, C.c_size_t(max(self.nbytes, 1)), C.byref(p)))
        self.ptr = p.value
        ctx._bufs.add(self)  # Context.close() frees what is still alive (wc_dev_free needs the live ctx)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.ctx._ck(self.ctx.lib.wc_h2d(self.ctx.h, C.c_void_p(self.ptr), R.ptr(arr), C.c_size_t(arr.nbytes)))
        return self

    def download(self, dtype, count):
        out = np.zeros(count, dtype)
        self.ctx._ck(self.ctx.lib.wc_d2h(self.ctx.h, R.ptr(out), C.c_void_p(self.ptr), C.c_size_t(out.nbytes)))
        return out

    def free(self):
        if self.ptr and self.ctx.h:
            self.ctx.lib.wc_dev_free(self.ctx.h, C.c_void_p(self.ptr))
        self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """wc_ctx wrapper: one GPU, one stream."""

    def __init__(self, device=0, params=None):
        self.lib = load()
        self.params = params or default_params()
        self._bufs = weakref.WeakSet()
        h = C.c_void_p(0)
        rc = self.lib.wc_ctx_create(C.byref(self.params), C.c_int(device), C.byref(h))
        if rc != WC_OK:
            raise WildcatError(rc, "wc_ctx_create failed (no gfx950 device visible?)")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            for b in list(self._bufs):  # buffers outliving the context would leak (wc_dev_free(NULL, p) is an error)
                b.free()
            self.lib.wc_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != WC_OK:
            raise WildcatError(rc, self.lib.wc_last_error(self.h).decode())

    def set_params(self, params):
        """wc_ctx_set_params; parameters that fail wc_params_check raise WildcatError(11) and the context keeps what it had"""
        self._ck(self.lib.wc_ctx_set_params(self.h, C.byref(params)))
        self.params = params

    def get_params(self):
        """a copy of the parameters the context holds (wc_ctx_get_params)"""
        p = R.Params()
        self._ck(self.lib.wc_ctx_get_params(self.h, C.byref(p)))
        return p

    def selftest_factor32(self, a, variant, reps=5):
        """-> (L, L^-1, shader clocks, ok) of the 32 x 32 SPD matrix a by the solve's diagonal-block kernel (wc_selftest_factor32)"""
        a = np.ascontiguousarray(a, np.float64)
        L, X = np.zeros((32, 32)), np.zeros((32, 32))
        clk = (C.c_longlong * 2)()
        self._ck(self.lib.wc_selftest_factor32(self.h, C.c_int(variant), C.c_int(reps), R.ptr(a), R.ptr(L), R.ptr(X), clk))
        return L, X, int(clk[0]), bool(clk[1])

    def selftest_fx_eig3(self, a):
        """-> (ascending eigenvalues, eigenvector of the smallest, closed form accepted) of the symmetric 3 x 3 matrix a by the default
        extraction path's closed-form solver on the device (wc_selftest_fx_eig3)"""
        a = np.ascontiguousarray(a, np.float64).reshape(9)
        out = np.zeros(8)
        self._ck(self.lib.wc_selftest_fx_eig3(self.h, R.ptr(a), R.ptr(out)))
        return out[0:3].copy(), out[3:6].copy(), bool(out[6])

    def set_dev_option(self, name, value):
        """a development option of this context (include/wildcat_hip.h: wc_ctx_set_dev_option)"""
        self._ck(self.lib.wc_ctx_set_dev_option(self.h, name.encode(), C.c_int(int(value))))

    def set_stream(self, stream_ptr):
        self._ck(self.lib.wc_ctx_set_stream(self.h, C.c_void_p(stream_ptr)))

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        return DeviceBuffer(self, arr.nbytes).upload(arr)

    def sync(self):
        self._ck(self.lib.wc_sync(self.h))

    def download_raw(self, d_ptr, nbytes):
        """bytes at a raw device pointer (e.g. the buffer handed to an all-reduce callback) -> uint8 array"""
        out = np.zeros(int(nbytes), np.uint8)
        self._ck(self.lib.wc_d2h(self.h, R.ptr(out), C.c_void_p(d_ptr), C.c_size_t(out.nbytes)))
        return out

    def upload_raw(self, d_ptr, arr):
        arr = np.ascontiguousarray(arr)
        self._ck(self.lib.wc_h2d(self.h, C.c_void_p(d_ptr), R.ptr(arr), C.c_size_t(arr.nbytes)))

    def timer_start(self):
        self._ck(self.lib.wc_timer_start(self.h))

    def timer_stop_ms(self):
        ms = C.c_float(0)
        self._ck(self.lib.wc_timer_stop_ms(self.h, C.byref(ms)))
        return ms.value

    def map_create(self, voxel, reserve_voxels=0, moments=False):
        """a voxel-downsampled point map in HBM (wc_map_create_ex; moments: WC_MAP_MOMENTS, for surfels() and nearest_plane()); close()
        it before the context"""
        return PointMap(self, voxel, reserve_voxels, moments)

    # ---- extraction ---------------------------------------------------------------------------------------------
    def points_desc(self, d_points, n):
        """descriptor for a device-resident array of 48-byte hilti_ros::Point records"""
        return R.Points(d_points.ptr, d_points.ptr + 24, 48, 48, n)

    def voxel_keys(self, points):
        d = self.to_device(points)
        out = self.alloc(12 * len(points))
        desc = self.points_desc(d, len(points))
        self._ck(self.lib.wc_voxel_keys(self.h, C.byref(desc), C.c_void_p(out.ptr)))
        return out.download(np.int32, 3 * len(points)).reshape(-1, 3)

    def extract_enqueue(self, desc, d_out, d_ids, cap, t_lo=1.0, t_hi=0.0):
        self._ck(self.lib.wc_extract_surfels_enqueue(self.h, C.byref(desc), C.c_double(t_lo), C.c_double(t_hi), C.c_void_p(d_out.ptr),
                                                     C.c_void_p(d_ids.ptr if d_ids else 0), C.c_uint64(cap)))

    def extract_finish(self):
        n = C.c_uint64(0)
        self._ck(self.lib.wc_extract_surfels_finish(self.h, C.byref(n)))
        return int(n.value)

    def extract_batch_prepare(self, jobs):
        """jobs: list of (desc, d_out, d_ids or None, cap, t_lo, t_hi) -> (enqueue(), finish() -> [n_surfels per sweep]): K sweeps
        through one launch chain (wc_extract_surfels_batch_*)"""
        K = len(jobs)
        arr = (R.SweepJob * K)()
        for k, (desc, d_out, d_ids, cap, t_lo, t_hi) in enumerate(jobs):
            arr[k].pts, arr[k].t_lo, arr[k].t_hi = desc, t_lo, t_hi
            arr[k].d_out, arr[k].d_ids, arr[k].cap = d_out.ptr, (d_ids.ptr if d_ids else 0), cap
        counts = (C.c_uint64 * K)()
        enq, fin, ck, h = self.lib.wc_extract_surfels_batch_enqueue, self.lib.wc_extract_surfels_batch_finish, self._ck, self.h

        def enqueue():
            ck(enq(h, arr, C.c_int(K)))

        def finish():
            ck(fin(h, counts, C.c_int(K)))
            return [int(c) for c in counts]

        return enqueue, finish

    def prepare_extract(self, desc, d_out, d_ids, cap, t_lo=1.0, t_hi=0.0):
        """the same enqueue / finish pair with the ctypes argument objects built once: a sweep takes ~80 us, building them
        anew for every call is several us of host turn-around.  -> (enqueue(), finish() -> n_surfels)"""
        args = (self.h, C.byref(desc), C.c_double(t_lo), C.c_double(t_hi), C.c_void_p(d_out.ptr), C.c_void_p(d_ids.ptr if d_ids else 0),
                C.c_uint64(cap))
        n = C.c_uint64(0)
        n_ref = C.byref(n)
        f_enq, f_fin, h, ck = self.lib.wc_extract_surfels_enqueue, self.lib.wc_extract_surfels_finish, self.h, self._ck

        def enqueue():
            rc = f_enq(*args)
            if rc:
                ck(rc)

        def finish():
            rc = f_fin(h, n_ref)
            if rc:
                ck(rc)
            return n.value

        return enqueue, finish

    def set_exact_sums(self, exact):
        """extraction arithmetic: False (default) = order-independent integer moments, True = the reference's summation order"""
        self.params.exact_sums = 1 if exact else 0
        self.set_params(self.params)

    def extract_path_info(self):
        """-> dict(fast=the last sweep was completed by the fast path, fallbacks=sweeps handed to the exact path so far, flags=status bits of
        the last default-path sweep (64: it fell back), why=bit i: call site i of fx_fallback() fired in the LAST SWEEP THAT FELL BACK (it keeps its
        value through later sweeps that do not; csrc/extract_fast.inc: 13 a child's PCA near a gate, 14 the root's, 15 a temporal cluster's,
        FxWhy::gap - 7 in k_fx_nodes, 17 in k_fx_walk - a stamp gap within 8 ticks of cluster_gap, the rest capacities),
        long_lists=the last fast sweep had long record lists: the next one merges them first (k_fx_merge),
        runs=pipelines the last sweep enqueued (1: no repeat), path=bits of the pipeline that completed it (1 default path, 2 wide
        keys, 4 run-binned point sort, 8 time-bin surfel order), lds_cap=runs per bucket the run-binned sort takes in LDS)"""
        w = (C.c_uint32 * 64)()
        self._ck(self.lib.wc_debug_status(self.h, w))
        return dict(fast=bool(w[61]), fallbacks=int(w[60]), flags=int(w[62]), why=int(w[63]), long_lists=bool(w[59]),
                    runs=int(w[56]), path=int(w[57]), lds_cap=int(w[58]))

    def extract_profile(self, enable=True):
        """True / 1: HIP events after every kernel group of the stage (each event costs ~5 us of stream time); 2: only the first
        and the last one (extract_stage_ms then reports the whole stage under "point_sort"); False: off"""
        self._ck(self.lib.wc_extract_profile(self.h, C.c_int(int(enable))))

    def extract_stage_ms(self):
        ms = (C.c_float * 5)()
        self._ck(self.lib.wc_extract_stage_ms(self.h, ms))
        return dict(zip(("init", "point_sort", "roots_stream", "roots_emit", "slot_order"), [float(v) for v in ms]))

    def extract_surfels(self, points, hint=True, cap=None):
        """host convenience: upload POINT array, extract, download -> (surfels, ids).  hint: True = the sweep's own time range,
        False = none (the library reads it back), (t_lo, t_hi) = explicit range"""
        n = len(points)
        assert points.dtype.itemsize == 48, "POINT records are 48 bytes (np.concatenate packs the dtype: use synth.concat_points)"
        cap = cap or max(1024, (3 * n) // 20 + 1)
        d_pts = self.to_device(points) if n else self.alloc(48)
        d_out, d_ids = self.alloc(cap * 144), self.alloc(cap * 16)
        desc = self.points_desc(d_pts, n)
        if isinstance(hint, tuple):
            t_lo, t_hi = hint
        elif hint and n:
            t_lo, t_hi = float(points["time"][0]), float(points["time"][-1])
        else:
            t_lo, t_hi = 1.0, 0.0
        self.extract_enqueue(desc, d_out, d_ids, cap, t_lo, t_hi)
        m = self.extract_finish()
        return d_out.download(R.SURFEL, m), d_ids.download(R.SURFEL_ID, m)

    # ---- one cloud over several GPUs (csrc/route.hip) --------------------------------------------------------------------
    def set_comm(self, comm):
        """comm: object with .rank, .world and methods allreduce(ptr, count), alltoallv(send_ptr, send_bytes, recv_ptr, recv_bytes),
        allgatherv(send_ptr, send_bytes, recv_ptr, recv_bytes) on raw device pointers (see dist.py); None removes it"""
        if comm is None:
            self._comm = None
            self._ck(self.lib.wc_ctx_set_comm(self.h, C.c_void_p(0)))
            return
        world = comm.world

        def guard(fn):
            def wrapped(*a):
                try:
                    fn(*a)
                    return 0
                except Exception as e:  # pragma: no cover
                    print("communicator callback failed:", repr(e))
                    return 1

            return wrapped

        ar = R.COMM_ALLREDUCE(guard(lambda user, p, n: comm.allreduce(p, n)))
        a2a = R.COMM_ALLTOALLV(guard(lambda user, s, sb, r, rb: comm.alltoallv(s, [sb[i] for i in range(world)], r, [rb[i] for i in range(world)])))
        ag = R.COMM_ALLGATHERV(guard(lambda user, s, n, r, rb: comm.allgatherv(s, n, r, [rb[i] for i in range(world)])))
        c = R.Comm(None, comm.rank, world, ar, a2a, ag, 0)
        self._comm = (c, ar, a2a, ag, comm)  # keep the trampolines alive
        self._ck(self.lib.wc_ctx_set_comm(self.h, C.byref(c)))

    def comm_rccl_init(self, rank, world, unique_id):
        """the in-library RCCL communicator (csrc/comm.hip); unique_id: the 128 bytes of rccl_unique_id() of rank 0"""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._ck(self.lib.wc_comm_rccl_init(self.h, C.c_int(rank), C.c_int(world), buf))

    def comm_allreduce_probe(self, count, reps=50):
        """microseconds per all-reduce of `count` doubles through the installed communicator (wc_comm_allreduce_probe)"""
        us = C.c_double(0)
        self._ck(self.lib.wc_comm_allreduce_probe(self.h, C.c_uint64(int(count)), C.c_int(int(reps)), C.byref(us)))
        return float(us.value)

    def comm_rccl_destroy(self):
        self._ck(self.lib.wc_comm_rccl_destroy(self.h))

    def route_partition(self, d_points, n, world, desc=None, fill=None):
        """-> (DeviceBuffer of wc_route_point[n], counts[world]).  desc: a wc_points descriptor of the caller's (any strides) instead of
        the 48-byte records of d_points; fill: a byte value the output holds before the call, so that a record the call leaves
        unwritten shows (tests)"""
        d_send = self.alloc(24 * max(n, 1))
        if fill is not None:
            d_send.upload(np.full(24 * max(n, 1), fill, np.uint8))
        counts = (C.c_uint64 * world)()
        if desc is None:
            desc = self.points_desc(d_points, n)
        self._ck(self.lib.wc_route_partition(self.h, C.byref(desc), C.c_int(world), C.c_void_p(d_send.ptr), counts))
        return d_send, np.array(list(counts), np.uint64)

    def route_desc(self, d_route_points, n):
        return R.Points(d_route_points.ptr, d_route_points.ptr + 16, 24, 24, n)

    def extract_surfels_sharded(self, d_points, n, t_lo, t_hi, cap=None, out=None):
        """this rank's slice (device POINT array) -> (surfels, ids, count, points owned) of the voxels this rank owns;
        out = (d_out, d_ids, cap) reuses buffers"""
        if out is not None:
            d_out, d_ids, cap = out
        else:
            cap = cap or max(1024, (3 * n) // 20 + 1) * 4
            d_out, d_ids = self.alloc(cap * 144), self.alloc(cap * 16)
        desc = self.points_desc(d_points, n)
        m, owned = C.c_uint64(0), C.c_uint64(0)
        self._ck(self.lib.wc_extract_surfels_sharded(self.h, C.byref(desc), C.c_double(t_lo), C.c_double(t_hi), C.c_void_p(d_out.ptr),
                                                     C.c_void_p(d_ids.ptr), C.c_uint64(cap), C.byref(m), C.byref(owned)))
        return d_out, d_ids, int(m.value), int(owned.value)

    def merge_surfels(self, lists, id_lists=None, want_ids=True, fill=None):
        """host convenience: k sorted SURFEL arrays (+ ids) -> merged (surfels, ids).  id_lists None: no ids go in (only the stamps
        compare) and none come out; want_ids False: the ids steer the merge and only the surfels are written -> (surfels, None) in both
        cases.  fill: a byte value the outputs hold before the call, so that a record the call leaves unwritten shows (tests)"""
        counts = (C.c_uint64 * len(lists))(*[len(a) for a in lists])
        n = sum(len(a) for a in lists)
        want_ids = want_ids and id_lists is not None
        d_in = self.to_device(np.concatenate(lists))
        d_ids = self.to_device(np.concatenate(id_lists)) if id_lists is not None else None
        d_out, d_oid = self.alloc(144 * max(n, 1)), (self.alloc(16 * max(n, 1)) if want_ids else None)
        if fill is not None:
            for b in (d_out, d_oid):
                if b:
                    b.upload(np.full(b.nbytes, fill, np.uint8))
        self._ck(self.lib.wc_merge_surfels(self.h, C.c_void_p(d_in.ptr), C.c_void_p(d_ids.ptr if d_ids else 0), counts, C.c_int(len(lists)),
                                           C.c_void_p(d_out.ptr), C.c_void_p(d_oid.ptr if d_oid else 0)))
        return d_out.download(R.SURFEL, n), (d_oid.download(R.SURFEL_ID, n) if want_ids else None)

    def gather_surfels_device(self, d_local, d_local_ids, n_local, d_out, d_out_ids, cap, want_rc=False):
        """wc_gather_surfels into caller buffers (device) -> number of surfels of the merged, replicated list.  d_local_ids / d_out_ids
        None: NULL (no ids gathered / none written).  want_rc: -> (return code, *h_n_out) instead of raising - WC_ERR_CAPACITY leaves the
        needed count in *h_n_out"""
        m = C.c_uint64(0)
        rc = self.lib.wc_gather_surfels(self.h, C.c_void_p(d_local.ptr if d_local else 0), C.c_void_p(d_local_ids.ptr if d_local_ids else 0),
                                        C.c_uint64(n_local), C.c_void_p(d_out.ptr if d_out else 0), C.c_void_p(d_out_ids.ptr if d_out_ids else 0),
                                        C.c_uint64(cap), C.byref(m))
        if want_rc:
            return rc, int(m.value)
        self._ck(rc)
        return int(m.value)

    def gather_surfels(self, d_local, d_local_ids, n_local, cap, want_ids=True):
        """-> (surfels, ids) of the merged, replicated list; d_local_ids None or want_ids False: see merge_surfels"""
        want_ids = want_ids and d_local_ids is not None
        d_out, d_oid = self.alloc(144 * max(cap, 1)), (self.alloc(16 * max(cap, 1)) if want_ids else None)
        m = self.gather_surfels_device(d_local, d_local_ids, n_local, d_out, d_oid, cap)
        return d_out.download(R.SURFEL, m), (d_oid.download(R.SURFEL_ID, m) if want_ids else None)

    # ---- sweep preparation (row f-1) -------------------------------------------------------------------------------------
    def prefilter_device(self, d_in, n, ext_quat, ext_t, min_range, max_range, blind_min, blind_max, d_out, cap, prev_time=None, d_kept_times=None):
        """wc_prefilter_points (prev_time None) or wc_prefilter_points_checked on device buffers of the caller -> (return code, *h_n_out,
        monotonic or None).  WC_ERR_CAPACITY is returned, not raised: *h_n_out and the first `cap` records are valid then."""
        m, mono = C.c_uint64(0), C.c_int(1)
        v = lambda a: R.ptr(np.ascontiguousarray(a, np.float64))  # noqa: E731
        head = (self.h, C.c_void_p(d_in.ptr), C.c_uint64(n), v(ext_quat), v(ext_t), C.c_double(min_range), C.c_double(max_range), v(blind_min),
                v(blind_max), C.c_void_p(d_out.ptr), C.c_uint64(cap), C.byref(m))
        if prev_time is None:
            rc = self.lib.wc_prefilter_points(*head)
        else:
            rc = self.lib.wc_prefilter_points_checked(*head, C.c_double(prev_time), C.c_void_p(d_kept_times.ptr if d_kept_times else None),
                                                      C.byref(mono))
        if rc not in (WC_OK, WC_ERR_CAPACITY):
            self._ck(rc)
        return rc, int(m.value), (None if prev_time is None else bool(mono.value))

    def prefilter_points(self, points, ext_quat, ext_t, min_range, max_range, blind_min, blind_max, cap=None):
        """-> survivors.  cap: capacity of the output (default: every point fits); WC_ERR_CAPACITY raises"""
        n = len(points)
        cap = n if cap is None else int(cap)
        d_in, d_out = self.to_device(points), self.alloc(48 * max(cap, 1))
        rc, m, _ = self.prefilter_device(d_in, n, ext_quat, ext_t, min_range, max_range, blind_min, blind_max, d_out, cap)
        self._ck(rc)
        return d_out.download(R.POINT, m)

    def prefilter_points_checked(self, points, ext_quat, ext_t, min_range, max_range, blind_min, blind_max, prev_time=-np.inf, cap=None,
                                 kept_times=True):
        """-> (survivors, their stamps as the library packed them, the reference's CHECK at lidar_odometry.cc:491 held).  cap: capacity of
        both outputs (default: every point fits); kept_times=False passes d_kept_times = NULL and returns None for the stamps"""
        n = len(points)
        cap = n if cap is None else int(cap)
        d_in, d_out = self.to_device(points), self.alloc(48 * max(cap, 1))
        d_t = self.alloc(8 * max(cap, 1)) if kept_times else None
        rc, k, mono = self.prefilter_device(d_in, n, ext_quat, ext_t, min_range, max_range, blind_min, blind_max, d_out, cap, prev_time, d_t)
        self._ck(rc)
        return d_out.download(R.POINT, k), (d_t.download(np.float64, k) if kept_times else None), mono

    def undistort_sweep_packed(self, points, imu, keep_on_device=False):
        """-> (xyz float32 (n, 3), time float64 (n,)): the 20 bytes per point the extraction reads"""
        n = len(points)
        d_in, d_imu = self.to_device(points), self.to_device(imu)
        d_xyz, d_t = self.alloc(12 * max(n, 1)), self.alloc(8 * max(n, 1))
        self._ck(self.lib.wc_undistort_sweep_packed(self.h, C.c_void_p(d_in.ptr), C.c_uint64(n), C.c_void_p(d_imu.ptr), C.c_uint64(len(imu)),
                                                    C.c_void_p(d_xyz.ptr), C.c_void_p(d_t.ptr)))
        if keep_on_device:
            return d_xyz, d_t
        return d_xyz.download(np.float32, 3 * n).reshape(-1, 3), d_t.download(np.float64, n)

    def undistort_sweep(self, points, imu):
        n = len(points)
        d_in, d_out, d_imu = self.to_device(points), self.alloc(48 * max(n, 1)), self.to_device(imu)
        self._ck(self.lib.wc_undistort_sweep(self.h, C.c_void_p(d_in.ptr), C.c_uint64(n), C.c_void_p(d_imu.ptr), C.c_uint64(len(imu)), C.c_void_p(d_out.ptr)))
        return d_out.download(R.POINT, n)

    # ---- pose update / window problem ------------------------------------------------------------------------------
    def update_surfel_poses(self, d_imu, n_imu, d_surf, d_pose, d_in_body, n):
        self._ck(self.lib.wc_update_surfel_poses(self.h, C.c_void_p(d_imu.ptr), C.c_uint64(n_imu), C.c_void_p(d_surf.ptr), C.c_void_p(d_pose.ptr),
                                                 C.c_void_p(d_in_body.ptr), C.c_uint64(n)))

    def reverse_copy_surfels(self, d_src_surf, d_src_pose, n, d_dst_surf, d_dst_pose):
        """dst[j] = src[n - 1 - j] for surfels and poses (wc_reverse_copy_surfels); asynchronous on the context's stream"""
        self._ck(self.lib.wc_reverse_copy_surfels(self.h, C.c_void_p(d_src_surf.ptr), C.c_void_p(d_src_pose.ptr), C.c_uint64(n),
                                                  C.c_void_p(d_dst_surf.ptr), C.c_void_p(d_dst_pose.ptr)))

    def window_build(self, d_surf, d_pose, d_pairs, n_pairs, imu, sample_times, grav, fix_first_pos, d_fix_surf=None, d_fix_pose=None,
                     d_pairs_fix=None, n_pairs_fix=0, sharded=False):
        """imu: host IMU_STATE array (or None); sample_times/grav: host arrays.  sharded: wc_window_build_sharded - a collective of
        the ctx's communicator, every rank passes the SAME replicated arguments and the library takes this rank's share"""
        st = np.ascontiguousarray(sample_times, np.float64)
        gr = np.ascontiguousarray(grav, np.float64)
        self._ns = len(st)
        null = C.c_void_p(0)
        fn = self.lib.wc_window_build_sharded if sharded else self.lib.wc_window_build
        self._ck(fn(
            self.h, C.c_void_p(d_surf.ptr), C.c_void_p(d_pose.ptr), C.c_void_p(d_pairs.ptr) if d_pairs else null, C.c_uint64(n_pairs),
            C.c_void_p(d_fix_surf.ptr) if d_fix_surf else null, C.c_void_p(d_fix_pose.ptr) if d_fix_pose else null,
            C.c_void_p(d_pairs_fix.ptr) if d_pairs_fix else null, C.c_uint64(n_pairs_fix),
            R.ptr(imu) if imu is not None and len(imu) else null, C.c_uint64(len(imu) if imu is not None else 0), R.ptr(st), C.c_uint64(len(st)),
            R.ptr(gr), C.c_int(int(fix_first_pos))))

    def window_reduce_bytes(self):
        """bytes one linearisation's all-reduce carries (0: the problem is not sharded)"""
        self.lib.wc_window_reduce_bytes.restype = C.c_uint64
        return int(self.lib.wc_window_reduce_bytes(self.h))

    def window_counts(self):
        c = (C.c_uint64 * 4)()
        self._ck(self.lib.wc_window_counts(self.h, c))
        return list(c)

    def window_evaluate(self, x, want_residuals=False):
        x = np.ascontiguousarray(x, np.float64)
        cost = C.c_double(0)
        if want_residuals:
            nb, nu, ni, _ = self.window_counts()
            d_res = self.alloc(8 * (nb + nu + 12 * ni))
            self._ck(self.lib.wc_window_evaluate(self.h, R.ptr(x), C.byref(cost), C.c_void_p(d_res.ptr)))
            return cost.value, d_res.download(np.float64, nb + nu + 12 * ni)
        self._ck(self.lib.wc_window_evaluate(self.h, R.ptr(x), C.byref(cost), C.c_void_p(0)))
        return cost.value

    def window_linearize(self, x):
        x = np.ascontiguousarray(x, np.float64)
        n = 12 * self._ns
        d_H, d_g = self.alloc(8 * n * n), self.alloc(8 * n)
        cost = C.c_double(0)
        self._ck(self.lib.wc_window_linearize(self.h, R.ptr(x), C.c_void_p(d_H.ptr), C.c_void_p(d_g.ptr), C.byref(cost)))
        return d_H.download(np.float64, n * n).reshape(n, n), d_g.download(np.float64, n), cost.value

    def window_linearize_only(self, x):
        """linearise without copying H / g out (benchmarks)"""
        x = np.ascontiguousarray(x, np.float64)
        cost = C.c_double(0)
        self._ck(self.lib.wc_window_linearize(self.h, R.ptr(x), C.c_void_p(0), C.c_void_p(0), C.byref(cost)))
        return cost.value

    def window_linearize_timed(self, x, reps=20):
        """device ms of one linearisation: `reps` of them back to back between two HIP events"""
        x = np.ascontiguousarray(x, np.float64)
        ms = C.c_float(0)
        self._ck(self.lib.wc_window_linearize_timed(self.h, R.ptr(x), int(reps), C.byref(ms)))
        return ms.value

    def window_solve(self, x):
        x = np.ascontiguousarray(x, np.float64).copy()
        s = R.SolveSummary()
        first = np.zeros(len(x))
        self._ck(self.lib.wc_window_solve(self.h, R.ptr(x), C.byref(s), R.ptr(first)))
        return x, s, first

    def window_set_allreduce(self, fn):
        """fn(d_ptr: int, count: int) -> None; kept alive on the context"""
        CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64)

        def _tramp(user, ptr, count):
            try:
                fn(ptr, count)
                return 0
            except Exception as e:  # pragma: no cover
                print("allreduce callback failed:", e)
                return 1

        self._cb = CB(_tramp) if fn else C.cast(None, CB)
        self._ck(self.lib.wc_window_set_allreduce(self.h, self._cb, C.c_void_p(0)))

    # ---- correspondence ---------------------------------------------------------------------------------------------
    def match_device(self, d_q_surf, d_q_pose, nq, d_t_surf, d_t_pose, nt, same_set, d_pairs, cap, d_knn_idx=None, d_knn_d2=None, sharded=False):
        """sharded: wc_match_sharded - a collective of the ctx's communicator (every rank, same replicated arguments)"""
        n = C.c_uint64(0)
        if sharded:
            self._ck(self.lib.wc_match_sharded(self.h, C.c_void_p(d_q_surf.ptr), C.c_void_p(d_q_pose.ptr), C.c_uint64(nq), C.c_void_p(d_t_surf.ptr),
                                               C.c_void_p(d_t_pose.ptr), C.c_uint64(nt), C.c_int(1 if same_set else 0), C.c_void_p(d_pairs.ptr),
                                               C.c_uint64(cap), C.byref(n)))
            return int(n.value)
        self._ck(self.lib.wc_match(self.h, C.c_void_p(d_q_surf.ptr), C.c_void_p(d_q_pose.ptr), C.c_uint64(nq), C.c_void_p(d_t_surf.ptr),
                                   C.c_void_p(d_t_pose.ptr), C.c_uint64(nt), C.c_int(1 if same_set else 0), C.c_void_p(d_pairs.ptr), C.c_uint64(cap),
                                   C.byref(n), C.c_void_p(d_knn_idx.ptr if d_knn_idx else 0), C.c_void_p(d_knn_d2.ptr if d_knn_d2 else 0)))
        return int(n.value)

    def match_stats(self):
        """what the last wc_match on this context touched, per sampled query (wc_match_stats)"""
        out = (C.c_double * 8)()
        self._ck(self.lib.wc_match_stats(self.h, out))
        n = max(out[4], 1.0)
        return {"nodes_per_query": out[0] / n, "leaves_per_query": out[1] / n, "points_per_query": out[2] / n, "exact_per_query": out[3] / n,
                "sampled_queries": int(out[4]), "tree_depth": int(out[5]), "top_levels": int(out[6]), "targets": int(out[7])}

    def match_pair_device(self, d_sld_surf, d_sld_pose, n_sld, d_fix_surf, d_fix_pose, n_fix, d_pairs_sld, cap_sld, d_pairs_fix, cap_fix, sharded=False):
        """both searches of an outer iteration side by side (wc_match_pair; sharded: wc_match_pair_sharded, a collective)
        -> (n_pairs_sld, n_pairs_fix)"""
        nb, nu = C.c_uint64(0), C.c_uint64(0)
        fn = self.lib.wc_match_pair_sharded if sharded else self.lib.wc_match_pair
        self._ck(fn(self.h, C.c_void_p(d_sld_surf.ptr), C.c_void_p(d_sld_pose.ptr), C.c_uint64(n_sld), C.c_void_p(d_fix_surf.ptr),
                                        C.c_void_p(d_fix_pose.ptr), C.c_uint64(n_fix), C.c_void_p(d_pairs_sld.ptr), C.c_uint64(cap_sld), C.byref(nb),
                                        C.c_void_p(d_pairs_fix.ptr), C.c_uint64(cap_fix), C.byref(nu)))
        return int(nb.value), int(nu.value)

    def match(self, q_surf, q_pose, t_surf, t_pose, same_set, want_knn=False, sharded=False):
        """host convenience -> pairs[PAIR] (and the raw k-NN table if want_knn)"""
        nq, nt = len(q_surf), len(t_surf)
        dq, dqp = self.to_device(q_surf), self.to_device(q_pose)
        if same_set:
            dt, dtp = dq, dqp
        else:
            dt, dtp = self.to_device(t_surf), self.to_device(t_pose)
        d_pairs = self.alloc(8 * max(nq, 1))
        k = self.params.knn_k
        d_idx = self.alloc(4 * max(nq, 1) * k) if want_knn else None
        d_d2 = self.alloc(8 * max(nq, 1) * k) if want_knn else None
        n = self.match_device(dq, dqp, nq, dt, dtp, nt, same_set, d_pairs, nq, d_idx, d_d2, sharded=sharded)
        pairs = d_pairs.download(R.PAIR, n)
        if want_knn:
            return pairs, d_idx.download(np.uint32, nq * k).reshape(nq, k), d_d2.download(np.float64, nq * k).reshape(nq, k)
        return pairs


def map_reg_params(max_dist, min_points=3, sigma0=0.05 / 6, cauchy_a=0.0):
    """wc_map_reg_params (sigma0: wc_params.surfel_sigma0's default; cauchy_a = 0: no loss, the window's is 0.4)"""
    return R.MapRegParams(float(max_dist), int(min_points), 0, float(sigma0), float(cauchy_a))


def map_align_opts(params, max_iterations=20, tol_rot=1e-6, tol_trans=1e-6, min_used=6, min_pivot=1e-9):
    """wc_map_align_opts around a wc_map_reg_params (min_pivot: a design choice, include/wildcat_hip.h: wc_map_align)"""
    return R.MapAlignOpts(params, int(max_iterations), int(min_used), float(tol_rot), float(tol_trans), float(min_pivot))


def map_carve_params(max_range, min_range=0.0, shell=1, min_rays=1, max_steps=4096):
    """wc_map_carve_params"""
    return R.MapCarveParams(float(min_range), float(max_range), int(shell), int(min_rays), int(max_steps), 0)


def _carve_dict(r):
    return {k: int(getattr(r, k)) for k in ("rays_used", "rays_skipped", "steps", "voxels_removed", "points_removed")}


def map_raycast_params(max_range, min_range=0.0, first_step=0, end_shell=0, min_points=1, max_steps=4096):
    """wc_map_raycast_params"""
    return R.MapRaycastParams(float(min_range), float(max_range), int(first_step), int(end_shell), int(min_points), int(max_steps))


def _raycast_dict(r):
    return {k: int(getattr(r, k)) for k in ("rays_cast", "rays_skipped", "hits", "tested")}


def _pose12(T):
    T = np.ascontiguousarray(np.asarray(T, np.float64).reshape(-1)[:12])
    assert T.size == 12, "T: 3 x 4 (or 4 x 4) row-major"
    return T.copy()


def _summary_dict(s):
    return dict(initial_cost=s.initial_cost, final_cost=s.final_cost, iterations=s.iterations, termination=s.termination, n_used=int(s.n_used),
                n_found=int(s.n_found), last_step=np.array(list(s.last_step)))


def map_pyramid_opts(levels, params=None, **kw):
    """one wc_map_align_opts per map of `levels`: `params` (a wc_map_reg_params; default map_reg_params' own) with max_dist = the
    level's voxel size, and map_align_opts' keywords -> list in the order of `levels`"""
    p = params if params is not None else map_reg_params(1.0)
    return [map_align_opts(map_reg_params(m.voxel, p.min_points, p.sigma0, p.cauchy_a), **kw) for m in levels]


def map_align_pyramid_device(levels, desc, T, opts_list):
    """wc_map_align_pyramid on points already in HBM: levels[0] runs first (the coarsest first), level l with opts_list[l] from the pose
    level l - 1 left -> (T (3, 4), [summary dict per level])"""
    n = len(levels)
    assert n >= 1 and len(opts_list) == n, "one wc_map_align_opts per level"
    ctx = levels[0].ctx
    T = _pose12(T)
    handles = (C.c_void_p * n)(*[m.h.value for m in levels])
    opts, summ = (R.MapAlignOpts * n)(*opts_list), (R.MapAlignSummary * n)()
    ctx._ck(ctx.lib.wc_map_align_pyramid(ctx.h, handles, C.c_uint32(n), C.byref(desc), R.ptr(T), opts, summ))
    return T.reshape(3, 4), [_summary_dict(s) for s in summ]


def map_align_pyramid(levels, points, T, opts_list=None, params=None, **kw):
    """coarse-to-fine registration of POINT records or an (n, 3) float32 array against the maps of `levels`, coarsest first (pass
    PointMap.pyramid()'s list reversed), from the pose T -> (T (3, 4), [summary dict per level]); opts_list: one wc_map_align_opts per
    level, or map_pyramid_opts(levels, params, **kw)"""
    if opts_list is None:
        opts_list = map_pyramid_opts(levels, params, **kw)
    with levels[0]._uploaded(points) as (desc, _):
        return map_align_pyramid_device(levels, desc, T, opts_list)


def _poses12(Ts):
    """K poses, each 3 x 4 (or 4 x 4) row-major -> (K, 12) float64, a fresh contiguous array"""
    Ts = np.asarray(Ts, np.float64)
    K = len(Ts)
    Ts = Ts.reshape(K, -1)[:, :12] if K else np.zeros((0, 12))
    assert Ts.shape == (K, 12), "Ts: K poses, each 3 x 4 (or 4 x 4) row-major"
    return np.ascontiguousarray(Ts).copy()


def map_align_pyramid_batch_device(levels, desc, Ts, opts_list):
    """wc_map_align_pyramid_batch on points already in HBM: K starts Ts through the maps of `levels` (coarsest first), level l with
    opts_list[l] -> (Ts (K, 3, 4), [[summary dict per hypothesis] per level], status (K,) int32: 0, or the error code of a hypothesis
    that was dropped on the way - its later summaries are zero)"""
    n = len(levels)
    assert n >= 1 and len(opts_list) == n, "one wc_map_align_opts per level"
    ctx = levels[0].ctx
    Ts = _poses12(Ts)
    K = len(Ts)
    handles = (C.c_void_p * n)(*[m.h.value for m in levels])
    opts, summ, status = (R.MapAlignOpts * n)(*opts_list), (R.MapAlignSummary * max(n * K, 1))(), np.zeros(K, np.int32)
    ctx._ck(ctx.lib.wc_map_align_pyramid_batch(ctx.h, handles, C.c_uint32(n), C.byref(desc), R.ptr(Ts), C.c_uint32(K), opts, summ, R.ptr(status)))
    return Ts.reshape(K, 3, 4), [[_summary_dict(summ[l * K + h]) for h in range(K)] for l in range(n)], status


def map_align_pyramid_batch(levels, points, Ts, opts_list=None, params=None, **kw):
    """map_align_pyramid for K starts in one pass: POINT records or an (n, 3) float32 array against the maps of `levels`, coarsest first
    -> as map_align_pyramid_batch_device; opts_list: one wc_map_align_opts per level, or map_pyramid_opts(levels, params, **kw)"""
    if opts_list is None:
        opts_list = map_pyramid_opts(levels, params, **kw)
    with levels[0]._uploaded(points) as (desc, _):
        return map_align_pyramid_batch_device(levels, desc, Ts, opts_list)


def map_align_best(summaries, status, min_used):
    """wc_map_align_best (needs no GPU): the winner among K summaries (dicts with termination, n_used, final_cost) with their statuses
    -> its index, or -1 when no hypothesis is eligible.  Most inliers first, then the lower cost, then the lower index"""
    K = len(summaries)
    summ, best = (R.MapAlignSummary * max(K, 1))(), C.c_int32(0)
    for h, d in enumerate(summaries):
        summ[h].termination, summ[h].n_used, summ[h].final_cost = int(d["termination"]), int(d["n_used"]), float(d["final_cost"])
    status = np.ascontiguousarray(status, np.int32).reshape(-1)
    assert len(status) == K
    rc = load().wc_map_align_best(summ, R.ptr(status) if K else None, C.c_uint32(K), C.c_uint64(int(min_used)), C.byref(best))
    if rc != WC_OK:
        raise WildcatError(rc, "wc_map_align_best refused its arguments")
    return int(best.value)


def pose_yaw_grid(T, K):
    """wc_pose_yaw_grid (needs no GPU): K starts (Rz(2 pi k / K) R | t) of the pose T = (R | t) -> (K, 3, 4); entry 0 is T itself"""
    T, K = _pose12(T), int(K)
    out = np.zeros((K, 12))
    rc = load().wc_pose_yaw_grid(R.ptr(T), C.c_uint32(K), R.ptr(out) if K else None)
    if rc != WC_OK:
        raise WildcatError(rc, "wc_pose_yaw_grid refused its arguments")
    return out.reshape(K, 3, 4)


def pose_grid(T, n_yaw, n_xyz, step):
    """wc_pose_grid (needs no GPU): n_yaw headings x n_xyz[0] x n_xyz[1] x n_xyz[2] positions spaced by step around the pose T, centred
    on its translation in world axes -> (K, 3, 4), pose ((k n0 + i0) n1 + i1) n2 + i2; the rotations are pose_yaw_grid's"""
    T = _pose12(T)
    n = np.ascontiguousarray(n_xyz, np.uint32).reshape(-1)
    step = np.ascontiguousarray(step, np.float64).reshape(-1)
    assert n.size == 3 and step.size == 3, "n_xyz and step: three entries each"
    K = int(n_yaw) * int(n[0]) * int(n[1]) * int(n[2])
    if not 1 <= K <= 2**20:
        raise WildcatError(11, "wc_pose_grid: between 1 and 2^20 poses")
    out = np.zeros((K, 12))
    rc = load().wc_pose_grid(R.ptr(T), C.c_uint32(int(n_yaw)), R.ptr(n), R.ptr(step), R.ptr(out))
    if rc != WC_OK:
        raise WildcatError(rc, "wc_pose_grid refused its arguments")
    return out.reshape(K, 3, 4)


def map_ct_align_opts(params, max_iterations=20, tol_rot=1e-6, tol_trans=1e-6, min_used=12, min_pivot=1e-9, prior=(0.0, 0.0, 0.0, 0.0)):
    """wc_map_ct_align_opts around a wc_map_reg_params; prior: the four information weights (begin rotation, begin translation, end
    rotation, end translation)"""
    return R.MapCtAlignOpts(params, int(max_iterations), int(min_used), float(tol_rot), float(tol_trans), float(min_pivot),
                            (C.c_double * 4)(*[float(w) for w in prior]))


def _pose_rec(pose):
    """(pos (3,), quat (4,) = (w, x, y, z)) or seven numbers -> wc_pose"""
    p = np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in pose]) if len(pose) == 2 else np.asarray(pose, np.float64).reshape(-1)
    assert p.size == 7, "a pose: pos (3) and quat (4) = (w, x, y, z)"
    return R.Pose((C.c_double * 3)(*p[:3]), (C.c_double * 4)(*p[3:]))


def _pose_pair(rec):
    return np.array(list(rec.pos)), np.array(list(rec.quat))


def _ct_summary_dict(s):
    return dict(initial_cost=s.initial_cost, final_cost=s.final_cost, iterations=s.iterations, termination=s.termination, n_used=int(s.n_used),
                n_found=int(s.n_found), n_outside=int(s.n_outside), last_step=np.array(list(s.last_step)), prior_cost=s.prior_cost)


def pose_interp_move(pose_begin, pose_end, t_begin, t_end, xyz, times):
    """wc_pose_interp_move (needs no GPU): the device's interpolation and move of wc_map_linearize_ct on the host -> (n, 3) float32, NaN
    rows for the stamps outside [t_begin, t_end]"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    times = np.ascontiguousarray(times, np.float64).reshape(-1)
    assert len(times) == len(xyz)
    out = np.zeros((len(xyz), 3), np.float32)
    b, e = _pose_rec(pose_begin), _pose_rec(pose_end)
    rc = load().wc_pose_interp_move(C.byref(b), C.byref(e), C.c_double(t_begin), C.c_double(t_end), R.ptr(xyz), R.ptr(times), C.c_uint64(len(xyz)),
                                    R.ptr(out))
    if rc != WC_OK:
        raise WildcatError(rc, "wc_pose_interp_move refused its arguments")
    return out


def map_ct_step(ne, prior=(0.0, 0.0, 0.0, 0.0), acc=None, min_pivot=1e-9):
    """wc_map_ct_step (needs no GPU): the 12 x 12 Gauss-Newton step of a MAP_CT_NORMAL_EQ record with the prior weights and the running
    sum of steps acc -> xi (12,), or None when a pivot falls below min_pivot"""
    ne = np.ascontiguousarray(ne, R.MAP_CT_NORMAL_EQ).reshape(1)
    prior = np.ascontiguousarray(prior, np.float64).reshape(4)
    acc = np.zeros(12) if acc is None else np.ascontiguousarray(acc, np.float64).reshape(12)
    xi = np.zeros(12)
    rc = load().wc_map_ct_step(R.ptr(ne), R.ptr(prior), R.ptr(acc), C.c_double(min_pivot), R.ptr(xi))
    if rc == 13:  # WC_ERR_NUMERIC
        return None
    if rc != WC_OK:
        raise WildcatError(rc, "wc_map_ct_step refused its arguments")
    return xi


def map_move_state(vox, mom, voxel, T):
    """wc_map_move_state (needs no GPU): the records of a state (MAP_VOXEL array; mom: (n, 9) int64 or None) of a map of voxel size
    `voxel`, each moved by the rigid T (3 x 4) as wc_map_merge_moved moves it -> (vox, mom or None, records rejected); a rejected
    record is all zeros"""
    vox = np.ascontiguousarray(vox, R.MAP_VOXEL).reshape(-1)
    n = len(vox)
    if mom is not None:
        mom = np.ascontiguousarray(mom, np.int64).reshape(-1, 9)
        assert len(mom) == n, "one row of nine moment words per record"
    out = np.zeros(n, R.MAP_VOXEL)
    out_mom = None if mom is None else np.zeros((n, 9), np.int64)
    if n == 0:  # (nothing to move; the call itself still checks voxel and T)
        vox, mom = np.zeros(1, R.MAP_VOXEL), (None if mom is None else np.zeros((1, 9), np.int64))
    o, om = (out, out_mom) if n else (np.zeros(1, R.MAP_VOXEL), None if mom is None else np.zeros((1, 9), np.int64))
    T12 = None if T is None else _pose12(T)
    rej = C.c_uint64(0)
    rc = load().wc_map_move_state(R.ptr(vox), None if mom is None else R.ptr(mom), C.c_uint64(n), C.c_double(voxel),
                                  None if T12 is None else R.ptr(T12), R.ptr(o), None if om is None else R.ptr(om), C.byref(rej))
    if rc != WC_OK:
        raise WildcatError(rc, "wc_map_move_state refused its arguments")
    return out, out_mom, int(rej.value)


def map_score_top(scores, M, min_hit=0):
    """wc_map_score_top (needs no GPU): the indices of the M best MAP_SCORE records - n_bad == 0 and n_hit >= min_hit; larger n_hit
    first, then the smaller index -> int32 array of the min(M, eligible) indices"""
    scores = np.ascontiguousarray(scores, R.MAP_SCORE).reshape(-1)
    K, M = len(scores), int(M)
    idx, cnt = np.full(max(M, 1), -1, np.int32), C.c_uint32(0)
    rc = load().wc_map_score_top(R.ptr(scores) if K else None, C.c_uint32(K), C.c_uint32(M), C.c_uint32(int(min_hit)), R.ptr(idx), C.byref(cnt))
    if rc != WC_OK:
        raise WildcatError(rc, "wc_map_score_top refused its arguments")
    return idx[: cnt.value].copy()


def map_cc_params(connectivity=26, min_points=1, drop_sparse=False, reserved=0):
    """a wc_map_cc_params record (PointMap.components, .remove_small, map_label_keys)"""
    return R.MapCcParams(int(connectivity), int(min_points), R.MAP_CC_DROP_SPARSE if drop_sparse else 0, int(reserved))


_CC_OUT = ("voxels", "nodes", "components", "largest")


def map_label_keys(keys, counts, connectivity=26, min_points=1, cap_comps=None, params=None):
    """wc_map_label_keys (needs no GPU): the connected components of an exported map - keys (n, 3) int32 strictly ascending, counts (n,)
    uint32, as PointMap.export() returns them -> (labels (n,) uint32, MAP_COMPONENT array, dict(voxels, nodes, components, largest)).
    cap_comps (tests): the records' capacity; when it is too small a WildcatError with code WC_ERR_CAPACITY carries the dict as .out"""
    keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
    counts = np.ascontiguousarray(counts, np.uint32).reshape(-1)
    assert len(counts) == len(keys), "one count per key"
    n = len(keys)
    p = params if params is not None else map_cc_params(connectivity, min_points)
    labels = np.zeros(max(n, 1), np.uint32)
    comps = np.zeros(max(n if cap_comps is None else int(cap_comps), 1), R.MAP_COMPONENT)
    out = (C.c_uint64 * 4)()
    rc = load().wc_map_label_keys(R.ptr(keys) if n else None, R.ptr(counts) if n else None, C.c_uint64(n), C.byref(p), R.ptr(labels), R.ptr(comps),
                                  C.c_uint64(n if cap_comps is None else int(cap_comps)), out)
    res = dict(zip(_CC_OUT, [int(x) for x in out]))
    if rc != WC_OK:
        e = WildcatError(rc, "wc_map_label_keys: " + ("capacity" if rc == WC_ERR_CAPACITY else "refused its arguments"))
        e.out = res if rc == WC_ERR_CAPACITY else None
        raise e
    return labels[:n].copy(), comps[: res["components"]].copy(), res


class PointMap:
    """wc_map: the device-resident voxel-downsampled map (DownSamplingVoxel, surfel_extraction.cc:228-261, over every insert)"""

    def __init__(self, ctx, voxel, reserve_voxels=0, moments=False):
        self.ctx, self.lib, self.voxel, self.moments = ctx, ctx.lib, float(voxel), bool(moments)
        h = C.c_void_p(0)
        flags = C.c_uint32(R.MAP_MOMENTS if moments else 0)
        ctx._ck(self.lib.wc_map_create_ex(ctx.h, C.c_double(voxel), C.c_uint64(int(reserve_voxels)), flags, C.byref(h)))
        self.h = h

    def insert_device(self, desc):
        """points already in HBM (a wc_points descriptor) -> points of this call not inserted (non-finite / out of range)"""
        rej = C.c_uint64(0)
        self.ctx._ck(self.lib.wc_map_insert(self.ctx.h, self.h, C.byref(desc), C.byref(rej)))
        return int(rej.value)

    @contextlib.contextmanager
    def _uploaded(self, points, out_dtype=None):
        """POINT records or an (n, 3) float32 array in HBM for the length of a with block -> (its wc_points descriptor, a device buffer
        for one out_dtype record per point, or None); both are freed on the way out"""
        points = np.ascontiguousarray(points)
        if points.dtype == R.POINT:
            stride = 48
        else:
            points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
            stride = 12
        n = len(points)
        d = self.ctx.to_device(points) if n else None
        d_out = self.ctx.alloc(out_dtype.itemsize * max(n, 1)) if out_dtype is not None else None
        try:
            yield R.Points(d.ptr if d else 0, 0, stride, 0, n), d_out
        finally:
            for b in (d_out, d):
                if b:
                    b.free()

    def insert(self, points):
        """POINT records or an (n, 3) float32 array (uploaded for the call) -> points not inserted"""
        with self._uploaded(points) as (desc, _):
            return self.insert_device(desc)

    def nearest_device(self, desc, max_dist, d_hits, want_count=True):
        """queries already in HBM (a wc_points descriptor) -> MAP_HIT records in d_hits (wc_map_nearest); returns the number found, or
        None without waiting when want_count is False"""
        n = C.c_uint64(0)
        self.ctx._ck(self.lib.wc_map_nearest(self.ctx.h, self.h, C.byref(desc), C.c_double(max_dist), C.c_void_p(d_hits.ptr if d_hits else 0),
                                             C.byref(n) if want_count else None))
        return int(n.value) if want_count else None

    def nearest(self, queries, max_dist=np.inf):
        """POINT records or an (n, 3) float32 array (uploaded for the call) -> MAP_HIT array: per query the nearest centroid among the
        27 voxels around it, within max_dist (count = 0: none)"""
        with self._uploaded(queries, R.MAP_HIT) as (desc, d_hits):
            self.nearest_device(desc, max_dist, d_hits)
            return d_hits.download(R.MAP_HIT, desc.n)

    def knn_device(self, desc, params, d_hits, d_within=None, want_counts=True):
        """queries already in HBM (a wc_points descriptor) -> params.k MAP_HIT records per query in d_hits and, if given, one uint32 per
        query in d_within (wc_map_knn, params: R.MapKnnParams); returns (queries with a neighbour, records written, sum of within), or
        None without waiting when want_counts is False"""
        out = (C.c_uint64 * 3)()
        self.ctx._ck(self.lib.wc_map_knn(self.ctx.h, self.h, C.byref(desc), C.byref(params), C.c_void_p(d_hits.ptr if d_hits else 0),
                                         C.c_void_p(d_within.ptr if d_within else 0), out if want_counts else None))
        return tuple(int(x) for x in out) if want_counts else None

    def knn(self, queries, k, max_dist=np.inf, reach=1, min_points=1, not_own=False):
        """POINT records or an (n, 3) float32 array (uploaded for the call) -> (hits (n, k) MAP_HIT, within (n,) uint32): per query the
        centroids of the voxels around it - 27 with reach 1, 125 with reach 2 - that hold min_points points and lie within max_dist,
        nearest first, ties by voxel index; the records past the last one found are misses (count = 0).  within is the number of such
        voxels, not capped by k.  not_own leaves the query's own voxel out"""
        params = R.MapKnnParams(float(max_dist), int(k), int(reach), int(min_points), R.MAP_KNN_NOT_OWN if not_own else 0)
        with self._uploaded(queries) as (desc, _):
            d_hits = self.ctx.alloc(R.MAP_HIT.itemsize * max(desc.n * max(int(k), 1), 1))
            d_within = self.ctx.alloc(4 * max(desc.n, 1))
            try:
                self.knn_device(desc, params, d_hits, d_within, want_counts=False)
                return d_hits.download(R.MAP_HIT, desc.n * int(k)).reshape(desc.n, int(k)), d_within.download(np.uint32, desc.n)
            finally:
                d_hits.free()
                d_within.free()

    def crop(self, lo, hi):
        """keeps the voxels that intersect the box [lo, hi] (+-inf allowed) and compacts the table (wc_map_crop) -> voxels removed"""
        lo, hi = (C.c_double * 3)(*[float(x) for x in lo]), (C.c_double * 3)(*[float(x) for x in hi])
        n = C.c_uint64(0)
        self.ctx._ck(self.lib.wc_map_crop(self.ctx.h, self.h, lo, hi, C.byref(n)))
        return int(n.value)

    def carve_device(self, desc, origin, params):
        """points already in HBM (a wc_points descriptor) as the ends of rays from origin (wc_map_carve) -> the result as a dict"""
        o = (C.c_double * 3)(*[float(x) for x in origin])
        res = R.MapCarveResult()
        self.ctx._ck(self.lib.wc_map_carve(self.ctx.h, self.h, C.byref(desc), o, C.byref(params), C.byref(res)))
        return _carve_dict(res)

    def carve(self, points, origin, max_range, min_range=0.0, shell=1, min_rays=1, max_steps=4096):
        """POINT records or an (n, 3) float32 array (uploaded for the call): the voxels that at least min_rays of the rays origin -> point
        pass through, farther than `shell` voxels from the ray's end, and in which no point of the call lies, are selected and counted
        (wc_map_carve; it does not remove them: carve_remove() does) -> dict(rays_used, rays_skipped, steps, voxels_removed, points_removed)"""
        with self._uploaded(points) as (desc, _):
            return self.carve_device(desc, origin, map_carve_params(max_range, min_range, shell, min_rays, max_steps))

    def carve_remove_device(self, desc, origin, params):
        """carve_device() that also removes what it selects, in place (wc_map_carve_remove) -> what carve_device() would have returned"""
        o = (C.c_double * 3)(*[float(x) for x in origin])
        res = R.MapCarveResult()
        self.ctx._ck(self.lib.wc_map_carve_remove(self.ctx.h, self.h, C.byref(desc), o, C.byref(params), C.byref(res)))
        return _carve_dict(res)

    def carve_remove(self, points, origin, max_range, min_range=0.0, shell=1, min_rays=1, max_steps=4096):
        """carve() that also removes the voxels it selects: their slots keep a tombstone until the table is next replaced
        (wc_map_carve_remove) -> the dict carve() would have returned on the same map"""
        with self._uploaded(points) as (desc, _):
            return self.carve_remove_device(desc, origin, map_carve_params(max_range, min_range, shell, min_rays, max_steps))

    def remove_device(self, d_keys, n):
        """n voxel indices ((n, 3) int32) already in HBM (wc_map_remove_keys) -> dict(voxels_removed, points_removed, keys_unused)"""
        out = (C.c_uint64 * 3)()
        self.ctx._ck(self.lib.wc_map_remove_keys(self.ctx.h, self.h, C.c_void_p(d_keys.ptr if d_keys else 0), C.c_uint64(int(n)), out))
        return dict(zip(("voxels_removed", "points_removed", "keys_unused"), [int(x) for x in out]))

    def remove(self, keys):
        """the voxels with these indices ((n, 3) int32, any order, uploaded for the call) removed in place -> dict(voxels_removed,
        points_removed, keys_unused: keys that are absent, out of the key range, or second and later copies of a key)"""
        keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
        d = self.ctx.to_device(keys) if len(keys) else None
        try:
            return self.remove_device(d, len(keys))
        finally:
            if d:
                d.free()

    def tombstones(self):
        """-> (tombstones in the table now, purges so far) (wc_map_tombstones; host state, no wait)"""
        out = (C.c_uint64 * 2)()
        self.ctx._ck(self.lib.wc_map_tombstones(self.ctx.h, self.h, out))
        return int(out[0]), int(out[1])

    def components_device(self, params, d_keys, d_label, cap, d_comps, cap_comps):
        """labels (and voxel indices, component records: either may be None) into HBM (wc_map_components) -> (return code,
        dict(voxels, nodes, components, largest)): WC_ERR_CAPACITY leaves the needed counts in the dict"""
        out = (C.c_uint64 * 4)()
        rc = self.lib.wc_map_components(self.ctx.h, self.h, C.byref(params), C.c_void_p(d_keys.ptr if d_keys else 0),
                                        C.c_void_p(d_label.ptr if d_label else 0), C.c_uint64(int(cap)), C.c_void_p(d_comps.ptr if d_comps else 0),
                                        C.c_uint64(int(cap_comps)), out)
        return rc, dict(zip(_CC_OUT, [int(x) for x in out]))

    def components(self, connectivity=26, min_points=1):
        """the connected components of the occupied voxels with at least min_points points under 6 / 18 / 26 connectivity -> (keys (n, 3)
        int32 in export()'s order, labels (n,) uint32 - MAP_NO_COMPONENT for a voxel below min_points -, MAP_COMPONENT array in ascending
        order of the components' smallest key, dict(voxels, nodes, components, largest))"""
        p = map_cc_params(connectivity, min_points)
        rc, res = self.components_device(p, None, None, 0, None, 0)
        n, nc = res["voxels"], res["components"]
        if n == 0:
            self.ctx._ck(rc)
            return np.zeros((0, 3), np.int32), np.zeros(0, np.uint32), np.zeros(0, R.MAP_COMPONENT), res
        if rc not in (WC_OK, WC_ERR_CAPACITY):
            self.ctx._ck(rc)
        bk, bl, bc = self.ctx.alloc(12 * n), self.ctx.alloc(4 * n), self.ctx.alloc(R.MAP_COMPONENT.itemsize * max(nc, 1))
        try:
            rc, res = self.components_device(p, bk, bl, n, bc, nc)
            self.ctx._ck(rc)
            return (bk.download(np.int32, 3 * n).reshape(-1, 3), bl.download(np.uint32, n), bc.download(R.MAP_COMPONENT, res["components"]), res)
        finally:
            for b in (bk, bl, bc):
                b.free()

    def remove_small(self, min_voxels, min_comp_points=0, connectivity=26, min_points=1, drop_sparse=False):
        """removes in place every component with fewer than min_voxels voxels or fewer than min_comp_points points (0: that test is off);
        drop_sparse: the voxels below min_points too (wc_map_remove_small) -> dict(components, components_removed, voxels_removed,
        points_removed)"""
        p = map_cc_params(connectivity, min_points, drop_sparse)
        out = (C.c_uint64 * 4)()
        self.ctx._ck(self.lib.wc_map_remove_small(self.ctx.h, self.h, C.byref(p), C.c_uint32(int(min_voxels)), C.c_uint64(int(min_comp_points)), out))
        return dict(zip(("components", "components_removed", "voxels_removed", "points_removed"), [int(x) for x in out]))

    def raycast_device(self, desc, origin, params, d_hits, want_result=True):
        """points already in HBM (a wc_points descriptor) as the ends of rays from origin -> MAP_RAY_HIT records in d_hits
        (wc_map_raycast); returns the counters as a dict, or None without waiting when want_result is False"""
        o = (C.c_double * 3)(*[float(x) for x in origin])
        res = R.MapRaycastResult()
        self.ctx._ck(self.lib.wc_map_raycast(self.ctx.h, self.h, C.byref(desc), o, C.byref(params), C.c_void_p(d_hits.ptr if d_hits else 0),
                                             C.byref(res) if want_result else None))
        return _raycast_dict(res) if want_result else None

    def raycast(self, points, origin, max_range, min_range=0.0, first_step=0, end_shell=0, min_points=1, max_steps=4096):
        """POINT records or an (n, 3) float32 array (uploaded for the call) as the ends of rays from origin -> (MAP_RAY_HIT array: per
        ray the first voxel with at least min_points points among the tested positions of its walk - those from first_step on and at
        least end_shell voxels from the ray's end -, count = 0: none; dict(rays_cast, rays_skipped, hits, tested))"""
        with self._uploaded(points, R.MAP_RAY_HIT) as (desc, d_hits):
            res = self.raycast_device(desc, origin, map_raycast_params(max_range, min_range, first_step, end_shell, min_points, max_steps), d_hits)
            return d_hits.download(R.MAP_RAY_HIT, desc.n), res

    def raycast_dirs(self, origin, dirs, reach, **kw):
        """cast in a direction up to a reach: raycast() of the end points origin + reach * dir (reach: one number or one per row of dirs),
        formed in float64 on the host and cast to float32.  It is the END POINT that defines the ray - its voxel, its walk and the scale of
        t (range = t * |end - origin|) are those of the rounded float32 end, not of the direction.  max_range defaults to +inf"""
        o = np.asarray(origin, np.float64).reshape(3)
        d = np.asarray(dirs, np.float64).reshape(-1, 3)
        ends = (o + np.asarray(reach, np.float64).reshape(-1, 1) * d).astype(np.float32)
        kw.setdefault("max_range", np.inf)
        return self.raycast(ends, o, **kw)

    def size(self):
        """-> (voxels, points inserted)"""
        v, p = C.c_uint64(0), C.c_uint64(0)
        self.ctx._ck(self.lib.wc_map_size(self.ctx.h, self.h, C.byref(v), C.byref(p)))
        return int(v.value), int(p.value)

    def info(self):
        """-> dict(slots, growths, rejected, bytes)"""
        out = (C.c_uint64 * 4)()
        self.ctx._ck(self.lib.wc_map_info(self.ctx.h, self.h, out))
        return dict(zip(("slots", "growths", "rejected", "bytes"), [int(x) for x in out]))

    def export_device(self, d_xyz, d_count, d_keys, cap):
        """-> (return code, n): WC_ERR_CAPACITY leaves the needed count in n"""
        n = C.c_uint64(0)
        rc = self.lib.wc_map_export(self.ctx.h, self.h, C.c_void_p(d_xyz.ptr if d_xyz else 0), C.c_void_p(d_count.ptr if d_count else 0),
                                    C.c_void_p(d_keys.ptr if d_keys else 0), C.c_uint64(int(cap)), C.byref(n))
        return rc, int(n.value)

    def export(self):
        """-> (xyz (n, 3) float32 centroids, counts (n,) uint32, keys (n, 3) int32) in ascending (kx, ky, kz) order"""
        n, _ = self.size()
        if n == 0:
            return np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), np.zeros((0, 3), np.int32)
        bx, bc, bk = self.ctx.alloc(12 * n), self.ctx.alloc(4 * n), self.ctx.alloc(12 * n)
        try:
            rc, m = self.export_device(bx, bc, bk, n)
            self.ctx._ck(rc)
            return bx.download(np.float32, 3 * m).reshape(-1, 3), bc.download(np.uint32, m), bk.download(np.int32, 3 * m).reshape(-1, 3)
        finally:
            for b in (bx, bc, bk):
                b.free()

    def surfels_device(self, d_out, cap):
        """MAP_SURFEL records into d_out (wc_map_export_surfels) -> (return code, n): WC_ERR_CAPACITY leaves the needed count in n"""
        n = C.c_uint64(0)
        rc = self.lib.wc_map_export_surfels(self.ctx.h, self.h, C.c_void_p(d_out.ptr if d_out else 0), C.c_uint64(int(cap)), C.byref(n))
        return rc, int(n.value)

    def surfels(self):
        """-> MAP_SURFEL array: one record per occupied voxel, in export()'s order (a map created with moments=True)"""
        rc, n = self.surfels_device(None, 0)
        if n == 0:
            self.ctx._ck(rc)
            return np.zeros(0, R.MAP_SURFEL)
        d_out = self.ctx.alloc(R.MAP_SURFEL.itemsize * n)
        try:
            rc, m = self.surfels_device(d_out, n)
            self.ctx._ck(rc)
            return d_out.download(R.MAP_SURFEL, m)
        finally:
            d_out.free()

    def state_device(self, d_vox, d_mom, cap):
        """MAP_VOXEL records into d_vox and (n, 9) int64 moment words into d_mom (either may be None) (wc_map_export_state)
        -> (return code, n): WC_ERR_CAPACITY leaves the needed count in n"""
        n = C.c_uint64(0)
        rc = self.lib.wc_map_export_state(self.ctx.h, self.h, C.c_void_p(d_vox.ptr if d_vox else 0), C.c_void_p(d_mom.ptr if d_mom else 0),
                                          C.c_uint64(int(cap)), C.byref(n))
        return rc, int(n.value)

    def state(self):
        """-> (MAP_VOXEL array, (n, 9) int64 moment words or None on a plain map): the table's integer sums themselves, one record per
        occupied voxel in export()'s order"""
        rc, n = self.state_device(None, None, 0)
        if n == 0:
            self.ctx._ck(rc)
            return np.zeros(0, R.MAP_VOXEL), (np.zeros((0, 9), np.int64) if self.moments else None)
        d_vox = self.ctx.alloc(R.MAP_VOXEL.itemsize * n)
        d_mom = self.ctx.alloc(72 * n) if self.moments else None
        try:
            rc, m = self.state_device(d_vox, d_mom, n)
            self.ctx._ck(rc)
            return d_vox.download(R.MAP_VOXEL, m), (d_mom.download(np.int64, 9 * m).reshape(-1, 9) if d_mom else None)
        finally:
            for b in (d_vox, d_mom):
                if b:
                    b.free()

    def absorb_device(self, d_vox, d_mom, n, want_count=True):
        """n MAP_VOXEL records (and their moment words, or None) already in HBM added to the map by key (wc_map_absorb) -> records
        rejected, or None without waiting when want_count is False"""
        rej = C.c_uint64(0)
        self.ctx._ck(self.lib.wc_map_absorb(self.ctx.h, self.h, C.c_void_p(d_vox.ptr if d_vox else 0), C.c_void_p(d_mom.ptr if d_mom else 0),
                                            C.c_uint64(int(n)), C.byref(rej) if want_count else None))
        return int(rej.value) if want_count else None

    def absorb(self, vox, mom=None):
        """a state (MAP_VOXEL array; mom: (n, 9) int64, needed by a map with moments), uploaded for the call -> records rejected.  The
        records need not be sorted, duplicate keys add up"""
        vox = np.ascontiguousarray(vox, R.MAP_VOXEL)
        n = len(vox)
        if mom is not None:
            mom = np.ascontiguousarray(mom, np.int64).reshape(-1, 9)
            assert len(mom) == n, "one row of nine moment words per record"
        d_vox = self.ctx.to_device(vox) if n else None
        d_mom = self.ctx.to_device(mom) if (mom is not None and n) else None
        try:
            return self.absorb_device(d_vox, d_mom, n)
        finally:
            for b in (d_vox, d_mom):
                if b:
                    b.free()

    def merge(self, other):
        """this map becomes the map of its own points and other's (wc_map_merge: table to table on the device); other is not modified"""
        self.ctx._ck(self.lib.wc_map_merge(self.ctx.h, self.h, other.h))

    def merge_moved(self, other, T, want_counts=True):
        """other, a map built in another frame, added to this map under the rigid T (3 x 4: other's frame to this one's), every voxel
        moved as one Gaussian (wc_map_merge_moved: table to table on the device) -> [voxels applied, points applied, voxels rejected,
        points rejected], or None without waiting when want_counts is False; other is not modified"""
        out = (C.c_uint64 * 4)()
        T12 = None if T is None else _pose12(T)
        self.ctx._ck(self.lib.wc_map_merge_moved(self.ctx.h, self.h, other.h, None if T12 is None else R.ptr(T12), out if want_counts else None))
        return [int(x) for x in out] if want_counts else None

    def moved(self, T):
        """-> a new PointMap of this map's voxel size and flags that holds this map moved by T: an empty map plus merge_moved"""
        m = PointMap(self.ctx, self.voxel, moments=self.moments)
        try:
            m.merge_moved(self, T)
        except WildcatError:
            m.close()
            raise
        return m

    def coarsen(self, factor, moments=None):
        """-> a new PointMap of voxel size float(factor) * voxel that holds this map's voxels gathered factor^3 to one, exactly
        (wc_map_coarsen); moments: None follows this map, False drops them, True needs a map with moments.  This map is not modified"""
        mom = self.moments if moments is None else bool(moments)
        h = C.c_void_p(0)
        self.ctx._ck(self.lib.wc_map_coarsen(self.ctx.h, self.h, C.c_uint32(int(factor)), C.c_uint32(R.MAP_MOMENTS if mom else 0), C.byref(h)))
        m = object.__new__(PointMap)
        m.ctx, m.lib, m.voxel, m.moments, m.h = self.ctx, self.lib, float(int(factor)) * self.voxel, mom, h
        return m

    def pyramid(self, factor, n_levels):
        """-> [this map, coarsen(factor) of it, coarsen(factor) of that, ...]: n_levels maps, finest first; the caller closes levels 1 ..."""
        levels = [self]
        try:
            for _ in range(1, int(n_levels)):
                levels.append(levels[-1].coarsen(factor))
        except WildcatError:
            for m in levels[1:]:
                m.close()
            raise
        return levels

    def nearest_plane_device(self, desc, max_dist, min_points, d_hits, want_count=True):
        """queries already in HBM (a wc_points descriptor) -> MAP_PLANE_HIT records in d_hits (wc_map_nearest_plane); returns the number
        of voxels found, or None without waiting when want_count is False"""
        n = C.c_uint64(0)
        self.ctx._ck(self.lib.wc_map_nearest_plane(self.ctx.h, self.h, C.byref(desc), C.c_double(max_dist), C.c_uint32(int(min_points)),
                                                   C.c_void_p(d_hits.ptr if d_hits else 0), C.byref(n) if want_count else None))
        return int(n.value) if want_count else None

    def nearest_plane(self, queries, max_dist=np.inf, min_points=3):
        """POINT records or an (n, 3) float32 array (uploaded for the call) -> MAP_PLANE_HIT array: nearest()'s record per query, and
        the plane of the voxel found (flags bit 1) where it holds at least min_points points"""
        with self._uploaded(queries, R.MAP_PLANE_HIT) as (desc, d_hits):
            self.nearest_plane_device(desc, max_dist, min_points, d_hits)
            return d_hits.download(R.MAP_PLANE_HIT, desc.n)

    def linearize_device(self, desc, T, params, d_rows=None):
        """points already in HBM (a wc_points descriptor) moved by T (3 x 4 row-major) -> MAP_NORMAL_EQ record (wc_map_linearize: the
        point-to-plane normal equations against the map's planes); d_rows: a DeviceBuffer for one MAP_REG_ROW per point, or None"""
        out = np.zeros(1, R.MAP_NORMAL_EQ)
        T = _pose12(T)
        self.ctx._ck(self.lib.wc_map_linearize(self.ctx.h, self.h, C.byref(desc), R.ptr(T), C.byref(params), R.ptr(out),
                                               C.c_void_p(d_rows.ptr if d_rows else 0)))
        return out[0]

    def linearize(self, points, T, params=None, want_rows=False, **kw):
        """POINT records or an (n, 3) float32 array (uploaded for the call) -> MAP_NORMAL_EQ record, or (record, MAP_REG_ROW array)
        with want_rows; params: a wc_map_reg_params, or its fields as keywords (max_dist defaults to the voxel size)"""
        if params is None:
            kw.setdefault("max_dist", self.voxel)
            params = map_reg_params(**kw)
        with self._uploaded(points, R.MAP_REG_ROW if want_rows else None) as (desc, d_rows):
            ne = self.linearize_device(desc, T, params, d_rows)
            return (ne, d_rows.download(R.MAP_REG_ROW, desc.n)) if want_rows else ne

    def align_device(self, desc, T, opts):
        """wc_map_align on points already in HBM -> (T (3, 4), summary dict)"""
        T = _pose12(T)
        summ = R.MapAlignSummary()
        self.ctx._ck(self.lib.wc_map_align(self.ctx.h, self.h, C.byref(desc), R.ptr(T), C.byref(opts), C.byref(summ)))
        return T.reshape(3, 4), _summary_dict(summ)

    def align(self, points, T, opts=None, params=None, **kw):
        """Gauss-Newton registration of POINT records or an (n, 3) float32 array against the map, from the pose T -> (T (3, 4), summary
        dict: initial_cost, final_cost, iterations, termination (0 converged, 1 max_iterations, 2 failure), n_used, n_found, last_step);
        opts: a wc_map_align_opts, or params (a wc_map_reg_params, default max_dist = the voxel size) and map_align_opts' keywords"""
        if opts is None:
            opts = map_align_opts(params if params is not None else map_reg_params(self.voxel), **kw)
        with self._uploaded(points) as (desc, _):
            return self.align_device(desc, T, opts)

    @contextlib.contextmanager
    def _uploaded_stamped(self, points, times=None):
        """POINT records (their own stamps), or an (n, 3) float32 array with `times` (n,) float64, in HBM for the length of a with block
        -> the wc_points descriptor with its time pointer set; freed on the way out"""
        points = np.ascontiguousarray(points)
        if points.dtype == R.POINT:
            assert times is None, "POINT records carry their stamps"
            bufs = [self.ctx.to_device(points)] if len(points) else []
            desc = R.Points(bufs[0].ptr, bufs[0].ptr + 24, 48, 48, len(points)) if bufs else R.Points(0, 0, 48, 48, 0)
        else:
            points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
            times = np.ascontiguousarray(times, np.float64).reshape(-1)
            assert len(times) == len(points), "one stamp per point"
            bufs = [self.ctx.to_device(points), self.ctx.to_device(times)] if len(points) else []
            desc = R.Points(bufs[0].ptr, bufs[1].ptr, 12, 8, len(points)) if bufs else R.Points(0, 0, 12, 8, 0)
        try:
            yield desc
        finally:
            for b in bufs:
                b.free()

    def linearize_ct_device(self, desc, pose_begin, pose_end, t_begin, t_end, params, d_rows=None, d_xyz_out=None):
        """stamped points already in HBM, the poses (pos, quat) at t_begin and t_end -> MAP_CT_NORMAL_EQ record (wc_map_linearize_ct);
        d_rows: a DeviceBuffer for one MAP_CT_ROW per point, d_xyz_out: one for n x 3 floats (the moved points), or None"""
        out = np.zeros(1, R.MAP_CT_NORMAL_EQ)
        b, e = _pose_rec(pose_begin), _pose_rec(pose_end)
        self.ctx._ck(self.lib.wc_map_linearize_ct(self.ctx.h, self.h, C.byref(desc), C.byref(b), C.byref(e), C.c_double(t_begin), C.c_double(t_end),
                                                  C.byref(params), R.ptr(out), C.c_void_p(d_rows.ptr if d_rows else 0),
                                                  C.c_void_p(d_xyz_out.ptr if d_xyz_out else 0)))
        return out[0]

    def linearize_ct(self, points, pose_begin, pose_end, t_begin, t_end, params=None, times=None, want_rows=False, want_xyz=False, **kw):
        """a raw sweep - POINT records, or an (n, 3) float32 array with times - registered in continuous time between two poses ->
        MAP_CT_NORMAL_EQ record, followed by the MAP_CT_ROW array with want_rows and the moved points (n, 3) float32 with want_xyz;
        params: a wc_map_reg_params, or its fields as keywords (max_dist defaults to the voxel size)"""
        if params is None:
            kw.setdefault("max_dist", self.voxel)
            params = map_reg_params(**kw)
        with self._uploaded_stamped(points, times) as desc:
            n = int(desc.n)
            d_rows = self.ctx.alloc(72 * max(n, 1)) if want_rows else None
            d_xyz = self.ctx.alloc(12 * max(n, 1)) if want_xyz else None
            try:
                out = [self.linearize_ct_device(desc, pose_begin, pose_end, t_begin, t_end, params, d_rows, d_xyz)]
                if want_rows:
                    out.append(d_rows.download(R.MAP_CT_ROW, n))
                if want_xyz:
                    out.append(d_xyz.download(np.float32, 3 * n).reshape(n, 3))
            finally:
                for b in (d_rows, d_xyz):
                    if b:
                        b.free()
        return out[0] if len(out) == 1 else tuple(out)

    def align_ct_device(self, desc, pose_begin, pose_end, t_begin, t_end, opts):
        """wc_map_align_ct on stamped points already in HBM -> ((pos, quat) of begin, (pos, quat) of end, summary dict)"""
        b, e, summ = _pose_rec(pose_begin), _pose_rec(pose_end), R.MapCtAlignSummary()
        self.ctx._ck(self.lib.wc_map_align_ct(self.ctx.h, self.h, C.byref(desc), C.byref(b), C.byref(e), C.c_double(t_begin), C.c_double(t_end),
                                              C.byref(opts), C.byref(summ)))
        return _pose_pair(b), _pose_pair(e), _ct_summary_dict(summ)

    def align_ct(self, points, pose_begin, pose_end, t_begin, t_end, opts=None, params=None, times=None, **kw):
        """Gauss-Newton registration of a raw sweep in continuous time, from the poses at t_begin and t_end -> as align_ct_device; opts: a
        wc_map_ct_align_opts, or params (a wc_map_reg_params, default max_dist = the voxel size) and map_ct_align_opts' keywords"""
        if opts is None:
            opts = map_ct_align_opts(params if params is not None else map_reg_params(self.voxel), **kw)
        with self._uploaded_stamped(points, times) as desc:
            return self.align_ct_device(desc, pose_begin, pose_end, t_begin, t_end, opts)

    def linearize_batch_device(self, desc, Ts, params):
        """wc_map_linearize_batch on points already in HBM: K poses Ts -> (MAP_NORMAL_EQ array (K,), status (K,) int32); record h is
        byte-equal to linearize_device's for pose h where status[h] is 0, and zero where it is not"""
        Ts = _poses12(Ts)
        K = len(Ts)
        out, status = np.zeros(K, R.MAP_NORMAL_EQ), np.zeros(K, np.int32)
        self.ctx._ck(self.lib.wc_map_linearize_batch(self.ctx.h, self.h, C.byref(desc), R.ptr(Ts) if K else None, C.c_uint32(K), C.byref(params),
                                                     R.ptr(out) if K else None, R.ptr(status) if K else None))
        return out, status

    def linearize_batch(self, points, Ts, params=None, **kw):
        """POINT records or an (n, 3) float32 array (uploaded for the call) and K poses -> as linearize_batch_device; params: a
        wc_map_reg_params, or its fields as keywords (max_dist defaults to the voxel size)"""
        if params is None:
            kw.setdefault("max_dist", self.voxel)
            params = map_reg_params(**kw)
        with self._uploaded(points) as (desc, _):
            return self.linearize_batch_device(desc, Ts, params)

    def score_batch_device(self, desc, Ts, min_points=1):
        """wc_map_score_batch on points already in HBM: K poses Ts -> MAP_SCORE array (K,): per pose the points that land in a voxel
        holding at least min_points points (n_hit), inside the key range (n_in), and sent to a non-finite point (n_bad)"""
        Ts = _poses12(Ts)
        K = len(Ts)
        out, params = np.zeros(K, R.MAP_SCORE), R.MapScoreParams(int(min_points), 0)
        self.ctx._ck(self.lib.wc_map_score_batch(self.ctx.h, self.h, C.byref(desc), R.ptr(Ts) if K else None, C.c_uint32(K), C.byref(params),
                                                 R.ptr(out) if K else None))
        return out

    def score_batch(self, points, Ts, min_points=1):
        """POINT records or an (n, 3) float32 array (uploaded for the call) and K poses -> as score_batch_device"""
        with self._uploaded(points) as (desc, _):
            return self.score_batch_device(desc, Ts, min_points)

    def align_batch_device(self, desc, Ts, opts):
        """wc_map_align_batch on points already in HBM: K starts in lockstep -> (Ts (K, 3, 4), [summary dict per hypothesis], status (K,)
        int32), each hypothesis as align_device leaves it"""
        Ts = _poses12(Ts)
        K = len(Ts)
        summ, status = (R.MapAlignSummary * max(K, 1))(), np.zeros(K, np.int32)
        self.ctx._ck(self.lib.wc_map_align_batch(self.ctx.h, self.h, C.byref(desc), R.ptr(Ts) if K else None, C.c_uint32(K), C.byref(opts), summ,
                                                 R.ptr(status) if K else None))
        return Ts.reshape(K, 3, 4), [_summary_dict(summ[h]) for h in range(K)], status

    def align_batch(self, points, Ts, opts=None, params=None, **kw):
        """align for K starts in one pass (at most max_iterations + 1 rounds of one linearize_batch each) -> as align_batch_device; opts
        and params as align's"""
        if opts is None:
            opts = map_align_opts(params if params is not None else map_reg_params(self.voxel), **kw)
        with self._uploaded(points) as (desc, _):
            return self.align_batch_device(desc, Ts, opts)

    def clear(self):
        self.ctx._ck(self.lib.wc_map_clear(self.ctx.h, self.h))

    def close(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.lib.wc_map_destroy(self.ctx.h, self.h)
        self.h = None


class Odometry:
    """the C++ LidarOdometry facade (host/lidar_odometry.h) through its flat C wrapper (host/odom_c_api.cc)"""

    def __init__(self, device=0):
        so = os.path.join(os.path.dirname(_CSRC), "host", "libwildcat_odometry.so")
        load()
        self.lib = C.CDLL(so)
        self.lib.wc_odom_create.restype = C.c_void_p
        self.lib.wc_odom_num_samples.restype = C.c_uint64
        self.lib.wc_odom_append_ms.restype = C.c_double
        self.h = C.c_void_p(self.lib.wc_odom_create(C.c_int(device)))

    def close(self):
        if self.h:
            self.lib.wc_odom_destroy(self.h)
            self.h = None

    def add_imu(self, t, acc, gyr):
        a, g = (C.c_double * 3)(*acc), (C.c_double * 3)(*gyr)
        self.lib.wc_odom_add_imu(self.h, C.c_double(t), a, g)

    def add_scan(self, points):
        assert points.dtype == R.POINT
        self.lib.wc_odom_add_scan(self.h, R.ptr(points), C.c_uint64(len(points)))

    def stage_ms(self):
        """wall time [ms] of the last completed sweep's stages + its LM iterations (host/lidar_odometry.cc)"""
        out = (C.c_double * 8)()
        self.lib.wc_odom_stage_ms(self.h, out)
        names = ("predict_undistort", "extract_poses", "match", "build", "solve", "update", "shrink")
        d = dict(zip(names, [float(v) for v in out[:7]]))
        d["lm_iterations"] = int(out[7])
        d["append"] = float(self.lib.wc_odom_append_ms(self.h))  # upload + pre-filter of the completing message, in front of the stages
        return d

    def extract_paths(self):
        """(sweeps extracted by the default integer-moment path, sweeps extracted in the reference's summation order)"""
        out = (C.c_int * 2)()
        self.lib.wc_odom_extract_paths(self.h, out)
        return out[0], out[1]

    def set_fill_outputs(self, on):
        """what the reference publishes after a sweep (lidar_odometry.cc:582-602) as plain data: markers, sweep, tf"""
        self.lib.wc_odom_set_fill_outputs(self.h, C.c_int(1 if on else 0))

    def outputs(self):
        """-> dict(markers (n, 14): position, orientation wxyz, scale, rgba; scan: POINT records of the published sweep; stamp;
        tf: stamp, origin (3), rotation xyzw (4))"""
        self.lib.wc_odom_markers.restype = C.c_uint64
        self.lib.wc_odom_scan_in_world.restype = C.c_uint64
        n = int(self.lib.wc_odom_markers(self.h, None, C.c_uint64(0)))
        m = np.zeros((max(n, 1), 14))
        self.lib.wc_odom_markers(self.h, R.ptr(m), C.c_uint64(n))
        k = int(self.lib.wc_odom_scan_in_world(self.h, None, C.c_uint64(0), None, None))
        pts = np.zeros(max(k, 1), R.POINT)
        stamp, tf = C.c_double(0), np.zeros(8)
        self.lib.wc_odom_scan_in_world(self.h, R.ptr(pts), C.c_uint64(k), C.byref(stamp), R.ptr(tf))
        return dict(markers=m[:n], scan=pts[:k], stamp=stamp.value, tf=tf)

    def set_map_voxel(self, voxel):
        """the accumulated map (LioConfig::map_voxel_size): 0 = off, 0.01 .. 4.0 = (re-)created empty"""
        rc = self.lib.wc_odom_set_map_voxel(self.h, C.c_double(voxel))
        if rc != 0:
            raise WildcatError(rc, "wc_odom_set_map_voxel(%r)" % voxel)

    def map_size(self):
        """-> (voxels, points inserted, points rejected)"""
        out = (C.c_uint64 * 3)()
        self.lib.wc_odom_map_size(self.h, out)
        return int(out[0]), int(out[1]), int(out[2])

    def map_export(self):
        """-> (xyz (n, 3) float32 centroids, counts (n,) uint32) in ascending voxel-index order"""
        self.lib.wc_odom_map_export.restype = C.c_uint64
        n = int(self.map_size()[0])
        xyz, cnt = np.zeros((max(n, 1), 3), np.float32), np.zeros(max(n, 1), np.uint32)
        m = int(self.lib.wc_odom_map_export(self.h, R.ptr(xyz), R.ptr(cnt), C.c_uint64(n)))
        assert m == n
        return xyz[:n], cnt[:n]

    def map_clear(self):
        self.lib.wc_odom_map_clear(self.h)

    def map_query(self, xyz, max_dist):
        """nearest map voxel of every row of xyz ((n, 3) float32) within max_dist -> MAP_HIT array (LidarOdometry::QueryMap)"""
        if not max_dist > 0:
            raise WildcatError(11, "map_query: max_dist must be > 0")
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        hits = np.zeros(len(xyz), R.MAP_HIT)
        self.lib.wc_odom_map_query.restype = C.c_uint64
        self.lib.wc_odom_map_query(self.h, R.ptr(xyz), C.c_uint64(len(xyz)), C.c_double(max_dist), R.ptr(hits))
        return hits

    def map_query_knn(self, xyz, k, max_dist=np.inf, reach=1, min_points=1, not_own=False):
        """PointMap.knn of every row of xyz ((n, 3) float32) against the facade's map -> (hits (n, k) MAP_HIT, within (n,) uint32)
        (LidarOdometry::QueryMapKnn); without a map every record is a miss"""
        k = int(k)
        if not (max_dist > 0 and 1 <= k <= 16 and reach in (1, 2) and min_points >= 1):
            raise WildcatError(11, "map_query_knn: max_dist must be > 0, k in 1 .. 16, reach 1 or 2, min_points >= 1")
        params = R.MapKnnParams(float(max_dist), k, int(reach), int(min_points), R.MAP_KNN_NOT_OWN if not_own else 0)
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        hits, within = np.zeros((len(xyz), k), R.MAP_HIT), np.zeros(len(xyz), np.uint32)
        self.lib.wc_odom_map_query_knn.restype = C.c_uint64
        self.lib.wc_odom_map_query_knn(self.h, R.ptr(xyz), C.c_uint64(len(xyz)), C.byref(params), R.ptr(hits), R.ptr(within))
        return hits, within

    def map_crop(self, lo, hi):
        """keeps the map's voxels that intersect the box [lo, hi] -> voxels removed (LidarOdometry::CropMap)"""
        lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
        if not np.all(lo <= hi):
            raise WildcatError(11, "map_crop: NaN bound or lo > hi")
        self.lib.wc_odom_map_crop.restype = C.c_uint64
        return int(self.lib.wc_odom_map_crop(self.h, (C.c_double * 3)(*lo), (C.c_double * 3)(*hi)))

    def set_map_surfels(self, on):
        """LioConfig::map_surfels: the map re-created empty, with (True) or without second moments"""
        self.lib.wc_odom_set_map_surfels(self.h, C.c_int(1 if on else 0))

    def map_surfels(self):
        """-> MAP_SURFEL array of the map's voxels (LidarOdometry::ExportMapSurfels); empty without map_surfels"""
        self.lib.wc_odom_map_surfels.restype = C.c_uint64
        n = int(self.lib.wc_odom_map_surfels(self.h, None, C.c_uint64(0)))
        out = np.zeros(max(n, 1), R.MAP_SURFEL)
        m = int(self.lib.wc_odom_map_surfels(self.h, R.ptr(out), C.c_uint64(n)))
        assert m == n
        return out[:n]

    def map_query_planes(self, xyz, max_dist, min_points=3):
        """wc_map_nearest_plane of every row of xyz ((n, 3) float32) -> MAP_PLANE_HIT array (LidarOdometry::QueryMapPlanes)"""
        if not max_dist > 0 or min_points < 3:
            raise WildcatError(11, "map_query_planes: max_dist must be > 0 and min_points >= 3")
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        hits = np.zeros(len(xyz), R.MAP_PLANE_HIT)
        self.lib.wc_odom_map_query_planes.restype = C.c_uint64
        self.lib.wc_odom_map_query_planes(self.h, R.ptr(xyz), C.c_uint64(len(xyz)), C.c_double(max_dist), C.c_uint32(int(min_points)), R.ptr(hits))
        return hits

    def map_linearize(self, xyz, T, params, want_rows=False):
        """wc_map_linearize of every row of xyz ((n, 3) float32) moved by T against the map's planes (LidarOdometry::LinearizeAgainstMap)
        -> MAP_NORMAL_EQ record (with want_rows: (record, MAP_REG_ROW array)), or None without a map or with map_surfels off"""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        out, rows, T = np.zeros(1, R.MAP_NORMAL_EQ), np.zeros(max(len(xyz), 1), R.MAP_REG_ROW), _pose12(T)
        ok = self.lib.wc_odom_map_linearize(self.h, R.ptr(xyz), C.c_uint64(len(xyz)), R.ptr(T), C.byref(params), R.ptr(out),
                                            R.ptr(rows) if want_rows else None)
        if not ok:
            return None
        return (out[0], rows[: len(xyz)]) if want_rows else out[0]

    def map_align(self, xyz, T, opts):
        """wc_map_align of xyz ((n, 3) float32) from the pose T (LidarOdometry::AlignToMap) -> (T (3, 4), summary dict), or None without
        a map or with map_surfels off"""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        T, summ = _pose12(T), R.MapAlignSummary()
        if not self.lib.wc_odom_map_align(self.h, R.ptr(xyz), C.c_uint64(len(xyz)), R.ptr(T), C.byref(opts), C.byref(summ)):
            return None
        return T.reshape(3, 4), _summary_dict(summ)

    def map_align_sweep(self, points, pose_begin, pose_end, opts, insert=False):
        """wc_map_align_ct of a raw sweep of POINT records (body frame, with stamps) against the map, from the poses (pos, quat) at the
        sweep's smallest and largest stamp (LidarOdometry::AlignSweepToMap); insert: the registered sweep is inserted into the map ->
        ((pos, quat) of begin, (pos, quat) of end, summary dict), or None where map_align returns None or the sweep spans no interval"""
        points = np.ascontiguousarray(points)
        assert points.dtype == R.POINT, "POINT records"
        b, e, summ = _pose_rec(pose_begin), _pose_rec(pose_end), R.MapCtAlignSummary()
        if not self.lib.wc_odom_map_align_sweep(self.h, R.ptr(points), C.c_uint64(len(points)), C.byref(b), C.byref(e), C.byref(opts), C.byref(summ),
                                                C.c_int(1 if insert else 0)):
            return None
        return _pose_pair(b), _pose_pair(e), _ct_summary_dict(summ)

    def map_relocalize(self, xyz, T, factor, n_levels, opts):
        """coarse-to-fine wc_map_align of xyz ((n, 3) float32) from the rough pose T (LidarOdometry::RelocalizeToMap): n_levels - 1
        coarser levels built from the map by chained wc_map_coarsen(factor), run coarsest first with `opts` (the finest level's) and
        max_dist multiplied by factor^l -> (T (3, 4), [summary dict per level, coarsest first]), or None where map_align returns None
        or a level's voxel size would exceed 4.0"""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n_levels = int(n_levels)
        T, summ = _pose12(T), (R.MapAlignSummary * max(n_levels, 1))()
        if not 1 <= n_levels <= 8 or not self.lib.wc_odom_map_relocalize(self.h, R.ptr(xyz), C.c_uint64(len(xyz)), R.ptr(T), C.c_uint32(int(factor)),
                                                                          C.c_uint32(n_levels), C.byref(opts), summ):
            return None
        return T.reshape(3, 4), [_summary_dict(s) for s in summ]

    def map_relocalize_search(self, xyz, T, n_yaw, factor, n_levels, opts):
        """map_relocalize when the heading is unknown (LidarOdometry::RelocalizeSearch): n_yaw starts pose_yaw_grid(T, n_yaw) through the
        levels in one batched pass, the winner by map_align_best on the finest level with opts.min_used -> (T (3, 4) of the winner,
        [[summary dict per hypothesis] per level, coarsest first], the winner's index), or None where map_relocalize returns None, for
        n_yaw outside 1 .. 1024, or when no hypothesis is eligible"""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n_levels, K = int(n_levels), int(n_yaw)
        if not 1 <= n_levels <= 8 or not 1 <= K <= 1024:
            return None
        T, summ, best = _pose12(T), (R.MapAlignSummary * (n_levels * K))(), C.c_int32(-1)
        if not self.lib.wc_odom_map_relocalize_search(self.h, R.ptr(xyz), C.c_uint64(len(xyz)), R.ptr(T), C.c_uint32(K), C.c_uint32(int(factor)),
                                                      C.c_uint32(n_levels), C.byref(opts), summ, C.byref(best)):
            return None
        return T.reshape(3, 4), [[_summary_dict(summ[l * K + h]) for h in range(K)] for l in range(n_levels)], int(best.value)

    def map_relocalize_global(self, xyz, T, n_yaw, n_xyz, step, top_m, factor, n_levels, opts):
        """map_relocalize when neither heading nor position is known (LidarOdometry::RelocalizeGlobal): the poses pose_grid(T, n_yaw, n_xyz,
        step) scored on the coarsest level (PointMap.score_batch, min_points 1), the top_m best (map_score_top, min_hit = opts.min_used)
        through the levels in one batched pass in rank order, the winner by map_align_best on the finest level -> (T (3, 4) of the winner,
        [[summary dict per candidate, rank order] per level, coarsest first], the winner's rank), or None where map_relocalize returns None,
        for top_m outside 1 .. 1024, for a refused grid, or when no candidate or no aligned hypothesis is eligible"""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n_levels, M = int(n_levels), int(top_m)
        n = np.ascontiguousarray(n_xyz, np.uint32).reshape(-1)
        step = np.ascontiguousarray(step, np.float64).reshape(-1)
        if not 1 <= n_levels <= 8 or not 1 <= M <= 1024 or n.size != 3 or step.size != 3:
            return None
        T, summ, best = _pose12(T), (R.MapAlignSummary * (n_levels * M))(), C.c_int32(-1)
        if not self.lib.wc_odom_map_relocalize_global(self.h, R.ptr(xyz), C.c_uint64(len(xyz)), R.ptr(T), C.c_uint32(int(n_yaw)), R.ptr(n),
                                                      R.ptr(step), C.c_uint32(M), C.c_uint32(int(factor)), C.c_uint32(n_levels), C.byref(opts),
                                                      summ, C.byref(best)):
            return None
        return T.reshape(3, 4), [[_summary_dict(summ[l * M + h]) for h in range(M)] for l in range(n_levels)], int(best.value)

    def map_save(self, path):
        """the map's exact state as the canonical file of host/map_file.h (LidarOdometry::SaveMap) -> True, or False without a map or
        when the file cannot be written"""
        return bool(self.lib.wc_odom_map_save(self.h, os.fsencode(path)))

    def map_load(self, path, merge=False):
        """a file map_save wrote, absorbed into the map - re-created empty first unless merge (LidarOdometry::LoadMap) -> True, or False
        (the map untouched) without a map, for a file the decoder refuses, another voxel size, or a file without moments with map_surfels on"""
        return bool(self.lib.wc_odom_map_load(self.h, os.fsencode(path), C.c_int(1 if merge else 0)))

    def map_merge_file(self, path, T, factor, n_levels, opts):
        """a file map_save wrote in ANOTHER frame, aligned to the map from the rough pose T (the file's frame to the map's) through
        map_relocalize's levels on the file's centroids, then merged under the pose found, every voxel moved as one Gaussian
        (LidarOdometry::MergeMapFile, wc_map_merge_moved) -> (T (3, 4), [summary dict per level, coarsest first]), or None (the map
        untouched) where map_load or map_relocalize refuses, or when the alignment ends with termination 2 or under opts.min_used"""
        n_levels = int(n_levels)
        T, summ = _pose12(T), (R.MapAlignSummary * max(n_levels, 1))()
        if not 1 <= n_levels <= 8 or not self.lib.wc_odom_map_merge_file(self.h, os.fsencode(path), R.ptr(T), C.c_uint32(int(factor)),
                                                                          C.c_uint32(n_levels), C.byref(opts), summ):
            return None
        return T.reshape(3, 4), [_summary_dict(s) for s in summ]

    def set_map_keep_radius(self, radius):
        """LioConfig::map_keep_radius: after every sweep the map keeps the cube of this half-side around the sensor; 0 = unbounded"""
        rc = self.lib.wc_odom_set_map_keep_radius(self.h, C.c_double(radius))
        if rc != 0:
            raise WildcatError(rc, "wc_odom_set_map_keep_radius(%r)" % radius)

    def map_carve(self, xyz, origin, max_range, min_range=0.0, shell=1, min_rays=1, max_steps=4096):
        """wc_map_carve of the facade's map with the rows of xyz ((n, 3) float32) as the ends of rays from origin (LidarOdometry::CarveMap)
        -> the result as a dict (what the rays select; the map is not modified), or None without a map or with arguments the library refuses"""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        o = (C.c_double * 3)(*[float(x) for x in origin])
        params, res = map_carve_params(max_range, min_range, shell, min_rays, max_steps), R.MapCarveResult()
        if not self.lib.wc_odom_map_carve(self.h, R.ptr(xyz), C.c_uint64(len(xyz)), o, C.byref(params), C.byref(res)):
            return None
        return _carve_dict(res)

    def map_carve_remove(self, xyz, origin, max_range, min_range=0.0, shell=1, min_rays=1, max_steps=4096):
        """map_carve() that also removes what it selects from the facade's map (LidarOdometry::CarveMapRemove) -> the dict map_carve()
        would have returned, or None without a map or with arguments the library refuses"""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        o = (C.c_double * 3)(*[float(x) for x in origin])
        params, res = map_carve_params(max_range, min_range, shell, min_rays, max_steps), R.MapCarveResult()
        if not self.lib.wc_odom_map_carve_remove(self.h, R.ptr(xyz), C.c_uint64(len(xyz)), o, C.byref(params), C.byref(res)):
            return None
        return _carve_dict(res)

    def map_remove(self, keys):
        """wc_map_remove_keys of the facade's map for the voxel indices keys ((n, 3) int32) (LidarOdometry::RemoveMapVoxels)
        -> dict(voxels_removed, points_removed, keys_unused), or None without a map"""
        keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
        out = (C.c_uint64 * 3)()
        if not self.lib.wc_odom_map_remove_keys(self.h, R.ptr(keys) if len(keys) else None, C.c_uint64(len(keys)), out):
            return None
        return dict(zip(("voxels_removed", "points_removed", "keys_unused"), [int(x) for x in out]))

    def map_components(self, connectivity=26, min_points=1):
        """wc_map_components of the facade's map (LidarOdometry::MapComponents) -> (keys, labels, MAP_COMPONENT array, dict(voxels, nodes,
        components, largest)) as PointMap.components(), or None without a map or with arguments the library refuses"""
        p, out = map_cc_params(connectivity, min_points), (C.c_uint64 * 4)()
        f = self.lib.wc_odom_map_components
        if not f(self.h, C.byref(p), None, None, C.c_uint64(0), None, C.c_uint64(0), out):  # (the sizes; 1 only for an empty map)
            if not out[0]:
                return None
        n, nc = int(out[0]), int(out[2])
        keys, labels, comps = np.zeros((max(n, 1), 3), np.int32), np.zeros(max(n, 1), np.uint32), np.zeros(max(nc, 1), R.MAP_COMPONENT)
        if n and not f(self.h, C.byref(p), R.ptr(keys), R.ptr(labels), C.c_uint64(n), R.ptr(comps), C.c_uint64(nc), out):
            return None
        return keys[:n], labels[:n], comps[:nc], dict(zip(_CC_OUT, [int(x) for x in out]))

    def map_remove_small(self, min_voxels, min_comp_points=0, connectivity=26, min_points=1, drop_sparse=False):
        """wc_map_remove_small of the facade's map (LidarOdometry::RemoveSmallMapComponents) -> dict(components, components_removed,
        voxels_removed, points_removed), or None without a map or with arguments the library refuses"""
        p, out = map_cc_params(connectivity, min_points, drop_sparse), (C.c_uint64 * 4)()
        if not self.lib.wc_odom_map_remove_small(self.h, C.byref(p), C.c_uint32(int(min_voxels)), C.c_uint64(int(min_comp_points)), out):
            return None
        return dict(zip(("components", "components_removed", "voxels_removed", "points_removed"), [int(x) for x in out]))

    def set_map_carve(self, max_range, shell=1, min_rays=2):
        """LioConfig::map_carve_range / _shell / _min_rays: after every sweep's insert the sweep's own rays remove the voxels they
        contradict (wc_map_carve_remove from the sensor's position); max_range 0 = off"""
        rc = self.lib.wc_odom_set_map_carve(self.h, C.c_double(max_range), C.c_uint32(int(shell)), C.c_uint32(int(min_rays)))
        if rc != 0:
            raise WildcatError(rc, "wc_odom_set_map_carve(%r, %r, %r)" % (max_range, shell, min_rays))

    def map_raycast(self, xyz, origin, max_range, min_range=0.0, first_step=0, end_shell=0, min_points=1, max_steps=4096):
        """wc_map_raycast of the facade's map with the rows of xyz ((n, 3) float32) as the ends of rays from origin (LidarOdometry::CastMap)
        -> (MAP_RAY_HIT array, dict of the counters), or None without a map or with arguments the library refuses"""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        o = (C.c_double * 3)(*[float(x) for x in origin])
        params, res = map_raycast_params(max_range, min_range, first_step, end_shell, min_points, max_steps), R.MapRaycastResult()
        hits = np.zeros(max(len(xyz), 1), R.MAP_RAY_HIT)
        if not self.lib.wc_odom_map_raycast(self.h, R.ptr(xyz), C.c_uint64(len(xyz)), o, C.byref(params), R.ptr(hits), C.byref(res)):
            return None
        return hits[: len(xyz)], _raycast_dict(res)

    def map_ms(self):
        """wall time [ms] of the last sweep's map step (not part of stage_ms())"""
        self.lib.wc_odom_map_ms.restype = C.c_double
        return float(self.lib.wc_odom_map_ms(self.h))

    def set_residual_log(self, on):
        """the reference's residual histograms before / after every solve (lidar_odometry.cc:56-94, :547-549, :568-570)"""
        self.lib.wc_odom_set_residual_log(self.h, C.c_int(1 if on else 0))

    def residual_log(self):
        self.lib.wc_odom_residual_log.restype = C.c_uint64
        n = int(self.lib.wc_odom_residual_log(self.h, None, C.c_uint64(0)))
        buf = C.create_string_buffer(n + 1)
        self.lib.wc_odom_residual_log(self.h, buf, C.c_uint64(n + 1))
        return buf.value.decode()

    def set_dev_option(self, name, value):
        rc = self.lib.wc_odom_set_dev_option(self.h, name.encode(), C.c_int(int(value)))
        if rc != 0:
            raise WildcatError(rc, "wc_odom_set_dev_option(%s)" % name)

    def set_quirks(self, on):
        self.lib.wc_odom_set_quirks(self.h, C.c_int(1 if on else 0))

    def config(self):
        """LioConfig's reference fields as a dict (wc_odom_get_config)"""
        c = R.OdomConfig()
        self.lib.wc_odom_get_config(self.h, C.byref(c))
        return c.to_dict()

    def set_config(self, **fields):
        """change the named fields of the configuration (wc_odom_set_config): the IMU noise model, ranges, blind box, extrinsics, imu_rate,
        sample_dt, the durations, gravity_norm, the iteration limits.  Only before the first add_imu / add_scan.  Refused - WildcatError(11),
        nothing changed - when the parameters derived from it fail wc_params_check or a timing value is not finite and positive"""
        c = R.OdomConfig()
        self.lib.wc_odom_get_config(self.h, C.byref(c))
        c.update(**fields)
        rc = self.lib.wc_odom_set_config(self.h, C.byref(c))
        if rc != WC_OK:
            self.lib.wc_odom_config_error.restype = C.c_char_p
            raise WildcatError(rc, self.lib.wc_odom_config_error(self.h).decode())

    def ctx_params(self):
        """a copy of the wc_params the facade's context holds"""
        p = R.Params()
        rc = self.lib.wc_odom_ctx_params(self.h, C.byref(p))
        assert rc == WC_OK, rc
        return p

    def set_exact_sums(self, on):
        self.lib.wc_odom_set_exact_sums(self.h, C.c_int(1 if on else 0))

    def import_state(self, samples23, imu):
        """test hook: continue from another run's sample / IMU states (LidarOdometry::ImportState)"""
        samples23 = np.ascontiguousarray(samples23, dtype=np.float64)
        imu = np.ascontiguousarray(imu)
        assert samples23.shape[1] == 23 and imu.dtype == R.IMU_STATE
        rc = self.lib.wc_odom_import_state(self.h, R.ptr(samples23), C.c_uint64(len(samples23)), R.ptr(imu), C.c_uint64(len(imu)))
        assert rc == 0, "import_state: the window's sample / IMU state counts differ"

    def sweeps(self):
        return int(self.lib.wc_odom_sweeps(self.h))

    def samples(self):
        n = int(self.lib.wc_odom_num_samples(self.h))
        out = np.zeros((n, 15))
        for i in range(n):
            self.lib.wc_odom_sample(self.h, C.c_uint64(i), R.ptr(out[i]))
        return out

    def set_keep_pair_stamps(self, on):
        self.lib.wc_odom_set_keep_pair_stamps(self.h, C.c_int(1 if on else 0))

    def pair_stamps(self, which):
        """test hook: (first, second) surfel timestamps of the last sweep's correspondences (0: sliding, 1: fixed window) -> float64[n, 2]"""
        self.lib.wc_odom_pair_stamps.restype = C.c_uint64
        n = int(self.lib.wc_odom_pair_stamps(self.h, C.c_int(which), None, C.c_uint64(0)))
        out = np.zeros(max(n, 2))
        self.lib.wc_odom_pair_stamps(self.h, C.c_int(which), R.ptr(out), C.c_uint64(n))
        return out[:n].reshape(-1, 2)

    def fixed_times(self):
        self.lib.wc_odom_fixed_times.restype = C.c_uint64
        n = int(self.lib.wc_odom_fixed_times(self.h, None, C.c_uint64(0)))
        out = np.zeros(max(n, 1))
        self.lib.wc_odom_fixed_times(self.h, R.ptr(out), C.c_uint64(n))
        return out[:n]

    def stats(self):
        s = np.zeros(8)
        self.lib.wc_odom_stats(self.h, R.ptr(s))
        return dict(zip(("sld_surfels", "fix_surfels", "binary", "unary", "lm_iters", "cost0", "cost1", "termination"), s.tolist()))
