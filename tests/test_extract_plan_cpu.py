"""The host-side decisions of an extraction (csrc/extract_plan.h), without a GPU: which pipeline a sweep starts on, which one
repeats it for which status flag, what the context remembers, and the table / grid sizes.  The header is driven through its g++
instantiation in the facade library (host/odom_c_api.cc: wc_host_ex_plan, wc_host_ex_sizes).  Every expected value below was read
off wc_extract_surfels_enqueue / wc_extract_surfels_finish as they stood before the decisions moved into the header."""
import ctypes as C
import os

import pytest

from wildcat_slam_amd import lib

FX, WIDE, RUN, BIN = 1, 2, 4, 8  # ExPath bits (ex_path_bits)
KEY_RANGE, SLOT_OVERFLOW, TIME_RANGE, BUCKET, SLOT_BIN, LDS, FX_FALLBACK = 1, 2, 4, 8, 16, 32, 64  # kFlag*
FIELDS = ("general_calls", "lds_cap", "unordered", "fx_backoff", "fx_skip_calls", "fx_spill_full", "fx_fallbacks", "fx_last_flags",
          "fx_last_why", "fx_dirty", "fx_ctrl_ready")


@pytest.fixture(scope="module")
def host():
    lib.load()
    so = os.path.join(os.path.dirname(lib.so_path()), "..", "host", "libwildcat_odometry.so")
    return C.CDLL(os.path.abspath(so))


class Plan:
    """an ExMemory (fresh context unless told otherwise) and the path of the sweep in flight"""

    def __init__(self, host, path=0, **mem):
        self.host = host
        self.mem = dict(dict.fromkeys(FIELDS, 0), lds_cap=256, **mem)
        self.path = path

    def _call(self, op, a, b):
        m = (C.c_uint32 * 11)(*[self.mem[f] for f in FIELDS])
        p = C.c_uint32(self.path)
        rc = self.host.wc_host_ex_plan(C.c_int(op), m, C.byref(p), C.c_uint32(a), C.c_uint64(b))
        self.mem, self.path = dict(zip(FIELDS, [int(v) for v in m])), int(p.value)
        return rc

    def first(self, fx_ok, no_bucket_sort=False):
        self._call(0, int(fx_ok), int(no_bucket_sort))
        return self.path

    def next(self, flags, why=0):
        """-> the path the sweep is repeated on, or None: no repeat"""
        before = self.path
        if self._call(1, flags, why):
            return self.path
        assert self.path == before  # a sweep that stands keeps its path
        return None

    def learn(self, runs, n):
        self._call(2, runs, n)
        return bool(self.mem["unordered"])

    def __getitem__(self, f):
        return self.mem[f]


def test_first_path_of_a_fresh_context(host):
    assert Plan(host).first(fx_ok=True) == FX | BIN
    assert Plan(host).first(fx_ok=False) == RUN | BIN
    assert Plan(host).first(fx_ok=False, no_bucket_sort=True) == BIN


def test_no_flags_no_repeat(host):
    for path in (FX | BIN, RUN | BIN, BIN, WIDE | BIN, RUN, 0, WIDE):
        p = Plan(host, path)
        before = dict(p.mem)
        assert p.next(0) is None
        assert p.mem == before
    # flags that are errors, not rungs
    assert Plan(host, RUN | BIN).next(SLOT_OVERFLOW | TIME_RANGE) is None
    assert Plan(host, FX | BIN).next(SLOT_OVERFLOW) is None


def test_lds_overflow_doubles_the_capacity_then_takes_the_radix_sort(host):
    p = Plan(host, RUN | BIN)
    assert p.next(LDS) == RUN | BIN and p["lds_cap"] == 512 and p["general_calls"] == 0
    assert p.next(LDS) == RUN | BIN and p["lds_cap"] == 1024 and p["general_calls"] == 0
    assert p.next(LDS) == BIN and p["lds_cap"] == 1024 and p["general_calls"] == 15  # still too large at the maximum = a bucket overflow
    assert p.next(0) is None
    # the capacity is sticky: the next sweep starts with it, on the radix sort for 15 sweeps
    for left in range(14, -1, -1):
        assert p.first(fx_ok=False) == BIN and p["general_calls"] == left
    assert p.first(fx_ok=False) == RUN | BIN and p["lds_cap"] == 1024
    # the radix sort raises no LDS flag; if one were there, nothing would follow from it
    assert Plan(host, BIN).next(LDS) is None


def test_bucket_overflow_takes_the_radix_sort(host):
    for flags in (BUCKET, BUCKET | LDS):  # (with a bucket overflow there is no doubling first)
        p = Plan(host, RUN | BIN)
        assert p.next(flags) == BIN and p["general_calls"] == 15 and p["lds_cap"] == 256
    assert Plan(host, BIN).next(BUCKET) is None


def test_key_range_takes_wide_keys_without_the_general_calls_side_effect(host):
    for flags in (KEY_RANGE, KEY_RANGE | LDS, KEY_RANGE | BUCKET, KEY_RANGE | LDS | BUCKET):
        for path in (RUN | BIN, BIN):
            p = Plan(host, path)
            assert p.next(flags) == WIDE | BIN, (flags, path)
            assert p["general_calls"] == 0 and p["lds_cap"] == 256
    assert Plan(host, WIDE | BIN).next(KEY_RANGE) is None  # already wide: the error is reported
    assert Plan(host, WIDE).next(KEY_RANGE) is None


def test_slot_bin_overflow_takes_the_radix_slot_order_once(host):
    for path in (RUN | BIN, BIN, WIDE | BIN):  # same keys, same point sort
        p = Plan(host, path)
        assert p.next(SLOT_BIN) == path & ~BIN
        assert p.next(SLOT_BIN) is None
        assert p["general_calls"] == 0
    assert Plan(host, WIDE | BIN).next(SLOT_BIN) == WIDE  # wide keys: the radix point sort stays


def test_the_checks_keep_their_order(host):
    # LDS before slot bins, bucket before slot bins, key range before slot bins: the slot order is judged by the repeat's own flags
    p = Plan(host, RUN | BIN)
    assert p.next(LDS | SLOT_BIN) == RUN | BIN and p["lds_cap"] == 512
    assert Plan(host, RUN | BIN).next(BUCKET | SLOT_BIN) == BIN
    assert Plan(host, RUN | BIN).next(KEY_RANGE | SLOT_BIN) == WIDE | BIN
    assert Plan(host, WIDE | BIN).next(KEY_RANGE | SLOT_BIN) == WIDE


@pytest.mark.parametrize("flag", [FX_FALLBACK, KEY_RANGE, SLOT_BIN, TIME_RANGE])
def test_default_path_falls_back_to_the_exact_path(host, flag):
    for calls_before, expect in ((0, RUN | BIN), (1, RUN | BIN), (2, BIN), (15, BIN)):  # run_sort iff general_calls is 0 AFTER enqueue's decrement
        p = Plan(host, general_calls=calls_before, fx_ctrl_ready=1)
        assert p.first(fx_ok=True) == FX | BIN
        assert p["general_calls"] == max(0, calls_before - 1)
        assert p.next(flag | SLOT_OVERFLOW) == expect
        assert (p["fx_fallbacks"], p["fx_last_flags"], p["fx_dirty"], p["fx_ctrl_ready"]) == (1, flag | SLOT_OVERFLOW, 1, 0)
        assert p["general_calls"] == max(0, calls_before - 1)


def test_default_path_backs_off_exponentially(host):
    p = Plan(host, fx_ctrl_ready=1)
    seen = []
    for _ in range(7):
        p.path = FX | BIN
        assert p.next(FX_FALLBACK) == RUN | BIN
        seen.append((p["fx_backoff"], p["fx_skip_calls"]))
    assert seen == [(1, 0), (2, 1), (4, 3), (8, 7), (16, 15), (32, 31), (32, 31)]
    assert p["fx_fallbacks"] == 7
    # the skipped sweeps start on the exact path
    assert p.first(fx_ok=True) == RUN | BIN and p["fx_skip_calls"] == 30
    assert p.first(fx_ok=False) == RUN | BIN and p["fx_skip_calls"] == 30  # (a sweep the default path would not take anyway does not count)
    # a success resets the back-off (not the sweeps still to be skipped)
    p.path = FX | BIN
    assert p.next(0) is None
    assert p["fx_backoff"] == 0 and p["fx_skip_calls"] == 30 and p["fx_last_flags"] == 0
    p.path = FX | BIN
    assert p.next(FX_FALLBACK) == RUN | BIN and (p["fx_backoff"], p["fx_skip_calls"]) == (1, 0)
    # new parameters / development options
    p.mem.update(fx_backoff=8, fx_skip_calls=7)
    p._call(3, 0, 0)
    assert (p["fx_backoff"], p["fx_skip_calls"]) == (0, 0)


def test_spill_full_is_sticky(host):
    p = Plan(host, FX | BIN)
    assert p.next(FX_FALLBACK, why=1 << 2) == RUN | BIN and p["fx_last_why"] == 4 and p["fx_spill_full"] == 0
    p.path = FX | BIN
    assert p.next(FX_FALLBACK, why=(1 << 4) | 1) == RUN | BIN and p["fx_last_why"] == 17 and p["fx_spill_full"] == 1
    p.path = FX | BIN
    assert p.next(FX_FALLBACK, why=1 << 23) == RUN | BIN and p["fx_last_why"] == 1 << 23 and p["fx_spill_full"] == 1
    p.path = FX | BIN
    assert p.next(0, why=1) is None and p["fx_last_why"] == 1 << 23 and p["fx_spill_full"] == 1  # (read on a fall-back only)


def test_unordered_is_learned_from_run_sorted_sweeps_only(host):
    assert Plan(host, RUN | BIN).learn(26, 100) is True  # runs * 4 > n
    assert Plan(host, RUN | BIN).learn(25, 100) is False
    assert Plan(host, RUN | BIN, unordered=1).learn(25, 100) is False
    assert Plan(host, RUN).learn(26, 100) is True
    for path in (BIN, WIDE | BIN, WIDE, 0):  # general or wide: nothing is learned
        assert Plan(host, path).learn(26, 100) is False
        assert Plan(host, path, unordered=1).learn(1, 100) is True
    assert Plan(host, RUN | BIN, unordered=1).learn(0, 100) is True  # no run count: nothing is learned


def test_quirk_the_fall_back_ignores_no_bucket_sort_and_sees_the_decremented_count(host):
    # the exact path's own start honours the option ...
    assert Plan(host).first(fx_ok=False, no_bucket_sort=True) == BIN
    # ... the default path's fall-back does not
    p = Plan(host)
    assert p.first(fx_ok=True, no_bucket_sort=True) == FX | BIN
    assert p.next(FX_FALLBACK) == RUN | BIN
    # general_calls = 1: a sweep that starts on the exact path takes the radix sort, one that falls back to it the run-binned sort
    p = Plan(host, general_calls=1)
    assert p.first(fx_ok=False) == BIN and p["general_calls"] == 0
    p = Plan(host, general_calls=1)
    assert p.first(fx_ok=True) == FX | BIN and p["general_calls"] == 0
    assert p.next(FX_FALLBACK) == RUN | BIN


def test_sizes(host):
    def sizes(n, max_layer=2, cluster_min=20, floor=0, last_splits=0):
        out = (C.c_uint64 * 5)()
        host.wc_host_ex_sizes(C.c_uint64(n), C.c_int(max_layer), C.c_int(cluster_min), C.c_uint64(floor), C.c_uint32(last_splits), out)
        return dict(zip(("slots", "bin_cap", "tiles", "ngrid", "g2"), [int(v) for v in out]))

    assert sizes(2880)["slots"] == 2880 * 3 // 20 + 1 == 433
    assert sizes(2880, floor=16 * 256)["slots"] == 4096  # the default path's floor
    assert sizes(1_000_000, floor=16 * 256)["slots"] == 150_001
    assert sizes(2880)["bin_cap"] == 64  # twice the mean count per time bin, 64 at least ...
    assert sizes(1_000_000)["bin_cap"] == 128  # 2 x 150 001 / 4096 = 73.2
    assert sizes(10_000_000)["bin_cap"] == 512  # ... kSlotBinMax at most
    assert [sizes(n)["tiles"] for n in (1, 1024, 1025, 125_000)] == [1, 1, 2, 123]
    assert [sizes(n)["ngrid"] for n in (64, 16_384, 100_000, 2_000_000)] == [64, 64, 390, 4096]
    assert sizes(100_000, last_splits=0)["g2"] == 64
    assert sizes(100_000, last_splits=256)["g2"] == 256
    assert sizes(100_000, last_splits=1000)["g2"] == 390  # never more than the sweep's node grid
    assert sizes(10_000_000, last_splits=5000)["g2"] == 2048
