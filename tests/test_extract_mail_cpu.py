"""The two mailbox words of the extraction's early count (csrc/extract_plan.h: ex_mail_*), without a GPU.  k_slot_emit stores them
as it starts - word A = ticket << 32 | count, word B = ticket << 32 | overflow << 31 | queued - and wc_extract_surfels_finish spins
until both carry the sweep's ticket.  The kernel and the host pack and unpack with the same constexpr functions; here they are
driven through their g++ instantiation in the facade library (host/odom_c_api.cc: wc_host_ex_mail_*)."""
import ctypes as C
import os

import pytest

from wildcat_slam_amd import lib

U32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def host():
    lib.load()
    so = os.path.join(os.path.dirname(lib.so_path()), "..", "host", "libwildcat_odometry.so")
    h = C.CDLL(os.path.abspath(so))
    h.wc_host_ex_mail_pack.restype = None
    h.wc_host_ex_mail_unpack.restype = C.c_int
    h.wc_host_ex_mail_next_ticket.restype = C.c_uint32
    return h


def pack(host, ticket, count, queued, overflow):
    out = (C.c_uint64 * 2)()
    host.wc_host_ex_mail_pack(C.c_uint32(ticket), C.c_uint32(count), C.c_uint32(queued), C.c_int(int(overflow)), out)
    return int(out[0]), int(out[1])


def unpack(host, a, b, ticket):
    """-> (arrived, count, queued, overflow)"""
    out = (C.c_uint32 * 3)()
    arrived = host.wc_host_ex_mail_unpack(C.c_uint64(a), C.c_uint64(b), C.c_uint32(ticket), out)
    return bool(arrived), int(out[0]), int(out[1]), bool(out[2])


@pytest.mark.parametrize("ticket", [1, 2, 0x7FFFFFFF, 0x80000000, U32])
@pytest.mark.parametrize("count", [0, 1, 31248, U32])
@pytest.mark.parametrize("queued", [0, 1, 4096, 0x7FFFFFFF])
@pytest.mark.parametrize("overflow", [False, True])
def test_round_trip(host, ticket, count, queued, overflow):
    a, b = pack(host, ticket, count, queued, overflow)
    assert a == (ticket << 32) | count
    assert b == (ticket << 32) | (int(overflow) << 31) | queued
    assert unpack(host, a, b, ticket) == (True, count, queued, overflow)


def test_a_queue_beyond_31_bits_saturates_and_leaves_the_flag_alone(host):
    for q in (0x80000000, U32):
        for overflow in (False, True):
            a, b = pack(host, 7, 5, q, overflow)
            assert unpack(host, a, b, 7) == (True, 5, 0x7FFFFFFF, overflow)


def test_arrival_needs_the_ticket_in_both_words(host):
    a, b = pack(host, 42, 1000, 3, False)
    a_old, b_old = pack(host, 41, 999, 0, True)  # the previous sweep's words
    assert unpack(host, a, b, 42)[0]
    assert not unpack(host, a_old, b, 42)[0]  # word A still the previous sweep's
    assert not unpack(host, a, b_old, 42)[0]  # word B still the previous sweep's
    assert not unpack(host, a_old, b_old, 42)[0]
    assert unpack(host, a_old, b_old, 41)[0]
    assert not unpack(host, 0, b, 42)[0]  # a mailbox never written
    assert not unpack(host, a, 0, 42)[0]
    assert not unpack(host, 0, 0, 42)[0]


def test_ticket_zero_never_arrives(host):
    assert not unpack(host, 0, 0, 0)[0]  # "no ticket" against a fresh mailbox
    a, b = pack(host, 0, 12, 1, False)
    assert not unpack(host, a, b, 0)[0]
    # count and queue length in the lower halves never pass for a ticket
    a, b = pack(host, 9, U32, 0x7FFFFFFF, True)
    assert not unpack(host, a, b, U32)[0] and not unpack(host, a, b, 0x7FFFFFFF)[0]


def test_the_sequence_skips_zero_on_wrap(host):
    nxt = host.wc_host_ex_mail_next_ticket
    assert nxt(C.c_uint32(0)) == 1  # a fresh context's first ticket
    assert nxt(C.c_uint32(1)) == 2
    assert nxt(C.c_uint32(U32 - 1)) == U32
    assert nxt(C.c_uint32(U32)) == 1  # not 0: 0 means "no ticket"
    t = U32 - 2
    seen = []
    for _ in range(5):
        t = nxt(C.c_uint32(t))
        seen.append(t)
    assert seen == [U32 - 1, U32, 1, 2, 3] and 0 not in seen
