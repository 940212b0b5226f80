"""The voxel map's exact state without a GPU: the restatement of map_state_ref.py against itself (the states of any split
of a cloud add up to the state of the cloud), and the canonical file's C++ codec (host/map_file.h, exported from the facade library as
wc_host_map_file_encode / wc_host_map_file_decode) against the numpy one - bytes, round trip, the committed v1 fixture, and every way
of refusing a file, each by its return code."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import map_state_ref as MS
from helpers import xyz_of
from wildcat_slam_amd import records as R
from wildcat_slam_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "map_state_v1.bin")
GOLDEN_V = 0.2


@pytest.fixture(scope="module")
def host():
    from wildcat_slam_amd import lib

    lib.load()
    h = C.CDLL(os.path.join(HERE, "..", "wildcat-slam_amd", "host", "libwildcat_odometry.so"))
    h.wc_host_map_file_encode.restype = C.c_uint64
    return h


@pytest.fixture(scope="module")
def cloud():
    return xyz_of(synth.g1_room(20000, seed=3))


def cxx_encode(host, voxel, vox, mom):
    vox = np.ascontiguousarray(vox, R.MAP_VOXEL)
    flags = C.c_uint32(1 if mom is not None else 0)
    m = np.ascontiguousarray(mom, np.int64) if mom is not None else None
    args = (C.c_double(voxel), flags, R.ptr(vox) if len(vox) else None, R.ptr(m) if m is not None and len(vox) else None, C.c_uint64(len(vox)))
    size = int(host.wc_host_map_file_encode(*args, None, C.c_uint64(0)))
    out = np.zeros(size, np.uint8)
    assert int(host.wc_host_map_file_encode(*args, R.ptr(out), C.c_uint64(size))) == size
    return out.tobytes()


def cxx_decode(host, data):
    """-> (code, voxel, flags, vox, mom) as map_state_ref.decode_ref.  The decoder sees a heap copy of exactly len(data) bytes"""
    buf = np.frombuffer(bytes(data), np.uint8).copy() if len(data) else np.zeros(0, np.uint8)
    voxel, flags, n = C.c_double(0), C.c_uint32(0), C.c_uint64(0)
    p = R.ptr(buf) if len(buf) else None
    code = host.wc_host_map_file_decode(p, C.c_uint64(len(buf)), C.byref(voxel), C.byref(flags), C.byref(n), None, None, C.c_uint64(0))
    if code != MS.OK:
        return code, None, None, None, None
    vox = np.zeros(n.value, R.MAP_VOXEL)
    mom = np.zeros((n.value, 9), np.int64) if flags.value & 1 else None
    code = host.wc_host_map_file_decode(p, C.c_uint64(len(buf)), None, None, None, R.ptr(vox) if n.value else None,
                                        R.ptr(mom) if mom is not None and n.value else None, C.c_uint64(n.value))
    return code, voxel.value, flags.value, vox, mom


def same_state(a, b):
    return a[0].tobytes() == b[0].tobytes() and ((a[1] is None and b[1] is None) or a[1].tobytes() == b[1].tobytes())


@pytest.mark.parametrize("v", [0.2, 0.05, float(np.float32(0.8))])
def test_states_of_a_split_add_up_to_the_state_of_the_cloud(cloud, v):
    whole = MS.state_of(cloud, v)
    rng = np.random.default_rng(11)
    part = rng.integers(0, 3, len(cloud))
    for pieces in ([cloud[0::2], cloud[1::2]], [cloud[:7001], cloud[7001:]], [cloud[part == j] for j in range(3)]):
        vox, mom, rej = MS.absorb_ref([MS.state_of(p, v) for p in pieces])
        assert rej == 0 and same_state((vox, mom), whole)
    vox, mom, rej = MS.absorb_ref([MS.state_of(p, v, moments=False) for p in (cloud[0::2], cloud[1::2])], moments=False)
    assert rej == 0 and mom is None and vox.tobytes() == whole[0].tobytes()


def test_absorb_ref_rejects_and_wraps():
    vox = np.zeros(6, R.MAP_VOXEL)
    vox["key"] = [[1, 2, 3], [2**20, 0, 0], [0, -(2**20), 0], [1, 2, 3], [4, 4, 4], [5, 5, 5]]
    vox["count"] = [2, 1, 1, 3, 0, 2**30 + 1]
    vox["sum"][0] = [2**63 - 1, -5, 7]
    vox["sum"][3] = [1, 5, -7]
    out, mom, rej = MS.absorb_ref([(vox, None)], moments=False)
    assert rej == 4 and mom is None and len(out) == 1
    assert out["key"][0].tolist() == [1, 2, 3] and out["count"][0] == 5 and out["sum"][0].tolist() == [-(2**63), 0, 0]
    vox["count"][5] = 2**30
    assert MS.absorb_ref([(vox, None)], moments=False)[2] == 3


@pytest.mark.parametrize("moments", [True, False])
def test_cxx_encoder_writes_the_numpy_encoders_bytes_and_decode_inverts_it(host, cloud, moments):
    for v, pts in ((0.2, cloud), (0.05, cloud[:3000]), (0.8, cloud[:0])):
        vox, mom = MS.state_of(pts, v, moments) if len(pts) else (np.zeros(0, R.MAP_VOXEL), np.zeros((0, 9), np.int64) if moments else None)
        ref = MS.encode_ref(v, vox, mom)
        assert len(ref) == 64 + len(vox) * (112 if moments else 40)
        assert cxx_encode(host, v, vox, mom) == ref
        for dec in (cxx_decode(host, ref), MS.decode_ref(ref)):
            assert dec[0] == MS.OK and dec[1] == v and dec[2] == (1 if moments else 0) and same_state((dec[3], dec[4]), (vox, mom))


def golden_state():
    """the fixture's content: a handful of voxels with moments - negative keys, both ends of the key range, a full count, sums of
    either sign"""
    pts = np.array([[0.05, 0.05, 0.05], [0.15, 0.1, 0.05], [0.07, 0.11, 0.19], [-0.05, -0.3, 0.61], [-0.01, -0.21, 0.7], [3.1, -2.2, 0.45]], np.float32)
    vox, mom = MS.state_of(pts, GOLDEN_V)
    edge = np.zeros(2, R.MAP_VOXEL)
    edge["key"], edge["count"] = [[-(2**20) + 1, 0, 5], [2**20 - 1, 2**20 - 1, -(2**20) + 1]], [2**30, 1]
    edge["sum"] = [[-(2**61), 2**61, -1], [123456789, -987654321, 0]]
    edge_mom = np.array([[-(2**45), 2**45, 3, 2**62, -(2**40), 0, 2**62, 1, 2**62], [7, -8, 9, 49, -56, 63, 64, -72, 81]], np.int64)
    return MS.absorb_ref([(vox, mom), (edge, edge_mom)])[:2]


def test_golden_fixture_pins_format_v1(host):
    data = open(GOLDEN, "rb").read()
    vox, mom = golden_state()
    assert data == MS.encode_ref(GOLDEN_V, vox, mom) and len(data) == 64 + 112 * len(vox) and 4 <= len(vox) <= 8
    assert data[:8] == b"WCMAPST1" and struct.unpack("<II", data[8:16]) == (1, 1)
    for dec in (cxx_decode(host, data), MS.decode_ref(data)):
        assert dec[0] == MS.OK and dec[1] == GOLDEN_V and same_state((dec[3], dec[4]), (vox, mom))
    dec = cxx_decode(host, data)
    assert cxx_encode(host, dec[1], dec[3], dec[4]) == data


def refused(host, data, code, what):
    got = cxx_decode(host, data)[0]
    assert got == code, (what, got, code)
    assert MS.decode_ref(data)[0] == code, what


def with_payload(data, payload):
    """the file with another payload and the checksum of that payload: what remains wrong is the payload's content"""
    return data[:40] + struct.pack("<Q", MS.fnv1a64(payload)) + data[48:64] + payload


def test_decoder_refuses_every_truncation_and_a_trailing_byte(host):
    data = open(GOLDEN, "rb").read()
    for cut in range(len(data)):
        refused(host, data[:cut], MS.BAD_LENGTH, ("truncated to", cut))
    refused(host, data + b"\0", MS.BAD_LENGTH, "a trailing byte")
    refused(host, b"", MS.BAD_LENGTH, "empty")


def test_decoder_refuses_a_flipped_bit_in_each_header_field_and_in_the_payload(host):
    data = open(GOLDEN, "rb").read()

    def flip(byte, bit):
        b = bytearray(data)
        b[byte] ^= 1 << bit
        return bytes(b)

    for byte in range(8):
        refused(host, flip(byte, 0), MS.BAD_MAGIC, ("magic", byte))
    for byte in range(8, 12):
        refused(host, flip(byte, 1), MS.BAD_VERSION, ("version", byte))
    refused(host, flip(12, 0), MS.BAD_LENGTH, "flags bit 0: the file has moments its flags deny")
    for byte, bit in ((12, 1), (12, 7), (13, 0), (15, 7)):
        refused(host, flip(byte, bit), MS.BAD_FLAGS, ("flags", byte, bit))
    # the voxel: sign, the exponent's top bits (the mantissa is not covered by the checksum: another valid size is another map, which
    # LoadMap refuses by comparing the size with its own)
    for byte, bit in ((23, 7), (23, 6), (23, 5), (23, 0)):
        refused(host, flip(byte, bit), MS.BAD_VOXEL, ("voxel", byte, bit))
    for byte in range(24, 32):
        refused(host, flip(byte, 0), MS.BAD_LENGTH, ("n", byte))
    for byte in range(32, 40):
        refused(host, flip(byte, 3), MS.BAD_POINTS, ("points", byte))
    for byte in range(40, 48):
        refused(host, flip(byte, 5), MS.BAD_CHECKSUM, ("checksum", byte))
    for byte in range(48, 64):
        refused(host, flip(byte, 2), MS.BAD_RESERVED, ("reserved", byte))
    for byte in (64, 64 + 12, 64 + 16, 64 + 39, 64 + 40 * 3 + 5, len(data) - 72, len(data) - 1):
        for bit in (0, 7):
            refused(host, flip(byte, bit), MS.BAD_CHECKSUM, ("payload", byte, bit))
    nan = data[:16] + struct.pack("<d", float("nan")) + data[24:]
    refused(host, nan, MS.BAD_VOXEL, "NaN")
    for v, code in ((0.01, MS.OK), (4.0, MS.OK), (0.009999, MS.BAD_VOXEL), (4.0000001, MS.BAD_VOXEL), (0.0, MS.BAD_VOXEL)):
        refused(host, data[:16] + struct.pack("<d", v) + data[24:], code, ("voxel", v))


def test_decoder_refuses_what_the_absorb_would_reject_and_what_is_not_canonical(host):
    vox, mom = golden_state()
    n = len(vox)

    def file_of(v, m):
        return MS.encode_ref(GOLDEN_V, v, m)

    swapped = np.arange(n)
    swapped[[1, 2]] = [2, 1]
    refused(host, file_of(vox[swapped], mom[swapped]), MS.BAD_ORDER, "swapped records")
    refused(host, file_of(vox[::-1], mom[::-1]), MS.BAD_ORDER, "descending")
    dup = np.array([0, 1, 1, 2])
    refused(host, file_of(vox[dup], mom[dup]), MS.BAD_ORDER, "a duplicate key")
    for axis in range(3):  # ascending in x alone is not enough: the later axes decide among equal earlier ones
        two = vox[:2].copy()
        two["key"] = 7
        two["key"][0][axis] = 8
        refused(host, file_of(two, mom[:2]), MS.BAD_ORDER, ("axis", axis))
        refused(host, file_of(two[::-1], mom[:2]), MS.OK, ("axis", axis))
    zero = vox.copy()
    zero["count"][2] = 0
    refused(host, file_of(zero, mom), MS.BAD_RECORD, "count 0")
    full = vox.copy()
    full["count"][2] = 2**30 + 1
    refused(host, file_of(full, mom), MS.BAD_RECORD, "count 2^30 + 1")
    for axis in range(3):
        for k, last in ((2**20, n - 1), (-(2**20), 0)):
            far = vox.copy()
            far["key"][last][axis] = k
            refused(host, file_of(far, mom), MS.BAD_RECORD, ("key", k, axis))
    # a right checksum over a payload whose points do not add up to the header's
    more = vox.copy()
    more["count"][1] += 1
    data = file_of(vox, mom)
    refused(host, with_payload(data, file_of(more, mom)[64:]), MS.BAD_POINTS, "points")
    # version 2, and a version-1 file of a plain state with the moments flag set
    refused(host, data[:8] + struct.pack("<I", 2) + data[12:], MS.BAD_VERSION, "version 2")
    plain = file_of(vox, None)
    refused(host, plain, MS.OK, "plain")
    refused(host, plain[:12] + struct.pack("<I", 1) + plain[16:], MS.BAD_LENGTH, "moments flag on a plain payload")


def test_header_declares_the_state_calls_and_the_libraries_export_them(host):
    from wildcat_slam_amd import lib

    declared = set(lib.declared_symbols())
    l = lib.load()
    for s in ("wc_map_export_state", "wc_map_absorb", "wc_map_merge"):
        assert s in declared and hasattr(l, s), s
    for s in ("wc_host_map_file_encode", "wc_host_map_file_decode", "wc_odom_map_save", "wc_odom_map_load"):
        assert hasattr(host, s), s
    assert R.MAP_VOXEL.itemsize == 40
