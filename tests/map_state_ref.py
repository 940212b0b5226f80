"""Restatement, without a GPU, of the voxel map's exact state (include/wildcat_hip.h: wc_map_export_state, wc_map_absorb, wc_map_merge)
and of its canonical file (host/map_file.h): the state of a cloud from map_surfel_ref.voxel_sums, the absorb as integer
additions by key with the rejection rule, and the file format in numpy."""
import struct

import numpy as np

import map_query_ref as Q
import map_surfel_ref as S
from wildcat_slam_amd import records as R

MAX_COUNT = 2**30
HEADER = 64
MAGIC = b"WCMAPST1"
# wc_map_file::Decode's codes
OK, BAD_MAGIC, BAD_VERSION, BAD_FLAGS, BAD_RESERVED, BAD_VOXEL, BAD_LENGTH, BAD_CHECKSUM, BAD_POINTS, BAD_RECORD, BAD_ORDER = range(11)
MASK64 = 2**64 - 1


def state_of(xyz, v, moments=True):
    """the state of the map of a cloud -> (MAP_VOXEL array in ascending key order, (n, 9) int64 moment words U_x U_y U_z M_xx .. M_zz,
    or None with moments=False)"""
    s = S.voxel_sums(xyz, v)
    vox = np.zeros(len(s["count"]), R.MAP_VOXEL)
    vox["key"], vox["count"], vox["sum"] = s["keys"], s["count"], s["Q"]
    return vox, (np.concatenate([s["U"], s["M"]], axis=1).astype(np.int64) if moments else None)


def rejected(vox):
    """the records wc_map_absorb counts and does not apply: |key| >= 2^20 on an axis, count == 0, count > 2^30"""
    k = vox["key"].astype(np.int64)
    return np.any(np.abs(k) >= Q.KEY_LIM, axis=1) | (vox["count"] == 0) | (vox["count"].astype(np.int64) > MAX_COUNT)


def absorb_ref(state_list, moments=True):
    """[(vox, mom or None), ...] added up by key -> (vox, mom or None, records rejected): Python integers wrapped to 64 bits, as the
    table's two's-complement adds; the result in ascending key order"""
    acc, n_rej = {}, 0
    for vox, mom in state_list:
        bad = rejected(vox)
        n_rej += int(bad.sum())
        for i in np.flatnonzero(~bad):
            words = [int(vox["count"][i])] + [int(x) for x in vox["sum"][i]]
            if moments:
                words += [int(x) for x in mom[i]]
            key = tuple(int(x) for x in vox["key"][i])
            old = acc.get(key)
            acc[key] = words if old is None else [a + b for a, b in zip(old, words)]
    keys = sorted(acc)  # (tuples: ascending (kx, ky, kz))
    wrap = lambda x: ((x + 2**63) & MASK64) - 2**63  # noqa: E731
    out = np.zeros(len(keys), R.MAP_VOXEL)
    out_mom = np.zeros((len(keys), 9), np.int64) if moments else None
    for j, key in enumerate(keys):
        w = acc[key]
        out["key"][j], out["count"][j], out["sum"][j] = key, w[0], [wrap(x) for x in w[1:4]]
        if moments:
            out_mom[j] = [wrap(x) for x in w[4:13]]
    return out, out_mom, n_rej


def fnv1a64(data):
    h = 0xCBF29CE484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001B3) & MASK64
    return h


def encode_ref(voxel, vox, mom=None):
    """the canonical file of a state (mom not None: with moments) -> bytes; nothing is validated, as in wc_map_file::Encode"""
    vox = np.ascontiguousarray(vox, R.MAP_VOXEL)
    payload = vox.astype(R.MAP_VOXEL.newbyteorder("<")).tobytes()
    if mom is not None:
        payload += np.ascontiguousarray(mom, np.int64).astype("<i8").tobytes()
    points = int(vox["count"].astype(np.uint64).sum()) & MASK64
    head = MAGIC + struct.pack("<IIdQQQ", 1, 1 if mom is not None else 0, float(voxel), len(vox), points, fnv1a64(payload)) + bytes(16)
    assert len(head) == HEADER
    return head + payload


def decode_ref(data):
    """-> (code, voxel, flags, vox, mom): wc_map_file::Decode restated, its checks in its order; everything but the code is None unless
    the code is OK, and mom is None for a file without moments"""
    data = bytes(data)
    fail = lambda code: (code, None, None, None, None)  # noqa: E731
    if len(data) < HEADER:
        return fail(BAD_LENGTH)
    if data[:8] != MAGIC:
        return fail(BAD_MAGIC)
    version, flags, voxel, n, points, check = struct.unpack("<IIdQQQ", data[8:48])
    if version != 1:
        return fail(BAD_VERSION)
    if flags & ~1:
        return fail(BAD_FLAGS)
    if any(data[48:64]):
        return fail(BAD_RESERVED)
    if not (0.01 <= voxel <= 4.0):
        return fail(BAD_VOXEL)
    per = 40 + (72 if flags & 1 else 0)
    if n * per != len(data) - HEADER:
        return fail(BAD_LENGTH)
    payload = data[HEADER:]
    if fnv1a64(payload) != check:
        return fail(BAD_CHECKSUM)
    vox = np.frombuffer(payload, R.MAP_VOXEL.newbyteorder("<"), n).astype(R.MAP_VOXEL)
    bad = rejected(vox)
    packed = Q.pack(np.where(bad[:, None], 0, vox["key"].astype(np.int64)))
    unordered = np.zeros(n, bool)
    unordered[1:] = packed[1:] <= packed[:-1]
    # the first offending record decides, a rejected one before its order (an unordered record after a rejected one is not reached)
    first_bad = int(np.flatnonzero(bad)[0]) if bad.any() else n
    unordered[first_bad:] = False
    first_unordered = int(np.flatnonzero(unordered)[0]) if unordered.any() else n
    if first_bad < n or first_unordered < n:
        return fail(BAD_RECORD if first_bad <= first_unordered else BAD_ORDER)
    if int(vox["count"].astype(np.uint64).sum()) != points:
        return fail(BAD_POINTS)
    mom = np.frombuffer(payload, "<i8", 9 * n, 40 * n).astype(np.int64).reshape(-1, 9) if flags & 1 else None
    return OK, voxel, flags, vox, mom
