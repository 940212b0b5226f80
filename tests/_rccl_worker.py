"""The in-library RCCL communicator with a world of one (csrc/comm.hip), in a process of its own (tests/test_route_gpu.py starts it):
librccl.so is dlopen()ed, ncclCommInitRank with one rank, and the sharded extraction + gather run their collectives (grouped
ncclSend / ncclRecv to self on the ctx stream) through it - the result is the plain call's, byte for byte.  Usage: python _rccl_worker.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "wildcat-slam_amd", "python"), HERE]

from test_route_gpu import _mixed_cloud  # noqa: E402
from wildcat_slam_amd import lib  # noqa: E402


def main():
    plain = lib.Context(0)
    ctx = lib.Context(0)
    try:
        uid = lib.rccl_unique_id()
        assert len(uid) == 128
        ctx.comm_rccl_init(0, 1, uid)
        pts = _mixed_cloud(150, 60_000, seed=21)
        s_ref, i_ref = plain.extract_surfels(pts)
        d_pts = ctx.to_device(pts)
        d_s, d_i, m, owned = ctx.extract_surfels_sharded(d_pts, len(pts), float(pts["time"][0]), float(pts["time"][-1]))
        assert owned == len(pts) and m == len(s_ref)
        ms, mi = ctx.gather_surfels(d_s, d_i, m, cap=m + 16)
        assert mi.tobytes() == i_ref.tobytes() and ms.tobytes() == s_ref.tobytes()
        ctx.comm_rccl_destroy()
    finally:
        ctx.close()
        plain.close()
    print("rccl world of one ok")


if __name__ == "__main__":
    main()
