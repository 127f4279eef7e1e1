"""GPU box: time of the topological thinning (vp_skeleton) of bunny's solid grid at n = 256, 512 and 1024, both modes, VP_ALGO_NAIVE against
VP_ALGO_TILED, interleaved in one process after warm-up, the mean over the rounds.  vp_skeleton blocks (the deleted count of every
iteration is read back), so a call is timed by the wall clock around it, read-backs included.  Per iteration: the mean over the whole run,
over its first half (a run stopped by max_iters) and over its second half (the difference), beside the time of nine copies of the grid --
the floor of a nine-launch iteration that touches every word, which the list of active blocks is there to go below.
  python tools/vox_skeleton.py [reps]        (default 3)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cuda_mesh_voxelization_amd import mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, SKEL_CURVE, SKEL_KERNEL, Frame
from cuda_mesh_voxelization_amd.pipeline import Engine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
eng = Engine(0)
ctx = eng.ctx


def wall(fn):
    eng.sync()
    t = time.perf_counter()
    out = fn()
    eng.sync()
    return (time.perf_counter() - t) * 1e3, out


print("%-6s %4s %-6s %-5s | %8s %6s %8s | %9s | %8s %8s %8s | %9s" %
      ("mesh", "n", "mode", "algo", "voxels", "iters", "deleted", "call ms", "ms/iter", "1st half", "2nd half", "9 copies"))
xyz, tri = M.import_mesh(M.asset("bunny.obj"))
dx, dt = eng.mesh_to_device(xyz, tri)
for n in (256, 512, 1024):
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    w = eng.voxelize(fr, dx, dt)
    tmp = torch.empty_like(w)
    nbytes = w.numel() * 4

    def copies():
        for _ in range(9):
            ctx.stream_copy(tmp.data_ptr(), w.data_ptr(), nbytes)
    copies()
    nine = sum(wall(copies)[0] for _ in range(reps)) / reps
    for mode, mname in ((SKEL_KERNEL, "kernel"), (SKEL_CURVE, "curve")):
        stats = {}
        for algo in (ALGO_NAIVE, ALGO_TILED):                                            # warm-up: buffers grown, code loaded
            stats[algo] = ctx.skeleton(fr, w.data_ptr(), mode, 0, 0, algo)
        assert stats[ALGO_NAIVE] == stats[ALGO_TILED]
        left, iters, deleted = stats[ALGO_TILED]
        half = max(1, iters // 2)
        full = {ALGO_NAIVE: 0.0, ALGO_TILED: 0.0}
        part = {ALGO_NAIVE: 0.0, ALGO_TILED: 0.0}
        for _ in range(reps):                                                            # interleaved: one of each per round
            for algo in (ALGO_NAIVE, ALGO_TILED):
                full[algo] += wall(lambda: ctx.skeleton(fr, w.data_ptr(), mode, 0, 0, algo))[0] / reps
                part[algo] += wall(lambda: ctx.skeleton(fr, w.data_ptr(), mode, half, 0, algo))[0] / reps
        for algo, aname in ((ALGO_NAIVE, "naive"), (ALGO_TILED, "tiled")):
            print("%-6s %4d %-6s %-5s | %8d %6d %8d | %9.3f | %8.4f %8.4f %8.4f | %9.4f" %
                  ("bunny", n, mname, aname, left, iters, deleted, full[algo], full[algo] / iters, part[algo] / half,
                   (full[algo] - part[algo]) / max(1, iters - half), nine), flush=True)
    del w, tmp
    ctx.release()
    torch.cuda.empty_cache()
