"""GPU box: time of the extended maxima (vp_extrema) of bunny's solid grid at n = 256 and 512 -- D^2 from vp_edt (UNSET seeds), VP_EXT_SQRT16,
h = 8 sixteenths of a voxel, both connectivities -- VP_ALGO_NAIVE against VP_ALGO_TILED, interleaved in one process after warm-up, the mean
over the rounds.  vp_extrema blocks (convergence is read back), so a call is timed by the wall clock around it, read-backs included; a call
is two reconstructions.  Rounds come from the timing table: NAIVE's rounds are its md_naive launches (the last batch of each
reconstruction runs to its end, the rounds after the fixed point return at once), TILED's rounds its md_brick launches.  Beside them the
markers the maxima give (vp_components_label) and the time of nine copies of the grid, the yardstick of the other tools.
  python tools/vox_extrema.py [reps]        (default 3)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cuda_mesh_voxelization_amd import mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, CONN_6, CONN_26, EDT_SEEDS_UNSET, EXT_MAXIMA, EXT_SQRT16, Frame
from cuda_mesh_voxelization_amd.pipeline import Engine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
H16 = 8
eng = Engine(0)
ctx = eng.ctx


def wall(fn):
    eng.sync()
    t = time.perf_counter()
    out = fn()
    eng.sync()
    return (time.perf_counter() - t) * 1e3, out


def launches(fn):
    ctx.prof_reset()
    ctx.prof_enable(True)
    fn()
    ctx.prof_enable(False)
    return {k: v["launches"] for k, v in ctx.prof().items()}


print("%-6s %4s %-4s %-5s | %9s %8s %7s %7s | %9s %7s %9s | %9s" %
      ("mesh", "n", "conn", "algo", "solid", "maxima", "markers", "max H", "call ms", "rounds", "ms/round", "9 copies"))
xyz, tri = M.import_mesh(M.asset("bunny.obj"))
dx, dt = eng.mesh_to_device(xyz, tri)
for n in (256, 512):
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    w = eng.voxelize(fr, dx, dt)
    d2 = eng.edt(fr, w, EDT_SEEDS_UNSET)
    tmp = torch.empty_like(w)
    nbytes = w.numel() * 4

    def copies():
        for _ in range(9):
            ctx.stream_copy(tmp.data_ptr(), w.data_ptr(), nbytes)
    copies()
    nine = sum(wall(copies)[0] for _ in range(reps)) / reps
    for conn in (CONN_6, CONN_26):
        def call(algo):
            return ctx.extrema(fr, d2.data_ptr(), w.data_ptr(), EXT_MAXIMA, EXT_SQRT16, H16, conn, algo)
        stats, rounds, markers = {}, {}, {}
        for algo, key in ((ALGO_NAIVE, "md_naive"), (ALGO_TILED, "md_brick")):           # warm-up: buffers grown, code loaded
            stats[algo] = call(algo)
            rounds[algo] = launches(lambda: call(algo))[key]
            ext = torch.as_tensor(eng.extrema(fr, d2, w, EXT_MAXIMA, EXT_SQRT16, H16, conn, algo)[2]).clone()
            markers[algo] = eng.components_label(fr, ext, conn)[1]
        assert stats[ALGO_NAIVE] == stats[ALGO_TILED] and markers[ALGO_NAIVE] == markers[ALGO_TILED]
        full = {ALGO_NAIVE: 0.0, ALGO_TILED: 0.0}
        for _ in range(reps):                                                            # interleaved: one of each per round
            for algo in (ALGO_NAIVE, ALGO_TILED):
                full[algo] += wall(lambda: call(algo))[0] / reps
        for algo, aname in ((ALGO_NAIVE, "naive"), (ALGO_TILED, "tiled")):
            solid, maxima, top, _ = stats[algo]
            print("%-6s %4d %-4d %-5s | %9d %8d %7d %7d | %9.3f %7d %9.4f | %9.4f" %
                  ("bunny", n, conn, aname, solid, maxima, markers[algo], top, full[algo], rounds[algo], full[algo] / rounds[algo], nine), flush=True)
        print("%-6s %4d %-4d naive / tiled = %.2f" % ("bunny", n, conn, full[ALGO_NAIVE] / full[ALGO_TILED]), flush=True)
    del w, tmp, d2
    ctx.release()
    torch.cuda.empty_cache()
