"""GPU box: time of the geodesic distance (vp_geodesic) inside bunny's solid grid at n = 256 and 512 from the seeds of its lowest occupied z
plane, the three metrics, VP_ALGO_NAIVE against VP_ALGO_TILED, interleaved in one process after warm-up, the mean over the rounds.
vp_geodesic blocks (convergence is read back), so a call is timed by the wall clock around it, read-backs included.  Rounds and launches
come from the timing table: NAIVE's rounds are its md_naive launches (the last batch runs to its end, the rounds after the fixed point
return at once), TILED's rounds its md_brick launches.  Beside them the time of nine copies of the grid, the yardstick of the other tools:
a floor for one pass over the bit grid, 32 times below one pass over D.
  python tools/vox_geodesic.py [reps]        (default 3)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cuda_mesh_voxelization_amd import mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, GEO_6, GEO_26, GEO_CHAMFER, Frame
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


def launches(fn):
    ctx.prof_reset()
    ctx.prof_enable(True)
    fn()
    ctx.prof_enable(False)
    return {k: v["launches"] for k, v in ctx.prof().items()}


print("%-6s %4s %-7s %-5s | %7s %9s %7s | %9s %7s %9s | %9s" %
      ("mesh", "n", "metric", "algo", "seeds", "reached", "max D", "call ms", "rounds", "ms/round", "9 copies"))
xyz, tri = M.import_mesh(M.asset("bunny.obj"))
dx, dt = eng.mesh_to_device(xyz, tri)
for n in (256, 512):
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    w = eng.voxelize(fr, dx, dt)
    planes = w.view(n, -1)                                                               # one row of words per z plane
    zmin = int(torch.nonzero((planes != 0).any(dim=1))[0])
    seeds = torch.zeros_like(w)
    seeds.view(n, -1)[zmin] = planes[zmin]
    tmp = torch.empty_like(w)
    nbytes = w.numel() * 4

    def copies():
        for _ in range(9):
            ctx.stream_copy(tmp.data_ptr(), w.data_ptr(), nbytes)
    copies()
    nine = sum(wall(copies)[0] for _ in range(reps)) / reps
    for metric, mname in ((GEO_6, "6"), (GEO_26, "26"), (GEO_CHAMFER, "chamfer")):
        stats, rounds = {}, {}
        for algo, key in ((ALGO_NAIVE, "md_naive"), (ALGO_TILED, "md_brick")):           # warm-up: buffers grown, code loaded
            stats[algo] = ctx.geodesic(fr, w.data_ptr(), seeds.data_ptr(), metric, algo)
            rounds[algo] = launches(lambda: ctx.geodesic(fr, w.data_ptr(), seeds.data_ptr(), metric, algo))[key]
        assert stats[ALGO_NAIVE] == stats[ALGO_TILED]
        full = {ALGO_NAIVE: 0.0, ALGO_TILED: 0.0}
        for _ in range(reps):                                                            # interleaved: one of each per round
            for algo in (ALGO_NAIVE, ALGO_TILED):
                full[algo] += wall(lambda: ctx.geodesic(fr, w.data_ptr(), seeds.data_ptr(), metric, algo))[0] / reps
        for algo, aname in ((ALGO_NAIVE, "naive"), (ALGO_TILED, "tiled")):
            used, reached, top, _ = stats[algo]
            print("%-6s %4d %-7s %-5s | %7d %9d %7d | %9.3f %7d %9.4f | %9.4f" %
                  ("bunny", n, mname, aname, used, reached, top, full[algo], rounds[algo], full[algo] / rounds[algo], nine), flush=True)
        print("%-6s %4d %-7s naive / tiled = %.2f" % ("bunny", n, mname, full[ALGO_NAIVE] / full[ALGO_TILED]), flush=True)
    del w, tmp, seeds
    ctx.release()
    torch.cuda.empty_cache()
