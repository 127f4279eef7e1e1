"""GPU box: device time of the interior fill (vp_fill_interior) on conservative grids, interleaved with the conservative voxelizer
(TILED) on the same mesh, frame and context, after warm-up.  Per case: the mean device time of the fill (hipEvent brackets per kernel,
vp_prof_*), the host wall time of the blocking call, its rounds, the nominal bytes per round (a round = three sweeps, each reading W and E
and writing E: 9 n^3/8 bytes) over the fill's kernel time, the kernel table of the fill, and the conservative time for scale.
  python tools/vox_fill.py [reps]        (default 10)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch

from cuda_mesh_voxelization_amd import mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_TILED, Frame
from cuda_mesh_voxelization_amd.pipeline import Engine
from fill_ref import maze

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
eng = Engine(0)
ctx = eng.ctx
FILL = ("fill_x", "fill_y", "fill_z", "fill_final")


def round_bytes(n):
    return 9 * n ** 3 // 8


cases = [("bunny x24", lambda: M.bunny(24), (512, 1024)),
         ("bimba", lambda: M.import_mesh(M.asset("bimba.obj")), (1024, 2048)),
         ("d20", lambda: M.import_mesh(M.asset("d20.obj")), (2048,)),
         ("maze", None, (1024,))]
print("%-10s %5s | %9s %9s %6s %9s | %9s | %s" % ("grid", "n", "fill ms", "wall ms", "rounds", "GB/s/rnd", "cvox ms",
                                                   "fill kernels: ms per call (launches per call)"))
for label, load, sizes in cases:
    for n in sizes:
        if load is None:                                            # the worst case: a serpentine corridor, no mesh
            words, _ = maze(n, seed=n)
            fr = Frame.make(n, 1.0 / n, np.zeros(3, np.float32))
            gc = torch.from_numpy(words.view(np.int32)).to(eng.device)

            def cvox():
                pass
        else:
            xyz, tri = load()
            dx, dt = eng.mesh_to_device(xyz, tri)
            origin, vs = M.frame([xyz], n)
            fr = Frame.make(n, vs, origin)
            gc = eng.new_grid(fr)

            def cvox():
                eng.voxelize_conservative(fr, dx, dt, out=gc, algo=ALGO_TILED)
        gf = eng.new_grid(fr)
        cvox()
        for _ in range(2):                                          # warm-up: flag ring and pinned copy allocated, code loaded
            eng.fill_interior(fr, gc, out=gf)
        eng.sync()
        tf = tw = tc = 0.0
        rounds = 0
        table = {}
        for _ in range(reps):                                       # interleaved: one of each per round
            ctx.prof_reset(); ctx.prof_enable(True)
            t0 = time.perf_counter()
            _, rounds = eng.fill_interior(fr, gc, out=gf)           # blocking: returns with the stream idle
            tw += time.perf_counter() - t0
            ctx.prof_enable(False)
            p = ctx.prof()
            tf += sum(v["ms"] for k, v in p.items() if k in FILL)
            for k, v in p.items():
                t = table.setdefault(k, [0.0, 0])
                t[0] += v["ms"]; t[1] += v["launches"]
            ctx.prof_reset(); ctx.prof_enable(True); cvox(); ctx.prof_enable(False)
            tc += sum(v["ms"] for v in ctx.prof().values())
        tf /= reps; tw = 1e3 * tw / reps; tc /= reps
        gbs = round_bytes(n) * rounds / (tf * 1e-3) / 1e9
        kern = "  ".join("%s %.4f (%d)" % (k, v[0] / reps, v[1] // reps) for k, v in table.items())
        print("%-10s %5d | %9.4f %9.3f %6d %9.0f | %9.4f | %s" % (label, n, tf, tw, rounds, gbs, tc, kern), flush=True)
        del gc, gf
        torch.cuda.empty_cache()
