"""GPU box: device time of the conservative surface voxelizer (vp_voxelize_conservative, TILED) per kernel, interleaved with the solid
TILED voxelizer on the same mesh, frame and context, after warm-up.  Per case: the mean device time of both (hipEvent brackets per
kernel, vp_prof_*), the ratio, the kernel table of the conservative run, and TILED == NAIVE of the conservative grid.
  python tools/vox_conservative.py [reps]        (default 20)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cuda_mesh_voxelization_amd import mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame
from cuda_mesh_voxelization_amd.pipeline import Engine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
eng = Engine(0)
ctx = eng.ctx
cases = [("bunny x24", lambda: M.bunny(24), (512, 1024)),
         ("d20", lambda: M.import_mesh(M.asset("d20.obj")), (512, 1024, 2048)),
         ("bimba", lambda: M.import_mesh(M.asset("bimba.obj")), (512, 1024, 2048))]
print("%-10s %9s %5s | %10s %10s %6s | %s" % ("mesh", "faces", "n", "cvox ms", "solid ms", "ratio", "conservative kernels: ms per call (launches per call)"))
for label, load, sizes in cases:
    xyz, tri = load()
    dx, dt = eng.mesh_to_device(xyz, tri)
    for n in sizes:
        origin, vs = M.frame([xyz], n)
        fr = Frame.make(n, vs, origin)
        gc = eng.new_grid(fr)
        gs = eng.new_grid(fr)

        def cvox():
            eng.voxelize_conservative(fr, dx, dt, out=gc, algo=ALGO_TILED)

        def solid():
            eng.voxelize(fr, dx, dt, out=gs, algo=ALGO_TILED)
        for _ in range(3):                                          # warm-up: workspaces grown, counts landed
            cvox(); solid()
        eng.sync()
        tc = ts = 0.0
        table = {}
        for _ in range(reps):                                       # interleaved: one of each per round
            ctx.prof_reset(); ctx.prof_enable(True); cvox(); ctx.prof_enable(False)
            p = ctx.prof()
            tc += sum(v["ms"] for v in p.values())
            for k, v in p.items():
                t = table.setdefault(k, [0.0, 0])
                t[0] += v["ms"]; t[1] += v["launches"]
            ctx.prof_reset(); ctx.prof_enable(True); solid(); ctx.prof_enable(False)
            ts += sum(v["ms"] for v in ctx.prof().values())
        tc /= reps; ts /= reps
        words = eng.words_to_numpy(gc).copy()
        eng.voxelize_conservative(fr, dx, dt, out=gc, algo=ALGO_NAIVE)
        eng.sync()
        same = np.array_equal(words, eng.words_to_numpy(gc))
        kern = "  ".join("%s %.4f (%d)" % (k, v[0] / reps, v[1] // reps) for k, v in table.items())
        print("%-10s %9d %5d | %10.4f %10.4f %6.2f | %s  set %d  tiled==naive %s" %
              (label, tri.shape[0], n, tc, ts, tc / ts, kern, int(np.unpackbits(words.view(np.uint8)).sum()), same), flush=True)
        del gc, gs, words
        torch.cuda.empty_cache()
