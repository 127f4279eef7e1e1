"""GPU box: device time of the ball morphology (vp_morph) on conservative grids, NAIVE and TILED on the same context, interleaved with
vp_csg on the same grid (a word-wise pass, 3 n^3/8 bytes: the streaming floor such a pass cannot beat), after warm-up.  Per row: the
mean device time of one call (hipEvent brackets per kernel, vp_prof_*) of TILED and of NAIVE, their ratio, the vp_csg pass and the ratio
of TILED to it.  The last row of each grid is the whole repair sequence dilate:4, fill, erode:4 (TILED; the fill is blocking).
  python tools/vox_morph.py [reps]        (default 5)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cuda_mesh_voxelization_amd import mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, MORPH_DILATE, MORPH_ERODE, OP_UNION, Frame
from cuda_mesh_voxelization_amd.pipeline import Engine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
eng = Engine(0)
ctx = eng.ctx


def timed(fn, keys):
    ctx.prof_reset(); ctx.prof_enable(True)
    fn()
    ctx.prof_enable(False)
    return sum(v["ms"] for k, v in ctx.prof().items() if k in keys)


cases = [("bunny x24", lambda: M.bunny(24), (512, 1024)),
         ("d20", lambda: M.import_mesh(M.asset("d20.obj")), (2048,))]
print("%-10s %5s %-14s | %10s %10s %8s | %9s %9s" % ("grid", "n", "op", "tiled ms", "naive ms", "naive/t", "csg ms", "tiled/csg"))
for label, load, sizes in cases:
    xyz, tri = load()
    dx, dt = eng.mesh_to_device(xyz, tri)
    for n in sizes:
        origin, vs = M.frame([xyz], n)
        fr = Frame.make(n, vs, origin)
        w = eng.voxelize_conservative(fr, dx, dt, algo=ALGO_TILED)
        nw = ~w
        out, a, b = eng.new_grid(fr), eng.new_grid(fr), eng.new_grid(fr)
        a.copy_(w); b.copy_(nw)
        for op, name, src in ((MORPH_DILATE, "dilate", w), (MORPH_ERODE, "erode", nw)):
            for r in (1, 2, 4, 8, 16):
                for algo in (ALGO_TILED, ALGO_NAIVE):                      # warm-up: tables uploaded, code loaded
                    eng.morph(fr, src, op, r, out=out, algo=algo)
                eng.csg(a, b, OP_UNION)
                eng.sync()
                tt = tn = tc = 0.0
                for _ in range(reps):                                       # interleaved: one of each per round
                    tt += timed(lambda: eng.morph(fr, src, op, r, out=out, algo=ALGO_TILED), ("morph",))
                    tn += timed(lambda: eng.morph(fr, src, op, r, out=out, algo=ALGO_NAIVE), ("morph_naive",))
                    tc += timed(lambda: eng.csg(a, b, OP_UNION), ("csg_words",))
                tt /= reps; tn /= reps; tc /= reps
                print("%-10s %5d %-14s | %10.4f %10.4f %8.2f | %9.4f %9.1f" % (label, n, "%s:%d" % (name, r), tt, tn, tn / tt, tc, tt / tc), flush=True)
        # the repair sequence (erode of a grid that is mostly solid, unlike the rows above)
        def repair(algo):
            d = eng.morph(fr, w, MORPH_DILATE, 4, out=out, algo=algo)
            f, _ = eng.fill_interior(fr, d, out=a)
            eng.morph(fr, f, MORPH_ERODE, 4, out=b, algo=algo)
        keys = ("morph", "morph_naive", "fill_x", "fill_y", "fill_z", "fill_final")
        repair(ALGO_TILED); repair(ALGO_NAIVE); eng.sync()
        tt = tn = tc = 0.0
        for _ in range(reps):
            tt += timed(lambda: repair(ALGO_TILED), keys)
            tn += timed(lambda: repair(ALGO_NAIVE), keys)
            tc += timed(lambda: eng.csg(a, b, OP_UNION), ("csg_words",))
        tt /= reps; tn /= reps; tc /= reps
        print("%-10s %5d %-14s | %10.4f %10.4f %8.2f | %9.4f %9.1f" % (label, n, "dil4,fill,ero4", tt, tn, tn / tt, tc, tt / tc), flush=True)
        del w, nw, out, a, b
        torch.cuda.empty_cache()
