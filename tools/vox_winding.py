"""GPU box: device time of the generalized winding number (vp_winding) at level 0.5 for d20, bimba, bunny and the bench bunny x 24 at
n = 256 and 512, with beta = 0 (every triangle exactly) and beta = 2 (far field): VP_ALGO_TILED split by timing key and VP_ALGO_NAIVE,
after warm-up, the mean over the rounds (hipEvent brackets per kernel, vp_prof_*; the stages book under the keys of the corresponding
mesh-distance stages).  A combination whose exact terms exceed `cap` (default 2e12) is skipped: beta = 0 is n^3 x T terms.
  python tools/vox_winding.py [reps] [cap]        (default 3)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cuda_mesh_voxelization_amd import mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame
from cuda_mesh_voxelization_amd.pipeline import Engine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
cap = float(sys.argv[2]) if len(sys.argv) > 2 else 2e12
eng = Engine(0)
ctx = eng.ctx
SETUP = ("md_setup", "md_scan", "md_write", "md_count")
TILED = SETUP + ("md_brick",)
NAIVE = SETUP + ("md_naive",)


def timed(fn):
    ctx.prof_reset(); ctx.prof_enable(True)
    fn()
    ctx.prof_enable(False)
    return {k: v["ms"] for k, v in ctx.prof().items()}


def meshes():
    yield ("d20",) + M.import_mesh(M.asset("d20.obj"))
    yield ("bimba",) + M.import_mesh(M.asset("bimba.obj"))
    yield ("bunny",) + M.import_mesh(M.asset("bunny.obj"))
    yield ("bunny x24",) + M.bunny(24)


print("%-10s %9s %5s %4s | %9s = %s | %9s = %s | %9s" %
      ("mesh", "triangles", "n", "beta", "tiled ms", " + ".join(k[3:] for k in TILED), "naive ms", " + ".join(k[3:] for k in NAIVE), "inside"))
for label, xyz, tri in meshes():
    dx, dt = eng.mesh_to_device(xyz, tri)
    for n in (256, 512):
        origin, vs = M.frame([xyz], n)
        fr = Frame.make(n, vs, origin)
        for beta in (0.0, 2.0):
            if beta == 0.0 and float(n) ** 3 * tri.shape[0] > cap:
                print("%-10s %9d %5d %4g | skipped: %.2g exact terms" % (label, tri.shape[0], n, beta, float(n) ** 3 * tri.shape[0]), flush=True)
                continue

            def run(algo, count=False): return ctx.winding(fr, dx.data_ptr(), dx.shape[0], dt.data_ptr(), dt.shape[0], beta, 0.5, algo, count=count)
            inside = run(ALGO_TILED, True)                                              # warm-up: buffers grown, code loaded
            run(ALGO_NAIVE)
            eng.sync()
            acc = {}
            for _ in range(reps):                                                        # interleaved: one of each per round
                for tag, algo in (("t", ALGO_TILED), ("n", ALGO_NAIVE)):
                    for key, val in timed(lambda: run(algo)).items(): acc[(tag, key)] = acc.get((tag, key), 0.0) + val
            t = {k: v / reps for k, v in acc.items()}
            tt = sum(t.get(("t", k), 0.0) for k in TILED)
            tn = sum(t.get(("n", k), 0.0) for k in NAIVE)
            print("%-10s %9d %5d %4g | %9.3f = %s | %9.3f = %s | %9d" %
                  (label, tri.shape[0], n, beta, tt, " + ".join("%.3f" % t.get(("t", k), 0.0) for k in TILED), tn,
                   " + ".join("%.3f" % t.get(("n", k), 0.0) for k in NAIVE), inside), flush=True)
        ctx.release()
        torch.cuda.empty_cache()
