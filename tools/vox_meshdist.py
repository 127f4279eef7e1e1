"""GPU box: device time of the mesh distance field (vp_mesh_distance), band 3, unsigned, with the nearest faces, for d20, bimba and the
bench bunny at n = 256, 512 and 1024: VP_ALGO_TILED split by timing key and VP_ALGO_NAIVE (its key volume is 8 n^3 bytes: 8 GiB at n = 1024, beside 8 GiB of outputs),
after warm-up, the mean over the rounds (hipEvent brackets per kernel, vp_prof_*).  Per row also the list length L -- the (triangle,
brick) pairs TILED listed -- and the (triangle, voxel) pairs per voxel that reach the per-pair bounds, 512 L / n^3.
  python tools/vox_meshdist.py [reps]        (default 5)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cuda_mesh_voxelization_amd import mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame
from cuda_mesh_voxelization_amd.pipeline import Engine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
BAND = 3
eng = Engine(0)
ctx = eng.ctx
TILED = ("md_setup", "md_scan", "md_count", "md_write", "md_brick", "md_fill")
NAIVE = ("md_prefill", "md_naive", "md_split")


def timed(fn):
    ctx.prof_reset(); ctx.prof_enable(True)
    fn()
    ctx.prof_enable(False)
    return {k: v["ms"] for k, v in ctx.prof().items()}


def meshes():
    yield ("d20",) + M.import_mesh(M.asset("d20.obj"))
    yield ("bimba",) + M.import_mesh(M.asset("bimba.obj"))
    yield ("bunny x24",) + M.bunny(24)


print("%-10s %9s %5s | %9s = %s | %9s = %s | %11s %10s" %
      ("mesh", "triangles", "n", "tiled ms", " + ".join(k[3:] for k in TILED), "naive ms", " + ".join(k[3:] for k in NAIVE), "list L", "pairs/voxel"))
for label, xyz, tri in meshes():
    dx, dt = eng.mesh_to_device(xyz, tri)
    for n in (256, 512, 1024):
        origin, vs = M.frame([xyz], n)
        fr = Frame.make(n, vs, origin)
        out = (torch.empty(fr.voxels, dtype=torch.float32, device=eng.device), torch.empty(fr.voxels, dtype=torch.int32, device=eng.device))

        def run(algo): eng.mesh_distance(fr, dx, dt, BAND, want_nearest=True, out=out, algo=algo)
        run(ALGO_TILED)                                                              # warm-up: buffers grown, code loaded
        entries = ctx.mesh_distance_list_entries()
        run(ALGO_NAIVE)
        eng.sync()
        acc = {}
        for _ in range(reps):                                                        # interleaved: one of each per round
            for tag, algo in (("t", ALGO_TILED), ("n", ALGO_NAIVE)):
                for key, val in timed(lambda: run(algo)).items(): acc[(tag, key)] = acc.get((tag, key), 0.0) + val
        t = {k: v / reps for k, v in acc.items()}
        tt = sum(t.get(("t", k), 0.0) for k in TILED)
        tn = sum(t.get(("n", k), 0.0) for k in NAIVE)
        print("%-10s %9d %5d | %9.3f = %s | %9.3f = %s | %11d %10.2f" %
              (label, tri.shape[0], n, tt, " + ".join("%.3f" % t.get(("t", k), 0.0) for k in TILED), tn,
               " + ".join("%.3f" % t.get(("n", k), float("nan")) for k in NAIVE), entries, 512.0 * entries / n ** 3), flush=True)
        del out
        ctx.release()
        torch.cuda.empty_cache()
