"""GPU box: device time of the local thickness (vp_thickness) of the solid grids of d20, bimba and bunny at n = 256 and 512 with
rmax = 4, 8 and 32: VP_ALGO_TILED split by timing key and VP_ALGO_NAIVE, interleaved in one process after warm-up, the mean over the rounds
(hipEvent brackets per kernel, vp_prof_*; the stages book under keys they share with vp_edt* and vp_mesh_distance).  Beside them: one
vp_edt (SEEDS_UNSET) of the same grid -- TILED runs two such transforms --, the share of the bricks th_brick owns (those with a set,
unsaturated voxel) and its share of the TILED time.  NAIVE costs the sum of the ball volumes; a row whose sum exceeds `cap` (default 2e10
pairs) is skipped and says so.
  python tools/vox_thickness.py [reps] [cap]        (default 3)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cuda_mesh_voxelization_amd import mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, EDT_SEEDS_UNSET, Frame
from cuda_mesh_voxelization_amd.pipeline import Engine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
cap = float(sys.argv[2]) if len(sys.argv) > 2 else 2e10
eng = Engine(0)
ctx = eng.ctx
EDT = ("edt_x", "edt_y", "edt_z")
TILED = EDT + ("edt_thresh", "md_brick", "md_fill")
NAIVE = ("edt_x", "edt_y_naive", "edt_z_naive", "md_naive", "edt_thresh")


def timed(fn):
    ctx.prof_reset(); ctx.prof_enable(True)
    fn()
    ctx.prof_enable(False)
    return {k: v["ms"] for k, v in ctx.prof().items()}


def pairs(fr, w, rmax):
    """the sum over the set voxels c of the number of voxels in the open ball of squared radius D(c), on the device"""
    n = fr.n
    e = eng.edt(fr, w, EDT_SEEDS_UNSET).view(n, n, n).to(torch.int64)
    a = torch.arange(n, device=eng.device)
    f = torch.minimum(a, n - 1 - a) + 1
    wall = torch.minimum(torch.minimum(f[:, None, None], f[None, :, None]), f[None, None, :]) ** 2
    d = torch.minimum(torch.minimum(e, wall), torch.tensor(rmax * rmax, device=eng.device))      # 0 on unset voxels: E = 0 there
    r = torch.arange(-rmax, rmax + 1, device=eng.device) ** 2
    q = (r[:, None, None] + r[None, :, None] + r[None, None, :]).reshape(-1)
    vol = torch.cumsum(torch.bincount(q, minlength=rmax * rmax + 1), 0)                           # vol[t - 1] = offsets with q < t
    d = d[d > 0]
    return int(vol[d - 1].sum())


print("%-6s %4s %4s | %9s = %s | %7s %7s | %7s | %10s %9s" %
      ("mesh", "n", "rmax", "tiled ms", " + ".join(TILED), "brick %", "owned %", "edt ms", "pairs", "naive ms"))
for name in ("d20", "bimba", "bunny"):
    xyz, tri = M.import_mesh(M.asset(name + ".obj"))
    dx, dt = eng.mesh_to_device(xyz, tri)
    for n in (256, 512):
        origin, vs = M.frame([xyz], n)
        fr = Frame.make(n, vs, origin)
        w = eng.voxelize(fr, dx, dt)
        dist = torch.empty(n ** 3, dtype=torch.int32, device=eng.device)
        for rmax in (4, 8, 32):
            work = pairs(fr, w, rmax)
            naive = work <= cap

            def run(algo): ctx.thickness(fr, w.data_ptr(), rmax, 0, algo)
            def edt(): ctx.edt(fr, w.data_ptr(), dist.data_ptr(), EDT_SEEDS_UNSET, ALGO_TILED)
            run(ALGO_TILED); edt()                                                      # warm-up: buffers grown, code loaded
            if naive: run(ALGO_NAIVE)
            eng.sync()
            t2, _ = eng.thickness(fr, w, rmax)
            nb = n // 8
            open_ = ((t2 > 0) & (t2 < rmax * rmax)).view(nb, 8, nb, 8, nb, 8)
            owned = float(open_.any(5).any(3).any(1).float().mean())
            acc = {}
            for _ in range(reps):                                                        # interleaved: one of each per round
                for tag, fn in (("t", lambda: run(ALGO_TILED)), ("e", edt)) + ((("n", lambda: run(ALGO_NAIVE)),) if naive else ()):
                    for key, val in timed(fn).items(): acc[(tag, key)] = acc.get((tag, key), 0.0) + val
            t = {k: v / reps for k, v in acc.items()}
            tt = sum(t.get(("t", k), 0.0) for k in TILED)
            te = sum(t.get(("e", k), 0.0) for k in EDT)
            tn = ("%9.3f" % sum(t.get(("n", k), 0.0) for k in NAIVE)) if naive else "  skipped"
            print("%-6s %4d %4d | %9.3f = %s | %7.1f %7.1f | %7.3f | %10.3g %s" %
                  (name, n, rmax, tt, " + ".join("%.3f" % t.get(("t", k), 0.0) for k in TILED), 100.0 * t.get(("t", "md_brick"), 0.0) / tt,
                   100.0 * owned, te, work, tn), flush=True)
        del w, dist
        ctx.release()
        torch.cuda.empty_cache()
