"""GPU box: time of the seeded watershed (vp_watershed) on two overlapping spheres (sphere.obj, radii r and 0.7 r, centres 1.2 r apart) at
n = 256 and 512: the influence zones of the two cores (no priority field: one level) and the flood of the exact squared distance map from
its high end, VP_ALGO_NAIVE against VP_ALGO_TILED, 6-connected, interleaved in one process after warm-up, the mean over the rounds.
Markers = the components of the solid eroded by 0.22 n voxels (vp_edt_morph + vp_components_label), priority = vp_edt's D2 to the
nearest unset voxel.  The quantum is 1 at n = 256 and 4 at n = 512, where D2 reaches 31,000 and quantum 1 is refused (the span bound).
vp_watershed blocks (the pre-pass and the convergence of every level are read back), so a call is timed by the wall clock around it,
read-backs included.  Rounds come from the timing table: NAIVE's rounds are its md_naive launches (every level runs whole batches, the
rounds after its fixed point return at once), TILED's rounds its md_brick launches; levels = the third statistic.
  python tools/vox_watershed.py [reps]        (default 2)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cuda_mesh_voxelization_amd import capi, mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame
from cuda_mesh_voxelization_amd.pipeline import Engine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 2
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
    out = fn()
    ctx.prof_enable(False)
    return {k: v["launches"] for k, v in ctx.prof().items()}, out


print("%-8s %4s %-5s %3s %-5s | %8s %9s %6s %6s | %10s %7s %9s" %
      ("solid", "n", "mode", "q", "algo", "markers", "labelled", "levels", "cut", "call ms", "rounds", "ms/round"))
xyz, tri = M.import_mesh(M.asset("sphere.obj"))
xyz = np.asarray(xyz, np.float32)
centre, radius = (xyz.max(0) + xyz.min(0)) / 2, float((xyz.max(0) - xyz.min(0)).max()) / 2
first = xyz - centre
second = first * np.float32(0.7) + np.array([1.2 * radius, 0, 0], np.float32)
for n in (256, 512):
    origin, vs = M.frame([first, second], n)
    fr = Frame.make(n, vs, origin)
    w = eng.voxelize(fr, *eng.mesh_to_device(first, tri))
    w |= eng.voxelize(fr, *eng.mesh_to_device(second, tri))
    cores = eng.edt_morph(fr, w, capi.MORPH_ERODE, int(0.22 * n))
    markers, count = eng.components_label(fr, cores, capi.CONN_6)
    assert count == 2, count
    d2 = eng.edt(fr, w, capi.EDT_SEEDS_UNSET)
    eng.sync()
    for mode, prio, q in (("zones", 0, 1), ("flood", d2.data_ptr(), 1 if n == 256 else 4)):
        def call(algo):
            return ctx.watershed(fr, w.data_ptr(), markers.data_ptr(), prio, capi.WS_DESCENDING, q, capi.CONN_6, algo)
        stats, rounds = {}, {}
        for algo, key in ((ALGO_NAIVE, "md_naive"), (ALGO_TILED, "md_brick")):           # warm-up: buffers grown, code loaded; the rounds
            table, stats[algo] = launches(lambda: call(algo))
            rounds[algo] = table[key]
        assert stats[ALGO_NAIVE] == stats[ALGO_TILED]
        full = {ALGO_NAIVE: 0.0, ALGO_TILED: 0.0}
        for _ in range(reps):                                                            # interleaved: one of each per round
            for algo in (ALGO_NAIVE, ALGO_TILED):
                full[algo] += wall(lambda: call(algo))[0] / reps
        for algo, aname in ((ALGO_NAIVE, "naive"), (ALGO_TILED, "tiled")):
            used, labelled, levels, cut = stats[algo]
            print("%-8s %4d %-5s %3d %-5s | %8d %9d %6d %6d | %10.3f %7d %9.4f" %
                  ("spheres", n, mode, q, aname, used, labelled, levels, cut, full[algo], rounds[algo], full[algo] / rounds[algo]), flush=True)
        print("%-8s %4d %-5s naive / tiled = %.2f, tiled ms / level = %.4f" %
              ("spheres", n, mode, full[ALGO_NAIVE] / full[ALGO_TILED], full[ALGO_TILED] / max(stats[ALGO_TILED][2], 1)), flush=True)
    del w, cores, markers, d2
    ctx.release()
    torch.cuda.empty_cache()
