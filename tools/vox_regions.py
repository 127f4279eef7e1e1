"""GPU box: time of the region analysis (vp_regions) on bunny.obj at n = 256 and 512, on two label volumes -- the 26-components of the solid
(vp_components_label: one large label and whatever specks there are) and the parts of its seeded watershed (markers = the 6-components of
the solid eroded by n / 32 voxels, priority = vp_edt's D2, quantum 1 at n = 256 and 4 at n = 512) -- each without and with the value field
(D2).  VP_ALGO_TILED, VP_ALGO_NAIVE and a device copy of the bytes the call must read (vp_stream_copy of 4 n^3 bytes, 8 n^3 with values: the
floor) run interleaved in one process after warm-up; the mean over the rounds.  vp_regions blocks (the totals are read back), so a call is
timed by the wall clock around it, read-back included; the copy is timed the same way, `inner` copies between two synchronisations.  The
per-key device times of one more TILED call (clear = md_fill, kernel = md_brick, finish = md_split) say which launch pays.
  python tools/vox_regions.py [rounds]        (default 3)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cuda_mesh_voxelization_amd import capi, mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame
from cuda_mesh_voxelization_amd.pipeline import Engine

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
eng = Engine(0)
ctx = eng.ctx


def wall(fn, inner=1):
    eng.sync()
    t = time.perf_counter()
    for _ in range(inner):
        fn()
    eng.sync()
    return (time.perf_counter() - t) * 1e3 / inner


print("%-10s %4s %-6s | %7s %9s %9s | %9s %9s %9s | %12s %13s | %s" %
      ("labels", "n", "values", "K", "voxels", "interf.", "tiled ms", "naive ms", "copy ms", "tiled / copy", "naive / tiled", "tiled: clear + kernel + finish ms"))
xyz, tri = M.import_mesh(M.asset("bunny.obj"))
xyz = np.asarray(xyz, np.float32)
for n in (256, 512):
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    w = eng.voxelize(fr, *eng.mesh_to_device(xyz, tri))
    d2 = eng.edt(fr, w, capi.EDT_SEEDS_UNSET)
    comp, kc = eng.components_label(fr, w, capi.CONN_26)
    cores = eng.edt_morph(fr, w, capi.MORPH_ERODE, n // 32)
    markers, km = eng.components_label(fr, cores, capi.CONN_6)
    parts, _, _ = eng.watershed(fr, w, markers, d2, capi.WS_DESCENDING, 1 if n == 256 else 4, capi.CONN_6)
    parts = parts.clone()
    src = torch.empty(2 * fr.voxels, dtype=torch.int32, device=eng.device)
    dst = torch.empty(2 * fr.voxels, dtype=torch.int32, device=eng.device)
    eng.sync()
    for lname, labels, K in (("components", comp, kc), ("parts", parts, km)):
        for values in (None, d2):
            vp = 0 if values is None else values.data_ptr()
            nbytes = fr.voxels * (4 if values is None else 8)

            def call(algo):
                return ctx.regions(fr, labels.data_ptr(), K, vp, algo)

            def copy():
                ctx.stream_copy(dst.data_ptr(), src.data_ptr(), nbytes)
            stats = {algo: call(algo) for algo in (ALGO_NAIVE, ALGO_TILED)}                  # warm-up: the table grown, code loaded
            wall(copy, 3)
            assert stats[ALGO_NAIVE] == stats[ALGO_TILED]
            ms = {"tiled": 0.0, "naive": 0.0, "copy": 0.0}
            for _ in range(rounds):                                                          # interleaved: one of each per round
                ms["tiled"] += wall(lambda: call(ALGO_TILED), 5) / rounds
                ms["naive"] += wall(lambda: call(ALGO_NAIVE)) / rounds
                ms["copy"] += wall(copy, 10) / rounds
            ctx.prof_reset()
            ctx.prof_enable(True)
            call(ALGO_TILED)
            ctx.prof_enable(False)
            keys = {k: v["ms"] for k, v in ctx.prof().items()}
            s = stats[ALGO_TILED]
            print("%-10s %4d %-6s | %7d %9d %9d | %9.3f %9.3f %9.3f | %12.2f %13.2f | %.3f + %.3f + %.3f" %
                  (lname, n, "none" if values is None else "D2", K, s[0], s[3], ms["tiled"], ms["naive"], ms["copy"], ms["tiled"] / ms["copy"],
                   ms["naive"] / ms["tiled"], keys.get("md_fill", 0.0), keys.get("md_brick", 0.0), keys.get("md_split", 0.0)), flush=True)
    del w, d2, comp, cores, markers, parts, src, dst
    ctx.release()
    torch.cuda.empty_cache()
