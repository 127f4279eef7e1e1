"""GPU box: device time of the connected-component calls (vp_components_label, vp_components_filter), TILED and NAIVE on the same context,
interleaved with vp_fill_interior and with a vp_stream_copy of the label call's algorithmic bytes (4 n^3 + n^3/8), after warm-up.  Per
row and connectivity: the mean device time of one call (hipEvent brackets per kernel, vp_prof_*; one event pair around the copy) of the TILED label call with its
per-kernel split, of the NAIVE label call, of the TILED filter (KEEP_LARGEST 1), of the fill and of the copy; the label call as a multiple
of the copy and the ratio NAIVE / TILED.
  python tools/vox_components.py [reps]        (default 5)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cuda_mesh_voxelization_amd import mesh as M
from cuda_mesh_voxelization_amd.capi import (ALGO_NAIVE, ALGO_TILED, COMP_KEEP_LARGEST, COMP_KERNELS, CONN_6, CONN_26, MORPH_DILATE, MORPH_ERODE,
                                             Frame)
from cuda_mesh_voxelization_amd.pipeline import Engine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
eng = Engine(0)
ctx = eng.ctx
LABEL_T = ("comp_init", "comp_merge", "comp_flatten", "comp_rank", "comp_relabel")
LABEL_N = ("comp_init_naive", "comp_merge_naive", "comp_flatten", "comp_rank", "comp_relabel")
FILL = ("fill_x", "fill_y", "fill_z", "fill_final")


def timed(fn):
    ctx.prof_reset(); ctx.prof_enable(True)
    fn()
    ctx.prof_enable(False)
    return {k: v["ms"] for k, v in ctx.prof().items()}


def debris_scene():
    """the bunny and 30 scaled copies of d20 above it (the scene of tests/test_components_gpu.py)"""
    bxyz, btri = M.import_mesh(M.asset("bunny.obj"))
    dxyz, dtri = M.import_mesh(M.asset("d20.obj"))
    lo, hi = bxyz.min(0), bxyz.max(0)
    ext = float((hi - lo).max())
    unit = (dxyz - (dxyz.min(0) + dxyz.max(0)) / 2) / float((dxyz.max(0) - dxyz.min(0)).max())
    xyz, tri, count = [bxyz], [btri], len(bxyz)
    for i in range(30):
        c = lo + ext * np.array([0.08 + 0.17 * (i % 6), 0.08 + 0.17 * (i // 6), 0.0], np.float32)
        c[2] = hi[2] + ext * 0.2
        xyz.append((unit * ext * (0.03 + 0.001 * i) + c).astype(np.float32))
        tri.append(dtri + count)
        count += len(dxyz)
    return np.concatenate(xyz).astype(np.float32), np.concatenate(tri).astype(np.uint32)


def grids():
    """(row label, n, frame, grid) one at a time"""
    xyz, tri = M.bunny(24)
    dx, dt = eng.mesh_to_device(xyz, tri)
    for n in (512, 1024):
        origin, vs = M.frame([xyz], n)
        fr = Frame.make(n, vs, origin)
        yield "bunny x24 solid", n, fr, eng.voxelize(fr, dx, dt)
        yield "bunny x24 conservative", n, fr, eng.voxelize_conservative(fr, dx, dt)
    n = 512
    fr = Frame.make(n, 1.0 / n, np.zeros(3, np.float32))
    g = torch.Generator(device=eng.device).manual_seed(7)
    bits = (torch.rand(n ** 3, device=eng.device, generator=g) < 0.20).view(-1, 32).to(torch.int64)
    words = (bits << torch.arange(32, device=eng.device)).sum(1)
    yield "random 0.20", n, fr, torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    sxyz, stri = debris_scene()
    origin, vs = M.frame([sxyz], n)
    fr = Frame.make(n, vs, origin)
    sx, st = eng.mesh_to_device(sxyz, stri)
    c = eng.voxelize_conservative(fr, sx, st)
    d = eng.morph(fr, c, MORPH_DILATE, 2)
    f, _ = eng.fill_interior(fr, d)
    yield "debris scene (repaired)", n, fr, eng.morph(fr, f, MORPH_ERODE, 2)


print("%-24s %5s %4s %9s | %9s = %s | %9s %7s | %9s | %8s %8s | %8s" %
      ("grid", "n", "conn", "K", "tiled ms", " + ".join(k[5:] for k in LABEL_T), "naive ms", "naive/t", "filter ms", "fill ms", "copy ms", "tiled/cp"))
for label, n, fr, w in grids():
    labels = torch.empty(fr.voxels, dtype=torch.int32, device=eng.device)
    out = eng.new_grid(fr)
    src = torch.empty(fr.voxels + fr.words, dtype=torch.int32, device=eng.device)
    dst = torch.empty_like(src)
    for conn in (CONN_6, CONN_26):
        def label_t(): return eng.components_label(fr, w, conn, ALGO_TILED, out=labels)
        def label_n(): return eng.components_label(fr, w, conn, ALGO_NAIVE, out=labels)
        def filt(): return eng.components_filter(fr, w, COMP_KEEP_LARGEST, 1, conn, out=out)
        def fill(): return eng.fill_interior(fr, w, out=out)
        def copy(): ctx.stream_copy(dst.data_ptr(), src.data_ptr(), src.numel() * 4)
        _, k = label_t(); label_n(); filt(); fill(); copy(); eng.sync()            # warm-up: buffers grown, code loaded
        acc = {}
        tt = tn = tf = tfill = tc = 0.0
        for _ in range(reps):                                                       # interleaved: one of each per round
            p = timed(label_t); tt += sum(p.get(key, 0.0) for key in LABEL_T)
            for key in LABEL_T: acc[key] = acc.get(key, 0.0) + p.get(key, 0.0)
            p = timed(label_n); tn += sum(p.get(key, 0.0) for key in LABEL_N)
            p = timed(filt); tf += sum(p.get(key, 0.0) for key in COMP_KERNELS)
            for key in ("comp_sizes", "comp_select", "comp_write"): acc[key] = acc.get(key, 0.0) + p.get(key, 0.0)
            p = timed(fill); tfill += sum(p.get(key, 0.0) for key in FILL)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)      # the copy has no timing key of its own
            a.record(); copy(); b.record(); b.synchronize(); tc += a.elapsed_time(b)
        tt, tn, tf, tfill, tc = (v / reps for v in (tt, tn, tf, tfill, tc))
        split = " + ".join("%.3f" % (acc[key] / reps) for key in LABEL_T)
        print("%-24s %5d %4d %9d | %9.3f = %s | %9.3f %7.2f | %9.3f | %8.3f %8.3f | %8.1f" %
              (label, n, conn, k, tt, split, tn, tn / tt, tf, tfill, tc, tt / tc), flush=True)
        print("%-24s %5s %4s %9s   filter adds: sizes %.3f + select %.3f + write %.3f" %
              ("", "", "", "", acc["comp_sizes"] / reps, acc["comp_select"] / reps, acc["comp_write"] / reps), flush=True)
    del labels, out, src, dst, w
    ctx.release()
    torch.cuda.empty_cache()
