"""GPU box: device time of the surface-nets calls (vp_surfnets_count + vp_surfnets), TILED and NAIVE on the same context, interleaved with
vp_extract_count + vp_extract in VP_EXTRACT_EXPOSED mode on the same grid (the nearest existing kernel: the same walk, one compaction) and
with one vp_stream_copy of the algorithmic bytes (n^3/8 read + 20 V + 16 Q written), after warm-up.  Per row: V, Q, the mean device time
of count + write without relaxation (hipEvent brackets per kernel, vp_prof_*; one event pair around the copy) with its per-kernel split,
one relaxation step (the mean over the 8 steps of a call), the same for NAIVE, the ratio NAIVE / TILED, the extract pair and the copy.
  python tools/vox_surfnets.py [reps]        (default 5)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cuda_mesh_voxelization_amd import mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, EXTRACT_EXPOSED, MORPH_DILATE, MORPH_ERODE, Frame
from cuda_mesh_voxelization_amd.pipeline import Engine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
STEPS = 8
eng = Engine(0)
ctx = eng.ctx
MESH_T = ("sn_cells", "sn_scan", "sn_verts", "sn_quads")
MESH_N = ("sn_cells_naive", "sn_scan", "sn_verts_naive", "sn_quads_naive")


def timed(fn):
    ctx.prof_reset(); ctx.prof_enable(True)
    fn()
    ctx.prof_enable(False)
    return {k: v["ms"] for k, v in ctx.prof().items()}


def debris_scene():
    """the bunny and 30 scaled copies of d20 above it (the scene of tools/vox_components.py and tests/test_components_gpu.py)"""
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
    e = eng.morph(fr, f, MORPH_ERODE, 2)
    yield "debris scene (repaired)", n, fr, eng.components_filter(fr, e, 0, 1)[0]


print("%-24s %5s %9s %9s | %8s = %s | %7s | %8s = %s | %7s | %7s | %8s %8s %8s" %
      ("grid", "n", "V", "Q", "tiled ms", " + ".join(k[3:] for k in MESH_T), "relax/1", "naive ms", " + ".join(k[3:] for k in MESH_T), "relax/1",
       "naive/t", "extract", "copy ms", "tiled/cp"))
for label, n, fr, w in grids():
    nv, nq = ctx.surfnets_count(fr, w.data_ptr(), ALGO_TILED)
    cells = torch.empty(nv, dtype=torch.int64, device=eng.device)
    xyz = torch.empty((nv, 3), dtype=torch.float32, device=eng.device)
    quads = torch.empty((nq, 4), dtype=torch.int32, device=eng.device)
    nbytes = (n ** 3 // 8 + 20 * nv + 16 * nq + 15) // 16 * 16
    src = torch.empty(nbytes, dtype=torch.uint8, device=eng.device)
    dst = torch.empty_like(src)
    nrec = ctx.extract_count(fr, w.data_ptr(), EXTRACT_EXPOSED)
    rec = torch.empty(nrec, dtype=torch.int64, device=eng.device)

    def mesh(algo, steps):
        ctx.surfnets_count(fr, w.data_ptr(), algo)
        ctx.surfnets(fr, w.data_ptr(), algo, steps, cells.data_ptr(), xyz.data_ptr(), quads.data_ptr(), nv, nq)

    def extract():
        ctx.extract_count(fr, w.data_ptr(), EXTRACT_EXPOSED)
        ctx.extract(fr, w.data_ptr(), EXTRACT_EXPOSED, None, rec.data_ptr(), None, nrec)

    def copy(): ctx.stream_copy(dst.data_ptr(), src.data_ptr(), nbytes)
    for algo in (ALGO_TILED, ALGO_NAIVE):                                           # warm-up: buffers grown, code loaded
        mesh(algo, 0); mesh(algo, STEPS)
    extract(); copy(); eng.sync()
    acc = {}
    te = tc = 0.0
    for _ in range(reps):                                                           # interleaved: one of each per round
        for algo in (ALGO_TILED, ALGO_NAIVE):
            p = timed(lambda: mesh(algo, 0))
            for key, val in p.items(): acc[(algo, key)] = acc.get((algo, key), 0.0) + val
            p = timed(lambda: mesh(algo, STEPS))
            for key in ("sn_relax", "sn_relax_naive"): acc[(algo, key)] = acc.get((algo, key), 0.0) + p.get(key, 0.0) / STEPS
        te += timed(extract).get("extract", 0.0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)          # the copy has no timing key of its own
        a.record(); copy(); b.record(); b.synchronize(); tc += a.elapsed_time(b)
    t = {k: v / reps for k, v in acc.items()}
    tt = sum(t[(ALGO_TILED, k)] for k in MESH_T)
    tn = sum(t[(ALGO_NAIVE, k)] for k in MESH_N)
    te, tc = te / reps, tc / reps
    print("%-24s %5d %9d %9d | %8.3f = %s | %7.3f | %8.3f = %s | %7.3f | %7.2f | %8.3f %8.3f %8.1f" %
          (label, n, nv, nq, tt, " + ".join("%.3f" % t[(ALGO_TILED, k)] for k in MESH_T), t[(ALGO_TILED, "sn_relax")],
           tn, " + ".join("%.3f" % t[(ALGO_NAIVE, k)] for k in MESH_N), t[(ALGO_NAIVE, "sn_relax_naive")], tn / tt, te, tc, tt / tc), flush=True)
    del cells, xyz, quads, src, dst, rec, w
    ctx.release()
    torch.cuda.empty_cache()
