"""GPU box: device time of vp_isonets (classification + count + records + placement + quads, no relaxation, with normals), TILED and NAIVE on
the same context, interleaved with vp_surfnets_count + vp_surfnets on the same inside grid (what the topology alone costs) and with one
vp_stream_copy of the algorithmic bytes (4 n^3 + n^3/8 read, 32 V + 16 Q written), after warm-up.  The field is vp_mesh_distance of
bunny x 24 with band 3, signed by the solid grid, meshed at iso 0 with the signed-square transform: the inside set is that grid.  Per row:
V, Q, the mean device time (hipEvent brackets per timing key, vp_prof_*; one event pair around the copy) with its split -- classification
and count book under sn_cells, records and placement under sn_verts -- then the three ratios.
  python tools/vox_isonets.py [reps]        (default 5)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cuda_mesh_voxelization_amd import mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, ISO_SIGNED_SQUARE, Frame
from cuda_mesh_voxelization_amd.pipeline import Engine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
BAND = 3
eng = Engine(0)
ctx = eng.ctx
MESH_T = ("sn_cells", "sn_scan", "sn_verts", "sn_quads")
MESH_N = ("sn_cells_naive", "sn_scan", "sn_verts_naive", "sn_quads_naive")


def timed(fn):
    ctx.prof_reset(); ctx.prof_enable(True)
    fn()
    ctx.prof_enable(False)
    return {k: v["ms"] for k, v in ctx.prof().items()}


print("%-12s %5s %9s %9s | %8s = %s | %8s = %s | %8s = %s | %8s | %8s %8s %8s" %
      ("field", "n", "V", "Q", "tiled ms", " + ".join(k[3:] for k in MESH_T), "naive ms", " + ".join(k[3:] for k in MESH_T),
       "surfnets", " + ".join(k[3:] for k in MESH_T), "copy ms", "tiled/cp", "tiled/sn", "naive/t"))
xyz, tri = M.bunny(24)
dx, dt = eng.mesh_to_device(xyz, tri)
for n in (512, 1024):
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    grid = eng.voxelize(fr, dx, dt)
    field = eng.mesh_distance(fr, dx, dt, BAND, sign_words=grid)
    nv, nq = ctx.isonets(fr, field.data_ptr(), ISO_SIGNED_SQUARE, 0.0, 0, True, ALGO_TILED)
    assert (nv, nq) == ctx.surfnets_count(fr, grid.data_ptr(), ALGO_TILED)
    cells = torch.empty(nv, dtype=torch.int64, device=eng.device)
    pos = torch.empty((nv, 3), dtype=torch.float32, device=eng.device)
    quads = torch.empty((nq, 4), dtype=torch.int32, device=eng.device)
    nbytes = (4 * n ** 3 + n ** 3 // 8 + 32 * nv + 16 * nq + 15) // 16 * 16
    src = torch.empty(nbytes, dtype=torch.uint8, device=eng.device)
    dst = torch.empty_like(src)

    def iso(algo): ctx.isonets(fr, field.data_ptr(), ISO_SIGNED_SQUARE, 0.0, 0, True, algo)

    def bits():
        ctx.surfnets_count(fr, grid.data_ptr(), ALGO_TILED)
        ctx.surfnets(fr, grid.data_ptr(), ALGO_TILED, 0, cells.data_ptr(), pos.data_ptr(), quads.data_ptr(), nv, nq)

    def copy(): ctx.stream_copy(dst.data_ptr(), src.data_ptr(), nbytes)
    iso(ALGO_TILED); iso(ALGO_NAIVE); bits(); copy(); eng.sync()                    # warm-up: buffers grown, code loaded
    acc = {}
    tc = 0.0
    for _ in range(reps):                                                           # interleaved: one of each per round
        for tag, fn in (("t", lambda: iso(ALGO_TILED)), ("n", lambda: iso(ALGO_NAIVE)), ("s", bits)):
            for key, val in timed(fn).items(): acc[(tag, key)] = acc.get((tag, key), 0.0) + val / reps
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)          # the copy has no timing key of its own
        a.record(); copy(); b.record(); b.synchronize(); tc += a.elapsed_time(b) / reps
    tt = sum(acc[("t", k)] for k in MESH_T)
    tn = sum(acc[("n", k)] for k in MESH_N)
    ts = sum(acc[("s", k)] for k in MESH_T)
    print("%-12s %5d %9d %9d | %8.3f = %s | %8.3f = %s | %8.3f = %s | %8.3f | %8.2f %8.2f %8.2f" %
          ("bunny x24", n, nv, nq, tt, " + ".join("%.3f" % acc[("t", k)] for k in MESH_T), tn, " + ".join("%.3f" % acc[("n", k)] for k in MESH_N),
           ts, " + ".join("%.3f" % acc[("s", k)] for k in MESH_T), tc, tt / tc, tt / ts, tn / tt), flush=True)
    del cells, pos, quads, src, dst, field, grid
    ctx.release()
    torch.cuda.empty_cache()
