"""GPU box: device time of the sparse voxel octree (vp_octree, vp_octree_expand) of the solid grids of bunny and d20 at n = 256, 512 and
1024: the build with VP_ALGO_TILED split by timing key (the stages book under keys they share with vp_mesh_distance) and with VP_ALGO_NAIVE
(skipped above `naive_max`, default 512: about 0.7 n^3 bytes of states and ranks, and one-workgroup scans over n^3 / 8 flags), the expand
with both algos, and beside them one vp_stream_copy of the grid's n^3 / 8 bytes in the same process -- the yardstick: the build reads the
grid twice and writes little.  Interleaved after warm-up, the mean over the rounds (hipEvent brackets per kernel, vp_prof_*; one event pair
around the copy).  The build blocks once between count and write; the device times leave that read-back out.
  python tools/vox_octree.py [reps] [naive_max]        (default 5 512)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cuda_mesh_voxelization_amd import mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame
from cuda_mesh_voxelization_amd.pipeline import Engine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
naive_max = int(sys.argv[2]) if len(sys.argv) > 2 else 512
eng = Engine(0)
ctx = eng.ctx
TILED = ("md_count", "md_scan", "md_write")
NAIVE = ("md_prefill", "md_scan", "md_naive")


def timed(fn):
    ctx.prof_reset(); ctx.prof_enable(True)
    fn()
    ctx.prof_enable(False)
    return {k: v["ms"] for k, v in ctx.prof().items()}


print("%-6s %5s %9s %6s | %9s = %s | %7s | %9s | %9s %9s | %8s" %
      ("mesh", "n", "nodes", "ratio", "tiled ms", " + ".join(TILED), "x copy", "naive ms", "expand t", "expand n", "copy ms"))
for name in ("bunny", "d20"):
    xyz, tri = M.import_mesh(M.asset(name + ".obj"))
    dx, dt = eng.mesh_to_device(xyz, tri)
    for n in (256, 512, 1024):
        origin, vs = M.frame([xyz], n)
        fr = Frame.make(n, vs, origin)
        w = eng.voxelize(fr, dx, dt)
        dst = torch.empty_like(w)
        naive = n <= naive_max

        def build(algo): return ctx.octree(fr, w.data_ptr(), algo)
        def copy(): ctx.stream_copy(dst.data_ptr(), w.data_ptr(), w.numel() * 4)
        if naive: build(ALGO_NAIVE)                                                      # warm-up: buffers grown, code loaded
        m = build(ALGO_TILED)
        nodes = eng.octree(fr, w, ALGO_TILED)[0].clone()                                  # the context's own buffer is rewritten by every build

        def expand(algo): ctx.octree_expand(fr, nodes.data_ptr(), m, algo)
        expand(ALGO_NAIVE); expand(ALGO_TILED); copy(); eng.sync()
        assert torch.equal(eng.octree_expand(fr, nodes), w)
        acc = {}
        tc = 0.0
        for _ in range(reps):                                                            # interleaved: one of each per round
            runs = [("t", lambda: build(ALGO_TILED)), ("et", lambda: expand(ALGO_TILED)), ("en", lambda: expand(ALGO_NAIVE))]
            if naive: runs.append(("n", lambda: build(ALGO_NAIVE)))
            for tag, fn in runs:
                for key, val in timed(fn).items(): acc[(tag, key)] = acc.get((tag, key), 0.0) + val
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)      # the copy has no timing key of its own
            a.record(); copy(); b.record(); b.synchronize(); tc += a.elapsed_time(b)
        t = {k: v / reps for k, v in acc.items()}
        tc /= reps
        tt = sum(t.get(("t", k), 0.0) for k in TILED)
        tn = ("%9.3f" % sum(t.get(("n", k), 0.0) for k in NAIVE)) if naive else "  skipped"
        print("%-6s %5d %9d %6.1f | %9.3f = %s | %7.1f | %s | %9.3f %9.3f | %8.4f" %
              (name, n, m, (n ** 3 / 8) / (8.0 * m), tt, " + ".join("%.3f" % t.get(("t", k), 0.0) for k in TILED), tt / tc, tn,
               t.get(("et", "md_fill"), 0.0), t.get(("en", "md_fill"), 0.0), tc), flush=True)
        del w, dst, nodes
        ctx.release()
        torch.cuda.empty_cache()
