"""GPU box: device time of the exact distance transform (vp_edt with SEEDS_BORDER, the transform behind vp_edt_sdf), TILED at every size
and NAIVE at n <= 256, interleaved on the same context with vp_jfa of the same grid, with vp_morph r = 32 against vp_edt_morph r = 32
(dilate) and with one vp_stream_copy per pass of the algorithmic bytes (x pass: n^3/8 read + 4 n^3 written; each column pass: 8 n^3),
after warm-up.  Per row: the mean device time over the rounds (hipEvent brackets per kernel, vp_prof_*; one event pair around each copy)
split by timing key, the copy of a pass's bytes beside each pass, the JFA and the ratio, and the two morphologies.
  python tools/vox_edt.py [reps]        (default 5)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cuda_mesh_voxelization_amd import mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, EDT_SEEDS_BORDER, JFA_PASS_KEYS, MORPH_DILATE, Frame
from cuda_mesh_voxelization_amd.pipeline import Engine

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
eng = Engine(0)
ctx = eng.ctx
EDT_T = ("surface", "edt_x", "edt_y", "edt_z")
EDT_N = ("surface", "edt_x", "edt_y_naive", "edt_z_naive")
JFA = ("surface", "jfa_init", "jfa_final") + tuple(JFA_PASS_KEYS)


def timed(fn):
    ctx.prof_reset(); ctx.prof_enable(True)
    fn()
    ctx.prof_enable(False)
    return {k: v["ms"] for k, v in ctx.prof().items()}


def grids():
    """(row label, n, frame, grid) one at a time"""
    xyz, tri = M.bunny(24)
    dx, dt = eng.mesh_to_device(xyz, tri)
    for n in (256, 512, 1024):
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


def copy_ms(dst, src, nbytes):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)          # the copy has no timing key of its own
    a.record(); ctx.stream_copy(dst.data_ptr(), src.data_ptr(), nbytes); b.record(); b.synchronize()
    return a.elapsed_time(b)


print("%-24s %5s | %8s = %s | %8s %8s | %9s | %8s %7s | %8s %8s" %
      ("grid", "n", "tiled ms", " + ".join(k for k in EDT_T), "copy x", "copy y/z", "naive ms", "jfa ms", "edt/jfa", "morph32", "edtmorph"))
for label, n, fr, w in grids():
    vox = n ** 3
    dist = torch.empty(vox, dtype=torch.int32, device=eng.device)
    sdf = torch.empty(vox, dtype=torch.float32, device=eng.device)
    out = eng.new_grid(fr)
    src = torch.empty(4 * vox, dtype=torch.uint8, device=eng.device)
    dst = torch.empty_like(src)
    naive = n <= 256

    def edt(algo): ctx.edt(fr, w.data_ptr(), dist.data_ptr(), EDT_SEEDS_BORDER, algo)
    def jfa(): eng.jfa(fr, w, out=sdf)
    def morph(): ctx.morph(fr, w.data_ptr(), out.data_ptr(), MORPH_DILATE, 32)
    def edt_morph(): ctx.edt_morph(fr, w.data_ptr(), out.data_ptr(), MORPH_DILATE, 32)
    edt(ALGO_TILED); jfa(); morph(); edt_morph()                                     # warm-up: buffers grown, code loaded
    if naive: edt(ALGO_NAIVE)
    copy_ms(dst, src, 4 * vox); eng.sync()
    acc = {}
    def add(tag, p):
        for key, val in p.items(): acc[(tag, key)] = acc.get((tag, key), 0.0) + val
    for _ in range(reps):                                                            # interleaved: one of each per round
        add("t", timed(lambda: edt(ALGO_TILED)))
        if naive: add("n", timed(lambda: edt(ALGO_NAIVE)))
        add("j", timed(jfa))
        add("m", timed(morph))
        add("e", timed(edt_morph))
        add("c", {"x": copy_ms(dst, src, (vox // 8 + 4 * vox) // 2 // 16 * 16), "yz": copy_ms(dst, src, 4 * vox)})   # a copy moves its bytes twice
    t = {k: v / reps for k, v in acc.items()}
    tt = sum(t.get(("t", k), 0.0) for k in EDT_T)
    tn = sum(t.get(("n", k), 0.0) for k in EDT_N) if naive else float("nan")
    tj = sum(t.get(("j", k), 0.0) for k in JFA)
    tm = t.get(("m", "morph"), 0.0)
    te = sum(v for (tag, _), v in t.items() if tag == "e")
    print("%-24s %5d | %8.3f = %s | %8.3f %8.3f | %9.3f | %8.3f %7.2f | %8.3f %8.3f" %
          (label, n, tt, " + ".join("%.3f" % t.get(("t", k), 0.0) for k in EDT_T), t[("c", "x")], t[("c", "yz")], tn, tj, tt / tj, tm, te), flush=True)
    del dist, sdf, out, src, dst, w
    ctx.release()
    torch.cuda.empty_cache()
