"""Every writer of the ABI against every record a context keeps about a caller's buffer (tests/ctx_history.py, part 1).

The records: what vp_jfa_start left (its grid range and its explicit workspace range; init ids at n = 32, a border mask at n = 96), the
count of vp_extract_count and the count of vp_surfnets_count.  The rule (include/vphip.h at vp_jfa_start): ANY output of ANY call of the ABI
that lands on ANY byte of a recorded range drops the record, and an output that merely touches the range does not.  One cell = establish
the record in the middle of one allocation, let one output of one writer land

    first   on the first 16 bytes of the range          inside  strictly inside it (or, larger than it, strictly around it)
    last    on its last 16 bytes                        before / after   ending exactly where it begins / beginning exactly where it ends

and make the dependent call (vp_jfa_run, vp_extract, vp_surfnets).  After an overlap it must return VP_ERR_INVALID, name the call to repeat,
and leave its outputs untouched (they are pre-filled with a pattern); after a neighbour it must be served and equal the CPU reference bit
for bit.  vp_ctx_workspace and vp_free do not let the caller choose the pointer: for the overlaps the range lies at the start / in the middle
/ at the end of the slot or of an allocation of vp_malloc, which is then handed out again or freed (vp_free counts as a write to the whole
allocation; the dependent call is refused before it launches anything, so the freed memory is never touched); for the neighbours a slot or
allocation ELSEWHERE is used, not one that touches the range -- "touching does not drop" is not tested for these two. vp_jfa, vp_jfa_start
and vp_jfa_run replace the vp_jfa_start record wherever their outputs land, so against that record they are refused in all five placements
and only the two counts see their grid_written calls.  The outputs of the dependent calls are sized for the worst case of ANY grid contents
plus one scan block, and the writers write zeros or next to nothing: even a library that wrongly served a call would write inside its
buffers.  The cells that do not run are listed with their reasons in ctx_history.expectation (tests/test_ctx_history_cpu.py prints and bounds
them)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from cuda_mesh_voxelization_amd import capi
from cuda_mesh_voxelization_amd.capi import ALGO_TILED

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctx_history as H  # noqa: E402

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A
SLOT = 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def inputs(dev):
    return H.prepare_inputs(dev)


@pytest.fixture(scope="module")
def cases(dev):
    """per grid side: the ball grid on the device and the uploaded expectations of the three dependent calls"""
    out = {}
    for n in (32, 96):
        c = H.record_case(n)
        d = {"words": torch.from_numpy(c["words"].view(np.int32)).to(dev), "sdf": torch.from_numpy(c["sdf"].view(np.int32)).to(dev)}
        for key, dt in (("records", np.int64), ("values", np.int32), ("cells", np.int64), ("xyz", np.int32), ("quads", np.int32)):
            if key in c:
                d[key] = torch.from_numpy(np.ascontiguousarray(c[key]).reshape(-1).view(dt)).to(dev)
        out[n] = d
    return out


class _Dependent:
    """The dependent call of one record: its outputs (pattern-filled before every call), the call, and the comparison with the reference."""

    def __init__(self, ctx, dev, rec, case):
        n = rec.n
        self.ctx, self.rec, self.case, self.fr = ctx, rec, case, H.unit_frame(n)
        i32 = lambda count: torch.empty(count, dtype=torch.int32, device=dev)
        if rec.kind.startswith("jfa"):
            self.outs = {"sdf": i32(n ** 3)}
            # the half of the pair (grid, workspace) that is not the recorded range
            self.other = case["words"].clone() if rec.kind == "jfa_work" else torch.empty(H.jfa_work_bytes(n), dtype=torch.uint8, device=dev)
        elif rec.kind == "extract":
            self.cap = n ** 3 + H.SCAN_BLOCK                                  # every voxel of any grid, plus one scan block
            self.outs = {"records": torch.empty(self.cap, dtype=torch.int64, device=dev), "values": i32(self.cap)}
            self.sdf_in = torch.arange(n ** 3, dtype=torch.float32, device=dev)
        else:
            self.vcap, self.qcap = (n + 1) ** 3 + H.SCAN_BLOCK, 3 * n * n * (n + 1) + H.SCAN_BLOCK
            self.outs = {"cells": torch.empty(self.vcap, dtype=torch.int64, device=dev), "xyz": i32(3 * self.vcap), "quads": i32(4 * self.qcap)}
        self.count = None

    def establish(self, rng):
        """rng: device pointer of the recorded range.  Its contents are (re)written first -- a cell before may have overwritten them."""
        ctx, rec, fr = self.ctx, self.rec, self.fr
        if rec.kind != "jfa_work":
            ctx.memcpy_d2d(rng, self.case["words"].data_ptr(), H.grid_bytes(rec.n))
        if rec.kind == "jfa_grid":
            ctx.jfa_start(fr, rng, self.other.data_ptr(), H.jfa_work_bytes(rec.n), ALGO_TILED)
        elif rec.kind == "jfa_work":
            ctx.jfa_start(fr, self.other.data_ptr(), rng, H.jfa_work_bytes(rec.n), ALGO_TILED)
        elif rec.kind == "extract":
            self.count = ctx.extract_count(fr, rng, capi.EXTRACT_EXPOSED)
            assert self.count == self.case["records"].numel()
            H.IN.ext_src = (fr, rng, capi.EXTRACT_EXPOSED, self.sdf_in.data_ptr(), self.count)
        else:
            self.count = ctx.surfnets_count(fr, rng, ALGO_TILED)
            assert self.count == (self.case["cells"].numel(), self.case["quads"].numel() // 4)
            H.IN.sn_src = (fr, rng) + self.count

    def call(self, rng):
        ctx, rec, fr, o = self.ctx, self.rec, self.fr, self.outs
        for t in o.values():
            t.view(torch.int32).fill_(PATTERN)
        if rec.kind == "jfa_grid":
            ctx.jfa_run(fr, rng, -math.inf, o["sdf"].data_ptr(), self.other.data_ptr(), H.jfa_work_bytes(rec.n), ALGO_TILED)
        elif rec.kind == "jfa_work":
            ctx.jfa_run(fr, self.other.data_ptr(), -math.inf, o["sdf"].data_ptr(), rng, H.jfa_work_bytes(rec.n), ALGO_TILED)
        elif rec.kind == "extract":
            ctx.extract(fr, rng, capi.EXTRACT_EXPOSED, self.sdf_in.data_ptr(), o["records"].data_ptr(), o["values"].data_ptr(), self.cap)
        else:
            ctx.surfnets(fr, rng, ALGO_TILED, 1, o["cells"].data_ptr(), o["xyz"].data_ptr(), o["quads"].data_ptr(), self.vcap, self.qcap)

    def untouched(self):
        self.ctx.sync()
        return [k for k, t in self.outs.items() if not bool((t.view(torch.int32) == PATTERN).all())]

    def wrong(self):
        """names of the outputs that differ from the reference (the unused tail of a worst-case buffer must still hold the pattern)"""
        self.ctx.sync()
        bad = []
        for k, t in self.outs.items():
            exp = self.case[k]
            got = t.view(exp.dtype)
            m = exp.numel()
            if not torch.equal(got[:m], exp) or not bool((got[m:].view(torch.int32) == PATTERN).all()):
                bad.append(k)
        return bad


NAMES = {"jfa_grid": "vp_jfa_start", "jfa_work": "vp_jfa_start", "extract": "vp_extract_count", "surfnets": "vp_surfnets_count"}


@pytest.mark.parametrize("rec", H.RECORDS, ids=H.rec_id)
@pytest.mark.parametrize("w", H.WRITERS, ids=lambda w: w.name)
def test_writer_against_record(dev, inputs, cases, w, rec):
    rbytes = H.range_bytes(rec)
    failures, ran, owned = [], 0, None
    ctx = capi.Context(0)
    try:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream, external=True)
        arena = torch.zeros(H.PAD + rbytes + H.PAD, dtype=torch.uint8, device=dev)       # [pad | recorded range | pad]: one allocation
        assert arena.data_ptr() % 16 == 0
        dep = _Dependent(ctx, dev, rec, cases[rec.n])
        for placement in H.PLACEMENTS:
            want, _ = H.expectation(w, rec, placement)
            if want == "skip":
                continue
            ran += 1
            inputs.sn_src = inputs.ext_src = None
            rng = arena.data_ptr() + H.PAD
            if w.kind in ("slot", "free") and want == "refused":
                # the context / the allocator chooses the pointer: the range lies at the start / in the middle / at the end of the slot
                # (asking for the slot again hands all of it out) or of an allocation of vp_malloc (which vp_free then frees)
                total = arena.numel()
                if w.kind == "slot":
                    base = ctx.workspace(SLOT, total)
                else:
                    base = owned = ctx.malloc(total)
                rng = base + {"first": 0, "inside": H.PAD, "last": total - rbytes}[placement]
            dep.establish(rng)
            if w.kind != rec.kind:
                inputs.sn_src = inputs.ext_src = None                      # a count of the writer's own
            if w.kind == "slot":
                ctx.workspace(SLOT, arena.numel() if want == "refused" else 64)        # "served": a slot elsewhere, not carved from the arena
            elif w.kind == "free":
                freed, owned = (owned, None) if want == "refused" else (ctx.malloc(64), owned)       # "served": an allocation elsewhere
                ctx.free(freed)
            else:
                nbytes = H.out_bytes(w, rec)
                off = H.place(nbytes, rbytes, placement)
                assert off % 16 == 0 and -H.PAD <= off and off + nbytes <= rbytes + H.PAD
                w.call(ctx, rng + off, nbytes)
            if want == "refused":
                try:
                    dep.call(rng)
                    failures.append("%s: served from a stale record" % placement)
                except capi.VPError as e:
                    if e.code != H.INVALID or NAMES[rec.kind] not in str(e):
                        failures.append("%s: refused with %s" % (placement, e))
                touched = dep.untouched()
                if touched:
                    failures.append("%s: outputs written: %s" % (placement, touched))
            else:
                try:
                    dep.call(rng)
                    bad = dep.wrong()
                    if bad:
                        failures.append("%s: differs from the reference: %s" % (placement, bad))
                except capi.VPError as e:
                    failures.append("%s: not served: %s" % (placement, e))
        ctx.sync()
    finally:
        inputs.sn_src = inputs.ext_src = None
        if owned is not None:                                                # a cell raised between vp_malloc and vp_free
            ctx.free(owned)
        ctx.close()
    assert ran > 0
    assert not failures, "%s against %s: %s" % (w.name, H.rec_id(rec), "; ".join(failures))
