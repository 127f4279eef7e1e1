"""What a vp_ctx keeps between calls -- the shared, GPU-free half of tests/test_ctx_records_gpu.py (part 1 below: every writer of the
ABI against every record the context keeps about a caller's buffer) and of tests/test_ctx_history_gpu.py (part 2: a catalogue of calls with
CPU references and the order in which every call follows every other one).  tests/test_ctx_history_cpu.py checks the tables themselves.
Nothing here touches a GPU at import; the callables of the tables do when they are called.

Part 2's map of vp_ctx (csrc/vp_internal.h) -- field: nodes that grow, fill or read it.
  vox.rec, tile_cnt, tile_off, tile_cur, pairs  vox_d20_* (record list, queue, tile stage); vox_fine_* leave rec at its floor (noLists on repeat)
  vox.scratch                                   vox_acc_* (accumulate = XOR through a scratch grid)
  jfa.none_row                                  jfa_tiled_96 / jfa_tiled_128 / jfa_startrun_128 (tile kernels: the row of "no seed" ids)
  jfa.work, jfa.started                         every jfa_* node (context-owned workspace; start + run in jfa_startrun_*); release frees / drops
  ws.slots[]                                    not reached: only the host forms use them, and those are excluded (they write no caller memory)
  ext.cnt, ext.off, ext.words/mode/n/total      extract_* (count + write)
  vox.total_host/event/pending/seen, vox.nbig_seen, vox.counts_known, vox.pending_job, vox.nolist_job
                                                every vox_*_tiled node: traversal (i) lets every count land, (ii) lets them land late or never; the
                                                self-loops are the "repeated job" of vox.nolist_job, every other predecessor is "another job"
  cvox.cnt, cvox.rec, cvox.base, cvox.host/event/pending, cvox.nbig_seen
                                                cvox_tiled_* (cvox_naive_* reads none of them)
  fill.flags, fill.host                         fill_*
  morph.tab, morph.tmp                          morph_dilate_* (table), morph_close_* (table + intermediate grid); morph_naive_* reads neither
  comp.cnt, comp.off, comp.host                 comp_label_*, comp_filter_*
  comp.labels, comp.sizes, comp.keep, comp.small   comp_filter_* (comp.sizes also comp_label_*: vp_components_sizes)
  sn.cnt, sn.off, sn.rank, sn.xyz, sn.words/n/algo/vertices/quads
                                                surfnets_tiled_* (2 relaxation steps: sn.xyz), surfnets_naive_* (rank volume of another size)
  edt.mask                                      edt_border_* ; edt.vol: edt_morph_* ; edt.vol2: edt_sdf_naive_* ; edt.tmp: edt_morph_* (close)
  md.keys                                       meshdist_naive_* ; md.rec, md.base, md.cnt, md.off, md.list, md.host, md.last_total: meshdist_tiled_*
  prof_on, prof_mask, prof_pending, prof_pool   traversal (ii): every ProfScope of every node
  device, cus, own_stream, stream               constant during a traversal (the tests run on the caller's stream)
The node `release` frees jfa.work, comp.labels, sn.rank, sn.xyz, edt.*, md.* between any two calls, so every op also runs as the first
after a release and regrows them.
No node: the tile kernels started from init ids.  On a whole grid the library starts every tile-kernel sequence (n >= 96) from the border
mask with the first two passes fused (jfa_tile_sequence in csrc/capi.hip); init ids feed the tile kernels only in the slab and window calls
of the multi-GPU drivers, which keep no state in a vp_ctx beyond jfa.none_row and are covered by tests/test_multi_gpu.py."""
import collections
import functools
import math
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from cuda_mesh_voxelization_amd import capi  # noqa: E402
from cuda_mesh_voxelization_amd.capi import ALGO_TILED, Frame, Window  # noqa: E402

INVALID = 10001

# =====================================================================================================================================
# Part 1: records about caller buffers, and every entry point that writes caller-addressed device memory
# =====================================================================================================================================
Record = collections.namedtuple("Record", "kind n")
# jfa_grid / jfa_work: the two ranges of the record of vp_jfa_start (the grid; an explicit workspace) -- at n = 32 the start leaves init ids
# (table kernel), at n = 96 a border mask (tile kernels); extract / surfnets: the grid vp_extract_count / vp_surfnets_count counted
RECORDS = [Record("jfa_grid", 32), Record("jfa_grid", 96), Record("jfa_work", 32), Record("jfa_work", 96), Record("extract", 32),
           Record("surfnets", 32)]
PLACEMENTS = ("first", "inside", "last", "before", "after")           # (a) (b) (c) and the two of (d)
PAD = 4 << 20                  # bytes in front of and behind the recorded range in the one allocation the cells carve up (>= any output)
SPARE = 4 << 20                # where the outputs of a writer go that are not under test
SCAN_BLOCK = 65536             # >= one scan block of vp_extract (65536 voxels) and of vp_surfnets (8192 cells), in records


def rec_id(rec):
    return "%s%d" % (rec.kind, rec.n)


def grid_bytes(n):
    return n ** 3 // 8


def jfa_work_bytes(n):
    return 2 * n ** 3 * 4 + n ** 3 // 8          # vp_jfa_workspace_bytes for n <= 1024


def range_bytes(rec):
    return jfa_work_bytes(rec.n) if rec.kind == "jfa_work" else grid_bytes(rec.n)


def unit_frame(n):
    return Frame.make(n, 1.0, (0.0, 0.0, 0.0))


@functools.lru_cache(maxsize=None)
def record_case(n):
    """The grid every record is taken of (a ball) and what the dependent calls must give for it, on the CPU:
    oracle.jfa; the numpy restatement of the EXPOSED records (as test_extract_records_match_numpy) with sdf[i] = i; surfnets_ref."""
    from oracle import oracle as O
    import surfnets_ref
    from fill_ref import bool_to_words
    s = n / 32.0
    vox = surfnets_ref.sphere(n, (15.3 * s, 16.1 * s, 15.7 * s), 100.0 * s * s)
    words = np.ascontiguousarray(bool_to_words(vox), np.uint32).reshape(-1)
    case = {"words": words, "sdf": O.jfa(words, n, 1.0, np.zeros(3, np.float32))}
    if n == 32:
        case["records"] = exposed_records(words, n)
        case["values"] = (case["records"] & np.uint64((1 << 40) - 1)).astype(np.float32)
        case["cells"], case["xyz"], case["quads"] = surfnets_ref.surfnets_numpy(words, n, 1)
    return case


def exposed_records(words, n):
    """vp_extract, VP_EXTRACT_EXPOSED: ordered records of the set voxels with an unset (or outside) face neighbour, index | face mask << 40"""
    occ = np.unpackbits(words.view(np.uint8), bitorder="little").reshape(n, n, n).astype(bool)       # [z, y, x]
    pad = np.pad(occ, 1)
    masks = np.zeros((n, n, n), np.uint64)
    for bit, (ax, d) in enumerate(((2, -1), (2, 1), (1, -1), (1, 1), (0, -1), (0, 1))):               # -X +X -Y +Y -Z +Z
        nb = np.roll(pad, -d, ax)[1:-1, 1:-1, 1:-1]
        masks |= (occ & ~nb).astype(np.uint64) << np.uint64(bit)
    lin = np.arange(n ** 3, dtype=np.uint64).reshape(n, n, n)
    sel = occ & (masks != 0)
    return lin[sel] | (masks[sel] << np.uint64(40))


# ---- the inputs of the writers (prepared once per module, outside the table) ----------------------------------------------------------
IN = None          # set by prepare_inputs


class _Inputs:
    pass


FEW = ((3, 4, 5), (9, 4, 5), (3, 11, 5), (3, 4, 13))       # four isolated voxels (x, y, z) of the 32^3 grid the counting writers count


def prepare_inputs(device):
    """Device tensors every writer reads: all-zero grids, id volumes and windows (ids 0 = the voxel (0, 0, 0): valid), a one-triangle mesh,
    a grid of four isolated voxels for the writers that need a count of their own.  The overwriting contents are therefore all-zero or
    nearly so; the outputs of the dependent calls are sized for any contents all the same."""
    import torch
    global IN
    z = lambda count, dt=torch.int32: torch.zeros(count, dtype=dt, device=device)
    I = _Inputs()
    I.fr32, I.fr96, I.fr128 = unit_frame(32), unit_frame(96), unit_frame(128)
    I.z32, I.z96, I.z128 = z(I.fr32.words), z(I.fr96.words), z(I.fr128.words)
    few = np.zeros(32 ** 3 // 32, np.uint32)
    for x, y, zz in FEW:
        few[(zz * 32 + y)] |= np.uint32(1 << x)
    I.few32 = torch.from_numpy(few.view(np.int32)).to(device)
    I.ids32, I.labels32 = z(32 ** 3), z(32 ** 3)
    I.win16, I.win8, I.cyc = z(16 * 96 * 96), z(8 * 96 * 96), z(32 * 128 * 128)
    I.xyz = torch.tensor([[4.2, 4.3, 4.1], [9.1, 5.2, 6.3], [5.5, 10.1, 7.2]], dtype=torch.float32, device=device)
    I.tri = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=device)
    I.sdf32 = torch.arange(32 ** 3, dtype=torch.float32, device=device)
    I.spare = torch.zeros(SPARE, dtype=torch.uint8, device=device)
    I.host64 = np.zeros(64, np.uint8)
    I.sn_src = I.ext_src = None          # the record's own grid and counts, where the writer is the call the record is for (see _surfnets)
    IN = I
    return I


def _p(t, off=0):
    return t.data_ptr() + off


def _sp(off=0):
    return IN.spare.data_ptr() + off


MB = 1 << 20
NEG = -math.inf


def _surfnets(which):
    """vp_surfnets needs a standing vp_surfnets_count: of its own four-voxel grid (V = 32, Q = 24), or -- against the record of that very
    count, which a count of another grid would replace -- of the record's grid itself (IN.sn_src)."""
    def call(ctx, dst, nbytes):
        if IN.sn_src is None:
            fr, g = IN.fr32, _p(IN.few32)
            nv, nq = ctx.surfnets_count(fr, g, ALGO_TILED)
            assert (nv, nq) == (32, 24)
        else:
            fr, g, nv, nq = IN.sn_src
        out = {"d_cells": _sp(), "d_xyz": _sp(MB), "d_quads": _sp(2 * MB)}
        out[which] = dst
        ctx.surfnets(fr, g, ALGO_TILED, 0, out["d_cells"], out["d_xyz"], out["d_quads"], nv, nq)
    return call


def _extract(which):
    """vp_extract likewise: its own count (VP_EXTRACT_SET of the four voxels) or the record's (IN.ext_src)"""
    def call(ctx, dst, nbytes):
        if IN.ext_src is None:
            fr, g, mode, sdf = IN.fr32, _p(IN.few32), capi.EXTRACT_SET, _p(IN.sdf32)
            cnt = ctx.extract_count(fr, g, mode)
            assert cnt == 4
        else:
            fr, g, mode, sdf, cnt = IN.ext_src
        out = {"d_records": _sp(), "d_values": _sp(MB)}
        out[which] = dst
        ctx.extract(fr, g, mode, sdf, out["d_records"], out["d_values"], cnt)
    return call


def _jfa_run(which):
    def call(ctx, dst, nbytes):
        sdf, work = (dst, _sp(MB)) if which == "d_sdf" else (_sp(), dst)
        ctx.jfa_start(IN.fr32, _p(IN.z32), work, jfa_work_bytes(32), ALGO_TILED)
        ctx.jfa_run(IN.fr32, _p(IN.z32), NEG, sdf, work, jfa_work_bytes(32), ALGO_TILED)
    return call


def _win(ptr, nbytes, planes):
    return Window.make(ptr, nbytes, planes, 0)


Writer = collections.namedtuple("Writer", "name nbytes call kind")
G32, V32, W32 = grid_bytes(32), 32 ** 3 * 4, jfa_work_bytes(32)
WIN8, WIN16, WIN96, WIN128_8, CYC = 8 * 96 * 96 * 4, 16 * 96 * 96 * 4, 96 * 96 * 96 * 4, 8 * 128 * 128 * 4, 32 * 128 * 128 * 4
PLANE32, PLANE96 = 32 * 32 // 8, 96 * 96 // 8


def _w(name, nbytes, call, kind=""):
    return Writer(name, nbytes, call, kind)


# One row per caller-addressed OUTPUT: "function" or "function:parameter" where a function has several.  call(ctx, dst_ptr, dst_bytes) makes
# the call so that this output is [dst_ptr, dst_ptr + dst_bytes); the other outputs go to IN.spare.  Slab frames and short counts keep the
# outputs small where the entry point serves them.  kind: "restart" = the call replaces the vp_jfa_start record itself; "slot" / "free" =
# the pointer is the context's / the allocator's to choose (the GPU test puts the range into the slot / into an allocation of vp_malloc and
# has it handed out again / freed); "surfnets" / "extract" = needs a count of its own.
# Not writers, by name: the host forms (*_host: they stage through the context's workspace slots and write no caller DEVICE memory -- the slots
# are reported through vp_ctx_workspace, which is in the table) and vp_multi_* (host arrays in, host arrays out, buffers of their own).
WRITERS = [
    _w("vp_free", 1, None, "free"),
    _w("vp_ctx_workspace", 0, None, "slot"),
    _w("vp_memset", 64, lambda c, d, nb: c.memset(d, 0, nb)),
    _w("vp_memcpy_d2d", 64, lambda c, d, nb: c.memcpy_d2d(d, _sp(), nb)),
    _w("vp_stream_copy", 64, lambda c, d, nb: c.stream_copy(d, _sp(), nb)),
    _w("vp_upload", 64, lambda c, d, nb: c.upload(d, IN.host64)),
    _w("vp_voxelize", 8 * PLANE32, lambda c, d, nb: c.voxelize(IN.fr32.slab(0, 8), d, _p(IN.xyz), 3, _p(IN.tri), 1, ALGO_TILED, False)),
    _w("vp_voxelize_conservative", 8 * PLANE32,
       lambda c, d, nb: c.voxelize_conservative(IN.fr32.slab(0, 8), d, _p(IN.xyz), 3, _p(IN.tri), 1, ALGO_TILED, False)),
    _w("vp_fill_interior", G32, lambda c, d, nb: c.fill_interior(IN.fr32, _p(IN.z32), d)),
    _w("vp_morph", G32, lambda c, d, nb: c.morph(IN.fr32, _p(IN.z32), d, capi.MORPH_DILATE, 1)),
    _w("vp_edt", V32, lambda c, d, nb: c.edt(IN.fr32, _p(IN.z32), d)),
    _w("vp_edt_sdf", V32, lambda c, d, nb: c.edt_sdf(IN.fr32, _p(IN.z32), NEG, d)),
    _w("vp_edt_morph", G32, lambda c, d, nb: c.edt_morph(IN.fr32, _p(IN.z32), d, capi.MORPH_DILATE, 1)),
    _w("vp_mesh_distance:d_dist2", V32, lambda c, d, nb: c.mesh_distance(IN.fr32, _p(IN.xyz), 3, _p(IN.tri), 1, 1, d, _sp())),
    _w("vp_mesh_distance:d_nearest", V32, lambda c, d, nb: c.mesh_distance(IN.fr32, _p(IN.xyz), 3, _p(IN.tri), 1, 1, _sp(), d)),
    _w("vp_components_label", V32, lambda c, d, nb: c.components_label(IN.fr32, _p(IN.z32), d)),
    _w("vp_components_sizes", 16, lambda c, d, nb: c.components_sizes(IN.fr32, _p(IN.labels32), 4, d)),
    _w("vp_components_filter", G32, lambda c, d, nb: c.components_filter(IN.fr32, _p(IN.z32), d, capi.COMP_KEEP_LARGEST, 1)),
    _w("vp_surfnets:d_cells", 32 * 8, _surfnets("d_cells"), "surfnets"),
    _w("vp_surfnets:d_xyz", 32 * 12, _surfnets("d_xyz"), "surfnets"),
    _w("vp_surfnets:d_quads", 24 * 16, _surfnets("d_quads"), "surfnets"),
    _w("vp_csg", 256, lambda c, d, nb: c.csg(d, _p(IN.z32), nb // 4, capi.OP_UNION)),
    _w("vp_jfa:d_sdf", V32, lambda c, d, nb: c.jfa(IN.fr32, _p(IN.z32), NEG, d, _sp(MB), W32, ALGO_TILED), "restart"),
    _w("vp_jfa:d_work", W32, lambda c, d, nb: c.jfa(IN.fr32, _p(IN.z32), NEG, _sp(), d, nb, ALGO_TILED), "restart"),
    _w("vp_jfa_start:d_work", W32, lambda c, d, nb: c.jfa_start(IN.fr32, _p(IN.z32), d, nb, ALGO_TILED), "restart"),
    _w("vp_jfa_run:d_sdf", V32, _jfa_run("d_sdf"), "restart"),
    _w("vp_jfa_run:d_work", W32, _jfa_run("d_work"), "restart"),
    _w("vp_jfa_init", 8 * 32 * 32 * 4, lambda c, d, nb: c.jfa_init(IN.fr32.slab(0, 8), _p(IN.z32), None, _p(IN.z32, 8 * PLANE32), d)),
    _w("vp_jfa_pass", V32, lambda c, d, nb: c.jfa_pass(IN.fr32, 1, _p(IN.ids32), None, None, d, ALGO_TILED)),
    _w("vp_jfa_finalize", V32, lambda c, d, nb: c.jfa_finalize(IN.fr32, _p(IN.z32), _p(IN.ids32), NEG, d)),
    _w("vp_jfa_last_pass:d_scratch", V32, lambda c, d, nb: c.jfa_last_pass(IN.fr32, _p(IN.ids32), None, None, d, _p(IN.z32), NEG, _sp())),
    _w("vp_jfa_last_pass:d_sdf", V32, lambda c, d, nb: c.jfa_last_pass(IN.fr32, _p(IN.ids32), None, None, _sp(MB), _p(IN.z32), NEG, d)),
    _w("vp_jfa_window_clear", WIN8, lambda c, d, nb: c.jfa_window_clear(IN.fr96, _win(d, nb, 8))),
    _w("vp_jfa_window_init", WIN8,
       lambda c, d, nb: c.jfa_window_init(IN.fr96.slab(0, 8), _p(IN.z96), None, _p(IN.z96, 8 * PLANE96), _win(d, nb, 8))),
    _w("vp_jfa_window_first_pass", WIN128_8, lambda c, d, nb: c.jfa_window_first_pass(IN.fr128.slab(0, 8), _p(IN.z128), _win(d, nb, 8))),
    _w("vp_jfa_window_first_two", WIN96, lambda c, d, nb: c.jfa_window_first_two(IN.fr96, _p(IN.z96), _win(d, nb, 96))),
    _w("vp_jfa_window_pass", WIN16,
       lambda c, d, nb: c.jfa_window_pass(IN.fr96.slab(0, 8), 1, _win(_p(IN.win16), WIN16, 16), _win(d, nb, 16))),
    _w("vp_jfa_window_last_pass:scratch", WIN16,
       lambda c, d, nb: c.jfa_window_last_pass(IN.fr96.slab(0, 8), _win(_p(IN.win16), WIN16, 16), _win(d, nb, 16), _p(IN.z96), NEG, _sp())),
    _w("vp_jfa_window_last_pass:d_sdf_region", WIN8,
       lambda c, d, nb: c.jfa_window_last_pass(IN.fr96.slab(0, 8), _win(_p(IN.win16), WIN16, 16), _win(_sp(MB), WIN16, 16), _p(IN.z96), NEG, d)),
    _w("vp_jfa_window_first_two_cyclic", CYC, lambda c, d, nb: c.jfa_window_first_two_cyclic(IN.fr128, _p(IN.z128), _win(d, nb, 32), 4, 0)),
    _w("vp_jfa_window_pass_cyclic", CYC,
       lambda c, d, nb: c.jfa_window_pass_cyclic(IN.fr128, 16, _win(_p(IN.cyc), CYC, 32), _win(d, nb, 32), 4, 0)),
    _w("vp_jfa_window_interleave", WIN8, lambda c, d, nb: c.jfa_window_interleave(IN.fr96, _win(_p(IN.win8), WIN8, 8), _win(d, nb, 8), 2, 4)),
    _w("vp_surface", 8 * PLANE32, lambda c, d, nb: c.surface(IN.fr32.slab(0, 8), _p(IN.z32), None, _p(IN.z32, 8 * PLANE32), d)),
    _w("vp_extract:d_records", 4 * 8, _extract("d_records"), "extract"),
    _w("vp_extract:d_values", 4 * 4, _extract("d_values"), "extract"),
]


def writer_function(w):
    return w.name.split(":")[0]


# Every non-const pointer parameter of the header is classified, by name: d_* is caller-addressed device memory, these are host memory
# or handles.  A parameter of neither kind fails header_prototypes' caller, so a new output cannot go unclassified.
HOST_POINTERS = {"ctx", "m", "out", "hip_stream", "total_ms", "launches", "list_entries", "lo", "hi", "id_bytes"}
WINDOWS_READ, WINDOWS_WRITTEN = {"in"}, {"out", "scratch", "w"}


def header_prototypes():
    """{function: [parameter, ...]} of every prototype of include/vphip.h, whatever it returns"""
    with open(os.path.join(ROOT, "include", "vphip.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    found = re.findall(r"\b[A-Za-z_][\w ]*?[\w*]\s*\b(vp_\w+)\s*\(([^;{()]*)\)\s*;", text, flags=re.S)
    return {name: [" ".join(q.split()) for q in params.split(",")] for name, params in found}


def header_device_outputs():
    """{entry point: [output parameter, ...]} -- the entry points of include/vphip.h that write caller-addressed device memory: a non-const pointer parameter named d_* (void** is a
    host pointer to a device pointer), a written window (the ids behind it) -- plus vp_ctx_workspace, which hands a buffer out to be filled.
    Raises on a pointer parameter it cannot classify."""
    found = collections.defaultdict(list)
    found["vp_ctx_workspace"].append("d_out")
    for name, params in header_prototypes().items():
        for p in params:
            m = re.match(r"^(const )?([\w ]+?) ?(\*+) ?(\w+)$", p)
            if not m:
                assert "*" not in p, (name, p)
                continue
            const, pointee, stars, arg = m.groups()
            if pointee == "vp_window":
                assert const and arg in WINDOWS_READ | WINDOWS_WRITTEN, "unclassified window parameter: %s(%s)" % (name, p)
                if arg in WINDOWS_WRITTEN:
                    found[name].append(arg)
            elif const or stars == "**" or arg.startswith("h_") or arg in HOST_POINTERS:
                assert not (stars == "**" and const), (name, p)
            else:
                assert arg.startswith("d_"), "unclassified pointer parameter: %s(%s)" % (name, p)
                found[name].append(arg)
    return dict(found)


def header_device_writers():
    return set(header_device_outputs())


def rounded16(nbytes):
    return (nbytes + 15) // 16 * 16


def out_bytes(w, rec):
    """bytes of the output under test (a multiple of 16: every placement keeps the 16-byte alignment the ABI asks for)"""
    if w.kind == rec.kind == "surfnets":
        c = record_case(rec.n)
        per = {"d_cells": len(c["cells"]) * 8, "d_xyz": len(c["cells"]) * 12, "d_quads": len(c["quads"]) * 16}
        return rounded16(per[w.name.split(":")[1]])
    if w.kind == rec.kind == "extract":
        c = record_case(rec.n)
        return rounded16(len(c["records"]) * (8 if w.name.endswith("d_records") else 4))
    return w.nbytes


def place(nbytes, rbytes, placement):
    """Byte offset of the output from the start of the recorded range [0, rbytes), or None where the geometry does not exist.
    first / last: the output covers exactly the first / last 16 bytes of the range; before / after: it ends exactly where the range begins /
    begins exactly where it ends; inside: strictly inside the range, 16 bytes clear of both ends -- for an output larger than the range the
    mirror image, the range strictly inside the output (an overlap no end of which coincides with an end of the other)."""
    if placement == "first":
        return 16 - nbytes
    if placement == "last":
        return rbytes - 16
    if placement == "before":
        return -nbytes
    if placement == "after":
        return rbytes
    if nbytes + 32 <= rbytes:
        return 16 + (rbytes - nbytes - 32) // 2 // 16 * 16
    if nbytes >= rbytes + 32:
        return -(16 + (nbytes - rbytes - 32) // 2 // 16 * 16)
    return None


# ---- the skipped cells, each with its reason ----------------------------------------------------------------------------------------------
SKIP_OWN_COUNT = ("the context keeps one count: the writer can only be the dependent call itself with an output on its own input grid, which "
                  "that call refuses on its own account (an output that overlaps d_words)")
SKIP_SAME_SIZE = "the output is as large as the range (within 32 bytes): it can lie neither strictly inside it nor strictly around it"


def expectation(w, rec, placement):
    """("refused" | "served" | "skip", reason or None) of the dependent call after the writer's output landed at `placement`"""
    overlap = placement in ("first", "inside", "last")
    if overlap and w.kind == rec.kind and w.kind in ("surfnets", "extract"):
        return ("skip", SKIP_OWN_COUNT)
    if w.kind not in ("slot", "free") and place(out_bytes(w, rec), range_bytes(rec), placement) is None:
        return ("skip", SKIP_SAME_SIZE)
    # one start serves one run, and only the LAST start stands: vp_jfa / vp_jfa_start / vp_jfa_run replace or consume the record wherever
    # their outputs land, so the run of the earlier start is refused in all five placements (the header: "exactly that start")
    if w.kind == "restart" and rec.kind.startswith("jfa"):
        return ("refused", None)
    return ("refused" if overlap else "served", None)


def skipped_cells():
    return [(w.name, rec_id(r), p, expectation(w, r, p)[1]) for w in WRITERS for r in RECORDS for p in PLACEMENTS if expectation(w, r, p)[0] == "skip"]


# =====================================================================================================================================
# Part 2: the catalogue of calls and the order in which every call follows every other
# =====================================================================================================================================
from cuda_mesh_voxelization_amd import mesh as M  # noqa: E402
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE  # noqa: E402

_memo = {}
SLACK = 16           # four-byte elements (64 bytes) of pattern behind every output: they must keep it


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def clear_memo():
    """forget every cached input and expectation (the reproducibility check of tests/test_ctx_history_cpu.py computes them twice)"""
    import meshdist_ref
    _memo.clear()
    meshdist_ref._cache.clear()
    record_case.cache_clear()


def mesh(name):
    return M.import_mesh(M.asset(name))


def mesh_frame(name, n):
    """(origin, vs) of the frame fitted to the mesh, as every per-feature test fits it"""
    return memo(("frame", name, n), lambda: M.frame([mesh(name)[0]], n))


def solid(name, n):
    """the reference voxelization of a mesh in its own frame: the input grid of most nodes"""
    from oracle import oracle as O
    origin, vs = mesh_frame(name, n)
    return memo(("solid", name, n), lambda: O.voxelize(mesh(name)[0], mesh(name)[1], n, vs, origin))


def specks(n):
    """a solid with loose voxels around it and holes in it: many components, something for open / close to do"""
    def make():
        rng = np.random.default_rng(1000 + n)
        return solid("bunny.obj", n) ^ (rng.random(n ** 3 // 32 * 32) < 0.004).reshape(-1, 32).dot(1 << np.arange(32, dtype=np.uint64)).astype(np.uint32)
    return memo(("specks", n), make)


def conservative(name, n):
    """the conservative surface of a mesh in its own frame, by the numpy restatement every conservative test uses (it lives in
    tests/test_conservative_cpu.py, where the other test modules import it from as well)"""
    from test_conservative_cpu import cvox_numpy
    origin, vs = mesh_frame(name, n)
    return memo(("cvox", name, n), lambda: np.ascontiguousarray(cvox_numpy(*mesh(name), n, vs, origin), np.uint32).reshape(-1))


def shell(n):
    """the conservative surface of d20: what vp_fill_interior is for"""
    return conservative("d20.obj", n)


def to_bool(words, n):
    from fill_ref import words_to_bool
    return words_to_bool(words, n)


def to_words(vox):
    from fill_ref import bool_to_words
    return np.ascontiguousarray(bool_to_words(vox), np.uint32).reshape(-1)


class Node:
    """One call (or the short fixed sequence that makes one operation) at one grid side.
    inputs()    {name: numpy array} uploaded once;  expected()  ({name: numpy array} the device outputs, {name: value} what comes back on
    the host), computed on the CPU by the reference the feature's own test uses and cached;  run(ctx, I, O) makes the call on device
    tensors I / O and returns the host values."""

    def __init__(self, name, n, frame_of, inputs, expected, run):
        self.name, self.n = name, n
        self._frame_of, self._inputs, self._expected, self._run = frame_of, inputs, expected, run

    @property
    def op(self):
        return self.name.rsplit("_", 1)[0]

    def frame(self):
        if self._frame_of is None:
            return unit_frame(self.n)
        origin, vs = mesh_frame(self._frame_of, self.n)
        return Frame.make(self.n, vs, origin)

    def inputs(self):
        return memo(("in", self.name), lambda: self._inputs(self))

    def expected(self):
        return memo(("exp", self.name), lambda: self._expected(self))

    def run(self, ctx, I, O):
        return self._run(self, ctx, I, O) or {}


def _meshin(name):
    return lambda node: {"xyz": mesh(name)[0], "tri": mesh(name)[1]}


def _vox_node(tag, name, n, algo, accumulate=False, is_conservative=False):
    from oracle import oracle as O

    def inputs(node):
        d = _meshin(name)(node)
        if accumulate:
            d["init"] = np.random.default_rng(7 + n).integers(0, 2 ** 32, n ** 3 // 32, dtype=np.uint64).astype(np.uint32)
        return d

    def expected(node):
        origin, vs = mesh_frame(name, n)
        if is_conservative:
            return {"grid": conservative(name, n)}, {}
        if accumulate:
            return {"grid": O.voxelize(*mesh(name), n, vs, origin, words=node.inputs()["init"].copy())}, {}
        return {"grid": solid(name, n)}, {}

    def run(node, ctx, I, Out):
        if accumulate:
            Out["grid"][:I["init"].numel()].copy_(I["init"])
        call = ctx.voxelize_conservative if is_conservative else ctx.voxelize
        call(node.frame(), Out["grid"].data_ptr(), I["xyz"].data_ptr(), I["xyz"].shape[0], I["tri"].data_ptr(), I["tri"].shape[0], algo, accumulate)
    return Node("%s_%d" % (tag, n), n, name, inputs, expected, run)


def _grid_node(tag, n, source, expected, call, frame_of=None):
    """a node that reads one grid `g` and writes what `expected` names"""
    return Node("%s_%d" % (tag, n), n, frame_of, lambda node: {"g": source(n)}, expected, call)


def _csg_node(n):
    from oracle import oracle as O

    def run(node, ctx, I, Out):
        Out["grid"][:I["a"].numel()].copy_(I["a"])
        ctx.csg(Out["grid"].data_ptr(), I["b"].data_ptr(), I["a"].numel(), capi.OP_DIFFERENCE)
    return Node("csg_%d" % n, n, None, lambda node: {"a": solid("bunny.obj", n), "b": solid("torus.obj", n)},
                lambda node: ({"grid": O.csg(solid("bunny.obj", n).copy(), solid("torus.obj", n), capi.OP_DIFFERENCE)}, {}),
                run)


def _oracle_sdf(n):
    from oracle import oracle as O
    origin, vs = mesh_frame("bunny.obj", n)
    return memo(("sdf", n), lambda: O.jfa(solid("bunny.obj", n), n, vs, origin))


def _bunny(n):
    return solid("bunny.obj", n)


def _surface_node(n):
    def run(node, ctx, I, Out):
        ctx.surface(node.frame(), I["g"].data_ptr(), None, None, Out["border"].data_ptr())
    return _grid_node("surface", n, _bunny, lambda node: ({"border": to_words((_oracle_sdf(n) == 0).reshape(n, n, n))}, {}), run, "bunny.obj")


def _jfa_node(tag, n, algo, split=False):
    def run(node, ctx, I, Out):
        fr, g, s = node.frame(), I["g"].data_ptr(), Out["sdf"].data_ptr()
        if split:
            ctx.jfa_start(fr, g, None, 0, algo)
            ctx.jfa_run(fr, g, NEG, s, None, 0, algo)
        else:
            ctx.jfa(fr, g, NEG, s, None, 0, algo)
    return _grid_node(tag, n, _bunny, lambda node: ({"sdf": _oracle_sdf(n)}, {}), run, "bunny.obj")


def _extract_node(n):
    def expected(node):
        rec = exposed_records(_bunny(n), n)
        return {"records": rec, "values": (rec & np.uint64((1 << 40) - 1)).astype(np.float32)}, {"count": int(rec.size)}

    def run(node, ctx, I, Out):
        fr, g = node.frame(), I["g"].data_ptr()
        cnt = ctx.extract_count(fr, g, capi.EXTRACT_EXPOSED)
        ctx.extract(fr, g, capi.EXTRACT_EXPOSED, I["sdf"].data_ptr(), Out["records"].data_ptr(), Out["values"].data_ptr(), Out["records"].numel() - SLACK * 4 // 8)
        return {"count": cnt}
    return Node("extract_%d" % n, n, None, lambda node: {"g": _bunny(n), "sdf": np.arange(n ** 3, dtype=np.float32)}, expected, run)


def _fill_node(n):
    from fill_ref import fill_numpy

    def run(node, ctx, I, Out):
        ctx.fill_interior(node.frame(), I["g"].data_ptr(), Out["grid"].data_ptr())          # (returns its rounds: not compared)
    return _grid_node("fill", n, shell, lambda node: ({"grid": np.ascontiguousarray(fill_numpy(shell(n), n), np.uint32)}, {}), run)


def _morph_node(tag, n, op, r, algo):
    from morph_ref import morph_numpy_sep

    def run(node, ctx, I, Out):
        ctx.morph(node.frame(), I["g"].data_ptr(), Out["grid"].data_ptr(), op, r, algo)
    return _grid_node(tag, n, specks, lambda node: ({"grid": np.ascontiguousarray(morph_numpy_sep(specks(n), n, op, r), np.uint32)}, {}), run)


def _edt_node(tag, n, kind):
    import edt_ref as E

    def expected(node):
        vox = to_bool(specks(n), n)
        if kind == "border":
            return {"dist2": E.edt_numpy(vox, E.BORDER).reshape(-1)}, {}
        if kind == "sdf":
            return {"sdf": E.sdf_numpy(vox, mesh_frame("bunny.obj", n)[1]).reshape(-1)}, {}
        return {"grid": to_words(E.morph_edt(vox, capi.MORPH_CLOSE, 3))}, {}

    def run(node, ctx, I, Out):
        fr, g = node.frame(), I["g"].data_ptr()
        if kind == "border":
            ctx.edt(fr, g, Out["dist2"].data_ptr(), capi.EDT_SEEDS_BORDER, ALGO_TILED)
        elif kind == "sdf":
            ctx.edt_sdf(fr, g, NEG, Out["sdf"].data_ptr(), ALGO_NAIVE)
        else:
            ctx.edt_morph(fr, g, Out["grid"].data_ptr(), capi.MORPH_CLOSE, 3, ALGO_TILED)
    return _grid_node(tag, n, specks, expected, run, "bunny.obj")


def _labels(n):
    from components_ref import label_reference
    def make():
        labels, k = label_reference(to_bool(specks(n), n), 26)
        return labels.reshape(-1).astype(np.uint32), k
    return memo(("labels", n), make)


def _comp_label_node(n):
    from components_ref import sizes_of

    def run(node, ctx, I, Out):
        fr = node.frame()
        k = ctx.components_label(fr, I["g"].data_ptr(), Out["labels"].data_ptr(), capi.CONN_26, ALGO_TILED)
        if k == Out["sizes"].numel() - SLACK:                       # (a wrong K is reported as such; the sizes array is sized for the right one)
            ctx.components_sizes(fr, Out["labels"].data_ptr(), k, Out["sizes"].data_ptr())
        return {"count": k}
    return _grid_node("comp_label", n, specks, lambda node: ({"labels": _labels(n)[0], "sizes": sizes_of(*_labels(n))}, {"count": _labels(n)[1]}), run)


def _comp_filter_node(n):
    from components_ref import KEEP_LARGEST, filter_labels

    def expected(node):
        words, kept = filter_labels(*_labels(n), KEEP_LARGEST, 1)
        return {"grid": np.ascontiguousarray(words, np.uint32)}, {"count": _labels(n)[1], "kept": kept}

    def run(node, ctx, I, Out):
        k, kept = ctx.components_filter(node.frame(), I["g"].data_ptr(), Out["grid"].data_ptr(), capi.COMP_KEEP_LARGEST, 1, capi.CONN_26, ALGO_TILED)
        return {"count": k, "kept": kept}
    return _grid_node("comp_filter", n, specks, expected, run)


def _surfnets_node(tag, n, algo, iterations):
    import surfnets_ref

    def expected(node):
        cells, xyz, quads = surfnets_ref.surfnets_numpy(_bunny(n), n, iterations)
        return ({"cells": cells, "xyz": np.ascontiguousarray(xyz, np.float32).reshape(-1), "quads": np.ascontiguousarray(quads, np.uint32).reshape(-1)},
                {"vertices": int(cells.size), "quads": int(quads.shape[0])})

    def run(node, ctx, I, Out):
        fr, g = node.frame(), I["g"].data_ptr()
        nv, nq = ctx.surfnets_count(fr, g, algo)
        ctx.surfnets(fr, g, algo, iterations, Out["cells"].data_ptr(), Out["xyz"].data_ptr(), Out["quads"].data_ptr(),
                     Out["cells"].numel() - SLACK * 4 // 8, (Out["quads"].numel() - SLACK) // 4)       # capacities: the data, not the pattern behind
        return {"vertices": nv, "quads": nq}
    return _grid_node(tag, n, _bunny, expected, run)


def _meshdist_node(tag, n, algo, band, full):
    import meshdist_ref

    def expected(node):
        origin, vs = mesh_frame("d20.obj", n)
        d, i = meshdist_ref.mesh_distance_f32(*mesh("d20.obj"), n, vs, origin, band, solid("d20.obj", n) if full else None)
        return ({"dist2": np.array(d), "nearest": np.array(i)} if full else {"dist2": np.array(d)}), {}

    def inputs(node):
        d = _meshin("d20.obj")(node)
        if full:
            d["sign"] = solid("d20.obj", n)
        return d

    def run(node, ctx, I, Out):
        ctx.mesh_distance(node.frame(), I["xyz"].data_ptr(), I["xyz"].shape[0], I["tri"].data_ptr(), I["tri"].shape[0], band, Out["dist2"].data_ptr(),
                          Out["nearest"].data_ptr() if full else 0, I["sign"].data_ptr() if full else 0, algo)
    return Node("%s_%d" % (tag, n), n, "d20.obj", inputs, expected, run)


def _release_node():
    def run(node, ctx, I, Out):
        ctx.release()
    return Node("release_0", 0, None, lambda node: {}, lambda node: ({}, {}), run)


def _catalogue():
    T, N_ = ALGO_TILED, ALGO_NAIVE
    nodes = []
    for n in (64, 128):      # 128: rows of a power-of-two number of uint4s (the 16-byte-per-lane prefix-XOR), 64: one word per lane
        nodes.append(_vox_node("vox_fine_tiled", "bunny.obj", n, T))
    for n in (64, 96):
        nodes.append(_vox_node("vox_d20_tiled", "d20.obj", n, T))
        nodes.append(_vox_node("vox_acc_tiled", "torus.obj", n, T, accumulate=True))
        nodes.append(_vox_node("cvox_tiled", "d20.obj", n, T, is_conservative=True))
    for n in (32, 96):
        nodes.append(_vox_node("vox_naive", "sphere.obj", n, N_))
        nodes.append(_csg_node(n))
        nodes.append(_surface_node(n))
        nodes.append(_extract_node(n))
        nodes.append(_edt_node("edt_border", n, "border"))
    for n in (32, 64):
        nodes.append(_vox_node("cvox_naive", "d20.obj", n, N_, is_conservative=True))
        nodes.append(_jfa_node("jfa_naive", n, N_))
        nodes.append(_fill_node(n))
        nodes.append(_morph_node("morph_dilate", n, capi.MORPH_DILATE, 2, T))
        nodes.append(_morph_node("morph_close", n, capi.MORPH_CLOSE, 5, T))
        nodes.append(_morph_node("morph_naive", n, capi.MORPH_ERODE, 1, N_))
        nodes.append(_edt_node("edt_sdf_naive", n, "sdf"))
        nodes.append(_edt_node("edt_morph", n, "morph"))
        nodes.append(_comp_label_node(n))
        nodes.append(_comp_filter_node(n))
        nodes.append(_surfnets_node("surfnets_tiled", n, T, 2))
        nodes.append(_surfnets_node("surfnets_naive", n, N_, 0))
        nodes.append(_meshdist_node("meshdist_tiled", n, T, 3, True))
        nodes.append(_meshdist_node("meshdist_naive", n, N_, 1, False))
    # vp_jfa TILED: the table kernel (64); the tile kernels, from the border mask with the first two passes fused (96: the smallest side,
    # 128: a power of two) -- whole grids never run the tile kernels from init ids (see the module's docstring)
    for n in (64, 96, 128):
        nodes.append(_jfa_node("jfa_tiled", n, T))
    for n in (64, 128):
        nodes.append(_jfa_node("jfa_startrun", n, T, split=True))
    nodes.append(_release_node())
    return nodes


CATALOGUE = _catalogue()
CIRCUIT_SEED = 20261018
CHUNK_CALLS = 300


def euler_circuit(count, seed=CIRCUIT_SEED):
    """Hierholzer on the complete digraph with self-loops on `count` nodes (in-degree = out-degree = count everywhere): a closed walk of
    count^2 edges that uses every ordered pair (u, v), u == v included, exactly once.  Returns its count^2 + 1 node indices."""
    import random
    rng = random.Random(seed)
    adj = []
    for _ in range(count):
        out = list(range(count))
        rng.shuffle(out)
        adj.append(out)
    stack, walk = [0], []
    while stack:
        u = stack[-1]
        if adj[u]:
            stack.append(adj[u].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


def chunks(walk, calls=CHUNK_CALLS):
    """The walk cut into pieces of about `calls` edges; every piece begins with the node the piece before ended with, so no pair is lost at a
    cut (that first call of a piece only sets the stage: its pair belongs to the piece before)."""
    edges = len(walk) - 1
    pieces = -(-edges // calls)
    size = -(-edges // pieces)
    return [walk[i:min(i + size, edges) + 1] for i in range(0, edges, size)]
