"""Z-slab path on ONE GPU: world_size ranks are emulated by threads, the point-to-point exchange by an
in-process loopback that implements the torch.distributed calls slab.py uses.  This drives the real
HIP kernels with slab frames and id windows (vp_jfa_window_*: halo planes next to the slab, whole slabs
a slab height away for the steps that span them, slab voxelize), which the single-GPU tests never do.  Results must be bit-identical to the whole-grid run."""
import queue
import threading

import numpy as np
import pytest
import torch

from cuda_mesh_voxelization_amd import mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame
from cuda_mesh_voxelization_amd.pipeline import Engine
from cuda_mesh_voxelization_amd.slab import HipSlabBackend, HybridSlabPipeline, SlabPipeline, TransposeSlabPipeline

pytestmark = pytest.mark.gpu


class _Req:
    def __init__(self, fn):
        self.fn = fn

    def wait(self):
        self.fn()


class LoopbackDist:
    """The subset of torch.distributed that slab.py touches, for ranks living in one process."""
    isend, irecv = "isend", "irecv"

    def __init__(self, rank, queues):
        self.rank, self.queues = rank, queues

    class P2POp:
        def __init__(self, op, tensor, peer):
            self.op, self.tensor, self.peer = op, tensor, peer

    def batch_isend_irecv(self, ops):
        reqs = []
        for o in ops:
            if o.op == "isend":
                self.queues[(self.rank, o.peer)].put(o.tensor.clone())
        for o in ops:
            if o.op == "irecv":
                def rx(o=o):
                    o.tensor.copy_(self.queues[(o.peer, self.rank)].get(timeout=120))
                reqs.append(_Req(rx))
        return reqs

    def all_to_all_single(self, output, input, output_split_sizes=None, input_split_sizes=None):
        world = max(b for _, b in self.queues) + 1
        at = 0
        for t in range(world):
            self.queues[(self.rank, t)].put(input[at:at + input_split_sizes[t]].clone())
            at += input_split_sizes[t]
        at = 0
        for s in range(world):
            output[at:at + output_split_sizes[s]].copy_(self.queues[(s, self.rank)].get(timeout=300))
            at += output_split_sizes[s]


def _run_slabs(world, frame, xyz, tri, algo, kind="halo", poison=None):
    queues = {(a, b): queue.Queue() for a in range(world) for b in range(world)}
    engines = [Engine(0) for _ in range(world)]
    pipes, errors = [], []
    for r in range(world):
        cls = {"halo": SlabPipeline, "hybrid": HybridSlabPipeline, "transpose": TransposeSlabPipeline, "transpose-p2p": TransposeSlabPipeline}[kind]
        extra = {"exchange": "p2p"} if kind == "transpose-p2p" else {}
        pipes.append(cls(HipSlabBackend(engines[r], poison=poison), frame, r, world, LoopbackDist(r, queues), **extra))
    meshes = [engines[r].mesh_to_device(xyz, tri) for r in range(world)]

    def work(r):
        try:
            torch.cuda.set_device(0)
            pipes[r].voxelize(meshes[r][0], meshes[r][1], algo=algo)
            pipes[r].jfa()
            torch.cuda.synchronize()
        except Exception as e:          # surface in the main thread
            errors.append((r, repr(e)))

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(600)
    assert not errors, errors
    if kind in ("hybrid", "transpose", "transpose-p2p"):         # every rank holds the whole bitmask there
        pw = frame.n * frame.n // 32
        words = np.concatenate([Engine.words_to_numpy(p.words[p.z0 * pw:p.z1 * pw]) for p in pipes])
    else:
        words = np.concatenate([Engine.words_to_numpy(p.words) for p in pipes])
    sdf = np.concatenate([p.sdf.cpu().numpy() for p in pipes])
    return words, sdf


@pytest.mark.parametrize("world,n,name,algo", [(2, 96, "bunny.obj", ALGO_TILED), (4, 128, "bunny.obj", ALGO_TILED),
                                               (8, 128, "torus.obj", ALGO_TILED), (4, 96, "d20.obj", ALGO_NAIVE),
                                               (2, 256, "bimba.obj", ALGO_TILED), (8, 256, "bunny.obj", ALGO_TILED),
                                               (4, 288, "bimba.obj", ALGO_TILED), (4, 1152, "bimba.obj", ALGO_TILED), (8, 1280, "bunny.obj", ALGO_TILED)])
def test_slabs_equal_whole_grid(engine, world, n, name, algo):
    """SlabPipeline (point-to-point halos before every pass): narrow passes with their halo planes next to the slab, the steps that span
    whole slabs (k >= nz) with the received slabs a slab height away (stride = nz).  n = 288 / 1152 / 1280: steps that are not powers of
    two; above n = 1024 the windows are in the 5-byte layout (two byte ranges per halo piece)."""
    import gc
    gc.collect(); torch.cuda.empty_cache()
    xyz, tri = M.import_mesh(M.asset(name))
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    ref_w = engine.voxelize(fr, dx, dt, algo=algo)
    ref_s = engine.jfa(fr, ref_w, algo=algo).cpu().numpy()
    ref_w = engine.words_to_numpy(ref_w)
    words, sdf = _run_slabs(world, fr, xyz, tri, algo)
    assert np.array_equal(words, ref_w)
    assert np.array_equal(sdf.view(np.uint32), ref_s.view(np.uint32))


@pytest.mark.parametrize("world,n,name,algo", [(2, 96, "bunny.obj", ALGO_TILED), (4, 96, "torus.obj", ALGO_NAIVE), (2, 256, "bimba.obj", ALGO_TILED),
                                               (8, 256, "bunny.obj", ALGO_TILED), (4, 512, "bimba.obj", ALGO_TILED), (8, 512, "bunny.obj", ALGO_TILED),
                                               (4, 1152, "bimba.obj", ALGO_TILED), (8, 1280, "bunny.obj", ALGO_TILED)])
def test_hybrid_slabs_equal_whole_grid(engine, world, n, name, algo):
    """HybridSlabPipeline with the real kernels: ghost planes for the wide passes inside id buffers that hold only the planes the rank
    touches (window addressing), sub-slab launches (boundary planes first) and halos sent a pass ahead for the narrow ones.  n = 1152 /
    1280: the 5-byte window layout (init ids / the first pass from the mask written in it, halos as two byte ranges)."""
    import gc
    gc.collect(); torch.cuda.empty_cache()
    xyz, tri = M.import_mesh(M.asset(name))
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    ref_w = engine.voxelize(fr, dx, dt, algo=algo)
    ref_s = engine.jfa(fr, ref_w, algo=algo).cpu().numpy()
    ref_w = engine.words_to_numpy(ref_w)
    words, sdf = _run_slabs(world, fr, xyz, tri, algo, kind="hybrid")
    assert np.array_equal(words, ref_w)
    assert np.array_equal(sdf.view(np.uint32), ref_s.view(np.uint32))


@pytest.mark.parametrize("world,n,name", [(2, 96, "bunny.obj"), (4, 128, "torus.obj"), (8, 256, "bunny.obj"), (4, 512, "bimba.obj")])
def test_ghost_slabs_equal_whole_grid(engine, world, n, name):
    """Communication-free variant: every emulated rank recomputes its ghost planes; no exchange at all."""
    from cuda_mesh_voxelization_amd.slab import GhostSlabPipeline
    xyz, tri = M.import_mesh(M.asset(name))
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    ref_w = engine.voxelize(fr, dx, dt)
    ref_s = engine.jfa(fr, ref_w).cpu().numpy()
    parts = []
    for r in range(world):
        pipe = GhostSlabPipeline(HipSlabBackend(engine), fr, r, world)
        pipe.voxelize(dx, dt)
        parts.append(pipe.jfa().cpu().numpy())
        del pipe
    sdf = np.concatenate(parts)
    assert np.array_equal(sdf.view(np.uint32), ref_s.view(np.uint32))


@pytest.mark.parametrize("world,n,poison", [(4, 1152, None), (8, 512, 0xA5), (2, 1280, 0xFF), (4, 1152, 0x5A)])
def test_ghost_windows_equal_whole_grid(engine, world, n, poison):
    """The ghost pipeline on id windows of the whole grid: plain 4-byte ids up to n = 1024, the word plane + byte plane above (here
    n = 1152 / 1280: regions that are not multiples of 8 k planes, chains of 9 / 10, 4-plane and 8-plane tiles with halo planes taken from
    the middle of a window).  Every rank's slab must equal the whole-grid run; the windows are 5 / 8 of two 8-byte volumes above n = 1024.
    `poison`: the word planes of the fresh windows are overwritten with an arbitrary byte -- the planes a pass reads without needing them
    (regions rounded outwards to whole tiles) must not matter (the test now also runs above n = 1024)."""
    import gc
    from cuda_mesh_voxelization_amd.slab import GhostSlabPipeline
    gc.collect(); torch.cuda.empty_cache()
    xyz, tri = M.import_mesh(M.asset("bimba.obj"))
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    ref_w = engine.voxelize(fr, dx, dt)
    ref_s = engine.jfa(fr, ref_w)
    nzv = fr.voxels // world
    for r in range(world):
        pipe = GhostSlabPipeline(HipSlabBackend(engine, poison=poison), fr, r, world)
        assert pipe.report()["id_window_bytes"] == fr.voxels * (5 if n > 1024 else 4)
        pipe.voxelize(dx, dt)
        s = pipe.jfa()
        assert torch.equal(s.view(torch.int32), ref_s[r * nzv:(r + 1) * nzv].view(torch.int32)), (r, poison)
        del pipe, s
        gc.collect(); torch.cuda.empty_cache()
    del ref_s, ref_w
    engine._work = None
    gc.collect(); torch.cuda.empty_cache()


def _window_parts(t, n, planes):
    """(word planes as [planes, n*n] int32, byte planes as [planes, n*n] uint8 or None) of an id window tensor"""
    vox = planes * n * n
    words = t[:vox * 4].view(torch.int32).view(planes, n * n)
    return words, (t[vox * 4:vox * 5].view(planes, n * n) if n > 1024 else None)


@pytest.mark.parametrize("world,n,name", [(2, 96, "bunny.obj"), (4, 128, "torus.obj"), (8, 128, "d20.obj"), (8, 256, "bunny.obj"), (2, 512, "bimba.obj"),
                                          (8, 512, "bunny.obj"), (4, 160, "sphere.obj"), (8, 1024, "bimba.obj"), (8, 1152, "bunny.obj"), (4, 1280, "bimba.obj"),
                                          (8, 768, "bunny.obj"), (2, 544, "torus.obj"), (4, 640, "bimba.obj"), (16, 256, "d20.obj")])
def test_cyclic_passes_equal_whole_grid_passes(engine, world, n, name):
    """Every pass of the cyclic phase, id for id: the window of rank r after the fused start and after each vp_jfa_window_pass_cyclic must
    hold exactly the planes r, r + world, ... of the whole-grid window after the same pass (vp_jfa_window_first_two / vp_jfa_window_pass:
    closed tiles at k = n/8, pair mode, compact ids above n = 1024, steps that are not powers of two at n = 96 / 160 / 1152 / 1280, the 4-KB
    tables off the powers of two at n = 544 / 640 / 768, sixteen ranks)."""
    import gc
    from cuda_mesh_voxelization_amd.capi import Window
    from cuda_mesh_voxelization_amd.slab import cyclic_passes
    gc.collect(); torch.cuda.empty_cache()
    ctx = engine.ctx
    xyz, tri = M.import_mesh(M.asset(name))
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    words = engine.voxelize(fr, dx, dt)
    border = torch.empty_like(words)
    ctx.surface(fr, words.data_ptr(), None, None, border.data_ptr())
    c = cyclic_passes(n, world)
    assert c >= 2 and ctx.jfa_cyclic_passes(fr, world) == c
    nzl = n // world
    whole = [torch.empty(ctx.jfa_window_bytes(fr, n), dtype=torch.uint8, device=engine.device) for _ in range(2)]
    mine = [[torch.empty(ctx.jfa_window_bytes(fr, nzl), dtype=torch.uint8, device=engine.device) for _ in range(2)] for _ in range(world)]
    W = lambda t, planes: Window.make(t.data_ptr(), t.numel(), planes, 0)

    def compare(cur, step):
        rw, rb = _window_parts(whole[cur], n, n)
        for r in range(world):
            gw, gb = _window_parts(mine[r][cur], n, nzl)
            assert torch.equal(gw, rw[r::world]), ("words", step, r)
            if rb is not None:
                assert torch.equal(gb, rb[r::world]), ("bytes", step, r)

    ctx.jfa_window_first_two(fr, border.data_ptr(), W(whole[0], n))
    for r in range(world):
        ctx.jfa_window_first_two_cyclic(fr, border.data_ptr(), W(mine[r][0], nzl), world, r)
    compare(0, n // 4)
    cur, k = 0, n // 8
    for _ in range(c - 2):
        ctx.jfa_window_pass(fr, k, W(whole[cur], n), W(whole[cur ^ 1], n))
        for r in range(world):
            ctx.jfa_window_pass_cyclic(fr, k, W(mine[r][cur], nzl), W(mine[r][cur ^ 1], nzl), world, r)
        cur ^= 1
        compare(cur, k)
        k //= 2
    assert k % world != 0 or k == 0
    # what the call refuses: a step that is not one of the cyclic ones, windows of the wrong size, overlapping windows
    from cuda_mesh_voxelization_amd.capi import VPError
    with pytest.raises(VPError):
        ctx.jfa_window_pass_cyclic(fr, k if k else 1, W(mine[0][0], nzl), W(mine[0][1], nzl), world, 0)
    with pytest.raises(VPError):
        ctx.jfa_window_pass_cyclic(fr, n // 8, W(whole[0], n), W(whole[1], n), world, 0)
    with pytest.raises(VPError):
        ctx.jfa_window_pass_cyclic(fr, n // 8, W(mine[0][0], nzl), W(mine[0][0], nzl), world, 0)
    del whole, mine
    gc.collect(); torch.cuda.empty_cache()


def test_window_interleave(engine):
    """vp_jfa_window_interleave: plane at + j * ranks + s of the output := plane s * count + j of the input, word planes and (n > 1024) byte planes"""
    from cuda_mesh_voxelization_amd.capi import VPError, Window
    ctx = engine.ctx
    for n, ranks, count, at, planes in ((128, 4, 3, 5, 20), (1056, 2, 2, 1, 6)):
        fr = Frame.make(n, 0.01, (0.0, 0.0, 0.0))
        src = torch.randint(0, 255, (ctx.jfa_window_bytes(fr, ranks * count),), dtype=torch.uint8, device=engine.device)
        dst = torch.zeros(ctx.jfa_window_bytes(fr, planes), dtype=torch.uint8, device=engine.device)
        ctx.jfa_window_interleave(fr, Window.make(src.data_ptr(), src.numel(), ranks * count, 0), Window.make(dst.data_ptr(), dst.numel(), planes, at), ranks, count)
        sw, sb = _window_parts(src, n, ranks * count)
        dw, db = _window_parts(dst, n, planes)
        for kind, a, b in (("w", sw, dw), ("b", sb, db)):
            if a is None:
                continue
            want = torch.zeros_like(b)
            want[at:at + ranks * count] = a.view(ranks, count, -1).transpose(0, 1).reshape(ranks * count, -1)
            assert torch.equal(b, want), (n, kind)
        with pytest.raises(VPError):
            ctx.jfa_window_interleave(fr, Window.make(src.data_ptr(), src.numel(), ranks * count, 0), Window.make(dst.data_ptr(), dst.numel(), planes, planes - 1), ranks, count)


@pytest.mark.parametrize("world,n,name,poison,kind", [(2, 96, "bunny.obj", None, "transpose"), (4, 128, "torus.obj", 0xA5, "transpose"), (8, 128, "d20.obj", None, "transpose"),
                                                      (8, 256, "bunny.obj", None, "transpose"), (2, 512, "bimba.obj", None, "transpose"), (8, 512, "bunny.obj", 0xFF, "transpose"),
                                                      (4, 160, "sphere.obj", None, "transpose"), (4, 1152, "bimba.obj", None, "transpose"), (8, 1280, "bunny.obj", 0x5A, "transpose"),
                                                      (4, 128, "torus.obj", 0xA5, "transpose-p2p"), (8, 512, "bunny.obj", None, "transpose-p2p"), (2, 96, "d20.obj", None, "transpose-p2p"),
                                                      (8, 1280, "bimba.obj", 0x5A, "transpose-p2p")])
def test_transpose_slabs_equal_whole_grid(engine, world, n, name, poison, kind):
    """TransposeSlabPipeline with the real kernels, all emulated ranks at once: cyclic planes for the steps that are multiples of the rank
    count, one all_to_all_single (in-process loopback), the weave, the remaining steps on the widened slab; "transpose-p2p": the planes as one
    batch of point-to-point operations, received straight into the slab window.  `poison`: the word planes of
    every fresh window are overwritten with an arbitrary byte -- planes nobody produces must not matter."""
    import gc
    gc.collect(); torch.cuda.empty_cache()
    xyz, tri = M.import_mesh(M.asset(name))
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    ref_w = engine.voxelize(fr, dx, dt)
    ref_s = engine.jfa(fr, ref_w).cpu().numpy()
    ref_w = engine.words_to_numpy(ref_w)
    words, sdf = _run_slabs(world, fr, xyz, tri, ALGO_TILED, kind=kind, poison=poison)
    assert np.array_equal(words, ref_w)
    assert np.array_equal(sdf.view(np.uint32), ref_s.view(np.uint32))


def test_transpose_falls_back_to_ghost_planes(engine):
    """three ranks: no cyclic distribution (not a power of two) -- the pipeline is the ghost pipeline and says so"""
    xyz, tri = M.import_mesh(M.asset("torus.obj"))
    n, world = 192, 3
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    ref_s = engine.jfa(fr, engine.voxelize(fr, dx, dt)).cpu().numpy()
    parts = []
    for r in range(world):
        pipe = TransposeSlabPipeline(HipSlabBackend(engine), fr, r, world, None)
        assert pipe.fallback is not None and pipe.report()["pipeline"] == "transpose->ghost"
        pipe.voxelize(dx, dt)
        parts.append(pipe.jfa().cpu().numpy())
    assert np.array_equal(np.concatenate(parts).view(np.uint32), ref_s.view(np.uint32))


def test_pipelines_refuse_grids_below_the_tile_kernels(engine):
    from cuda_mesh_voxelization_amd.slab import GhostSlabPipeline
    fr = Frame.make(64, 0.1, (0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="n >= 96"):
        GhostSlabPipeline(HipSlabBackend(engine), fr, 0, 2)


def test_halo_bytes_on_the_wire_above_n1024(engine):
    """What the halo / hybrid pipelines move and hold at n = 2048 x 8 (where the state no longer fits one GPU in 8-byte ids), from the byte
    ranges the exchange really posts (vp_jfa_window_span) and the window sizes the library reports -- without allocating 40-GiB windows:
    5 bytes per voxel on the wire instead of the 8 of round 4 (-37.5 %), and 35 GiB per hybrid window (was 56)."""
    from cuda_mesh_voxelization_amd.slab import hybrid_plan
    n, world = 2048, 8
    fr = Frame.make(n, 0.01, (0.0, 0.0, 0.0))
    nz = n // world
    spans = engine.ctx.jfa_window_span(fr, 3 * nz, nz - 16, nz)              # 16 halo planes below the slab of a halo-pipeline window
    assert [nb for _, nb in spans] == [16 * n * n * 4, 16 * n * n] and sum(nb for _, nb in spans) * 8 == 16 * n * n * 8 * 5
    assert spans[0][0] == (nz - 16) * n * n * 4 and spans[1][0] == 3 * nz * n * n * 4 + (nz - 16) * n * n
    wide, narrow = hybrid_plan(n, 3, world)
    planes = max(b1 + k for k, b0, b1 in wide[1:]) - min(b0 - k for k, b0, b1 in wide[1:])
    assert planes == 1792 and engine.ctx.jfa_window_bytes(fr, planes) == planes * n * n * 5 <= 35 * 2**30


def test_config4_n1024_four_slabs(engine):
    """BASELINE config 4 at its stated shape: 1,348,128 faces, n = 1024, four Z-slabs -- all three multi-GPU pipelines (RCCL-style
    halo exchange through the loopback; ghost planes without exchange; the hybrid of the two), four emulated ranks on one GPU
    with the real kernels, bit-identical to the single-GPU result."""
    import gc
    from cuda_mesh_voxelization_amd.slab import GhostSlabPipeline
    xyz, tri = M.bunny(24)
    n, world = 1024, 4
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    ref_w = engine.voxelize(fr, dx, dt)
    ref_s = engine.jfa(fr, ref_w).clone()
    engine._work = None
    gc.collect(); torch.cuda.empty_cache()
    nzv = fr.voxels // world
    for r in range(world):                                     # ghost planes: one rank at a time
        pipe = GhostSlabPipeline(HipSlabBackend(engine), fr, r, world)
        pipe.voxelize(dx, dt)
        s = pipe.jfa()
        assert torch.equal(s.view(torch.int32), ref_s[r * nzv:(r + 1) * nzv].view(torch.int32)), ("ghost", r)
        del pipe, s
        gc.collect(); torch.cuda.empty_cache()
    words, sdf = _run_slabs(world, fr, xyz, tri, ALGO_TILED)   # halo exchange: all ranks at once
    assert np.array_equal(words, engine.words_to_numpy(ref_w))
    assert np.array_equal(sdf.view(np.uint32), ref_s.cpu().numpy().view(np.uint32))
    del words, sdf
    gc.collect(); torch.cuda.empty_cache()
    words, sdf = _run_slabs(world, fr, xyz, tri, ALGO_TILED, kind="hybrid")   # ghost planes for k = 512, 256; halos for k <= 128
    assert np.array_equal(words, engine.words_to_numpy(ref_w))
    assert np.array_equal(sdf.view(np.uint32), ref_s.cpu().numpy().view(np.uint32))
    del words, sdf
    for w in (4, 8):                                           # transposed: cyclic planes for k >= w, one all-to-all, slabs for k < w
        gc.collect(); torch.cuda.empty_cache()
        words, sdf = _run_slabs(w, fr, xyz, tri, ALGO_TILED, kind="transpose")
        assert np.array_equal(words, engine.words_to_numpy(ref_w)), ("transpose", w)
        assert np.array_equal(sdf.view(np.uint32), ref_s.cpu().numpy().view(np.uint32)), ("transpose", w)
        del words, sdf


def test_config5_n2048_eight_ghost_slabs(engine):
    """BASELINE config 5 at its stated shape: the 10,785,024-face mesh, n = 2048 (5-byte id windows), eight Z-slabs, ghost-plane
    pipeline: every emulated rank's slab bit-identical to the single-GPU result (itself checked against the oracle's
    recorded run in test_gpu_parity.py)."""
    import gc
    from cuda_mesh_voxelization_amd.slab import GhostSlabPipeline
    gc.collect(); torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 230 * 2**30:
        pytest.skip("needs ~200 GiB of free HBM, %.0f GiB free" % (free / 2**30))
    xyz, tri = M.bunny(192)
    n, world = 2048, 8
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    ref_w = engine.voxelize(fr, dx, dt)
    ref_s = engine.jfa(fr, ref_w).clone()
    del ref_w
    engine._work = None
    gc.collect(); torch.cuda.empty_cache()
    nzv = fr.voxels // world
    pipe = None
    for r in range(world):
        pipe = None
        gc.collect(); torch.cuda.empty_cache()
        pipe = GhostSlabPipeline(HipSlabBackend(engine), fr, r, world)
        pipe.voxelize(dx, dt)
        s = pipe.jfa()
        assert torch.equal(s.view(torch.int32), ref_s[r * nzv:(r + 1) * nzv].view(torch.int32)), r
        del s
    del pipe, ref_s
    gc.collect(); torch.cuda.empty_cache()


def test_config5_n2048_eight_transposed_ranks(engine):
    """BASELINE config 5 (10,785,024 faces, n = 2048, 5-byte windows), eight ranks, transposed pipeline.  The ranks are walked one after
    the other on the one GPU: the cyclic phase of every rank first (its packed send buffer is kept, 5.3 GiB each), then the exchange --
    an all_to_all_single served from those buffers -- and the slab phase of every rank; every slab bit-identical to the one-GPU result."""
    import gc
    gc.collect(); torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < 230 * 2**30:
        pytest.skip("needs ~200 GiB of free HBM, %.0f GiB free" % (free / 2**30))
    xyz, tri = M.bunny(192)
    n, world = 2048, 8
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    ref_w = engine.voxelize(fr, dx, dt)
    ref_s = engine.jfa(fr, ref_w).clone()
    del ref_w
    engine._work = None
    gc.collect(); torch.cuda.empty_cache()
    sent = {}                                                   # (source rank, part) -> (tensor, split sizes)

    class StashDist:
        def __init__(self, rank):
            self.rank, self.part = rank, 0

        def all_to_all_single(self, output, input, output_split_sizes=None, input_split_sizes=None):
            at = 0
            for s_ in range(world):
                t, splits = sent[(s_, self.part)]
                off = sum(splits[:self.rank])
                output[at:at + output_split_sizes[s_]].copy_(t[off:off + splits[self.rank]])
                at += output_split_sizes[s_]
            self.part += 1

    pipes = []
    for r in range(world):
        pipe = TransposeSlabPipeline(HipSlabBackend(engine), fr, r, world, StashDist(r))
        assert pipe.fallback is None and pipe.plan["cyclic"][-1] == 8
        pipe.voxelize(dx, dt)
        pipe.pack(pipe.phase_a())
        pipe.release("cyc0", "cyc1")
        send = pipe.win["send"]
        for part, t in enumerate(pipe.be.win_spans(fr, send, 0, send.planes)):
            per_plane = t.numel() // send.planes
            sent[(r, part)] = (t, [(b - a) * per_plane for a, b in pipe.send_ranges])
        pipe.words = pipe.border = None                         # 2 GiB per rank; the slab phase needs the words again: re-voxelized below
        pipes.append(pipe)
        gc.collect(); torch.cuda.empty_cache()
    nzv = fr.voxels // world
    for r, pipe in enumerate(pipes):
        pipe.words = pipe.be.empty_u32(fr.words)
        pipe.voxelize(dx, dt)
        pipe.exchange()
        s = pipe.phase_b()
        assert torch.equal(s.view(torch.int32), ref_s[r * nzv:(r + 1) * nzv].view(torch.int32)), r
        assert pipe.bytes_received == 7 * pipe.count * n * n * 5 <= 5.5e9        # the one exchange of the job, per rank
        del s
        pipe.release("staging", "ids0", "ids1")
        pipe.words = pipe.sdf = None
        gc.collect(); torch.cuda.empty_cache()
    del pipes, sent, ref_s
    gc.collect(); torch.cuda.empty_cache()


@pytest.mark.parametrize("world,multi", [(2, "ghost"), (4, "ghost"), (4, "hybrid"), (2, "halo"), (2, "transpose"), (4, "transpose"), (4, "transpose-p2p"), (8, "ghost")])
def test_bench_multi_process_launch_on_shared_gpu(world, multi):
    """The driver's multi-GPU invocation (`python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`) end to end
    with one process per rank and the real kernels.  A one-GPU box cannot give every rank a device, so the ranks share it and
    rendezvous over gloo (VP_BENCH_SHARE_GPU=1, bench.py); everything else -- launcher env, barriers, max-over-ranks timing,
    the ghost-plane pipeline, the JSON line -- is the code the 8-GPU run executes."""
    import json, os, socket, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, VP_BENCH_SHARE_GPU="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", str(world), "--steps", "3", "--warmup", "1", "--grid-n", "256", "--multi", multi, "--full"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]                        # rank 0 prints ONE line
    # ... and the ranks' stdout carries nothing else: descriptor 1 of every rank points at stderr (RCCL prints a version banner with plain
    # printf under NCCL_DEBUG=VERSION, after the JSON line), the line leaves through a duplicate of the original descriptor
    assert [l for l in r.stdout.splitlines() if l.strip()] == lines, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == world and out["steps"] == 3 and out["scaling"] == "strong"
    assert out["config"]["world_size_seen"] == world and out["config"]["n"] == 256
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["multi"]["pipeline"] == multi.split("-")[0] and out["multi"].get("exchange", "a2a") == ("p2p" if multi.endswith("p2p") else "a2a")
    assert out["roofline"]["kernel"] == "jfa_dense" and out["roofline"]["launches"] > 0
    # the line verifies itself: every rank compared its slab with the one-GPU result on its own device, for the timed pipeline ...
    assert out["parity_ok"] is True and out["parity"]["parity_ok"] is True
    assert [r["rank"] for r in out["parity"]["per_rank"]] == list(range(world))
    assert all(r["bitmask_slab_equal"] and r["sdf_slab_equal"] for r in out["parity"]["per_rank"])
    # ... and for the OTHER pipelines, timed in the same job over shorter regions: `multi_alt` = the transposed one (one all_to_all_single --
    # here over gloo through HostStagedDist), then the remaining one of halo / ghost
    kinds = [k for k in ("transpose", "halo", "transpose-p2p", "ghost") if k != multi][:3]
    for key, kind in zip(["multi_alt"] + ["multi_alt_" + k.replace("-", "_") for k in kinds[1:]], kinds):
        alt = out[key]
        assert alt["pipeline"] == kind and alt["parity_ok"] is True, (key, alt.get("error"))
        assert alt["ms_per_step"] > 0 and alt["value"] > 0 and len(alt["per_rank"]) == world
        if kind == "ghost":
            assert alt["bytes_received_per_step_all_ranks"] == 0
        else:
            assert alt["bytes_received_per_step_all_ranks"] > 0       # ids really moved between the ranks
        if kind.startswith("transpose"):
            assert alt["report_rank0"]["pipeline"] == "transpose" and alt["report_rank0"]["cyclic_steps"][-1] % world == 0
            assert alt["report_rank0"]["exchange"] == ("p2p" if kind.endswith("p2p") else "a2a")
    assert out["multi"].get("hbm_bytes_this_rank", 0) > 0              # per-rank HBM footprint of the pipeline


@pytest.mark.parametrize("world", [1, 2])
def test_bench_bare_invocation_launches_its_own_ranks(world):
    """`python3 bench.py --gpus N` WITHOUT a launcher -- the shape of the command the driver runs for N = 1 -- must work for N > 1 too
    (VERDICT r04 #1): the parent starts the ranks as a fresh child before it touches any GPU, forwards rank 0's one JSON line and the
    child's exit code.  N = 1 stays what it was."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["VP_BENCH_SHARE_GPU"] = "1"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", str(world), "--grid-n", "256", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--full"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith('{"metric"'), r.stdout[-2000:]     # nothing but the line on stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == world and out["config"]["world_size_seen"] == world and out["config"]["n"] == 256
    assert out["value"] > 0 and out["steps"] == 3
    if world > 1:
        assert out["parity_ok"] is True and out["multi_alt"]["parity_ok"] is True and out["multi_alt"]["pipeline"] == "transpose"
        assert out["multi_alt_halo"]["parity_ok"] is True and out["multi_alt_transpose_p2p"]["parity_ok"] is True


def test_bench_plain_run_dumps_the_outputs_of_its_last_step(engine, tmp_path):
    """`bench.py --gpus 1` without --full times the step and measures nothing else; --dump-outputs writes what the last timed step handed
    its caller as float arrays (sdf and occupancy at a seeded sample of voxels, set voxels per z plane), 64 MiB at most -- equal to the
    same step run in this process."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n, d = 256, tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--grid-n", str(n), "--steps", "2", "--warmup", "1", "--dump-outputs", str(d)]
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith('{"metric"'), r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0 and out["unit"] == "Mvoxels/s" and out["dtype"] == "f32"
    assert not {"copy_peak", "n1024", "config3", "vox_large_triangles", "totals_incl_transfers", "cpu_baseline"} & set(out)
    assert set(out["kernels"]) == {"jfa_dense"} and out["roofline"]["launches"] > 0
    names = sorted(os.listdir(d))
    assert names == ["sample_index.npy", "sdf_sample.npy", "solid_per_plane.npy", "solid_sample.npy"]
    assert sum(os.path.getsize(d / f) for f in names) <= 64 << 20
    got = {f[:-4]: np.load(d / f) for f in names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    idx = got["sample_index"].astype(np.int64)
    assert idx.size == 1 << 21 and np.all(np.diff(idx) > 0) and idx[-1] < n ** 3
    xyz, tri = M.bunny(24)
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    g = engine.voxelize(fr, dx, dt, algo=ALGO_TILED)
    sdf = engine.jfa(fr, g, algo=ALGO_TILED)
    engine.sync()
    occ = np.unpackbits(engine.words_to_numpy(g).view(np.uint8), bitorder="little")
    assert np.array_equal(got["solid_sample"], occ[idx].astype(np.float32))
    assert np.array_equal(got["solid_per_plane"], occ.reshape(n, -1).sum(1).astype(np.float64))
    assert np.array_equal(got["sdf_sample"].view(np.uint32), sdf.cpu().numpy()[idx].view(np.uint32))
    del g, sdf, dx, dt


def test_bench_other_transport_hang_does_not_take_the_line_with_it():
    """bench.py runs the second transport of an N > 1 job under a watchdog: a transport that never returns (first contact with
    hardware the build never saw) must leave the timed pipeline's line and parity intact.  A limit of 1 ms stands in for the hang."""
    import json, os, socket, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, VP_BENCH_SHARE_GPU="1", MASTER_ADDR="127.0.0.1", VP_BENCH_ALT_TIMEOUT="0.001")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--grid-n", "256", "--full"]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    # exit code 2: the timed pipeline's line stands, but a status check must see that a transport never came back
    assert r.returncode != 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["parity_ok"] is True and out["parity"]["parity_ok"] is True
    assert out["multi_alt"]["parity_ok"] is None and "VP_BENCH_ALT_TIMEOUT" in out["multi_alt"]["error"]
    # VP_BENCH_LENIENT=1: the same, exit code 0
    r = subprocess.run(cmd, cwd=root, env=dict(env, VP_BENCH_LENIENT="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


def test_rccl_first_contact_with_one_rank(tmp_path):
    """What of the RCCL path CAN be exercised on a one-GPU box: a one-rank `nccl` process group (backend "nccl" IS RCCL on ROCm) running the
    exact calls of the transposed pipeline's exchange -- all_to_all_single on uint8 device tensors with explicit split sizes, between a
    kernel of this library that produces the send window and one that consumes the staging window on torch's current stream -- plus the
    barrier / all_reduce / all_gather the bench line uses.  With one rank the collective is a copy onto itself: the data path through the
    library's windows, the dtype and size handling and the stream ordering are real, the wire is not."""
    import os, subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import os, sys
        sys.path.insert(0, %r)
        import torch, torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29631")
        torch.cuda.set_device(0)
        try:
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        except Exception as e:
            print("SKIP", type(e).__name__, e); sys.exit(0)
        from cuda_mesh_voxelization_amd.capi import Frame, Window
        from cuda_mesh_voxelization_amd.pipeline import Engine
        eng = Engine(0)
        ok = True
        for n, planes in ((256, 24), (1056, 6)):                      # 4-byte ids; the 5-byte layout (two parts: two collectives)
            fr = Frame.make(n, 0.01, (0.0, 0.0, 0.0))
            nb = eng.ctx.jfa_window_bytes(fr, planes)
            send = torch.randint(0, 255, (nb,), dtype=torch.uint8, device="cuda")
            stag = torch.empty(nb, dtype=torch.uint8, device="cuda")
            out = torch.zeros(nb, dtype=torch.uint8, device="cuda")
            for off, cnt in eng.ctx.jfa_window_span(fr, planes, 0, planes):
                dist.all_to_all_single(stag[off:off + cnt], send[off:off + cnt], [cnt], [cnt])
            eng.ctx.jfa_window_interleave(fr, Window.make(stag.data_ptr(), nb, planes, 0), Window.make(out.data_ptr(), nb, planes, 0), 1, planes)
            torch.cuda.synchronize()
            ok = ok and bool(torch.equal(out, send))
        dist.barrier()
        t = torch.tensor([3.0], dtype=torch.float64, device="cuda"); dist.all_reduce(t, op=dist.ReduceOp.MAX)
        g = [torch.zeros(2, dtype=torch.int32, device="cuda")]; dist.all_gather(g, torch.tensor([1, 1], dtype=torch.int32, device="cuda"))
        ok = ok and t.item() == 3.0 and g[0].tolist() == [1, 1]
        dist.destroy_process_group()
        print("OK" if ok else "MISMATCH")
    """ % root)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    lines = [ln.strip() for ln in r.stdout.splitlines()]              # (RCCL prints a version banner of its own on stdout)
    skipped = [ln for ln in lines if ln.startswith("SKIP")]
    if skipped:
        pytest.skip("no RCCL process group on this box: " + skipped[0])
    assert r.returncode == 0 and "OK" in lines and "MISMATCH" not in lines, r.stdout[-2000:] + r.stderr[-3000:]
