"""Topological thinning on the GPU (vp_skeleton*, csrc/skeleton.hip) against the numpy restatement of tests/skeleton_ref.py, bit for bit and
statistics included: NAIVE, TILED and vp_skeleton_host on the hand cases and random grids at n = 32 (one word per row, every block touches
the wall), on the golden bunny, on slabs and bars whose faces sit at x = 31 / 32 and at block boundaries, with anchors and partial runs at
n = 64, on bunny's filled solid and a random grid at n = 96, on one solid at n = 128 against the C++ host form, on sparse bars at n = 1024
against the cropped reference; the device table; the list of active blocks; refusals, records, release, hand-over, timing keys; the CLI."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cuda_mesh_voxelization_amd import build, capi, mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import skeleton_ref as R  # noqa: E402
from test_skeleton_cpu import bunny64, check_exe, run_check  # noqa: E402,F401  (check_exe: the fixture that builds tests/cpp/skeleton_check.cpp)

pytestmark = pytest.mark.gpu
MODES = (R.KERNEL, R.CURVE)


def _frame(n):
    return Frame.make(n, 1.0, np.zeros(3, np.float32))


def _dev(engine, words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(engine.device)


def _run(engine, n, words, mode, max_iters=0, anchor=None, algo=ALGO_TILED):
    """(skeleton words, stats) of one device call, numpy"""
    fr = _frame(n)
    d = _dev(engine, words)
    a = None if anchor is None else _dev(engine, anchor)
    stats = engine.ctx.skeleton(fr, d.data_ptr(), mode, max_iters, 0 if a is None else a.data_ptr(), algo)
    ptr, rstats, side = engine.ctx.skeleton_result()
    assert ptr and side == n and rstats == stats
    g = np.empty(fr.words, np.uint32)
    engine.ctx.download(g, ptr)
    return g, stats


def _check_words(engine, n, words, mode, max_iters=0, anchor=None, tag=""):
    """NAIVE, TILED and the host entry point against the restatement on grid words"""
    exp, stats = R.thin_words(words, n, mode, max_iters, anchor)
    for algo in (ALGO_NAIVE, ALGO_TILED):
        g, s = _run(engine, n, words, mode, max_iters, anchor, algo)
        assert s == stats, (tag, mode, algo, s, stats)
        bad = g != exp
        assert not bad.any(), (tag, mode, algo, int(bad.sum()), np.flatnonzero(bad)[:4].tolist())
    g, s = engine.ctx.skeleton_host(_frame(n), words, mode, max_iters, anchor, ALGO_TILED)
    assert np.array_equal(g, exp) and s == stats, (tag, mode, "host")
    return exp, stats


def _check(engine, vox, mode, max_iters=0, anchor=None, tag=""):
    exp, stats = _check_words(engine, vox.shape[0], R.bool_to_words(vox), mode, max_iters, None if anchor is None else R.bool_to_words(anchor), tag)
    return R.words_to_bool(exp, vox.shape[0]), stats


# ---- n = 32 ---------------------------------------------------------------------------------------------------------------------
def test_hand_cases_at_32(engine):
    full = np.ones((32,) * 3, bool)
    assert _check(engine, full, R.KERNEL, tag="full")[1] == (1, 17, 32767)
    assert _check(engine, R.box(32, (5, 9, 3), (20, 17, 30)), R.KERNEL, tag="box")[1][0] == 1
    line = R.box(32, (4, 10, 20), (27, 11, 21))
    res, stats = _check(engine, line, R.CURVE, tag="line")
    assert np.array_equal(res, line) and stats == (23, 1, 0)
    assert _check(engine, line, R.KERNEL, tag="line")[1][0] == 1
    dot = R.box(32, (7, 7, 7), (8, 8, 8))
    for mode in MODES:
        assert _check(engine, dot, mode, tag="dot")[1] == (1, 1, 0)
        assert _check(engine, np.zeros((32,) * 3, bool), mode, tag="empty")[1] == (0, 1, 0)
        assert _check(engine, np.ones((32,) * 3, bool), mode, 1, tag="full, one iteration")[1][1] == 1
    res, _ = _check(engine, R.torus(32, (16, 16, 16), 9, 3), R.KERNEL, tag="torus")
    assert (R.neighbours26(res)[res] == 2).all()
    shell = R.ball(32, (16, 16, 16), 100) & ~R.ball(32, (16, 16, 16), 36)
    for mode in MODES:
        res, _ = _check(engine, shell, mode, tag="shell")
        assert not res[16, 16, 16] and R.euler(res) == 2


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("density", [0.1, 0.4, 0.6, 0.9])
def test_random_grids_at_32(engine, density, mode):
    _check(engine, R.random_grid(32, density, int(density * 100)), mode, tag="random %g" % density)


# ---- n = 64 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,expected", [(R.KERNEL, (410, 24)), (R.CURVE, (1292, 20))])
def test_golden_bunny(engine, mode, expected):
    res, stats = _check(engine, bunny64(), mode, tag="bunny64")
    assert stats[:2] == expected and R.euler(res) == -11


@pytest.mark.parametrize("mode", MODES)
def test_faces_at_word_and_block_boundaries(engine, mode):
    """slabs and bars whose faces sit at x = 31 / 32 and at y, z = 15 / 16 / 31 / 32 / 47 / 48: the fetch across words and across blocks"""
    n = 64
    for lo, hi in (((31, 4, 4), (33, 60, 60)), ((32, 15, 16), (37, 33, 48)), ((3, 16, 31), (61, 32, 33)), ((0, 0, 47), (64, 17, 64)),
                   ((27, 31, 15), (32, 49, 17)), ((30, 14, 14), (34, 18, 18))):
        _check(engine, R.box(n, lo, hi), mode, tag="box %s %s" % (lo, hi))
    both = R.box(n, (29, 2, 2), (35, 62, 9)) | R.box(n, (2, 29, 2), (62, 35, 9)) | R.box(n, (14, 14, 2), (18, 18, 62))
    _check(engine, both, mode, tag="three bars")


@pytest.mark.parametrize("mode", MODES)
def test_anchors_and_partial_runs_at_64(engine, mode):
    vox = bunny64()
    anchor = vox & R.random_grid(64, 0.01, 5)
    res, _ = _check(engine, vox, mode, anchor=anchor, tag="anchored bunny")
    assert (res & anchor).sum() == anchor.sum() > 0
    _check(engine, vox, mode, anchor=~vox, tag="anchor outside the solid")
    for k in (1, 3):
        _, stats = _check(engine, vox, mode, k, tag="bunny, %d iterations" % k)
        assert stats[1] == k
    _check(engine, vox, mode, 3, anchor, tag="anchored, 3 iterations")


# ---- n = 96 ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bunny_solid_96():
    from oracle import oracle as O
    xyz, tri = M.import_mesh(M.asset("bunny.obj"))
    origin, vs = M.frame([xyz], 96)
    return R.words_to_bool(O.voxelize(xyz, tri, 96, vs, origin), 96)


@pytest.mark.parametrize("mode", MODES)
def test_bunny_solid_at_96(engine, mode):
    vox = bunny_solid_96()
    _, stats = _check(engine, vox, mode, tag="bunny 96")
    assert 0 < stats[0] < vox.sum() / 20


@pytest.mark.parametrize("mode", MODES)
def test_random_grid_at_96(engine, mode):
    _check(engine, R.random_grid(96, 0.55, 96), mode, tag="random 96")


# ---- n = 128: against the C++ host form -----------------------------------------------------------------------------------------------
def test_solid_at_128_against_the_host_form(engine, check_exe, tmp_path):  # noqa: F811
    n = 128
    vox = R.ball(n, (50, 60, 64), 30 * 30) | R.box(n, (40, 56, 60), (127, 66, 70)) | R.torus(n, (80, 64, 30), 20, 6)
    words = R.bool_to_words(vox)
    for mode in MODES:
        got = run_check(check_exe, words, n, mode, 0, 32, "snt", str(tmp_path / "c"))
        for tag in ("naive", "tiled"):
            assert np.array_equal(got[tag][0], got["seq"][0]) and got[tag][1] == got["seq"][1], (mode, tag)
        g, s = _run(engine, n, words, mode)
        assert np.array_equal(g, got["seq"][0]) and s == got["seq"][1] and 0 < s[0] < 2000


# ---- n = 1024 ---------------------------------------------------------------------------------------------------------------------
def _bars_1024(case):
    n = 1024
    w = np.zeros((n, n, n // 32), np.uint32)                       # (z, y, word)

    def fill(x0, x1, y0, y1, z0, z1):
        row = np.zeros(n, bool)
        row[x0:x1] = True
        w[z0:z1, y0:y1, :] |= np.packbits(row, bitorder="little").view(np.uint32)
    if case == 0:                                                  # along x and along y in one slab of planes, crossing, both from wall to wall
        fill(0, n, 510, 513, 15, 17)
        fill(30, 33, 0, n, 14, 17)
        fill(1021, 1024, 0, n, 15, 18)
    else:                                                          # along z from wall to wall, and along x across block and word boundaries
        fill(510, 513, 1022, 1024, 0, n)
        fill(0, n, 1021, 1024, 511, 513)
    return w.reshape(-1)


@pytest.mark.parametrize("case,mode,iters", [(0, R.CURVE, 3), (1, R.KERNEL, 2)])
def test_sparse_bars_at_1024(engine, case, mode, iters):
    n = 1024
    words = _bars_1024(case)
    exp, stats = R.thin_words(words, n, mode, iters)
    assert stats[1] == iters and stats[2] > 0
    for algo in (ALGO_NAIVE, ALGO_TILED):
        g, s = _run(engine, n, words, mode, iters, None, algo)
        assert s == stats, (algo, s, stats)
        assert np.array_equal(g, exp), algo
    engine.ctx.release()
    torch.cuda.empty_cache()


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def test_device_table_equals_the_cpu_table(engine):
    cpu = capi.skeleton_table(ALGO_TILED)
    for algo in (ALGO_NAIVE, ALGO_TILED):
        assert np.array_equal(engine.ctx.skeleton_table_host(algo), cpu), algo


# ---- the list of active blocks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_blocks_that_never_change_come_out_untouched(engine, mode):
    """a solid in one corner keeps a few blocks busy for many iterations; a distant one-voxel line (curve mode: unchanged from the first
    iteration on) and a distant anchored box lie in blocks that leave the list after the first iteration and must come out as they went in"""
    n = 96
    solid = R.box(n, (1, 2, 3), (28, 30, 29))
    line = R.box(n, (40, 80, 81), (90, 81, 82))
    block = R.box(n, (66, 18, 50), (72, 24, 56))
    vox = solid | line | block
    res, stats = _check(engine, vox, mode, anchor=block, tag="corner solid, line, anchored box")
    assert np.array_equal(res & block, block) and stats[1] > 10
    if mode == R.CURVE:
        assert np.array_equal(res & line, line)
    else:
        assert int((res & line).sum()) == 1


# ---- refusals and shared state -----------------------------------------------------------------------------------------------------------
def test_result_is_null_before_a_build_and_after_a_release():
    ctx = capi.Context(0)
    try:
        assert ctx.skeleton_result() == (0, (0, 0, 0), 0)
        words = R.bool_to_words(R.random_grid(32, 0.5, 3))
        dw = ctx.malloc(words.nbytes)
        ctx.upload(dw, words)
        stats = ctx.skeleton(_frame(32), dw, R.CURVE)
        ptr, rstats, n = ctx.skeleton_result()
        assert ptr and rstats == stats and n == 32
        ctx.release()
        assert ctx.skeleton_result() == (0, (0, 0, 0), 0)
        ctx.free(dw)
    finally:
        ctx.close()


def test_refusals_leave_the_previous_result_and_the_outputs_untouched(engine):
    n = 32
    fr = _frame(n)
    words = R.bool_to_words(R.random_grid(n, 0.5, 5))
    before = _run(engine, n, words, R.CURVE)
    result = engine.ctx.skeleton_result()
    sentinel = torch.full((fr.words + 64,), 0x5A5A5A5A, dtype=torch.int32, device=engine.device)
    buf = sentinel.clone()
    wp = buf.data_ptr()
    slab = Frame.make(64, 1.0, np.zeros(3, np.float32), 0, 32)
    big = Frame.make(1056, 1.0, np.zeros(3, np.float32))
    lib = capi.lib()
    for frame, ptr, anchor, mode, algo, code in ((slab, wp, 0, R.CURVE, ALGO_TILED, 10002), (big, wp, 0, R.CURVE, ALGO_TILED, 10002),
                                                 (fr, 0, 0, R.CURVE, ALGO_TILED, 10001), (fr, wp + 4, 0, R.CURVE, ALGO_TILED, 10001),
                                                 (fr, wp, wp + 8, R.CURVE, ALGO_NAIVE, 10001), (fr, wp, 0, 2, ALGO_TILED, 10001),
                                                 (fr, wp, 0, -1, ALGO_NAIVE, 10001), (fr, wp, 0, R.KERNEL, 0, 10001), (fr, wp, 0, R.KERNEL, 3, 10001),
                                                 (fr, result[0], 0, R.CURVE, ALGO_TILED, 10001), (fr, wp, result[0], R.KERNEL, ALGO_NAIVE, 10001)):
        stats = (ctypes.c_uint64 * 3)(7, 8, 9)
        rc = lib.vp_skeleton(engine.ctx._h, ctypes.byref(frame), ctypes.c_void_p(ptr or None), ctypes.c_void_p(anchor or None), mode, 0, algo, stats)
        assert rc == code, (mode, algo, rc)
        assert list(stats) == [7, 8, 9]
        assert engine.ctx.skeleton_result() == result
    h = np.zeros(fr.words, np.uint32)
    for frame, mode, algo, code in ((slab, R.CURVE, ALGO_TILED, 10002), (fr, 5, ALGO_TILED, 10001), (fr, R.CURVE, 9, 10001)):
        with pytest.raises(capi.VPError) as e:
            engine.ctx.skeleton_host(frame, h, mode, 0, None, algo)
        assert e.value.code == code
    assert lib.vp_skeleton(None, ctypes.byref(fr), ctypes.c_void_p(wp), None, R.CURVE, 0, ALGO_TILED, None) == 10001
    engine.sync()
    assert torch.equal(buf, sentinel)
    g = np.empty(fr.words, np.uint32)
    engine.ctx.download(g, result[0])
    assert np.array_equal(g, before[0]) and engine.ctx.skeleton_result()[1] == before[1]


def test_result_survives_other_calls_and_feeds_them(engine):
    """hand-over: the components and the octree read the context's grid; it stands until the next vp_skeleton"""
    n = 64
    fr = _frame(n)
    vox = bunny64()
    skel, stats = engine.skeleton(fr, _dev(engine, R.bool_to_words(vox)), R.CURVE)
    exp, estats = R.thin(vox, R.CURVE)
    assert stats == estats and skel.data_ptr() == engine.ctx.skeleton_result()[0]
    labels, k = engine.components_label(fr, skel)
    assert k == 1 and int((labels != 0).sum()) == stats[0]
    nodes, _, _ = engine.octree(fr, skel)
    back = engine.octree_expand(fr, nodes.clone())
    engine.morph(fr, skel, capi.MORPH_DILATE, 1)
    engine.sync()
    assert np.array_equal(engine.words_to_numpy(back), R.bool_to_words(exp))
    assert np.array_equal(engine.words_to_numpy(skel), R.bool_to_words(exp))
    # what comes back cannot go in again without a copy: the grid would be read while it is written
    with pytest.raises(capi.VPError) as e:
        engine.ctx.skeleton(fr, skel.data_ptr(), R.CURVE)
    assert e.value.code == 10001
    again, astats = engine.skeleton(fr, skel.clone(), R.CURVE)
    assert astats == (stats[0], 1, 0) and np.array_equal(engine.words_to_numpy(again), R.bool_to_words(exp))


def test_pending_counts_on_the_result_grid_are_dropped(engine):
    n = 64
    fr = _frame(n)
    ctx = engine.ctx
    src = _dev(engine, R.bool_to_words(bunny64()))
    other = _dev(engine, R.bool_to_words(R.random_grid(96, 0.3, 2)))
    for grow in (False, True):
        ctx.skeleton(fr, src.data_ptr(), R.KERNEL, 2)
        skel = ctx.skeleton_result()[0]
        nv, nq = ctx.surfnets_count(fr, skel)                        # the skeleton is a grid like any other: counts may stand on it
        total = ctx.extract_count(fr, skel, 0)
        assert nv and nq and total
        if grow:
            ctx.skeleton(_frame(96), other.data_ptr(), R.KERNEL, 1)  # the buffer grows: the bytes the counts stood on are freed
        else:
            ctx.skeleton(fr, src.data_ptr(), R.KERNEL, 3)            # ... or written again in place
        cells = torch.empty(nv, dtype=torch.int64, device=engine.device)
        xyz = torch.empty(nv * 3, dtype=torch.float32, device=engine.device)
        quads = torch.empty(nq * 4, dtype=torch.int32, device=engine.device)
        with pytest.raises(capi.VPError) as e:
            ctx.surfnets(fr, skel, ALGO_TILED, 0, cells.data_ptr(), xyz.data_ptr(), quads.data_ptr(), nv, nq)
        assert e.value.code == 10001
        records = torch.empty(total, dtype=torch.int64, device=engine.device)
        with pytest.raises(capi.VPError) as e:
            ctx.extract(fr, skel, 0, 0, records.data_ptr(), 0, total)
        assert e.value.code == 10001
    # a count on a grid of the caller's stands through a build
    nv, nq = ctx.surfnets_count(fr, src.data_ptr())
    ctx.skeleton(fr, src.data_ptr(), R.KERNEL, 1)
    cells = torch.empty(nv, dtype=torch.int64, device=engine.device)
    xyz = torch.empty(nv * 3, dtype=torch.float32, device=engine.device)
    quads = torch.empty(nq * 4, dtype=torch.int32, device=engine.device)
    ctx.surfnets(fr, src.data_ptr(), ALGO_TILED, 0, cells.data_ptr(), xyz.data_ptr(), quads.data_ptr(), nv, nq)
    engine.sync()
    ctx.release()


def test_timing_keys(engine):
    n = 64
    fr = _frame(n)
    w = _dev(engine, R.bool_to_words(bunny64()))
    ctx = engine.ctx
    every = list(capi.EVERY_PROF_KEY)

    def keys(fn):
        ctx.prof_reset()
        ctx.prof_enable(True)
        fn()
        ctx.prof_enable(False)
        return {k: v["launches"] for k, v in ctx.prof().items()}
    i = 24                                                          # iterations of the kernel of the golden bunny
    assert keys(lambda: ctx.skeleton(fr, w.data_ptr(), R.KERNEL, 0, 0, ALGO_TILED)) == {"surface": 1 + i, "morph": 8 * i, "md_scan": 1 + i, "md_split": 1}
    assert keys(lambda: ctx.skeleton(fr, w.data_ptr(), R.KERNEL, 0, 0, ALGO_NAIVE)) == {"surface": 1 + i, "morph_naive": 8 * i, "md_split": 1}
    assert keys(lambda: ctx.skeleton(fr, w.data_ptr(), R.KERNEL, 2, 0, ALGO_TILED)) == {"surface": 3, "morph": 16, "md_scan": 3, "md_split": 1}
    assert keys(lambda: ctx.skeleton_table_host(ALGO_NAIVE)) == {"md_naive": 1}
    assert keys(lambda: ctx.skeleton_table_host(ALGO_TILED)) == {"md_brick": 1}
    assert list(capi.EVERY_PROF_KEY) == every and capi.lib().vp_abi_version() == 6


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_device_equals_host(tmp_path):
    cli = build.build_cli()
    n = 64
    dumps, lines = {}, {}
    for t in ("2", "1", "0"):
        d = tmp_path / ("t" + t)
        d.mkdir()
        p = subprocess.run([cli, M.asset("bunny.obj"), "-n", str(n), "-t", t, "--thickness", "8", "--skeleton", "curve", "-d", str(d / "x")],
                           capture_output=True, text=True, timeout=900, cwd=str(d))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert "Skeleton]: " in p.stdout
        lines[t] = [ln for ln in p.stdout.splitlines() if ln.startswith("skeleton")]
        dumps[t] = tuple(np.fromfile(str(d / ("x." + f)), np.uint32) for f in ("grid.u32", "skel.u32"))
    for t in ("2", "1"):
        assert lines[t] == lines["0"] and len(lines[t]) == 2
        for a, b in zip(dumps[t], dumps["0"]):
            assert np.array_equal(a, b), t
    exp, stats = R.thin_words(dumps["0"][0], n, R.CURVE)
    assert np.array_equal(dumps["0"][1], exp) and lines["0"][0] == "skeleton: %d voxels, %d iterations, %d deleted" % stats
    d = tmp_path / "only"
    d.mkdir()
    p = subprocess.run([cli, M.asset("bunny.obj"), "-n", str(n), "-t", "2", "--skeleton", "kernel:3", "--skeleton-only", "-e", "--surface-nets", "2",
                        "-d", str(d / "x")], capture_output=True, text=True, timeout=900, cwd=str(d))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert np.array_equal(np.fromfile(str(d / "x.grid.u32"), np.uint32), R.thin_words(dumps["0"][0], n, R.KERNEL, 3)[0])
    assert os.path.getsize(str(d / "out" / "skel_tiled_out.obj")) > 0
    for args in (["--skeleton-only"], ["--skeleton", "curve", "-g", "2"], ["--skeleton", "line"]):
        p = subprocess.run([cli, M.asset("d20.obj"), "-n", "32", "-t", "2"] + args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert p.returncode != 0, args
