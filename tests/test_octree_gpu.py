"""The sparse voxel octree on the GPU (vp_octree*, csrc/octree.hip) against the numpy restatement of tests/octree_ref.py, bit for bit --
nodes, level_offset, full_leaves and M of NAIVE, TILED and vp_octree_host -- and expand(build(g)) == g with both algos.  The sides are
those at which the code takes another path: n = 32 (P = 32: one block, the block's root is the tree's root), 64 (eight blocks: Morton
order between blocks), 96 (P = 128 > n: blocks outside the grid, three words per row, cells astride the edge), 128 (two levels above the
blocks), 160 (P = 256, five words per row), 256 (three upper levels); n = 1024 on the device against the C++ host form.  Then shared
state -- refusals, release, timing keys, other grids of the context as input -- and the CLI.  No test hands a device an invalid tree."""
import functools
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cuda_mesh_voxelization_amd import build, capi, mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import octree_ref as R  # noqa: E402
from test_octree_cpu import octree_exe, read_svo, run_build, same_tree  # noqa: E402,F401  (octree_exe: the fixture that builds tests/cpp/octree_check.cpp)

pytestmark = pytest.mark.gpu


def _frame(n):
    return Frame.make(n, 1.0, np.zeros(3, np.float32))


def _device(engine, words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(engine.device)


def _build(engine, n, d_words, algo):
    """(nodes, level_offset, full_leaves) of one device call, numpy"""
    m = engine.ctx.octree(_frame(n), d_words.data_ptr(), algo)
    d, count, lo, fl, side = engine.ctx.octree_result()
    assert d and count == m and side == n
    nodes = np.empty((m, 2), np.uint32)
    engine.ctx.download(nodes, d)
    return nodes, np.array(lo, np.uint32), np.array(fl, np.uint32)


def _check(engine, vox, tag, naive=True):
    """NAIVE, TILED and the host entry against the restatement; both expands and the host expand give the grid back"""
    n = vox.shape[0]
    words = R.bool_to_words(vox)
    exp = R.build_numpy(vox)
    d = _device(engine, words)
    for algo in (ALGO_NAIVE, ALGO_TILED) if naive else (ALGO_TILED,):
        got = _build(engine, n, d, algo)
        assert got[0].shape == exp[0].shape and np.array_equal(got[0], exp[0]), (tag, algo, got[0].shape, exp[0].shape,
                                                                               np.argwhere(got[0] != exp[0])[:4].tolist() if got[0].shape == exp[0].shape else None)
        assert np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2]), (tag, algo, got[1].tolist(), exp[1].tolist(), got[2].tolist(), exp[2].tolist())
        nodes, _, _ = engine.octree(_frame(n), d, algo)
        for ealgo in (ALGO_NAIVE, ALGO_TILED):
            back = engine.octree_expand(_frame(n), nodes, ealgo)
            engine.sync()
            assert torch.equal(back, d), (tag, algo, ealgo, int((back != d).sum()))
    host = engine.ctx.octree_host(_frame(n), words, ALGO_TILED)
    assert all(np.array_equal(a, b) for a, b in zip(host, exp)), (tag, "host")
    assert np.array_equal(engine.ctx.octree_expand_host(_frame(n), exp[0], ALGO_TILED), words), (tag, "expand host")
    assert R.popcount_from_full_leaves(exp[2], n) == int(vox.sum())
    return exp


@functools.lru_cache(maxsize=None)
def _mesh_grid(engine, name, n, kind):
    xyz, tri = M.import_mesh(M.asset(name))
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    if kind == "solid":
        g = engine.voxelize(fr, dx, dt)
    else:
        g = engine.voxelize_conservative(fr, dx, dt)
        if kind == "filled":
            g = engine.fill_interior(fr, g)[0]
    engine.sync()
    return engine.words_to_numpy(g).copy()


# ---- the sizes ----------------------------------------------------------------------------------------------------------------------
def test_at_32_the_block_root_is_the_tree_root(engine):
    for tag, vox in (("empty", np.zeros((32,) * 3, bool)), ("full", np.ones((32,) * 3, bool)), ("one voxel", R.single(32, 31, 0, 17))):
        exp = _check(engine, vox, tag + " at 32")
        assert len(exp[0]) == (5 if tag == "one voxel" else 1)
    assert R.build_numpy(np.ones((32,) * 3, bool))[0].tolist() == [[0xFFFF, 0]]
    for k, density in enumerate((0.03, 0.5, 0.97)):
        vox = R.random_bool(32, density, 170 + k)
        _check(engine, vox, "random %g at 32" % density)
        _check(engine, ~vox, "complement of random %g at 32" % density)


def test_at_64_morton_order_between_blocks(engine):
    _check(engine, np.ones((64,) * 3, bool), "full 64")
    assert R.counts_of(_check(engine, R.box(64, 8, 40), "box at 64")[1], 64) == [1, 8, 26, 0, 0, 0]
    assert R.counts_of(_check(engine, R.single(64, 40, 3, 21), "one voxel at 64")[1], 64) == [1] * 6
    _check(engine, R.random_bool(64, 0.5, 64), "random 0.5 at 64")


def test_at_96_blocks_outside_the_grid_and_cells_astride_the_edge(engine):
    assert R.counts_of(_check(engine, np.ones((96,) * 3, bool), "full 96")[1], 96) == [1, 7, 0, 0, 0, 0, 0]
    assert R.counts_of(_check(engine, R.ball(96, (48, 48, 48), 1600), "ball at 96")[1], 96) == [1, 8, 26, 113, 391, 1384, 3769]
    _check(engine, R.random_bool(96, 0.97, 96), "random 0.97 at 96")


@pytest.mark.parametrize("kind", ["shell", "filled"])
def test_bunny_at_96(engine, kind):
    vox = R.words_to_bool(_mesh_grid(engine, "bunny.obj", 96, kind), 96)
    assert vox.any() and not vox.all()
    _check(engine, vox, "bunny %s at 96" % kind)


def test_at_128_two_levels_above_the_blocks(engine):
    assert R.counts_of(_check(engine, R.ball(128, (64, 64, 64), 2500), "ball at 128")[1], 128) == [1, 8, 56, 176, 668, 2245, 5884]
    for name in ("bunny.obj", "torus.obj"):
        vox = R.words_to_bool(_mesh_grid(engine, name, 128, "solid"), 128)
        assert vox.any()
        _check(engine, vox, name + " at 128")


def test_at_160_five_words_per_row(engine):
    _check(engine, R.random_bool(160, 0.9, 160), "random 0.9 at 160")
    vox = R.words_to_bool(_mesh_grid(engine, "d20.obj", 160, "solid"), 160)
    assert vox.any()
    _check(engine, vox, "d20 at 160")


def test_bunny_at_256_three_upper_levels(engine):
    vox = R.words_to_bool(_mesh_grid(engine, "bunny.obj", 256, "solid"), 256)
    exp = _check(engine, vox, "bunny at 256")
    assert len(exp[0]) > 30000


def test_a_tree_built_at_96_expands_into_128_as_the_zero_padded_grid(engine):
    vox = R.ball(96, (48, 48, 48), 1600)
    nodes, lo, fl = engine.octree(_frame(96), _device(engine, R.bool_to_words(vox)), ALGO_TILED)
    padded = _device(engine, R.bool_to_words(R.embed(vox, 128)))
    for algo in (ALGO_NAIVE, ALGO_TILED):
        assert torch.equal(engine.octree_expand(_frame(128), nodes, algo), padded), algo
    again, lo2, fl2 = engine.octree(_frame(128), padded, ALGO_TILED)
    assert lo2 == lo and fl2 == fl and len(again) == 5692


# ---- n = 1024 -------------------------------------------------------------------------------------------------------------------------
def test_boxes_at_1024_against_the_host_form(engine, octree_exe, tmp_path):
    """TILED only, compared on the device: a few misaligned boxes and one set voxel.  The host form is VOX::BuildOctree<OPENMP>, the same
    function as SEQUENTIAL, which the CPU suite pins to the restatement."""
    n = 1024
    boxes = [(37, 421, 100, 613, 5, 77), (500, 1024, 0, 31, 900, 1024), (640, 705, 640, 705, 640, 705), (1, 2, 1022, 1024, 511, 513)]
    words = R.boxes_words(n, boxes + [(1000, 1001, 17, 18, 300, 301)])
    pop = sum((b[1] - b[0]) * (b[3] - b[2]) * (b[5] - b[4]) for b in boxes) + 1
    tree, back = run_build(octree_exe, words, n, 32, "o", str(tmp_path / "h"))["omp"]
    assert np.array_equal(back, words) and tree["M"] > 1000
    fr = _frame(n)
    d = _device(engine, words)
    nodes, lo, fl = engine.octree(fr, d, ALGO_TILED)
    assert len(nodes) == tree["M"] and lo == tree["lo"].tolist() and fl == tree["fl"].tolist()
    assert torch.equal(nodes, _device(engine, tree["nodes"].reshape(-1).copy()).view(-1, 2))
    assert torch.equal(engine.octree_expand(fr, nodes, ALGO_TILED), d)
    assert sum(fl[l] * (1024 >> (l + 1)) ** 3 for l in range(10)) == pop
    del nodes, d
    engine.ctx.release()
    torch.cuda.empty_cache()


# ---- other grids of the context go in directly -----------------------------------------------------------------------------------------
def test_the_thin_grid_and_a_winding_grid_feed_octree_directly(engine):
    n = 64
    fr = _frame(n)
    vox = R.ball(n, (32, 32, 32), 400)
    vox[30:34, 30:34, :] = True
    d = _device(engine, R.bool_to_words(vox))
    _, thin = engine.thickness(fr, d, 8, 9)
    nodes, lo, fl = engine.octree(fr, thin, ALGO_TILED)
    engine.sync()
    thin_np = engine.words_to_numpy(thin).copy().view(np.uint32)
    exp = R.build_numpy(R.words_to_bool(thin_np, n))
    assert thin_np.any() and np.array_equal(nodes.cpu().numpy().view(np.uint32), exp[0]) and lo == exp[1].tolist() and fl == exp[2].tolist()
    xyz, tri = M.import_mesh(M.asset("torus.obj"))
    origin, vs = M.frame([xyz], n)
    mfr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    _, inside = engine.winding(mfr, dx, dt)
    nodes, lo, fl = engine.octree(mfr, inside, ALGO_NAIVE)
    engine.sync()
    inside_np = engine.words_to_numpy(inside).copy().view(np.uint32)
    exp = R.build_numpy(R.words_to_bool(inside_np, n))
    assert inside_np.any() and np.array_equal(nodes.cpu().numpy().view(np.uint32), exp[0]) and fl == exp[2].tolist()
    assert torch.equal(engine.octree_expand(mfr, nodes), inside)


# ---- refusals and shared state ---------------------------------------------------------------------------------------------------------
NULL_RESULT = (0, 0, [0] * 11, [0] * 11, 0)


def test_result_is_null_before_a_build_and_after_a_release():
    ctx = capi.Context(0)
    try:
        assert ctx.octree_result() == NULL_RESULT and ctx.octree_expand_result() == (0, 0)
        words = R.random_grid(32, 0.9, 3)
        dw = ctx.malloc(words.nbytes)
        ctx.upload(dw, words)
        m = ctx.octree(_frame(32), dw, ALGO_TILED)
        d, count, lo, fl, n = ctx.octree_result()
        assert d and count == m == lo[10] and n == 32 and lo[:2] == [0, 1]
        assert ctx.octree_expand_result() == (0, 0)
        ctx.octree_expand(_frame(32), d, m, ALGO_TILED)
        g, side = ctx.octree_expand_result()
        back = np.empty_like(words)
        ctx.download(back, g)
        assert g and side == 32 and np.array_equal(back, words)
        # the context's grid is a grid like any other: it goes straight back into a build, and gives the same tree
        assert ctx.octree(_frame(32), g, ALGO_NAIVE) == m and ctx.octree_result()[2:4] == (lo, fl)
        ctx.release()
        assert ctx.octree_result() == NULL_RESULT and ctx.octree_expand_result() == (0, 0)
        ctx.free(dw)
    finally:
        ctx.close()


def test_refusals_leave_the_previous_result_and_a_sentinel_untouched(engine):
    n = 32
    words = R.random_grid(n, 0.5, 5)
    fr = _frame(n)
    d = _device(engine, words)
    before = _build(engine, n, d, ALGO_TILED)
    result = engine.ctx.octree_result()
    assert result[1] * 8 >= fr.words * 4                               # the node buffer holds a whole grid: it can be offered as one
    sentinel = torch.full((fr.words + 64,), 0x5A5A5A5A, dtype=torch.int32, device=engine.device)
    buf = sentinel.clone()
    wp = buf.data_ptr()
    slab = Frame.make(64, 1.0, np.zeros(3, np.float32), 0, 32)
    big = Frame.make(2048, 1.0, np.zeros(3, np.float32))
    for frame, ptr, algo, code in ((slab, wp, ALGO_TILED, 10002), (big, wp, ALGO_TILED, 10002), (fr, 0, ALGO_TILED, 10001),
                                   (fr, wp + 4, ALGO_TILED, 10001), (fr, wp, 0, 10001), (fr, wp, 3, 10001),
                                   (fr, result[0], ALGO_TILED, 10001), (fr, result[0], ALGO_NAIVE, 10001)):
        with pytest.raises(capi.VPError) as e:
            engine.ctx.octree(frame, ptr, algo)
        assert e.value.code == code, (algo, e.value.code)
        assert engine.ctx.octree_result() == result
    # expand: the same envelope, and the context's own grid is refused as nodes; the grid of the last expand stays as it is
    engine.ctx.octree_expand(fr, result[0], result[1], ALGO_TILED)
    grid = engine.ctx.octree_expand_result()
    assert grid[0] and grid[1] == n
    for frame, nodes_ptr, count, algo, code in ((slab, result[0], result[1], ALGO_TILED, 10002), (big, result[0], result[1], ALGO_TILED, 10002),
                                                (fr, 0, result[1], ALGO_TILED, 10001), (fr, result[0], 0, ALGO_TILED, 10001),
                                                (fr, result[0], 1 << 28, ALGO_TILED, 10001), (fr, result[0] + 8, result[1] - 1, ALGO_NAIVE, 10001),
                                                (fr, result[0], result[1], 0, 10001), (fr, result[0], result[1], 3, 10001),
                                                (fr, grid[0], 1, ALGO_TILED, 10001), (fr, grid[0] + 16, 4, ALGO_NAIVE, 10001)):
        with pytest.raises(capi.VPError) as e:
            engine.ctx.octree_expand(frame, nodes_ptr, count, algo)
        assert e.value.code == code, (count, algo, e.value.code)
        assert engine.ctx.octree_expand_result() == grid and engine.ctx.octree_result() == result
    back = np.empty(fr.words, np.uint32)
    engine.ctx.download(back, grid[0])
    assert np.array_equal(back, words)
    h = np.zeros(fr.words, np.uint32)
    for frame, algo, code in ((slab, ALGO_TILED, 10002), (fr, 9, 10001)):
        with pytest.raises(capi.VPError) as e:
            engine.ctx.octree_host(frame, h, algo)
        assert e.value.code == code
    # a capacity below the count: refused
    with pytest.raises(capi.VPError) as e:
        engine.ctx.octree_host(fr, words, ALGO_TILED, capacity=3)
    assert e.value.code == 10001
    # the host expand refuses what the validator refuses, before anything is uploaded
    bad = before[0].copy()
    bad[0, 0] |= 0x10000
    with pytest.raises(capi.VPError) as e:
        engine.ctx.octree_expand_host(fr, bad, ALGO_TILED)
    assert e.value.code == 10001
    engine.sync()
    assert torch.equal(buf, sentinel)
    again = _build(engine, n, d, ALGO_TILED)
    assert all(np.array_equal(a, b) for a, b in zip(before, again))


def test_buffers_are_released_and_regrown(engine):
    n = 256
    fr = _frame(n)
    w = _device(engine, np.tile(R.random_grid(64, 0.9, 9), 64))         # any words will do: noise, so the tree is large
    ctx = engine.ctx
    first = engine.octree(fr, w, ALGO_TILED)
    kept = first[0].clone()
    engine.sync()
    assert len(kept) * 8 > fr.voxels // 8                                # worse than the grid: the buffer is sized from the count
    torch.cuda.empty_cache()
    before = torch.cuda.mem_get_info()[0]
    ctx.release()
    freed = torch.cuda.mem_get_info()[0] - before
    assert freed >= len(kept) * 8, freed
    assert ctx.octree_result() == NULL_RESULT and ctx.octree_expand_result() == (0, 0)
    again = engine.octree(fr, w, ALGO_TILED)
    engine.sync()
    assert torch.equal(kept, again[0]) and first[1:] == again[1:]
    ctx.release()
    torch.cuda.empty_cache()


def test_timing_keys(engine):
    n = 64
    fr = _frame(n)
    w = _device(engine, R.random_grid(n, 0.5, 4))
    ctx = engine.ctx
    every = list(capi.EVERY_PROF_KEY)

    def keys(fn):
        ctx.prof_reset()
        ctx.prof_enable(True)
        fn()
        ctx.prof_enable(False)
        return {k: v["launches"] for k, v in ctx.prof().items()}
    assert keys(lambda: ctx.octree(fr, w.data_ptr(), ALGO_TILED)) == {"md_count": 1, "md_scan": 1, "md_write": 1}
    assert keys(lambda: ctx.octree(fr, w.data_ptr(), ALGO_NAIVE)) == {"md_prefill": 1, "md_scan": 1, "md_naive": 1}
    d, m = ctx.octree_result()[:2]
    for algo in (ALGO_NAIVE, ALGO_TILED):
        assert keys(lambda: ctx.octree_expand(fr, d, m, algo)) == {"md_fill": 1}
    assert torch.equal(engine.octree_expand(fr, engine.octree(fr, w)[0]), w)
    assert list(capi.EVERY_PROF_KEY) == every and len(capi.EVERY_PROF_KEY) == 55 and len(capi.HEADER_PROF_KEYS) == 64
    for i, name in enumerate(capi.HEADER_PROF_KEYS):
        assert capi.lib().vp_prof_name(i).decode() == name


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_every_type_writes_the_same_file(octree_exe, tmp_path):
    cli = build.build_cli()
    n = 64
    for k, args in enumerate(([], ["--morph", "dilate:2,fill,erode:2"], [M.asset("torus.obj"), "-p", "1"])):
        files = {}
        for t in ("2", "1", "0"):
            d = tmp_path / ("c%dt%s" % (k, t))
            d.mkdir()
            p = subprocess.run([cli, M.asset("bunny.obj")] + args + ["-n", str(n), "-t", t, "--octree", "-d", str(d / "x")], capture_output=True,
                               text=True, timeout=900, cwd=str(d))
            assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
            assert "Octree]: " in p.stdout and "octree: n 64, P 64, nodes " in p.stdout
            svo = glob.glob(str(d / "out" / "*.svo"))
            assert len(svo) == 1
            files[t] = open(svo[0], "rb").read()
            q = subprocess.run([octree_exe, "read", svo[0], "t" if t == "2" else "s", str(d / "back")], capture_output=True, text=True, timeout=300)
            assert q.returncode == 0, q.stdout + q.stderr
            dump = np.fromfile(str(d / "x.grid.u32"), np.uint32)
            assert dump.any() and np.array_equal(np.fromfile(str(d / "back.grid.u32"), np.uint32), dump), (k, t)
        assert files["2"] == files["1"] == files["0"], k
    p = subprocess.run([cli, M.asset("d20.obj"), "-n", "64", "-t", "2", "--octree", "-g", "2"], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    assert p.returncode != 0
