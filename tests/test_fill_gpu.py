"""Interior fill on the GPU (vp_fill_interior): hand cases, random grids near the percolation threshold of the empty phase and
serpentine mazes against the numpy reference of tests/fill_ref.py; convex meshes, exact at every size (fill(conservative) ==
conservative | solid); closed meshes against the host flood of `vpcli --fill`; open meshes and soups; refusals and the state the call
shares with the rest of the context; the CLI composition (fill before CSG and sdf)."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from cuda_mesh_voxelization_amd import build, capi, mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_TILED, Frame
from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fill_ref import bool_to_words, fill_numpy, hand_cases, maze, random_grid, words_to_bool  # noqa: E402
from test_conservative_cpu import cvox_numpy  # noqa: E402
from test_export import _check_file, _check_sdf_files  # noqa: E402

pytestmark = pytest.mark.gpu

FILL_HIP = os.path.join(os.path.dirname(capi.__file__), "csrc", "fill.hip")


def _batch():
    with open(FILL_HIP) as f:
        return int(re.search(r"constexpr uint32_t kFillBatch = (\d+);", f.read()).group(1))


@pytest.fixture(scope="module")
def cli():
    return build.build_cli()


def _unit_frame(n):
    return Frame.make(n, 1.0 / n, np.zeros(3, np.float32))


def _fill(engine, n, words):
    fr = _unit_frame(n)
    d = torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).to(engine.device)
    out, rounds = engine.fill_interior(fr, d)
    engine.sync()
    return engine.words_to_numpy(out).copy(), rounds


def _frame(xyz, n):
    origin, vs = M.frame([xyz], n)
    return Frame.make(n, vs, origin), origin, vs


@pytest.mark.parametrize("n", [32, 64, 96])
def test_hand_cases(engine, n):
    for name, vox, exp in hand_cases(n):
        words = bool_to_words(vox)
        got, rounds = _fill(engine, n, words)
        assert np.array_equal(got, bool_to_words(exp)), (n, name, np.argwhere(words_to_bool(got, n) != exp)[:8].tolist())
        assert np.array_equal(got, fill_numpy(words, n)), (n, name)
        assert rounds >= 1, (n, name)


@pytest.mark.parametrize("n", [32, 64, 128])
@pytest.mark.parametrize("density", [0.2, 0.5, 0.65, 0.69, 0.75])
def test_random_grids(engine, n, density):
    for seed in range(3):
        words = random_grid(n, density, 1000 * n + int(100 * density) + seed)
        got, _ = _fill(engine, n, words)
        exp = fill_numpy(words, n)
        assert np.array_equal(got, exp), (n, density, seed, int(np.count_nonzero(got != exp)))


@pytest.mark.parametrize("n", [64, 256])
def test_maze(engine, n):
    words, length = maze(n, seed=n)
    assert length > 4 * n
    got, rounds = _fill(engine, n, words)
    exp = fill_numpy(words, n)
    assert np.array_equal(got, exp), (n, int(np.count_nonzero(got != exp)))
    assert not np.array_equal(exp, words)                   # the isolated cavities were filled
    assert rounds > _batch(), rounds                        # more than one batch ran: the batch and early-exit logic was exercised


def test_maze_runs_three_batches(engine):
    """the smallest maze whose rounds fill more than two batches: both halves of the flag ring (csrc/round_ring.h) are reused"""
    n = 32
    words, _ = maze(n, seed=n)
    got, rounds = _fill(engine, n, words)
    assert np.array_equal(got, fill_numpy(words, n)), int(np.count_nonzero(got != fill_numpy(words, n)))
    assert rounds > 2 * _batch(), rounds


def _convex(xyz, tri):
    v = xyz.astype(np.float64)
    t = tri.astype(np.int64)
    nrm = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 1]])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    side = np.einsum("fk,fvk->fv", nrm, v[None, :, :] - v[t[:, 0]][:, None, :])
    scale = np.abs(v).max()
    return bool(np.all(side <= 1e-5 * scale) or np.all(side >= -1e-5 * scale))


@pytest.mark.parametrize("name", ["d20.obj", "sphere.obj"])
def test_convex_meshes_exact(engine, name):
    """a voxel outside both the conservative and the solid grid has a box disjoint from the convex body, so a monotone axis path of
    such boxes reaches the boundary: fill(conservative) == conservative | solid, exactly, at every size"""
    xyz, tri = M.import_mesh(M.asset(name))
    assert _convex(xyz, tri), name
    dx, dt = engine.mesh_to_device(xyz, tri)
    for n in (32, 160, 512, 1024, 2048):
        fr, _, _ = _frame(xyz, n)
        c = engine.voxelize_conservative(fr, dx, dt)
        s = engine.voxelize(fr, dx, dt)
        f, rounds = engine.fill_interior(fr, c)
        engine.sync()
        bad = torch.nonzero(f != (c | s))
        assert bad.numel() == 0, (name, n, rounds, bad[:4].tolist())
        assert bool((s != 0).any()), (name, n)
        del c, s, f
        torch.cuda.empty_cache()


def _host_fill(cli, path, n, tmp_path, t=3):
    prefix = str(tmp_path / "host")
    p = subprocess.run([cli, path, "-n", str(n), "-t", str(t), "--conservative", "--fill", "-d", prefix], capture_output=True, text=True,
                       timeout=3000, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return np.fromfile(prefix + ".grid.u32", np.uint32)


def _closed(engine, cli, tmp_path, path, n, t=3):
    xyz, tri = M.import_mesh(path)
    fr, _, _ = _frame(xyz, n)
    dx, dt = engine.mesh_to_device(xyz, tri)
    c = engine.voxelize_conservative(fr, dx, dt)
    s = engine.voxelize(fr, dx, dt)
    f, _ = engine.fill_interior(fr, c)
    engine.sync()
    assert bool(((s & ~f) == 0).all()), (path, n)           # fill(conservative) contains the solid
    got = engine.words_to_numpy(f).copy()
    host = np.empty_like(got)
    engine.ctx.fill_interior_host(fr, engine.words_to_numpy(c).copy(), host)
    assert np.array_equal(host, got), (path, n)
    exp = _host_fill(cli, path, n, tmp_path, t)
    assert np.array_equal(got, exp), (path, n, int(np.count_nonzero(got != exp)))


@pytest.mark.parametrize("name", ["bunny.obj", "bimba.obj", "torus.obj"])
def test_closed_meshes_equal_the_host_flood(engine, cli, tmp_path, name):
    for n in (64, 256, 512):
        _closed(engine, cli, tmp_path, M.asset(name), n, t=0 if n == 64 else 3)


def test_bunny24_1024_equals_the_host_flood(engine, cli, tmp_path):
    path = str(tmp_path / "bunny24.obj")
    M.export_obj(path, *M.bunny(24))
    _closed(engine, cli, tmp_path, path, 1024)


def _cap_removed_sphere():
    xyz, tri = M.import_mesh(M.asset("sphere.obj"))
    lo, hi = xyz[:, 2].min(), xyz[:, 2].max()
    c, r = 0.5 * (lo + hi), 0.5 * (hi - lo)
    cz = xyz[tri.astype(np.int64)].mean(axis=1)[:, 2]
    keep = cz - c <= 0.6 * r
    assert 0 < np.count_nonzero(~keep) < tri.shape[0] // 2
    return xyz, np.ascontiguousarray(tri[keep])


@pytest.mark.parametrize("n", [64, 256])
def test_open_sphere_leaks(engine, n):
    xyz, tri = _cap_removed_sphere()
    fr, _, _ = _frame(xyz, n)
    dx, dt = engine.mesh_to_device(xyz, tri)
    c = engine.voxelize_conservative(fr, dx, dt)
    f, _ = engine.fill_interior(fr, c)
    engine.sync()
    assert torch.equal(f, c), n


def test_soup_fills_like_the_indexed_mesh(engine):
    xyz, tri = M.import_mesh(M.asset("bimba.obj"))
    sx = np.ascontiguousarray(xyz[tri.reshape(-1).astype(np.int64)])
    st = np.arange(sx.shape[0], dtype=np.uint32).reshape(-1, 3)
    for n in (64, 256):
        fr, _, _ = _frame(xyz, n)
        res = []
        for v, t in ((xyz, tri), (sx, st)):
            dx, dt = engine.mesh_to_device(v, t)
            c = engine.voxelize_conservative(fr, dx, dt)
            f, _ = engine.fill_interior(fr, c)
            engine.sync()
            res.append(engine.words_to_numpy(f).copy())
        assert np.array_equal(res[0], res[1]), n
        assert words_to_bool(res[0], n).sum() > 0


def _refused(code, fn):
    with pytest.raises(capi.VPError) as e:
        fn()
    assert e.value.code == code, (e.value.code, code)


def test_refusals_leave_the_output_untouched(engine):
    n = 64
    fr = _unit_frame(n)
    words = torch.from_numpy(random_grid(n, 0.5, 3).view(np.int32)).to(engine.device)
    sentinel = torch.full((2 * fr.words,), 0x5A5A5A5A, dtype=torch.int32, device=engine.device)
    out = sentinel.clone()
    ctx = engine.ctx
    slab = Frame.make(n, 1.0 / n, np.zeros(3, np.float32), 0, 32)
    _refused(10002, lambda: ctx.fill_interior(slab, words.data_ptr(), out.data_ptr()))
    bad = Frame.make(48, 1.0 / 48, np.zeros(3, np.float32))
    _refused(10002, lambda: ctx.fill_interior(bad, words.data_ptr(), out.data_ptr()))
    _refused(10001, lambda: ctx.fill_interior(fr, 0, out.data_ptr()))
    _refused(10001, lambda: ctx.fill_interior(fr, words.data_ptr(), 0))
    # overlapping in / out: the output starts inside the input and runs past it
    both = sentinel.clone()
    _refused(10001, lambda: ctx.fill_interior(fr, both.data_ptr(), both.data_ptr() + 4 * (fr.words // 2)))
    _refused(10001, lambda: ctx.fill_interior(fr, both.data_ptr(), both.data_ptr()))
    engine.sync()
    assert torch.equal(out, sentinel)
    assert torch.equal(both, sentinel)
    h = np.zeros(fr.words, np.uint32)
    _refused(10002, lambda: ctx.fill_interior_host(slab, h, h))


def test_host_form_in_place(engine):
    n = 96
    vox, exp = hand_cases(n)[2][1:]                         # the hollow shell
    h = bool_to_words(vox)
    engine.ctx.fill_interior_host(_unit_frame(n), h, h)
    assert np.array_equal(h, bool_to_words(exp))


def test_jfa_start_is_dropped_by_a_fill(engine):
    xyz, tri = M.import_mesh(M.asset("bunny.obj"))
    fr, _, _ = _frame(xyz, 128)
    dx, dt = engine.mesh_to_device(xyz, tri)
    src = engine.voxelize_conservative(fr, dx, dt)
    g = engine.voxelize(fr, dx, dt)
    out = torch.empty(fr.voxels, dtype=torch.float32, device=engine.device)
    engine.ctx.jfa_start(fr, g.data_ptr(), None, 0, ALGO_TILED)
    engine.fill_interior(fr, src, out=g)
    with pytest.raises(capi.VPError) as e:
        engine.ctx.jfa_run(fr, g.data_ptr(), -math.inf, out.data_ptr(), None, 0, ALGO_TILED)
    assert e.value.code == 10001
    engine.ctx.jfa_start(fr, g.data_ptr(), None, 0, ALGO_TILED)      # a fresh start serves the run
    engine.ctx.jfa_run(fr, g.data_ptr(), -math.inf, out.data_ptr(), None, 0, ALGO_TILED)
    engine.sync()


def test_cli_composition(cli, tmp_path):
    n = 64
    meshes = [M.asset("bimba.obj"), M.asset("bunny.obj")]
    dumps = {}
    for t in (2, 0):
        d = tmp_path / ("t%d" % t)
        d.mkdir()
        p = subprocess.run([cli] + meshes + ["-n", str(n), "-t", str(t), "--conservative", "--fill", "-p", "1", "-s", "-e", "-d",
                                              str(d / "x")], capture_output=True, text=True, cwd=str(d), timeout=900)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert re.search(r"Fill\]?: [0-9.]+ ms", p.stdout), p.stdout[-2000:]
        dumps[t] = (np.fromfile(str(d / "x.grid.u32"), np.uint32), np.fromfile(str(d / "x.sdf.f32"), np.float32))
    (gw, gs), (hw, hs) = dumps[2], dumps[0]
    assert np.array_equal(gw, hw) and np.array_equal(gs.view(np.uint32), hs.view(np.uint32))
    xyz = [M.import_mesh(m)[0] for m in meshes]
    origin, vs = O.frame(xyz, n)
    exp_w = np.zeros_like(gw)
    for m in meshes:
        exp_w |= fill_numpy(cvox_numpy(*M.import_mesh(m), n, vs, origin), n)
    assert np.array_equal(gw, exp_w)
    sdf = O.jfa(gw, n, vs, origin)
    assert np.array_equal(gs.view(np.uint32), sdf.view(np.uint32))
    out = tmp_path / "t2" / "out"
    _check_file(str(out / "csg_vox_tiled_out.obj"), *O.grid_to_mesh_compressed(gw, n, vs, origin))
    _check_sdf_files(out, "tiled", O.grid_to_mesh_cubes(gw, sdf, n, vs, origin), O.grid_to_point_cloud(gw, sdf, n, vs, origin))
