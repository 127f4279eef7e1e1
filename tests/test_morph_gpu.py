"""Ball morphology on the GPU (vp_morph): hand cases and random grids against the numpy restatements of tests/morph_ref.py, both
algorithms; NAIVE == TILED on conservative mesh grids and against the host restatement of `vpcli --morph`; the algebra on grids up to
n = 2048, checked on the device; the repair the feature is for (an open sphere: dilate -> fill -> erode) through the engine and the CLI;
refusals and the state the call shares with the rest of the context."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cuda_mesh_voxelization_amd import build, capi, mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame
from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fill_ref import fill_numpy  # noqa: E402
from morph_ref import (CLOSE, DILATE, ERODE, OPEN, ball, bool_to_words, hand_cases, morph_numpy, morph_numpy_sep, random_grid,  # noqa: E402
                       words_to_bool)
from test_conservative_cpu import cvox_numpy  # noqa: E402
from test_export import _check_file, _check_sdf_files  # noqa: E402

pytestmark = pytest.mark.gpu

ALGOS = (ALGO_NAIVE, ALGO_TILED)
OPS = (DILATE, ERODE, OPEN, CLOSE)
NAMES = {DILATE: "dilate", ERODE: "erode", OPEN: "open", CLOSE: "close"}


@pytest.fixture(scope="module")
def cli():
    return build.build_cli()


def _unit_frame(n):
    return Frame.make(n, 1.0 / n, np.zeros(3, np.float32))


def _dev(engine, words):
    return torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32)).to(engine.device)


def _morph(engine, n, words, op, r, algo):
    out = engine.morph(_unit_frame(n), _dev(engine, words), op, r, algo=algo)
    engine.sync()
    return engine.words_to_numpy(out).copy()


def _frame(xyz, n):
    origin, vs = M.frame([xyz], n)
    return Frame.make(n, vs, origin), origin, vs


@pytest.mark.parametrize("n", [32, 64, 96, 160])
def test_hand_cases(engine, n):
    for r in (1, 2, 5, 9):
        for name, op, vox, exp in hand_cases(n, r):
            words = bool_to_words(vox)
            for algo in ALGOS:
                got = _morph(engine, n, words, op, r, algo)
                assert np.array_equal(got, bool_to_words(exp)), (n, r, name, algo, np.argwhere(words_to_bool(got, n) != exp)[:8].tolist())
    # all four ops with both algos on the single voxel in the middle and its complement, and r = 0
    v = np.zeros((n, n, n), bool)
    v[n // 2, n // 2 + 1, n // 2 - 1] = True
    for words in (bool_to_words(v), bool_to_words(~v)):
        for op in OPS:
            for r in (0, 3):
                exp = morph_numpy_sep(words, n, op, r)
                for algo in ALGOS:
                    assert np.array_equal(_morph(engine, n, words, op, r, algo), exp), (n, op, r, algo)


@pytest.mark.parametrize("n", [32, 64, 128])
@pytest.mark.parametrize("r", [1, 2, 3, 5, 8, 16, 32])
def test_random_grids(engine, n, r):
    for density in (0.001, 0.02, 0.5):
        words = random_grid(n, density, 7000 * n + 10 * r + int(1000 * density))
        for op, w in ((DILATE, words), (ERODE, ~words)):
            exp = morph_numpy_sep(w, n, op, r)
            if r <= 3:
                assert np.array_equal(morph_numpy(w, n, op, r), exp)
            for algo in ALGOS:
                got = _morph(engine, n, w, op, r, algo)
                assert np.array_equal(got, exp), (n, r, density, NAMES[op], algo, int(np.count_nonzero(got != exp)))
    words = random_grid(n, 0.3, n + r)
    for op in (OPEN, CLOSE):
        exp = morph_numpy_sep(words, n, op, min(r, 5))
        for algo in ALGOS:
            assert np.array_equal(_morph(engine, n, words, op, min(r, 5), algo), exp), (n, r, NAMES[op], algo)


@pytest.mark.parametrize("n", [288, 384])
def test_rows_that_are_not_a_power_of_two_wide(engine, n):
    """n / 32 = 9 (one word per lane) and 12 (four words per lane, the last tile in x partial), LDS tiles (r = 2, 9) and rows from global
    memory (r = 13)"""
    words = random_grid(n, 0.002, n)
    for r in (2, 9, 13):
        for op, w in ((DILATE, words), (ERODE, ~words)):
            a = _morph(engine, n, w, op, r, ALGO_NAIVE)
            b = _morph(engine, n, w, op, r, ALGO_TILED)
            assert np.array_equal(a, b), (n, r, NAMES[op], int(np.count_nonzero(a != b)))
            if r == 2:
                assert np.array_equal(a, morph_numpy_sep(w, n, op, r)), (n, r, NAMES[op])


def _vpcli(cli, tmp_path, args, tag, timeout=3000):
    prefix = str(tmp_path / tag)
    p = subprocess.run([cli] + args + ["-d", prefix], capture_output=True, text=True, timeout=timeout, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return prefix, p.stdout


# the steps the host restatement (vpcli -t 3) replays at n = 512, per mesh
HOST_STEPS = {"bunny.obj": ((DILATE, 3), (ERODE, 7)), "bimba.obj": ((CLOSE, 3), (OPEN, 1)), "d20.obj": ((OPEN, 7), (CLOSE, 16))}


@pytest.mark.parametrize("name", ["bunny.obj", "bimba.obj", "d20.obj"])
def test_naive_equals_tiled_on_mesh_grids(engine, cli, tmp_path, name):
    xyz, tri = M.import_mesh(M.asset(name))
    dx, dt = engine.mesh_to_device(xyz, tri)
    for n in (256, 512):
        fr, _, _ = _frame(xyz, n)
        c = engine.voxelize_conservative(fr, dx, dt)
        a, b = engine.new_grid(fr), engine.new_grid(fr)
        for r in (1, 3, 7, 16):
            for op in OPS:
                engine.morph(fr, c, op, r, out=a, algo=ALGO_NAIVE)
                engine.morph(fr, c, op, r, out=b, algo=ALGO_TILED)
                engine.sync()
                assert torch.equal(a, b), (name, n, r, NAMES[op], int((a != b).sum()))
                if op in (DILATE, ERODE):
                    assert not torch.equal(a, c), (name, n, r, NAMES[op])
        if n == 512:
            steps = HOST_STEPS[name]
            g = c
            for op, r in steps:
                g = engine.morph(fr, g, op, r)
            engine.sync()
            arg = ",".join("%s:%d" % (NAMES[op], r) for op, r in steps)
            prefix, out = _vpcli(cli, tmp_path, [M.asset(name), "-n", str(n), "-t", "3", "--conservative", "--morph", arg], "host")
            host = np.fromfile(prefix + ".grid.u32", np.uint32)
            got = engine.words_to_numpy(g)
            assert np.array_equal(got, host), (name, arg, int(np.count_nonzero(got != host)))
            assert out.count("Morph]: ") == len(steps)


def _subset(a, b):
    return bool(((a & ~b) == 0).all())


def _large_grid(engine, kind, n):
    xyz, tri = M.import_mesh(M.asset("d20.obj")) if kind == "d20" else M.bunny(24)
    fr, _, _ = _frame(xyz, n)
    dx, dt = engine.mesh_to_device(xyz, tri)
    return fr, engine.voxelize_conservative(fr, dx, dt)


@pytest.mark.parametrize("kind", ["d20", "bunny24"])
@pytest.mark.parametrize("n", [1024, 2048])
def test_large_grids_algebra_on_the_device(engine, kind, n):
    fr, w = _large_grid(engine, kind, n)
    nw = ~w
    a, b, t = engine.new_grid(fr), engine.new_grid(fr), engine.new_grid(fr)
    for r in (1, 4, 16):
        engine.morph(fr, w, ERODE, r, out=a)
        engine.morph(fr, nw, DILATE, r, out=b)
        engine.sync()
        assert torch.equal(a, ~b), (kind, n, r)                           # erode(W) == ~dilate(~W)
        engine.morph(fr, w, DILATE, r, out=a)
        engine.sync()
        assert _subset(w, a) and not torch.equal(a, w), (kind, n, r)       # dilate contains W
        engine.morph(fr, a, ERODE, r, out=b)                               # close by hand == close
        engine.morph(fr, w, CLOSE, r, out=t)
        engine.sync()
        assert torch.equal(b, t) and _subset(w, t), (kind, n, r)
        engine.morph(fr, t, CLOSE, r, out=a)
        engine.sync()
        assert torch.equal(a, t), (kind, n, r)                             # close is idempotent
        # open on the dilated shell (the open of a thin shell is empty): a subset of its input, idempotent
        engine.morph(fr, w, DILATE, 2, out=a)
        engine.morph(fr, a, OPEN, r, out=t)
        engine.sync()
        assert _subset(t, a), (kind, n, r)
        engine.morph(fr, t, OPEN, r, out=b)
        engine.sync()
        assert torch.equal(b, t), (kind, n, r)
        engine.morph(fr, w, OPEN, r, out=t)
        engine.sync()
        assert _subset(t, w), (kind, n, r)
    if n == 1024:                                                          # the two algorithms agree here as well
        engine.morph(fr, w, CLOSE, 4, out=a, algo=ALGO_NAIVE)
        engine.morph(fr, w, CLOSE, 4, out=b, algo=ALGO_TILED)
        engine.sync()
        assert torch.equal(a, b), (kind, n)
    del w, nw, a, b, t
    torch.cuda.empty_cache()


def test_single_voxel_at_2048_has_the_ball_popcount(engine):
    n = 2048
    fr = _unit_frame(n)
    w = engine.new_grid(fr)
    w.zero_()
    x, y, z = 1055, 1000, 700                                             # x = 32 * 32 + 31: bit 31 of its word, the ball crosses the word edge
    w[(z * n + y) * (n // 32) + x // 32] = -(1 << 31)
    out = engine.new_grid(fr)
    for r in (1, 4, 16, 32):
        for algo in ALGOS:
            engine.morph(fr, w, DILATE, r, out=out, algo=algo)
            engine.sync()
            nz = out[torch.nonzero(out).reshape(-1)].cpu().numpy().view(np.uint32)
            assert O.popcount(nz) == int(ball(r).sum()), (r, algo)
    del w, out
    torch.cuda.empty_cache()


# ---- the repair the feature is for -------------------------------------------------------------------------------------------------

def _subdivide(xyz, tri):
    """every triangle into four, the new vertices pushed out to the sphere of the mesh"""
    c = 0.5 * (xyz.min(0) + xyz.max(0)).astype(np.float64)
    rad = np.linalg.norm(xyz - c, axis=1).mean()
    t = tri.astype(np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    ue, inv = np.unique(e, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    mid = 0.5 * (xyz[ue[:, 0]].astype(np.float64) + xyz[ue[:, 1]])
    mid = c + (mid - c) * (rad / np.linalg.norm(mid - c, axis=1))[:, None]
    nv, f = xyz.shape[0], t.shape[0]
    m01, m12, m20 = nv + inv[:f], nv + inv[f:2 * f], nv + inv[2 * f:]
    nt = np.concatenate([np.stack([t[:, 0], m01, m20], 1), np.stack([t[:, 1], m12, m01], 1), np.stack([t[:, 2], m20, m12], 1),
                         np.stack([m01, m12, m20], 1)])
    return np.concatenate([xyz, mid.astype(np.float32)]), nt.astype(np.uint32)


def _open_sphere(tmp_path):
    """assets/sphere.obj has edges of about 9 voxels at n = 128, so the faces around one of its vertices leave a hole 17 voxels wide.  Two
    midpoint subdivisions quarter that: the five faces around vertex 22 then leave a hole 4.2 voxels wide.  Returns the paths and arrays of
    the intact and the open mesh (as the importer reads them back) and the removed faces."""
    xyz, tri = M.import_mesh(M.asset("sphere.obj"))
    for _ in range(2):
        xyz, tri = _subdivide(xyz, tri)
    gone = np.any(tri.astype(np.int64) == 22, axis=1)
    assert gone.sum() == 5
    paths = {}
    for tag, t in (("intact", tri), ("open", tri[~gone]), ("patch", tri[gone])):
        paths[tag] = str(tmp_path / (tag + ".obj"))
        M.export_obj(paths[tag], xyz, t)
    return paths, xyz, tri, gone


def test_open_sphere_is_repaired_by_dilate_fill_erode(engine, cli, tmp_path):
    n, R = 128, 3
    paths, xyz, tri, gone = _open_sphere(tmp_path)
    fr, origin, vs = _frame(xyz, n)
    ring = np.unique(tri[gone].astype(np.int64))
    ring = xyz[ring[ring != 22]].astype(np.float64)
    width = np.sqrt(((ring[:, None] - ring[None]) ** 2).sum(-1)).max() / float(vs)
    assert 1.0 < width <= 2 * R - 1, width                               # wider than a voxel, at most 2 R - 1 voxels
    # the references first, on the CPU
    c_open = cvox_numpy(xyz, tri[~gone], n, vs, origin)
    c_full = cvox_numpy(xyz, tri, n, vs, origin)
    assert np.array_equal(fill_numpy(c_open, n), c_open)                  # the fill alone leaks: the hole is a real hole

    def pipe_numpy(c):
        return morph_numpy_sep(fill_numpy(morph_numpy_sep(c, n, DILATE, R), n), n, ERODE, R)
    exp_open, exp_full = pipe_numpy(c_open), pipe_numpy(c_full)

    def pipe_gpu(t, algo):
        dx, dt = engine.mesh_to_device(xyz, np.ascontiguousarray(t))
        c = engine.voxelize_conservative(fr, dx, dt)
        f0, _ = engine.fill_interior(fr, c)
        d = engine.morph(fr, c, DILATE, R, algo=algo)
        f, _ = engine.fill_interior(fr, d)
        e = engine.morph(fr, f, ERODE, R, algo=algo)
        engine.sync()
        return engine.words_to_numpy(c).copy(), engine.words_to_numpy(f0).copy(), engine.words_to_numpy(e).copy()

    for algo in ALGOS:
        c, f0, got = pipe_gpu(tri[~gone], algo)
        assert np.array_equal(c, c_open) and np.array_equal(f0, c)        # the GPU fill alone returns the conservative grid
        assert np.array_equal(got, exp_open), (algo, int(np.count_nonzero(got != exp_open)))
        vox = words_to_bool(got, n)
        assert vox[n // 2, n // 2, n // 2]                                # the centre of the sphere is inside
        _, _, full = pipe_gpu(tri, algo)
        assert np.array_equal(full, exp_full)
        # differs from the intact sphere's result only within 2 R voxels (Chebyshev) of the removed faces' voxels
        patch = words_to_bool(cvox_numpy(xyz, tri[gone], n, vs, origin), n)
        zz, yy, xx = np.nonzero(patch)
        for q in zip(*np.nonzero(vox != words_to_bool(full, n))):
            assert np.min(np.maximum(np.maximum(np.abs(zz - q[0]), np.abs(yy - q[1])), np.abs(xx - q[2]))) <= 2 * R, q

    # the same input through the CLI: -t 2 equals -t 0 in grid and sdf bits, and the exporter files are right
    dumps = {}
    for t in (2, 0):
        d = tmp_path / ("t%d" % t)
        d.mkdir()
        # only the device run exports (-e): at n = 128 the cube file of the solid is about 1 GB, and the host run is compared in bits alone
        p = subprocess.run([cli, paths["open"], "-n", str(n), "-t", str(t), "--conservative", "--morph", "dilate:3,fill,erode:3", "-s"]
                           + (["-e"] if t == 2 else []) + ["-d", str(d / "x")], capture_output=True, text=True, cwd=str(d), timeout=1800)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert p.stdout.count("Morph]: ") == 2 and "Fill]: " in p.stdout, p.stdout[-2000:]
        dumps[t] = (np.fromfile(str(d / "x.grid.u32"), np.uint32), np.fromfile(str(d / "x.sdf.f32"), np.float32))
    (gw, gs), (hw, hs) = dumps[2], dumps[0]
    assert np.array_equal(gw, hw) and np.array_equal(gs.view(np.uint32), hs.view(np.uint32))
    rxyz, rtri = M.import_mesh(paths["open"])                             # the frame the CLI computed: from the vertices the file lists
    o2, vs2 = O.frame([rxyz], n)
    exp_cli = morph_numpy_sep(fill_numpy(morph_numpy_sep(cvox_numpy(rxyz, rtri, n, vs2, o2), n, DILATE, R), n), n, ERODE, R)
    assert np.array_equal(gw, exp_cli)
    sdf = O.jfa(gw, n, vs2, o2)
    assert np.array_equal(gs.view(np.uint32), sdf.view(np.uint32))
    out = tmp_path / "t2" / "out"
    _check_file(str(out / "tiled_open.obj"), *O.grid_to_mesh_compressed(gw, n, vs2, o2))
    _check_sdf_files(out, "tiled", O.grid_to_mesh_cubes(gw, sdf, n, vs2, o2), O.grid_to_point_cloud(gw, sdf, n, vs2, o2))


# ---- refusals and shared state -----------------------------------------------------------------------------------------------------

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
    wp, op_ = words.data_ptr(), out.data_ptr()
    slab = Frame.make(n, 1.0 / n, np.zeros(3, np.float32), 0, 32)
    _refused(10002, lambda: ctx.morph(slab, wp, op_, DILATE, 1))
    bad = Frame.make(48, 1.0 / 48, np.zeros(3, np.float32))
    _refused(10002, lambda: ctx.morph(bad, wp, op_, DILATE, 1))
    for algo in ALGOS:
        _refused(10002, lambda: ctx.morph(fr, wp, op_, DILATE, 33, algo))
        _refused(10001, lambda: ctx.morph(fr, wp, op_, 4, 1, algo))
        _refused(10001, lambda: ctx.morph(fr, wp, op_, -1, 1, algo))
    _refused(10001, lambda: ctx.morph(fr, wp, op_, DILATE, 1, 0))
    _refused(10001, lambda: ctx.morph(fr, wp, op_, DILATE, 1, 3))
    _refused(10001, lambda: ctx.morph(fr, 0, op_, DILATE, 1))
    _refused(10001, lambda: ctx.morph(fr, wp, 0, DILATE, 1))
    _refused(10001, lambda: ctx.morph(fr, wp, op_ + 4, DILATE, 1))        # not 16-byte aligned
    both = sentinel.clone()
    _refused(10001, lambda: ctx.morph(fr, both.data_ptr(), both.data_ptr() + 4 * (fr.words // 2), DILATE, 1))
    _refused(10001, lambda: ctx.morph(fr, both.data_ptr(), both.data_ptr(), CLOSE, 0))
    engine.sync()
    assert torch.equal(out, sentinel)
    assert torch.equal(both, sentinel)
    h = np.zeros(fr.words, np.uint32)
    _refused(10002, lambda: ctx.morph_host(slab, h, h, DILATE, 1))
    _refused(10002, lambda: ctx.morph_host(fr, h, h, DILATE, 33))
    _refused(10001, lambda: ctx.morph_host(fr, h, h, 7, 1))


def test_host_form_in_place(engine):
    n = 96
    for op in OPS:
        for algo in ALGOS:
            h = random_grid(n, 0.02 if op in (DILATE, CLOSE) else 0.9, 11 + op)
            exp = morph_numpy_sep(h, n, op, 4)
            engine.ctx.morph_host(_unit_frame(n), h, h, op, 4, algo)
            assert np.array_equal(h, exp), (op, algo)


def test_jfa_start_is_dropped_by_a_morph(engine):
    xyz, tri = M.import_mesh(M.asset("bunny.obj"))
    fr, _, _ = _frame(xyz, 128)
    dx, dt = engine.mesh_to_device(xyz, tri)
    src = engine.voxelize_conservative(fr, dx, dt)
    g = engine.voxelize(fr, dx, dt)
    out = torch.empty(fr.voxels, dtype=torch.float32, device=engine.device)
    engine.ctx.jfa_start(fr, g.data_ptr(), None, 0, ALGO_TILED)
    engine.morph(fr, src, DILATE, 2, out=g)
    with pytest.raises(capi.VPError) as e:
        engine.ctx.jfa_run(fr, g.data_ptr(), -math.inf, out.data_ptr(), None, 0, ALGO_TILED)
    assert e.value.code == 10001
    engine.ctx.jfa_start(fr, g.data_ptr(), None, 0, ALGO_TILED)      # a fresh start serves the run
    engine.ctx.jfa_run(fr, g.data_ptr(), -math.inf, out.data_ptr(), None, 0, ALGO_TILED)
    engine.sync()


def test_a_morph_between_two_fills_leaves_the_fill_alone(engine):
    xyz, tri = M.import_mesh(M.asset("bimba.obj"))
    fr, _, _ = _frame(xyz, 256)
    dx, dt = engine.mesh_to_device(xyz, tri)
    c = engine.voxelize_conservative(fr, dx, dt)
    f1, _ = engine.fill_interior(fr, c)
    m = engine.morph(fr, c, CLOSE, 5)                                 # grows and writes the context's intermediate grid
    f2, _ = engine.fill_interior(fr, c)
    m2 = engine.morph(fr, c, CLOSE, 5)
    engine.sync()
    assert torch.equal(f1, f2) and torch.equal(m, m2)
    assert not torch.equal(f1, c)


def test_open_and_close_book_two_launches(engine):
    n = 128
    fr = _unit_frame(n)
    w = _dev(engine, random_grid(n, 0.3, 5))
    ctx = engine.ctx
    for algo, key in ((ALGO_TILED, "morph"), (ALGO_NAIVE, "morph_naive")):
        for op, launches in ((DILATE, 1), (ERODE, 1), (OPEN, 2), (CLOSE, 2)):
            ctx.prof_reset()
            ctx.prof_enable(True)
            engine.morph(fr, w, op, 3, algo=algo)
            ctx.prof_enable(False)
            p = ctx.prof()
            assert p[key]["launches"] == launches, (algo, op, p)
            assert p[key]["ms"] > 0.0
            other = "morph_naive" if key == "morph" else "morph"
            assert other not in p or p[other]["launches"] == 0
