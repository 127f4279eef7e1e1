"""The generalized winding number on the GPU (vp_winding*, csrc/winding.hip) against the numpy restatement of tests/winding_ref.py, bit for
bit: NAIVE and TILED, the field and the inside grid, on the hand cases and the small meshes at n = 32 with beta 0, 1 and 2 and the levels
0.5 and 1.5, on d20 and torus at n = 64 and 96 (the uneven pyramid) with the same betas and levels, on a mesh scaled out of the frame (clamped leaves) and on one far from
the origin; bunny at n = 96 and 128 against the host form; the hand-over of the inside grid to vp_mesh_distance; the result pointers before
a build and after a release; refusals that leave the previous result alone; two grid sides in one context; the counts and the start that
stood on an inside grid whose buffers a larger build frees.
The brute force (beta = 0) of the torus at n = 64 and 96 is compared with the host form, like bunny: its numpy restatement takes tens of
seconds there.  The empty mesh also goes through vp_winding_host."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from cuda_mesh_voxelization_amd import capi, mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshdist_ref as MD  # noqa: E402
import winding_ref as R  # noqa: E402
from test_winding_cpu import check_exe, hand_meshes, open_sphere, run_check, unit_frame  # noqa: E402,F401  (check_exe: the fixture that builds tests/cpp/winding_check.cpp)

pytestmark = pytest.mark.gpu

ALGOS = (ALGO_NAIVE, ALGO_TILED)
F = np.float32


@functools.lru_cache(maxsize=None)
def _case(name, n):
    if name == "open":
        xyz, tri, origin, vs = open_sphere()
    else:
        xyz, tri = M.import_mesh(M.asset(name))
        origin, vs = M.frame([xyz], n)
    return xyz, tri, origin, vs


def _run(engine, fr, dx, dt, beta, level, algo):
    """(w as uint32, inside words, inside count) of one call, numpy"""
    count = engine.ctx.winding(fr, dx.data_ptr(), dx.shape[0], dt.data_ptr(), dt.shape[0], beta, level, algo, count=True)
    dw, dg, n = engine.ctx.winding_result()
    assert dw and dg and n == fr.n
    w, g = np.empty(fr.voxels, np.uint32), np.empty(fr.voxels // 32, np.uint32)
    engine.ctx.download(w, dw)
    engine.ctx.download(g, dg)
    return w, g, count


def _check(engine, xyz, tri, n, vs, origin, betas, levels, tag):
    xyz, tri = np.ascontiguousarray(xyz, F).reshape(-1, 3), np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    for beta in betas:
        S = R.winding_sums(xyz, tri, n, vs, origin, beta)
        for level in levels:
            exp_w, exp_g = R.finish(S, level)
            exp_w = exp_w.view(np.uint32)
            for algo in ALGOS:
                w, g, count = _run(engine, fr, dx, dt, beta, level, algo)
                assert np.array_equal(w, exp_w), (tag, beta, algo, int((w != exp_w).sum()), np.argwhere(w != exp_w)[:4].tolist())
                assert np.array_equal(g, exp_g), (tag, beta, level, algo, int((g != exp_g).sum()))
                assert count == int(np.unpackbits(exp_g.view(np.uint8)).sum()), (tag, beta, level, algo)


def test_hand_cases(engine):
    for label, (xyz, tri) in hand_meshes().items():
        _check(engine, xyz, tri, 32, *unit_frame(), (0.0, 1.0, 2.0), (0.5, 1.5), label)
    bad_xyz = np.array([[4.2, 5.1, 6.3], [25.7, 8.4, 7.9], [12.3, 27.6, 9.2], [np.nan, 1, 1], [np.inf, 2, 2]], F)
    bad = np.array([[0, 1, 9], [0, 3, 2], [4, 1, 2], [0, 0, 1], [0, 1, 2]], np.uint32)       # index, NaN, inf, repeated vertex; one valid
    _check(engine, bad_xyz, bad, 32, *unit_frame(), (0.0, 2.0), (0.5,), "invalid triangles mixed in")
    _check(engine, bad_xyz, bad[:4], 32, *unit_frame(), (0.0, 2.0), (0.5, 0.0), "nothing contributes")
    _check(engine, np.zeros((0, 3), F), np.zeros((0, 3), np.uint32), 32, *unit_frame(), (0.0, 2.0), (0.5, 0.0), "no triangles")


@pytest.mark.parametrize("name", ["d20.obj", "torus.obj", "sphere.obj", "open"])
def test_meshes_at_32_against_the_numpy_restatement(engine, name):
    xyz, tri, origin, vs = _case(name, 32)
    _check(engine, xyz, tri, 32, vs, origin, (0.0, 1.0, 2.0), (0.5, 1.5), name)


@pytest.mark.parametrize("name,n,betas", [("d20.obj", 64, (0.0, 1.0, 2.0)), ("d20.obj", 96, (0.0, 1.0, 2.0)), ("torus.obj", 64, (1.0, 2.0)),
                                          ("torus.obj", 96, (1.0, 2.0))])
def test_meshes_at_64_and_96_the_uneven_pyramid(engine, name, n, betas):
    xyz, tri, origin, vs = _case(name, n)
    _check(engine, xyz, tri, n, vs, origin, betas, (0.5, 1.5), (name, n))


@pytest.mark.parametrize("n", [64, 96])
def test_torus_brute_force_at_64_and_96_against_the_host_form(engine, check_exe, n, tmp_path):
    """beta = 0 of the torus above n = 32 takes numpy tens of seconds; the reference here is the host form run over bricks in parallel, which
    the CPU suite pins to the numpy restatement (and to its sequential run) bit for bit.  The grids of both levels follow from its field."""
    xyz, tri, origin, vs = _case("torus.obj", n)
    host_w, host_g = run_check(check_exe, M.asset("torus.obj"), n, 0.0, 0.5, "o", str(tmp_path / "torus"))["omp"]
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    for level in (0.5, 1.5):
        exp_g = np.packbits((host_w.view(F) >= F(level)).reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1)
        if level == 0.5:
            assert np.array_equal(exp_g, host_g) and exp_g.any()
        for algo in ALGOS:
            w, g, count = _run(engine, fr, dx, dt, 0.0, level, algo)
            assert np.array_equal(w, host_w), (n, algo, int((w != host_w).sum()))
            assert np.array_equal(g, exp_g), (n, level, algo)
            assert count == int(np.unpackbits(exp_g.view(np.uint8)).sum())


def test_empty_mesh_through_the_host_entry_point(engine, check_exe, tmp_path):
    """vp_winding_host with no triangles (an OBJ of vertices only: null triangle array) through both device algos"""
    obj = str(tmp_path / "empty.obj")
    with open(obj, "w") as f:
        f.write("v 0 0 0\nv 1 0 0\nv 0 1 0\n")
    for level, word in ((0.5, 0), (0.0, 0xFFFFFFFF)):
        got = run_check(check_exe, obj, 32, 2.0, level, "snt", str(tmp_path / "empty"), unit_frame())
        for tag in ("seq", "naive", "tiled"):
            assert not got[tag][0].any() and (got[tag][1] == word).all(), (tag, level)
    w, g, count = engine.ctx.winding_host(Frame.make(32, *unit_frame()), np.zeros((0, 3), F), np.zeros((0, 3), np.uint32), 2.0, 0.0)
    assert not w.any() and (g == 0xFFFFFFFF).all() and count == 32 ** 3


def test_mesh_scaled_out_of_the_frame_clamps_its_leaves(engine):
    xyz, tri, origin, vs = _case("d20.obj", 32)
    mid = ((xyz.max(0) + xyz.min(0)) * F(0.5)).astype(F)
    big = ((xyz - mid) * F(3.0) + mid).astype(F)
    _check(engine, big, tri, 32, vs, origin, (0.0, 1.0, 2.0), (0.5,), "d20 x 3")


def test_mesh_far_from_the_origin(engine):
    xyz, tri, _, _ = _case("d20.obj", 32)
    moved = (xyz + np.array([81100.3, -40990.7, 6500.1], F)).astype(F)
    origin, vs = M.frame([moved], 32)
    _check(engine, moved, tri, 32, vs, origin, (0.0, 2.0), (0.5,), "d20 translated")


@pytest.mark.parametrize("n", [96, 128])
def test_bunny_tiled_equals_naive_equals_the_host_form(engine, check_exe, n, tmp_path):
    """numpy is too slow here.  The host form runs its bricks in parallel (VOX::ComputeWinding<OPENMP>): the same function as SEQUENTIAL,
    which the CPU suite pins to the restatement, and which takes minutes on this mesh."""
    xyz, tri, origin, vs = _case("bunny.obj", n)
    host_w, host_g = run_check(check_exe, M.asset("bunny.obj"), n, 2.0, 0.5, "o", str(tmp_path / "bunny"))["omp"]
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    for algo in ALGOS:
        w, g, count = _run(engine, fr, dx, dt, 2.0, 0.5, algo)
        assert np.array_equal(w, host_w), (n, algo, int((w != host_w).sum()))
        assert np.array_equal(g, host_g), (n, algo)
        assert 0 < count < n ** 3 and count == int(np.unpackbits(host_g.view(np.uint8)).sum())


def test_the_inside_grid_signs_the_mesh_distance(engine):
    n, band = 32, 3
    xyz, tri, origin, vs = _case("sphere.obj", n)
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    w, inside = engine.winding(fr, dx, dt, beta=2.0, level=0.5)
    dist = engine.mesh_distance(fr, dx, dt, band, sign_words=inside)
    engine.sync()
    exp_w, exp_g = R.winding_f32(xyz, tri, n, vs, origin, 2.0, 0.5)
    assert np.array_equal(w.cpu().numpy().view(np.uint32), exp_w.view(np.uint32))
    assert np.array_equal(inside.cpu().numpy().view(np.uint32), exp_g)
    exp_d, _ = MD.mesh_distance_f32(xyz, tri, n, vs, origin, band, exp_g)
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), exp_d.view(np.uint32))
    # the views are the context's buffers: the next build overwrites them in place
    assert w.data_ptr() == engine.ctx.winding_result()[0] and inside.data_ptr() == engine.ctx.winding_result()[1]


def test_result_is_null_before_a_build_and_after_a_release():
    ctx = capi.Context(0)
    try:
        assert ctx.winding_result() == (0, 0, 0)
        xyz, tri, origin, vs = _case("d20.obj", 32)
        fr = Frame.make(32, vs, origin)
        dx, dt = ctx.malloc(xyz.nbytes), ctx.malloc(tri.nbytes)
        ctx.upload(dx, xyz)
        ctx.upload(dt, tri)
        ctx.winding(fr, dx, len(xyz), dt, len(tri), 2.0, 0.5, ALGO_TILED)
        dw, dg, n = ctx.winding_result()
        assert dw and dg and n == 32
        ctx.release()
        assert ctx.winding_result() == (0, 0, 0)
        ctx.free(dx)
        ctx.free(dt)
    finally:
        ctx.close()


def test_refusals_leave_the_previous_result_as_it_was(engine):
    n = 32
    xyz, tri, origin, vs = _case("d20.obj", n)
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    before = _run(engine, fr, dx, dt, 2.0, 0.5, ALGO_TILED)
    ptrs = engine.ctx.winding_result()
    slab = Frame.make(64, vs, origin, 0, 32)
    big = Frame.make(2048, vs, origin)
    args = (dx.data_ptr(), dx.shape[0], dt.data_ptr(), dt.shape[0])
    for frame, beta, level, algo, code in ((slab, 2.0, 0.5, ALGO_TILED, 10002), (big, 2.0, 0.5, ALGO_TILED, 10002),
                                           (fr, 0.5, 0.5, ALGO_TILED, 10001), (fr, 65.0, 0.5, ALGO_TILED, 10001), (fr, -1.0, 0.5, ALGO_TILED, 10001),
                                           (fr, float("nan"), 0.5, ALGO_TILED, 10001), (fr, float("inf"), 0.5, ALGO_NAIVE, 10001),
                                           (fr, 2.0, float("nan"), ALGO_TILED, 10001), (fr, 2.0, float("inf"), ALGO_NAIVE, 10001),
                                           (fr, 2.0, 0.5, 7, 10001)):
        with pytest.raises(capi.VPError) as e:
            engine.ctx.winding(frame, *args, beta, level, algo)
        assert e.value.code == code, (beta, level, algo, e.value.code)
        assert engine.ctx.winding_result() == ptrs
    with pytest.raises(capi.VPError):
        engine.ctx.winding(fr, 0, 0, 0, 5, 2.0, 0.5, ALGO_TILED)                  # triangles without arrays
    dw, dg, _ = engine.ctx.winding_result()
    w, g = np.empty(fr.voxels, np.uint32), np.empty(fr.voxels // 32, np.uint32)
    engine.ctx.download(w, dw)
    engine.ctx.download(g, dg)
    assert np.array_equal(w, before[0]) and np.array_equal(g, before[1])


def test_two_sides_in_one_context_equal_a_fresh_context():
    xyz, tri, _, _ = _case("torus.obj", 32)
    got = {}
    for sides in ((64, 32), (32,)):
        ctx = capi.Context(0)
        try:
            dx, dt = ctx.malloc(xyz.nbytes), ctx.malloc(tri.nbytes)
            ctx.upload(dx, xyz)
            ctx.upload(dt, tri)
            for n in sides:
                origin, vs = M.frame([xyz], n)
                fr = Frame.make(n, vs, origin)
                for algo in ALGOS:
                    ctx.winding(fr, dx, len(xyz), dt, len(tri), 2.0, 0.5, algo)
                    dw, dg, side = ctx.winding_result()
                    assert side == n
                    w, g = np.empty(fr.voxels, np.uint32), np.empty(fr.voxels // 32, np.uint32)
                    ctx.download(w, dw)
                    ctx.download(g, dg)
                    got[(sides, n, algo)] = (w, g)
            ctx.free(dx)
            ctx.free(dt)
        finally:
            ctx.close()
    for algo in ALGOS:
        a, b = got[((64, 32), 32, algo)], got[((32,), 32, algo)]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), algo
    exp_w, exp_g = R.winding_f32(xyz, tri, 32, *M.frame([xyz], 32)[::-1], 2.0, 0.5)
    assert np.array_equal(got[((32,), 32, ALGO_TILED)][0], exp_w.view(np.uint32)) and np.array_equal(got[((32,), 32, ALGO_TILED)][1], exp_g)


def test_pending_records_are_dropped_when_the_result_buffers_grow():
    """The inside grid is a grid like any other: a vp_surfnets_count, a vp_extract_count and a vp_jfa_start may stand on it.  A vp_winding
    at a larger side frees the bytes they stood on (n = 32 -> 64 is the smallest pair of sides at which the 4 n^3 and the n^3 / 8 buffer
    both have to grow: 8 x the bytes against 25 % head-room), so the records go BEFORE the launch: each dependent call is refused and
    writes nothing."""
    ctx = capi.Context(0)
    try:
        xyz, tri, _, _ = _case("d20.obj", 32)
        dx, dt = ctx.malloc(xyz.nbytes), ctx.malloc(tri.nbytes)
        ctx.upload(dx, xyz)
        ctx.upload(dt, tri)
        fr, big = (Frame.make(n, *M.frame([xyz], n)[::-1]) for n in (32, 64))

        def build(frame):
            ctx.winding(frame, dx, len(xyz), dt, len(tri), 2.0, 0.5, ALGO_TILED)
            _, inside, side = ctx.winding_result()
            assert inside and side == frame.n
            return inside

        def pattern(nbytes):
            p = ctx.malloc(nbytes)
            ctx.memset(p, 0xA5, nbytes)
            return p, nbytes

        def untouched(*bufs):
            ctx.sync()
            for p, nbytes in bufs:
                h = np.empty(nbytes, np.uint8)
                ctx.download(h, p)
                assert (h == 0xA5).all()
                ctx.free(p)

        def refused(fn):
            with pytest.raises(capi.VPError) as e:
                fn()
            assert e.value.code == 10001

        inside = build(fr)
        nv, nq = ctx.surfnets_count(fr, inside)
        total = ctx.extract_count(fr, inside, 0)
        assert nv and nq and total
        mine = np.empty(fr.voxels // 32, np.uint32)                  # a copy for the grid of the caller's own below
        ctx.download(mine, inside)
        build(big)                                                   # the buffers grow: the bytes the counts stood on are freed
        cells, pos, quads, records = pattern(nv * 8), pattern(nv * 12), pattern(nq * 16), pattern(total * 8)
        refused(lambda: ctx.surfnets(fr, inside, ALGO_TILED, 0, cells[0], pos[0], quads[0], nv, nq))
        refused(lambda: ctx.extract(fr, inside, 0, 0, records[0], 0, total))
        untouched(cells, pos, quads, records)
        # the start, through a second build: released, the buffers are those of n = 32 again and have to grow again
        ctx.release()
        inside = build(fr)
        ctx.jfa_start(fr, inside, None, 0, ALGO_TILED)
        build(big)
        sdf = pattern(fr.voxels * 4)
        refused(lambda: ctx.jfa_run(fr, inside, -np.inf, sdf[0], None, 0, ALGO_TILED))
        untouched(sdf)
        # a count on a grid of the caller's own stands through a build
        own = ctx.malloc(mine.nbytes)
        ctx.upload(own, mine)
        assert ctx.surfnets_count(fr, own) == (nv, nq)
        build(fr)
        build(big)
        cells, pos, quads = pattern(nv * 8), pattern(nv * 12), pattern(nq * 16)
        ctx.surfnets(fr, own, ALGO_TILED, 0, cells[0], pos[0], quads[0], nv, nq)
        ctx.sync()
        h = np.empty(nq * 16, np.uint8)
        ctx.download(h, quads[0])
        assert not (h == 0xA5).all()                                 # served: the quads are written
        for p in (cells[0], pos[0], quads[0], own, dx, dt):
            ctx.free(p)
    finally:
        ctx.close()
