"""Local thickness on the GPU (vp_thickness*, csrc/thickness.hip) against the numpy restatement of tests/thickness_ref.py, bit for bit:
NAIVE, TILED and vp_thickness_host on the hand cases and random grids at n = 32 (one word per row, four bricks per side; at rmax = 32 the
halo leaves the grid on every side), on the dumbbell, the full grid and slabs whose faces sit around brick boundaries at n = 64, on a
random grid and on bunny's conservative shell and filled solid at n = 96; at n = 128 against the C++ host form; three bars at n = 1024
against the closed form, on the device; the thin grid and its count, its hand-over to the components and the surface nets; refusals,
records, release, timing keys; the CLI.

A NAIVE launch costs the sum of the ball volumes.  Every test computes that sum on the CPU from the reference D and launches NAIVE only
below thickness_ref.NAIVE_LIMIT = 2e8 pairs; `_naive_expected` names the cases that must stay below it, so that none drops out unseen.
Above it -- the full 64^3 grid at rmax 8 (3.2e8) and 32 (2.0e9), bunny's solid at 128^3 (5.4e8, 4.2e9), the torus at 128^3 and rmax 32
(3.6e8) -- TILED and the host form stand alone."""
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
import thickness_ref as R  # noqa: E402
from test_thickness_cpu import check_exe, run_check  # noqa: E402,F401  (check_exe: the fixture that builds tests/cpp/thickness_check.cpp)

pytestmark = pytest.mark.gpu


def _frame(n):
    return Frame.make(n, 1.0, np.zeros(3, np.float32))


def _bits(words):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little").astype(bool)


def _run(engine, n, words, rmax, thin2, algo):
    """(T2, thin words, thin count) of one device call, numpy"""
    fr = _frame(n)
    d = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(engine.device)
    count = engine.ctx.thickness(fr, d.data_ptr(), rmax, thin2, algo, count=True)
    dt, dg, side = engine.ctx.thickness_result()
    assert dt and dg and side == n
    t2, g = np.empty(fr.voxels, np.uint32), np.empty(fr.voxels // 32, np.uint32)
    engine.ctx.download(t2, dt)
    engine.ctx.download(g, dg)
    return t2, g, count


def _check(engine, vox, rmax, tag, naive=True, exp=None, D=None, thin2s=None):
    """NAIVE (below the limit), TILED and the host entry point against the restatement, T2 and the thin grids of four thresholds"""
    n = vox.shape[0]
    words = R.bool_to_words(vox)
    D = R.capped_radius(vox, rmax) if D is None else D
    exp = R.thickness_numpy(vox, rmax, D) if exp is None else exp
    pairs = R.ball_volume_sum(D)
    print("%s: n %d rmax %d, sum of ball volumes %.3g" % (tag, n, rmax, pairs))
    if naive:
        assert pairs < R.NAIVE_LIMIT, (tag, pairs)
    thin2s = (0, 1, R.thin2_of_width(min(3, 2 * rmax)), rmax * rmax) if thin2s is None else thin2s
    for k, thin2 in enumerate(thin2s):
        exp_thin = R.thin_numpy(vox, exp, thin2)
        exp_words = R.bool_to_words(exp_thin)
        for algo in (ALGO_NAIVE, ALGO_TILED) if naive and (k == 0 or pairs < 2e7) else (ALGO_TILED,):
            t2, g, count = _run(engine, n, words, rmax, thin2, algo)
            bad = t2 != exp.reshape(-1)
            assert not bad.any(), (tag, rmax, algo, int(bad.sum()), np.argwhere(bad.reshape(n, n, n))[:4].tolist())
            assert np.array_equal(g, exp_words), (tag, rmax, thin2, algo)
            assert count == int(exp_thin.sum()) == int(_bits(g).sum()), (tag, rmax, thin2, algo)
    t2, g, count = engine.ctx.thickness_host(_frame(n), words, rmax, thin2s[-1], ALGO_TILED)
    assert np.array_equal(t2, exp.reshape(-1)) and np.array_equal(g, R.bool_to_words(R.thin_numpy(vox, exp, thin2s[-1]))), (tag, rmax, "host")
    assert count == int(R.thin_numpy(vox, exp, thin2s[-1]).sum())
    return exp


# ---- n = 32 ---------------------------------------------------------------------------------------------------------------------
def test_hand_cases_at_32(engine):
    for name, rmax, vox, exp in R.hand_cases(32):
        if isinstance(exp, tuple) and "axis=1" in name:
            continue                                                 # the slabs across x and across z: y adds nothing that z does not
        got = _check(engine, vox, rmax, name, thin2s=(rmax * rmax,))
        if isinstance(exp, tuple):
            assert np.array_equal(got[exp[1]], exp[0][exp[1]]), name
        else:
            assert np.array_equal(got, exp), name


@pytest.mark.parametrize("density", [0.5, 0.97, 0.995])
@pytest.mark.parametrize("rmax", [1, 2, 5, 32])
def test_random_grids_at_32(engine, density, rmax):
    vox = R.words_to_bool(R.random_grid(32, density, 31 + rmax), 32)
    _check(engine, vox, rmax, "random %g" % density)
    if density == 0.995:
        _check(engine, ~vox, rmax, "complement of random %g" % density, thin2s=(1,))


def test_full_grid_at_32_the_halo_leaves_the_grid_on_every_side(engine):
    exp = _check(engine, np.ones((32,) * 3, bool), 32, "full 32")
    assert exp.max() == 256 and exp[0, 0, 0] == 4


# ---- n = 64 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rmax", [4, 8, 16])
def test_dumbbell(engine, rmax):
    vox = R.dumbbell()
    exp = _check(engine, vox, rmax, "dumbbell", thin2s=(0, 9, rmax * rmax))
    assert exp[32, 32, 32] == 4
    if rmax <= 8:
        assert exp[32, 32, 16] == rmax * rmax and int(R.thin_numpy(vox, exp, 9).sum()) == 99


@pytest.mark.parametrize("rmax,naive", [(4, True), (8, False), (32, False)])
def test_full_grid_at_64(engine, rmax, naive):
    """rmax = 32 saturates only at the two central planes of each axis: the eight centre voxels carry D = 32^2"""
    vox = np.ones((64,) * 3, bool)
    exp = _check(engine, vox, rmax, "full 64", naive=naive, thin2s=(rmax * rmax,))
    if rmax == 32:
        assert int((R.capped_radius(vox, 32) == 1024).sum()) == 8 and exp.max() == 1024 and exp.min() == 4


@pytest.mark.parametrize("lo,w", [(7, 9), (8, 8), (9, 7), (15, 2), (16, 17), (23, 18)])
def test_slabs_across_brick_boundaries_at_64(engine, lo, w):
    """faces at 8 k - 1, 8 k and 8 k + 1: the balls of the centre planes cross brick boundaries"""
    for axis in (0, 2):
        vox = R.slab(64, lo, w, axis)
        exp = _check(engine, vox, 12, "slab %d+%d axis %d" % (lo, w, axis), thin2s=(R.thin2_of_width(w), R.thin2_of_width(w + 1)))
        sl = [slice(16, 48)] * 3
        sl[axis] = slice(lo, lo + w)
        assert (exp[tuple(sl)] == ((w + 1) // 2) ** 2).all()


# ---- n = 96: three words per row, twelve bricks per side ------------------------------------------------------------------------------
def test_random_grid_at_96(engine):
    vox = R.words_to_bool(R.random_grid(96, 0.97, 96), 96)
    _check(engine, vox, 8, "random 0.97 at 96", thin2s=(2, 64))


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


@pytest.mark.parametrize("kind", ["shell", "filled"])
def test_bunny_at_96(engine, kind):
    vox = R.words_to_bool(_mesh_grid(engine, "bunny.obj", 96, kind), 96)
    assert vox.any() and not vox.all()
    _check(engine, vox, 8, "bunny %s at 96" % kind, thin2s=(R.thin2_of_width(4), 64))


# ---- n = 128: NAIVE == TILED == the C++ host form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,rmax,naive", [("torus.obj", "solid", 8, True), ("torus.obj", "solid", 32, False),
                                                  ("bunny.obj", "filled", 8, False), ("bunny.obj", "filled", 32, False)])
def test_at_128_against_the_host_form(engine, check_exe, tmp_path, name, kind, rmax, naive):
    """numpy is too slow here.  The host form runs its planes in parallel (VOX::LocalThickness<OPENMP>): the same function as SEQUENTIAL,
    which the CPU suite pins to the restatement.  D for the NAIVE condition comes from vp_edt, which has its own suite."""
    n = 128
    words = _mesh_grid(engine, name, n, kind)
    vox = R.words_to_bool(words, n)
    thin2 = rmax * rmax                                               # every voxel that is not saturated: these solids have no thin wall
    host_t2, host_thin, host_count = run_check(check_exe, words, n, rmax, thin2, 32, "o", str(tmp_path / "h"))["omp"]
    assert host_t2.max() > 1 and host_count == int(_bits(host_thin).sum()) == int(((host_t2 > 0) & (host_t2 < thin2)).sum())
    e = engine.edt(_frame(n), torch.from_numpy(words.view(np.int32)).to(engine.device), R.UNSET)
    engine.sync()
    pairs = R.ball_volume_sum(R.capped_radius(vox, rmax, e.cpu().numpy().view(np.uint32).reshape(n, n, n)))
    print("%s at 128, rmax %d: sum of ball volumes %.3g" % (name, rmax, pairs))
    assert (pairs < R.NAIVE_LIMIT) == naive
    for algo in (ALGO_NAIVE, ALGO_TILED) if naive else (ALGO_TILED,):
        t2, g, count = _run(engine, n, words, rmax, thin2, algo)
        assert np.array_equal(t2, host_t2), (name, rmax, algo, int((t2 != host_t2).sum()))
        assert np.array_equal(g, host_thin) and count == host_count, (name, rmax, algo)


# ---- n = 1024 ---------------------------------------------------------------------------------------------------------------------------
def test_three_bars_at_1024(engine):
    """TILED only, checked on the device: bars of z widths 3, 20 and 200 over x, y = 100 .. 899 at rmax 16 read ceil(w / 2)^2 = 4 and 100,
    and 256 (saturated) in the widest, everywhere at least rmax away from the bars' ends"""
    n, rmax = 1024, 16
    fr = _frame(n)
    words, bars = R.boxes_1024_words(n)
    d = torch.from_numpy(words.view(np.int32)).to(engine.device)
    thin2 = R.thin2_of_width(8)
    count = engine.ctx.thickness(fr, d.data_ptr(), rmax, thin2, ALGO_TILED, count=True)
    t2, thin = engine.thickness(fr, d, rmax, thin2)
    engine.sync()
    vol = t2.view(n, n, n)
    set_voxels = 800 * 800 * sum(w for _, w in bars)
    assert int((t2 != 0).sum()) == set_voxels and int(t2.max()) == 256
    for z0, w in bars:
        inner = vol[z0:z0 + w, 116:884, 116:884]
        exp = min(((w + 1) // 2) ** 2, 256)
        assert bool((inner == exp).all()), (w, int((inner != exp).sum()))
        assert not bool(vol[z0 - 1].any()) and not bool(vol[z0 + w].any())
        assert bool((vol[z0:z0 + w, 100:900, 100:900] >= 1).all())
    bits = thin.view(torch.uint8)
    pop = sum(int(((bits >> k) & 1).sum()) for k in range(8))
    assert pop == count and 3 * 800 * 800 <= count < 3 * 800 * 800 + 4 * 800 * 220 * 16
    tw = thin.view(n, n, n // 32)
    row = torch.from_numpy(words.reshape(n, n, n // 32)[100, 500].view(np.int32)).to(engine.device)
    assert bool((tw[100:103, 100:900] == row).all())                  # the 3-voxel bar is thin as a whole
    assert not bool(tw[300:320, 116:884, 4:27].any()) and not bool(tw[500:700, 116:884, 4:27].any())
    del t2, thin, vol, tw, d
    engine.ctx.release()
    torch.cuda.empty_cache()


# ---- the thin grid is a grid like any other ---------------------------------------------------------------------------------------------
def test_thin_grid_feeds_components_and_surface_nets(engine):
    n = 64
    vox = R.dumbbell()
    fr = _frame(n)
    d = torch.from_numpy(R.bool_to_words(vox).view(np.int32)).to(engine.device)
    t2, thin = engine.thickness(fr, d, 8, 9)
    engine.sync()
    assert t2.data_ptr() == engine.ctx.thickness_result()[0] and thin.data_ptr() == engine.ctx.thickness_result()[1]
    labels, k = engine.components_label(fr, thin)
    assert k == 1 and int((labels != 0).sum()) == 99                  # the rod between the balls: one component of 99 voxels
    nv, nq = engine.ctx.surfnets_count(fr, thin.data_ptr())
    # a 3 x 3 x 11 box: one quad per exposed voxel face, 2 (9 + 33 + 33), and one vertex per lattice point of its surface, 4 * 4 * 12 - 2 * 2 * 10
    assert nq == 150 and nv == 152
    # what comes back cannot go in again without a copy: the grid would be read while it is written
    with pytest.raises(capi.VPError) as e:
        engine.ctx.thickness(fr, thin.data_ptr(), 8, 9)
    assert e.value.code == 10001
    again, _ = engine.thickness(fr, thin.clone(), 8, 0)
    engine.sync()
    assert int(again.max()) == 4 and int((again != 0).sum()) == 99


# ---- refusals and shared state -----------------------------------------------------------------------------------------------------------
def test_result_is_null_before_a_build_and_after_a_release():
    ctx = capi.Context(0)
    try:
        assert ctx.thickness_result() == (0, 0, 0)
        words = R.random_grid(32, 0.9, 3)
        dw = ctx.malloc(words.nbytes)
        ctx.upload(dw, words)
        ctx.thickness(_frame(32), dw, 4, 0, ALGO_TILED)
        dt, dg, n = ctx.thickness_result()
        assert dt and dg and n == 32
        ctx.release()
        assert ctx.thickness_result() == (0, 0, 0)
        ctx.free(dw)
    finally:
        ctx.close()


def test_refusals_leave_the_previous_result_and_a_sentinel_untouched(engine):
    n = 32
    vox = R.words_to_bool(R.random_grid(n, 0.97, 5), n)
    words = R.bool_to_words(vox)
    fr = _frame(n)
    before = _run(engine, n, words, 5, 4, ALGO_TILED)
    ptrs = engine.ctx.thickness_result()
    sentinel = torch.full((fr.words + 64,), 0x5A5A5A5A, dtype=torch.int32, device=engine.device)
    buf = sentinel.clone()
    wp = buf.data_ptr()
    slab = Frame.make(64, 1.0, np.zeros(3, np.float32), 0, 32)
    big = Frame.make(2048, 1.0, np.zeros(3, np.float32))
    for frame, ptr, rmax, thin2, algo, code in ((slab, wp, 4, 0, ALGO_TILED, 10002), (big, wp, 4, 0, ALGO_TILED, 10002),
                                                (fr, 0, 4, 0, ALGO_TILED, 10001), (fr, wp + 4, 4, 0, ALGO_TILED, 10001),
                                                (fr, wp, 0, 0, ALGO_TILED, 10001), (fr, wp, 33, 0, ALGO_NAIVE, 10001),
                                                (fr, wp, 4, 17, ALGO_TILED, 10001), (fr, wp, 4, 0, 0, 10001), (fr, wp, 4, 0, 3, 10001),
                                                (fr, ptrs[0], 4, 0, ALGO_TILED, 10001), (fr, ptrs[1], 4, 0, ALGO_NAIVE, 10001)):
        with pytest.raises(capi.VPError) as e:
            engine.ctx.thickness(frame, ptr, rmax, thin2, algo)
        assert e.value.code == code, (rmax, thin2, algo, e.value.code)
        assert engine.ctx.thickness_result() == ptrs
    h = np.zeros(fr.words, np.uint32)
    for frame, rmax, thin2, algo, code in ((slab, 4, 0, ALGO_TILED, 10002), (fr, 40, 0, ALGO_TILED, 10001), (fr, 4, 17, ALGO_TILED, 10001),
                                           (fr, 4, 0, 9, 10001)):
        with pytest.raises(capi.VPError) as e:
            engine.ctx.thickness_host(frame, h, rmax, thin2, algo)
        assert e.value.code == code
    engine.sync()
    assert torch.equal(buf, sentinel)
    t2, g = np.empty(fr.voxels, np.uint32), np.empty(fr.voxels // 32, np.uint32)
    engine.ctx.download(t2, ptrs[0])
    engine.ctx.download(g, ptrs[1])
    assert np.array_equal(t2, before[0]) and np.array_equal(g, before[1])


def test_a_pending_jfa_start_is_dropped_when_the_result_buffers_take_its_grid(engine):
    n = 128
    fr = _frame(n)
    ctx = engine.ctx
    src = torch.from_numpy(R.random_grid(n, 0.5, 1).view(np.int32)).to(engine.device)
    other = torch.from_numpy(R.random_grid(160, 0.5, 2).view(np.int32)).to(engine.device)
    sdf = torch.empty(fr.voxels, dtype=torch.float32, device=engine.device)

    def refused(fn):
        with pytest.raises(capi.VPError) as e:
            fn()
        assert e.value.code == 10001

    for grow in (False, True):
        ctx.thickness(fr, src.data_ptr(), 2, 4)
        thin = ctx.thickness_result()[1]
        ctx.jfa_start(fr, thin, None, 0, ALGO_TILED)                  # the thin grid is a grid like any other: a start may stand on it
        if grow:
            ctx.thickness(_frame(160), other.data_ptr(), 2, 4)        # the buffers grow: the bytes of the start are freed
        else:
            ctx.thickness(fr, src.data_ptr(), 3, 4)                   # ... or written again in place
        refused(lambda: ctx.jfa_run(fr, thin, -np.inf, sdf.data_ptr(), None, 0, ALGO_TILED))
    # a start on a grid of the caller's stands through a build
    ctx.jfa_start(fr, src.data_ptr(), None, 0, ALGO_TILED)
    ctx.thickness(fr, src.data_ptr(), 2, 4)
    ctx.jfa_run(fr, src.data_ptr(), -np.inf, sdf.data_ptr(), None, 0, ALGO_TILED)
    engine.sync()
    assert torch.equal(sdf, engine.jfa(fr, src))


def test_buffers_are_released_and_regrown(engine):
    n = 256
    fr = _frame(n)
    w = torch.from_numpy(np.tile(R.random_grid(64, 0.97, 9), 64).view(np.int32)).to(engine.device)      # any words will do
    ctx = engine.ctx
    first = [t.clone() for t in engine.thickness(fr, w, 4, 4)]
    engine.sync()
    torch.cuda.empty_cache()
    before = torch.cuda.mem_get_info()[0]
    ctx.release()
    freed = torch.cuda.mem_get_info()[0] - before
    own = (4 + 4 + 2) * fr.voxels                                     # T2, the distance volume and the uint16 radii at least
    assert freed >= own, freed
    assert ctx.thickness_result() == (0, 0, 0)
    again = engine.thickness(fr, w, 4, 4)                              # and the next call regrows them
    engine.sync()
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert torch.cuda.mem_get_info()[0] <= before + (freed - own)
    ctx.release()
    torch.cuda.empty_cache()


def test_timing_keys(engine):
    n = 64
    fr = _frame(n)
    w = torch.from_numpy(R.random_grid(n, 0.97, 4).view(np.int32)).to(engine.device)
    ctx = engine.ctx
    every = list(capi.EVERY_PROF_KEY)

    def keys(fn):
        ctx.prof_reset()
        ctx.prof_enable(True)
        fn()
        ctx.prof_enable(False)
        return {k: v["launches"] for k, v in ctx.prof().items()}
    assert keys(lambda: ctx.thickness(fr, w.data_ptr(), 4, 4, ALGO_TILED)) == {"edt_x": 2, "edt_y": 2, "edt_z": 2, "edt_thresh": 2, "md_brick": 1,
                                                                             "md_fill": 1}
    assert keys(lambda: ctx.thickness(fr, w.data_ptr(), 4, 4, ALGO_TILED, count=True)) == {"edt_x": 2, "edt_y": 2, "edt_z": 2, "edt_thresh": 2,
                                                                                         "md_brick": 1, "md_fill": 1, "md_split": 1}
    assert keys(lambda: ctx.thickness(fr, w.data_ptr(), 4, 4, ALGO_NAIVE)) == {"edt_x": 1, "edt_y_naive": 1, "edt_z_naive": 1, "md_naive": 1,
                                                                             "edt_thresh": 1}
    assert list(capi.EVERY_PROF_KEY) == every and len(capi.EVERY_PROF_KEY) == 55 and len(capi.HEADER_PROF_KEYS) == 64
    for i, name in enumerate(capi.HEADER_PROF_KEYS):
        assert capi.lib().vp_prof_name(i).decode() == name


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------
def test_cli_device_equals_host(tmp_path):
    cli = build.build_cli()
    n = 64
    dumps = {}
    for t in ("2", "1", "0"):
        d = tmp_path / ("t" + t)
        d.mkdir()
        p = subprocess.run([cli, M.asset("bunny.obj"), "-n", str(n), "-t", t, "--thickness", "8:5", "-d", str(d / "x")], capture_output=True,
                           text=True, timeout=900, cwd=str(d))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert "Thickness]: " in p.stdout and "thin voxels (thinner than 5 voxels, T2 < 7): " in p.stdout
        dumps[t] = tuple(np.fromfile(str(d / ("x." + f)), np.uint32) for f in ("grid.u32", "thick.u32", "thin.u32"))
    for t in ("2", "1"):
        for a, b in zip(dumps[t], dumps["0"]):
            assert np.array_equal(a, b), t
    assert dumps["0"][1].max() > 4 and dumps["0"][2].any()
    d = tmp_path / "thin"
    d.mkdir()
    p = subprocess.run([cli, M.asset("bunny.obj"), "-n", str(n), "-t", "2", "--thickness", "8:5", "--thin-only", "-e", "--surface-nets", "2",
                        "-d", str(d / "x")], capture_output=True, text=True, timeout=900, cwd=str(d))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert np.array_equal(np.fromfile(str(d / "x.grid.u32"), np.uint32), dumps["0"][2])
    assert os.path.getsize(str(d / "out" / "thin_tiled_out.obj")) > 0
    for args in (["--thickness", "8", "--thin-only"], ["--thin-only"], ["--thickness", "8:5", "-g", "2"], ["--thickness", "40"],
                 ["--thickness", "8:17"]):
        p = subprocess.run([cli, M.asset("d20.obj"), "-n", "32", "-t", "2"] + args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert p.returncode != 0, args
