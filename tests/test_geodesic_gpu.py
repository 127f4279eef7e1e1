"""Geodesic distance on the GPU (vp_geodesic*, csrc/geodesic.hip) against the numpy restatement of tests/geodesic_ref.py, byte for byte and
statistics included, NAIVE and TILED x the three metrics: boxes that touch at a corner or along an edge on block seams, serpentines across
blocks and inside one block (longer than the sweep cap), fronts that meet on a torus, the golden bunny, seeds outside / equal to / partly
inside the mask, components, the full grid at n = 32 and 96 against the closed form; what a context keeps between calls, refusals, timing
keys, the CLI, vp_geodesic_host."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from cuda_mesh_voxelization_amd import build, capi, mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geodesic_ref as R  # noqa: E402
from test_geodesic_cpu import cli_line, label_reach, seam_box_obj  # noqa: E402

pytestmark = pytest.mark.gpu
ALGOS = (ALGO_NAIVE, ALGO_TILED)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frame(n):
    return Frame.make(n, 1.0, np.zeros(3, np.float32))


def _dev(engine, words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(engine.device)


def _fetch(ctx, n):
    """(D, reach words, stats) of the context's last result, numpy"""
    pd, pr, stats, side = ctx.geodesic_result()
    assert pd and pr and side == n
    d, r = np.empty(n ** 3, np.uint32), np.empty(n ** 3 // 32, np.uint32)
    ctx.download(d, pd)
    ctx.download(r, pr)
    return d, r, stats


def _run(engine, mask, seeds, metric, algo, ctx=None):
    """(D, reach words, stats) of one device call on two (z, y, x) bool grids"""
    ctx = ctx or engine.ctx
    n = mask.shape[0]
    m, s = _dev(engine, R.bool_to_words(mask)), _dev(engine, R.bool_to_words(seeds))
    stats = ctx.geodesic(_frame(n), m.data_ptr(), s.data_ptr(), metric, algo)
    d, r, rstats = _fetch(ctx, n)
    assert rstats == stats
    return d, r, stats


def _check(engine, name, metric, algo):
    """a named case of geodesic_ref against its shared reference"""
    mask, seeds = R.case(name)
    exp, reach, stats = R.expected(name, metric)
    d, r, s = _run(engine, mask, seeds, metric, algo)
    bad = d != exp.reshape(-1)
    assert not bad.any(), (name, metric, algo, int(bad.sum()), np.flatnonzero(bad)[:4].tolist())
    assert np.array_equal(r, R.bool_to_words(reach)), (name, metric, algo)
    assert s == stats, (name, metric, algo, s, stats)
    return exp, reach, stats


def sweep_cap():
    with open(os.path.join(os.path.dirname(capi.LIB_PATH), "csrc", "geodesic.hip")) as f:
        return int(re.search(r"^constexpr uint32_t kGeoSweeps = (\d+);", f.read(), re.M).group(1))


# ---- 1: corner and edge contact on block seams -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("kind", ["corner", "edge", "corner in", "edge in"])
def test_contact_on_block_seams(engine, kind, metric, algo):
    _, _, second = R.contact(kind)
    _, reach, stats = _check(engine, "contact " + kind, metric, algo)
    if metric == R.GEO_6:
        assert not (reach & second).any() and stats[1] == 4096       # no face step crosses: the second box reads NONE
    else:
        assert (reach & second).sum() == 4096 and stats[1] == 8192


def _block_of(idx):
    """the block (bx, by, bz) of every (z, y, x) row of idx"""
    return set(map(tuple, np.stack([idx[:, 2] // 32, idx[:, 1] // 16, idx[:, 0] // 16], axis=1).tolist()))


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("name", sorted(R.SEAMS))
def test_seeds_on_block_seams(engine, name, metric, algo):
    """a seed reads 0 from the start and is never lowered: the blocks that see it through their halo must run all the same"""
    mask, seeds = R.case(name)
    assert not (_block_of(np.argwhere(seeds)) & _block_of(np.argwhere(mask & ~seeds)))   # the seeds' blocks hold nothing else of the mask
    _, reach, stats = _check(engine, name, metric, algo)
    diagonal_only = "edge" in name or "corner" in name
    if metric == R.GEO_6 and diagonal_only:
        assert np.array_equal(reach, seeds) and stats[2] == 0
    else:
        assert np.array_equal(reach, mask) and stats[1] == int(mask.sum()) > stats[0]
        assert stats[2] == ((3 + diagonal_only + ("corner" in name)) if metric == R.GEO_CHAMFER else 1)


def test_cli_zmin_plane_under_a_block_seam(tmp_path):
    """`--geodesic zmin` where the lowest occupied plane is z = 15 at n = 32: the blocks below the seam hold nothing but seeds"""
    cli = build.build_cli()
    mesh = seam_box_obj(tmp_path)
    dumps, lines = {}, {}
    for t in ("2", "1", "0"):
        d = tmp_path / ("t" + t)
        d.mkdir()
        p = subprocess.run([cli, mesh, "-n", "32", "-t", t, "--geodesic", "zmin:6", "-d", str(d / "x")], capture_output=True, text=True, timeout=600, cwd=str(d))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        lines[t] = [ln for ln in p.stdout.splitlines() if ln.startswith("geodesic:")]
        dumps[t] = tuple(np.fromfile(str(d / ("x." + f)), np.uint32) for f in ("grid.u32", "geo.u32", "reach.u32"))
    vox = R.words_to_bool(dumps["0"][0], 32)
    assert int(np.flatnonzero(vox.any(axis=(1, 2)))[0]) == 15 and vox[16].any()
    exp, reach, stats = R.geodesic(vox, R.lowest_plane(vox), R.GEO_6)
    assert stats[1] == int(vox.sum()) > stats[0]
    for t in ("2", "1", "0"):
        assert lines[t] == [cli_line(stats, 32, int(vox.sum()))], t
        assert np.array_equal(dumps[t][1], exp.reshape(-1)) and np.array_equal(dumps[t][2], R.bool_to_words(reach)), t


# ---- 2 and 3: serpentines-------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("n", [32, 64])
def test_serpentine_across_blocks(engine, n, metric, algo):
    _, _, stats = _check(engine, "serpentine %d" % n, metric, algo)
    assert stats[:3] == (1, R.SERPENTINE_VOXELS[n], R.SERPENTINE_MAX[n][metric])


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("metric", R.METRICS)
def test_serpentine_inside_one_block_exceeds_the_sweep_cap(engine, metric, algo):
    mask, _, steps = R.comb()
    assert not mask[:, :, :][16:].any() and not mask[:, 16:].any()   # one block: x < 32, y < 16, z < 16
    # with diagonal steps the turns are cut short: GEO_26's distance to the end is the fewest steps any metric needs
    assert steps >= R.expected("comb", R.GEO_26)[2][2] > sweep_cap(), "the comb no longer outlasts the sweeps of one launch: build a longer maze"
    _, _, stats = _check(engine, "comb", metric, algo)
    assert stats[1] == steps + 1 and (metric != R.GEO_6 or stats[2] == steps)


# ---- 4: two fronts meeting --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("name", ["torus one seed", "torus two seeds", "bunny"])
def test_fronts_that_meet(engine, name, metric, algo):
    mask, _ = R.case(name)
    _, reach, stats = _check(engine, name, metric, algo)
    if name != "bunny":
        assert np.array_equal(reach, mask) and stats[0] == (2 if name == "torus two seeds" else 1)
    if name == "torus two seeds":
        assert stats[2] < R.expected("torus one seed", metric)[2][2]


# ---- 5: seeds and emptiness -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("metric", R.METRICS)
def test_seeds_and_emptiness(engine, metric, algo):
    _, _, stats = _check(engine, "seeds outside", metric, algo)
    assert stats == (0, 0, 0, 0)
    mask, _ = R.case("seeds equal mask")
    exp, _, stats = _check(engine, "seeds equal mask", metric, algo)
    assert (exp[mask] == 0).all() and stats[:3] == (int(mask.sum()), int(mask.sum()), 0)
    mask, seeds = R.case("seeds partly inside")
    _, _, stats = _check(engine, "seeds partly inside", metric, algo)
    assert 0 < stats[0] == int((mask & seeds).sum()) < int(seeds.sum())
    for name in ("two balls", "random sparse"):
        mask, seeds = R.case(name)
        _, reach, stats = _check(engine, name, metric, algo)
        assert np.array_equal(reach, label_reach(mask, seeds, metric))
        if name == "random sparse" or metric == R.GEO_6:             # the balls touch at a corner: only face steps keep them apart
            assert stats[1] < int(mask.sum())


# ---- 6: the grid boundary and sizes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("n", [32, 96])
def test_full_grid_against_the_closed_form(engine, n, metric, algo):
    for corner in (0, 1):
        exp, reach, stats = _check(engine, "full %d %d" % (n, corner), metric, algo)
        assert np.array_equal(exp, R.closed_form(n, metric, corner)) and reach.all() and stats[1] == n ** 3


# ---- 7: context history -------------------------------------------------------------------------------------------------------------------------
def test_context_history_and_release(engine):
    runs = (("torus two seeds", R.GEO_CHAMFER, ALGO_TILED), ("comb", R.GEO_6, ALGO_NAIVE), ("contact edge", R.GEO_26, ALGO_TILED),
            ("serpentine 32", R.GEO_26, ALGO_TILED), ("bunny", R.GEO_6, ALGO_NAIVE))
    ctx = capi.Context(0)
    try:
        assert ctx.geodesic_result() == (0, 0, (0, 0, 0, 0), 0)
        for name, metric, algo in runs:                             # n = 64, 32, 64, 32, 64 on one context
            mask, seeds = R.case(name)
            exp, reach, stats = R.expected(name, metric)
            d, r, s = _run(engine, mask, seeds, metric, algo, ctx)
            fresh = capi.Context(0)
            try:
                fd, fr, fs = _run(engine, mask, seeds, metric, algo, fresh)
            finally:
                fresh.close()
            assert np.array_equal(d, fd) and np.array_equal(r, fr) and s == fs == stats, name
            assert np.array_equal(d, exp.reshape(-1)) and np.array_equal(r, R.bool_to_words(reach)), name
        ctx.release()
        assert ctx.geodesic_result() == (0, 0, (0, 0, 0, 0), 0)
    finally:
        ctx.close()


# ---- 8: refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_result_untouched(engine):
    n = 32
    fr = _frame(n)
    mask, seeds = R.case("seeds partly inside")
    before = _run(engine, mask, seeds, R.GEO_CHAMFER, ALGO_TILED)
    pd, pr, rstats, side = result = engine.ctx.geodesic_result()
    buf = torch.zeros(fr.words + 64, dtype=torch.int32, device=engine.device)
    wp = buf.data_ptr()
    slab = Frame.make(64, 1.0, np.zeros(3, np.float32), 0, 32)
    big = Frame.make(1056, 1.0, np.zeros(3, np.float32))
    lib = capi.lib()
    for frame, m, s, metric, algo, code in ((slab, wp, wp, R.GEO_6, ALGO_TILED, 10002), (big, wp, wp, R.GEO_6, ALGO_TILED, 10002),
                                            (fr, 0, wp, R.GEO_6, ALGO_TILED, 10001), (fr, wp, 0, R.GEO_6, ALGO_NAIVE, 10001),
                                            (fr, wp + 4, wp, R.GEO_26, ALGO_TILED, 10001), (fr, wp, wp + 8, R.GEO_26, ALGO_NAIVE, 10001),
                                            (fr, wp, wp, 3, ALGO_TILED, 10001), (fr, wp, wp, -1, ALGO_NAIVE, 10001),
                                            (fr, wp, wp, R.GEO_CHAMFER, 0, 10001), (fr, wp, wp, R.GEO_CHAMFER, 3, 10001),
                                            (fr, pr, wp, R.GEO_CHAMFER, ALGO_TILED, 10001), (fr, pd, wp, R.GEO_CHAMFER, ALGO_NAIVE, 10001),
                                            (fr, wp, pr, R.GEO_6, ALGO_TILED, 10001), (fr, wp, pd, R.GEO_6, ALGO_NAIVE, 10001)):
        stats = (ctypes.c_uint64 * 4)(6, 7, 8, 9)
        rc = lib.vp_geodesic(engine.ctx._h, ctypes.byref(frame), ctypes.c_void_p(m or None), ctypes.c_void_p(s or None), metric, algo, stats)
        assert rc == code, (metric, algo, rc)
        assert list(stats) == [6, 7, 8, 9]
        assert engine.ctx.geodesic_result() == result
        d, r, st = _fetch(engine.ctx, n)
        assert np.array_equal(d, before[0]) and np.array_equal(r, before[1]) and st == before[2]
    h = np.zeros(fr.words, np.uint32)
    for frame, metric, algo, code in ((slab, R.GEO_6, ALGO_TILED, 10002), (fr, 5, ALGO_TILED, 10001), (fr, R.GEO_6, 9, 10001)):
        with pytest.raises(capi.VPError) as e:
            engine.ctx.geodesic_host(frame, h, h, metric, algo)
        assert e.value.code == code
    with pytest.raises(capi.VPError) as e:
        engine.ctx.geodesic_host(fr, h, h, R.GEO_6, ALGO_TILED, want=(False, False, False))
    assert e.value.code == 10001
    assert lib.vp_geodesic(None, ctypes.byref(fr), ctypes.c_void_p(wp), ctypes.c_void_p(wp), R.GEO_6, ALGO_TILED, None) == 10001
    d, r, st = _fetch(engine.ctx, n)
    assert np.array_equal(d, before[0]) and np.array_equal(r, before[1]) and st == before[2]


# ---- 9: timing keys -------------------------------------------------------------------------------------------------------------------------------
def test_timing_keys(engine):
    n = 64
    fr = _frame(n)
    mask, seeds = R.case("torus one seed")
    m, s = _dev(engine, R.bool_to_words(mask)), _dev(engine, R.bool_to_words(seeds))
    ctx = engine.ctx
    every = list(capi.EVERY_PROF_KEY)

    def keys(fn):
        ctx.prof_reset()
        ctx.prof_enable(True)
        fn()
        ctx.prof_enable(False)
        return {k: v["launches"] for k, v in ctx.prof().items()}
    tiled = keys(lambda: ctx.geodesic(fr, m.data_ptr(), s.data_ptr(), R.GEO_CHAMFER, ALGO_TILED))
    assert set(tiled) == {"md_fill", "md_split", "md_scan", "md_brick"}, tiled
    assert tiled["md_fill"] == 1 and tiled["md_split"] == 1 and tiled["md_brick"] >= 1
    assert tiled["md_scan"] == tiled["md_brick"] + 1                # a list in front of every round and the empty one that ends the loop
    naive = keys(lambda: ctx.geodesic(fr, m.data_ptr(), s.data_ptr(), R.GEO_CHAMFER, ALGO_NAIVE))
    assert set(naive) == {"md_fill", "md_split", "md_naive"}, naive
    assert naive["md_fill"] == 1 and naive["md_split"] == 1 and naive["md_naive"] >= 1
    assert list(capi.EVERY_PROF_KEY) == every and capi.lib().vp_abi_version() == 6


def test_naive_rounds_cross_the_flag_ring_twice(engine):
    """NAIVE with face steps on the serpentine at n = 32: against the y order of the launch a front gains about a voxel per round, so the
    rounds fill at least three batches of eight (csrc/round_ring.h) -- both halves of the flag ring are reused; the result is the reference's"""
    ctx = engine.ctx
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        _check(engine, "serpentine 32", R.GEO_6, ALGO_NAIVE)
    finally:
        ctx.prof_enable(False)
    launches = ctx.prof()["md_naive"]["launches"]
    assert launches >= 3 * 8 and launches % 8 == 0, launches


# ---- 10: the CLI ------------------------------------------------------------------------------------------------------------------------------------
def test_cli_device_equals_host(tmp_path):
    cli = build.build_cli()
    n = 64
    dumps, lines = {}, {}
    for t in ("2", "1", "0"):
        d = tmp_path / ("t" + t)
        d.mkdir()
        p = subprocess.run([cli, M.asset("bunny.obj"), "-n", str(n), "-t", t, "--geodesic", "zmin", "-d", str(d / "x")],
                           capture_output=True, text=True, timeout=900, cwd=str(d))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert "Geodesic]: " in p.stdout
        lines[t] = [ln for ln in p.stdout.splitlines() if ln.startswith("geodesic:")]
        dumps[t] = tuple(np.fromfile(str(d / ("x." + f)), np.uint32) for f in ("grid.u32", "geo.u32", "reach.u32"))
    for t in ("2", "1"):
        assert lines[t] == lines["0"] and len(lines[t]) == 1
        for a, b in zip(dumps[t], dumps["0"]):
            assert np.array_equal(a, b), t
    vox = R.words_to_bool(dumps["0"][0], n)
    exp, reach, stats = R.geodesic(vox, R.lowest_plane(vox), R.GEO_CHAMFER)
    assert np.array_equal(dumps["0"][1], exp.reshape(-1)) and lines["0"][0] == cli_line(stats, n, int(vox.sum()))


def test_cli_measures_the_centre_line(tmp_path):
    cli = build.build_cli()
    n = 64
    p = subprocess.run([cli, M.asset("bunny.obj"), "-n", str(n), "-t", "2", "--skeleton", "curve", "--skeleton-only", "--geodesic", "zmin:26",
                        "-d", str(tmp_path / "x")], capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    skel = R.words_to_bool(np.fromfile(str(tmp_path / "x.grid.u32"), np.uint32), n)
    assert np.array_equal(np.fromfile(str(tmp_path / "x.grid.u32"), np.uint32), np.fromfile(str(tmp_path / "x.skel.u32"), np.uint32))
    touching = label_reach(skel, R.lowest_plane(skel), R.GEO_26)   # the skeleton voxels of the components that touch the seed plane
    reached = int(re.search(r"^geodesic: n 64, seeds \d+, reached (\d+) of (\d+) set", p.stdout, re.M).group(1))
    assert reached == int(touching.sum()) > 0
    assert np.array_equal(np.fromfile(str(tmp_path / "x.reach.u32"), np.uint32), R.bool_to_words(touching))


# ---- 11: vp_geodesic_host ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", R.METRICS)
def test_host_entry_point(engine, metric):
    for kind, algo in (("corner", ALGO_TILED), ("edge in", ALGO_NAIVE)):
        name = "contact " + kind
        mask, seeds = R.case(name)
        mw, sw = R.bool_to_words(mask), R.bool_to_words(seeds)
        dev = _run(engine, mask, seeds, metric, algo)
        exp, reach, stats = R.expected(name, metric)
        for want in ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (True, False, False), (False, False, True)):
            d, r, s = engine.ctx.geodesic_host(_frame(64), mw, sw, metric, algo, want)
            assert (d is None) == (not want[0]) and (r is None) == (not want[1]) and (s is None) == (not want[2])
            assert d is None or (np.array_equal(d, dev[0]) and np.array_equal(d, exp.reshape(-1)))
            assert r is None or (np.array_equal(r, dev[1]) and np.array_equal(r, R.bool_to_words(reach)))
            assert s is None or s == dev[2] == stats


def test_engine_returns_views_of_the_context_buffers(engine):
    mask, seeds = R.case("bunny")
    fr = _frame(64)
    dist, reach, stats = engine.geodesic(fr, _dev(engine, R.bool_to_words(mask)), _dev(engine, R.bool_to_words(seeds)), capi.GEO_26)
    pd, pr, rstats, side = engine.ctx.geodesic_result()
    assert (dist.data_ptr(), reach.data_ptr(), stats, side) == (pd, pr, rstats, 64)
    exp, ereach, estats = R.expected("bunny", R.GEO_26)
    engine.sync()
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), exp.reshape(-1)) and stats == estats
    assert np.array_equal(engine.words_to_numpy(reach), R.bool_to_words(ereach))
    with pytest.raises(capi.VPError) as e:                          # what comes back cannot go in again without a copy
        engine.ctx.geodesic(fr, reach.data_ptr(), reach.data_ptr(), capi.GEO_26)
    assert e.value.code == 10001
    again = engine.geodesic(fr, reach.clone(), reach.clone(), capi.GEO_26)[2]
    assert again == (estats[1], estats[1], 0, int(np.flatnonzero(ereach.reshape(-1))[0]))
