"""Grayscale reconstruction and h-extrema on the GPU (vp_reconstruct*, vp_extrema*, csrc/reconstruct.hip) against the numpy restatement of
tests/reconstruct_ref.py, byte for byte and statistics included, NAIVE and TILED x connectivity 6 and 26 x both modes: gates between blocks
through a face, an edge or a corner, markers on block seams, the comb maze longer than the sweep cap, serpentines, values at the ends of
uint32, the identities against vp_geodesic and vp_fill_interior, duality and idempotence, empty cases, the three balls end to end, what a
context keeps between calls, refusals, timing keys, the largest side, the CLI, the host entry points."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

from cuda_mesh_voxelization_amd import capi
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed as E  # noqa: E402
import geodesic_ref as GR  # noqa: E402
import reconstruct_ref as R  # noqa: E402
import watershed_ref as WS  # noqa: E402

pytestmark = pytest.mark.gpu
ALGOS = (ALGO_NAIVE, ALGO_TILED)
TOP = R.TOP


def _frame(n):
    return Frame.make(n, 1.0, np.zeros(3, np.float32))


def _dev(engine, a):
    return torch.from_numpy(np.array(a).reshape(-1).view(np.int32)).to(engine.device)


def _bits(engine, domain):
    return None if domain is None else _dev(engine, R.bool_to_words(domain))


def _down(ctx, ptr, count):
    a = np.empty(count, np.uint32)
    ctx.download(a, ptr)
    return a


def _run(engine, F, G, domain, mode, conn, algo, ctx=None):
    """(R flat, stats) of one device call on (z, y, x) arrays"""
    ctx = ctx or engine.ctx
    n = G.shape[0]
    f, g, d = _dev(engine, F), _dev(engine, G), _bits(engine, domain)
    stats = ctx.reconstruct(_frame(n), f.data_ptr(), g.data_ptr(), 0 if d is None else d.data_ptr(), mode, conn, algo)
    pr, rstats, side = ctx.reconstruct_result()
    assert pr and side == n and rstats == stats
    return _down(ctx, pr, n ** 3), stats


def _same(got, exp, stats, estats, what):
    bad = got != exp.reshape(-1)
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:4].tolist(), got[bad][:4].tolist(), exp.reshape(-1)[bad][:4].tolist())
    assert stats == estats, (what, stats, estats)


def _check(engine, name, mode, conn, algo):
    exp, estats = R.expected(name, mode, conn)
    got, stats = _run(engine, *R.case(name), mode, conn, algo)
    _same(got, exp, stats, estats, (name, mode, conn, algo))
    return exp, estats


def _run_extrema(engine, values, domain, kind, scale, h, conn, algo, ctx=None):
    ctx = ctx or engine.ctx
    n = values.shape[0]
    v, d = _dev(engine, values), _bits(engine, domain)
    stats = ctx.extrema(_frame(n), v.data_ptr(), 0 if d is None else d.data_ptr(), kind, scale, h, conn, algo)
    pv, ph, pe, rstats, side = ctx.extrema_result()
    assert pv and ph and pe and side == n and rstats == stats
    return _down(ctx, pv, n ** 3), _down(ctx, ph, n ** 3), _down(ctx, pe, n ** 3 // 32), stats


def _check_extrema(engine, name, kind, h, conn, algo):
    values, domain, scale = R.extrema_case(name)
    V, H, Eb, estats = R.extrema_expected(name, kind, h, conn)
    v, hh, e, stats = _run_extrema(engine, values, domain, kind, scale, h, conn, algo)
    what = (name, kind, h, conn, algo)
    assert np.array_equal(v, V.reshape(-1)), what
    _same(hh, H, stats, estats, what)
    assert np.array_equal(e, R.bool_to_words(Eb).reshape(-1)), what
    return V, H, Eb, estats


def sweep_cap():
    with open(os.path.join(os.path.dirname(capi.LIB_PATH), "csrc", "reconstruct.hip")) as f:
        return int(re.search(r"^constexpr uint32_t kRecSweeps = (\d+);", f.read(), re.M).group(1))


# ---- 1: plateaus and ridges across block seams ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("conn", R.CONNS)
@pytest.mark.parametrize("name", sorted(R.GATES))
def test_a_block_reached_through_a_face_an_edge_or_a_corner(engine, name, conn, algo):
    exp, stats = _check(engine, "gate " + name, R.DILATION, conn, algo)
    inside = exp[R.block_box(R.GATES[name])]
    if conn == 6 and R.steps_of(name) > 1:
        assert not inside.any()                                     # at connectivity 6 nothing passes an edge or a corner
    else:
        assert (inside == 7).all() and stats[3] == 9 and stats[1] > 8192


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("conn", R.CONNS)
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("name", ["seams", "plateaus"])
def test_markers_and_plateaus_on_block_seams(engine, name, mode, conn, algo):
    _, stats = _check(engine, name + (" from above" if name == "plateaus" and mode == R.EROSION else ""), mode, conn, algo)
    assert stats[1] > 0


# ---- 2: the sweep cap --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("conn", R.CONNS)
def test_the_comb_outlasts_the_sweeps_of_one_launch(engine, conn, algo):
    F, G, steps = R.comb_field()
    assert not G[16:].any() and not G[:, 16:].any()                 # one block: x < 32, y < 16, z < 16
    # with diagonal steps the turns are cut short: GEO_26's distance to the end is the fewest row-to-row steps any connectivity needs
    assert steps >= GR.expected("comb", GR.GEO_26)[2][2] > sweep_cap(), "the comb no longer outlasts the sweeps of one launch: build a longer maze"
    exp, stats = _check(engine, "comb", R.DILATION, conn, algo)
    assert np.array_equal(exp == 5, G == 5) and stats[1] == steps


# ---- 3: serpentines ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("conn", R.CONNS)
@pytest.mark.parametrize("n", [64, 96])
def test_serpentine_across_blocks(engine, n, conn, algo):
    exp, stats = _check(engine, "serpentine %d" % n, R.DILATION, conn, algo)
    solid = R.case("serpentine %d" % n)[1] == 3
    assert np.array_equal(exp == 2, solid) and stats == (n ** 3, int(solid.sum()) - 1, 2 * int(solid.sum()), 2)
    assert n != 64 or int(solid.sum()) == GR.SERPENTINE_VOXELS[64]


# ---- 4: values at the ends of uint32 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("conn", R.CONNS)
@pytest.mark.parametrize("mode", R.MODES)
def test_values_at_the_ends_of_uint32(engine, mode, conn, algo):
    _check(engine, "ends", mode, conn, algo)
    _check(engine, "random 32", mode, conn, algo)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("kind", (R.MAXIMA, R.MINIMA))
def test_extrema_saturate_at_the_ends_of_uint32(engine, kind, algo):
    for h in (0, 1, TOP - 1, TOP):                                  # h = 0; h larger than every value but the ends
        V, H, Eb, stats = _check_extrema(engine, "ends", kind, h, 26, algo)
        if h == 0:
            assert np.array_equal(H, V) and stats[3] == 0
        if h == TOP:                                                # the marker is flat: H is flat, nothing stands out
            assert len(np.unique(H)) == 1 and not Eb.any()
    _check_extrema(engine, "sqrt", kind, 1 << 12, 6, algo)


# ---- 5: identities against existing features, compared on the device ----------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("conn,metric", [(6, capi.GEO_6), (26, capi.GEO_26)])
def test_binary_reconstruction_is_the_reach_grid_of_vp_geodesic(engine, conn, metric, algo):
    mask, seeds = GR.case("random sparse")
    n = mask.shape[0]
    fr = _frame(n)
    full = torch.full((n ** 3,), -1, dtype=torch.int32, device=engine.device)
    dm, ds = _dev(engine, GR.bool_to_words(mask)), _dev(engine, GR.bool_to_words(seeds))
    zero = torch.zeros_like(full)
    G = torch.where(_dev(engine, mask.astype(np.uint32)) != 0, full, zero)
    F = torch.where(_dev(engine, seeds.astype(np.uint32)) != 0, full, zero)
    rec, stats = engine.reconstruct(fr, F, G, None, capi.REC_DILATION, conn, algo)
    dist, reach, gstats = engine.geodesic(fr, dm, ds, metric, algo)
    engine.sync()
    assert torch.equal(rec != 0, dist != -1) and stats[1] + gstats[0] == gstats[1] < int(mask.sum())
    packed = (rec != 0).view(-1, 32).to(torch.int64).mul(1 << torch.arange(32, device=engine.device)).sum(1)
    assert torch.equal(packed, reach.to(torch.int64) & 0xFFFFFFFF)


@pytest.mark.parametrize("algo", ALGOS)
def test_erosion_from_the_grid_boundary_is_vp_fill_interior(engine, algo):
    import fill_ref
    n = 64
    shell = fill_ref.box_shell(n, (3, 4, 5), (40, 41, 42))          # a closed shell, a shell with a hole in it, and specks in and around both
    leak = fill_ref.box_shell(n, (44, 20, 9), (62, 50, 33))
    leak[20, 30, 44] = False
    shell = shell | leak | (np.random.default_rng(3).random((n, n, n)) < 0.02)
    words = np.ascontiguousarray(R.bool_to_words(shell), np.uint32)
    G = shell.astype(np.uint32)                                     # the binary field: 1 on the solid
    face = np.ones((n, n, n), bool)
    face[1:-1, 1:-1, 1:-1] = False
    F = np.where(face, G, 1).astype(np.uint32)                      # the marker: G on the grid boundary, 1 inside
    fr = _frame(n)
    rec, _ = engine.reconstruct(fr, _dev(engine, F), _dev(engine, G), None, capi.REC_EROSION, 6, algo)
    filled, _ = engine.fill_interior(fr, _dev(engine, words))
    engine.sync()
    packed = (rec != 0).view(-1, 32).to(torch.int64).mul(1 << torch.arange(32, device=engine.device)).sum(1)
    assert torch.equal(packed, filled.to(torch.int64) & 0xFFFFFFFF)
    assert int(torch.count_nonzero(rec)) > int(shell.sum())         # something was filled


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("conn", R.CONNS)
def test_duality_and_idempotence(engine, conn, algo):
    F, G, domain = R.case("random 32")
    fr = _frame(32)
    f, g, d = _dev(engine, F), _dev(engine, G), _bits(engine, domain)
    ero = engine.reconstruct(fr, f, g, d, capi.REC_EROSION, conn, algo)[0].clone()
    dil, dstats = engine.reconstruct(fr, ~f, ~g, d, capi.REC_DILATION, conn, algo)
    assert torch.equal(ero, ~dil)                                   # off the domain too: 0xFFFFFFFF against 0
    dil = dil.clone()
    again, astats = engine.reconstruct(fr, dil, ~g, d, capi.REC_DILATION, conn, algo)
    assert torch.equal(again, dil) and astats == (dstats[0], 0, dstats[2], dstats[3])


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("conn", R.CONNS)
@pytest.mark.parametrize("kind", (R.MAXIMA, R.MINIMA))
def test_extrema_at_h_0_are_the_plateau_regional_extrema(engine, kind, conn, algo):
    for name in ("hills", "hills domain"):
        values, domain, scale = R.extrema_case(name)
        V, H, Eb, stats = _check_extrema(engine, name, kind, 0, conn, algo)
        assert np.array_equal(Eb, R.extrema_plateaus(values, domain, kind, scale, 0, conn)) and stats[1] == int(Eb.sum()) > 0
    _check_extrema(engine, "hills", kind, 3, conn, algo)


# ---- 6: empty cases ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("mode", R.MODES)
def test_empty_cases(engine, mode, algo):
    exp, stats = _check(engine, "empty domain", mode, 26, algo)
    assert stats == (0, 0, 0, 0) and (exp == (TOP if mode == R.EROSION else 0)).all()
    _, stats = _check(engine, "zero marker", mode, 6, algo)
    assert stats[0] == 32 ** 3                                      # a NULL domain
    if mode == R.DILATION:
        assert stats[1:] == (0, 0, 0)
    _, stats = _check(engine, "marker above", R.DILATION, 26, algo)
    assert stats[1] == 0                                            # F >= G everywhere: nothing to do
    v, h, e, st = _run_extrema(engine, R.field(32, 40, 9), np.zeros((32, 32, 32), bool), R.MAXIMA if mode == R.DILATION else R.MINIMA, R.LINEAR, 2, 6, algo)
    assert st == (0, 0, 0, 0) and not e.any()


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("mode", R.MODES)
def test_a_larger_field_at_n_96(engine, mode, algo):
    _check(engine, "random 96", mode, 26, algo)


# ---- 7: the three balls end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("conn", R.CONNS)
def test_three_balls_end_to_end(engine, conn, algo):
    mask, d2 = R.three_balls()
    n = 64
    fr = _frame(n)
    V, H, Eb, estats = R.extrema_expected("balls", R.MAXIMA, 8, conn)
    markers, k = ndi.label(Eb, structure=R.footprint(conn))
    assert k == 3 and estats[1] == 3
    W, cut, wstats = WS.watershed(mask, markers.astype(np.uint32), V, WS.DESCENDING, 1, conn)
    dm = _dev(engine, R.bool_to_words(mask))
    dist = engine.edt(fr, dm, capi.EDT_SEEDS_UNSET, algo=algo)
    dist = torch.where(_dev(engine, mask.astype(np.uint32)) != 0, dist, torch.zeros_like(dist))      # D^2 on the solid, 0 outside
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), d2.reshape(-1))
    scaled, flat, ext, stats = engine.extrema(fr, dist, dm, capi.EXT_MAXIMA, capi.EXT_SQRT16, 8, conn, algo)
    assert stats == estats
    labels, count = engine.components_label(fr, ext.clone(), conn, algo)
    assert count == 3
    wl, wc, ws = engine.watershed(fr, dm, labels, scaled, capi.WS_DESCENDING, 1, conn, algo)
    engine.sync()
    assert ws == wstats and np.array_equal(wl.cpu().numpy().view(np.uint32), W.reshape(-1))
    assert sorted(int(W[c[2], c[1], c[0]]) for c, _ in R.THREE_BALLS) == [1, 2, 3]    # three labels, one per ball centre


# ---- 8: context behaviour --------------------------------------------------------------------------------------------------------------------------
def test_context_history_release_and_independence(engine):
    ctx = capi.Context(0)
    try:
        assert ctx.reconstruct_result() == (0, (0, 0, 0, 0), 0) and ctx.extrema_result() == (0, 0, 0, (0, 0, 0, 0), 0)
        for name, mode, conn, algo in (("seams", R.DILATION, 26, ALGO_TILED), ("random 32", R.EROSION, 6, ALGO_NAIVE), ("gate +x+y", R.DILATION, 26, ALGO_TILED),
                                       ("ends", R.EROSION, 26, ALGO_TILED)):          # n = 64, 32, 64, 32 on one context
            exp, estats = R.expected(name, mode, conn)
            got, stats = _run(engine, *R.case(name), mode, conn, algo, ctx)
            _same(got, exp, stats, estats, name)
        before = ctx.reconstruct_result()
        values, domain, scale = R.extrema_case("hills")
        V, H, Eb, estats = R.extrema_expected("hills", R.MAXIMA, 3, 6)
        v, h, e, stats = _run_extrema(engine, values, domain, R.MAXIMA, scale, 3, 6, ALGO_TILED, ctx)
        assert np.array_equal(h, H.reshape(-1)) and stats == estats
        assert ctx.reconstruct_result() == before                   # vp_extrema leaves vp_reconstruct_result alone
        assert np.array_equal(_down(ctx, before[0], 32 ** 3), got)
        kept = ctx.extrema_result()
        got2, _ = _run(engine, *R.case("random 32"), R.DILATION, 6, ALGO_NAIVE, ctx)
        assert ctx.extrema_result() == kept                         # and vice versa
        assert np.array_equal(_down(ctx, kept[1], 64 ** 3), H.reshape(-1)) and np.array_equal(_down(ctx, kept[2], 64 ** 3 // 32), R.bool_to_words(Eb).reshape(-1))
        ctx.release()
        assert ctx.reconstruct_result() == (0, (0, 0, 0, 0), 0) and ctx.extrema_result() == (0, 0, 0, (0, 0, 0, 0), 0)
    finally:
        ctx.close()


def test_refusals_leave_the_previous_results_untouched(engine):
    n = 32
    fr = _frame(n)
    ctx = engine.ctx
    rec_before = _run(engine, *R.case("random 32"), R.EROSION, 26, ALGO_TILED)
    values, domain, scale = R.extrema_case("sqrt")
    ext_before = _run_extrema(engine, values, domain, R.MAXIMA, scale, 300, 6, ALGO_TILED)
    rres, eres = ctx.reconstruct_result(), ctx.extrema_result()
    buf = torch.zeros(n ** 3 + 64, dtype=torch.int32, device=engine.device)
    wp = buf.data_ptr()
    slab = Frame.make(64, 1.0, np.zeros(3, np.float32), 0, 32)
    big = Frame.make(1056, 1.0, np.zeros(3, np.float32))
    lib = capi.lib()
    V = ctypes.c_void_p

    def unchanged():
        assert ctx.reconstruct_result() == rres and ctx.extrema_result() == eres
        assert np.array_equal(_down(ctx, rres[0], n ** 3), rec_before[0])
        for ptr, count, exp in zip(eres[:3], (n ** 3, n ** 3, n ** 3 // 32), ext_before[:3]):
            assert np.array_equal(_down(ctx, ptr, count), exp)

    pr, (pv, ph, pe) = rres[0], eres[:3]
    for frame, d, f, g, mode, conn, algo, code in (
            (slab, 0, wp, wp, 0, 6, ALGO_TILED, 10002), (big, 0, wp, wp, 0, 6, ALGO_NAIVE, 10002),
            (fr, 0, 0, wp, 0, 6, ALGO_TILED, 10001), (fr, 0, wp, 0, 0, 6, ALGO_TILED, 10001),
            (fr, wp + 4, wp, wp, 0, 6, ALGO_TILED, 10001), (fr, 0, wp + 8, wp, 0, 6, ALGO_NAIVE, 10001), (fr, 0, wp, wp + 4, 1, 26, ALGO_TILED, 10001),
            (fr, 0, wp, wp, 2, 6, ALGO_TILED, 10001), (fr, 0, wp, wp, -1, 6, ALGO_TILED, 10001),
            (fr, 0, wp, wp, 0, 18, ALGO_TILED, 10001), (fr, 0, wp, wp, 0, 6, 0, 10001), (fr, 0, wp, wp, 0, 6, 3, 10001),
            (fr, 0, pr, wp, 0, 6, ALGO_TILED, 10001), (fr, 0, wp, pr, 1, 26, ALGO_NAIVE, 10001), (fr, pr, wp, wp, 0, 6, ALGO_TILED, 10001)):
        stats = (ctypes.c_uint64 * 4)(6, 7, 8, 9)
        rc = lib.vp_reconstruct(ctx._h, ctypes.byref(frame), V(d or None), V(f or None), V(g or None), mode, conn, algo, stats)
        assert rc == code and list(stats) == [6, 7, 8, 9], (mode, conn, algo, rc)
        unchanged()
    for frame, d, v, kind, scale, conn, algo, code in (
            (slab, 0, wp, 0, 0, 6, ALGO_TILED, 10002), (big, 0, wp, 0, 0, 6, ALGO_TILED, 10002), (fr, 0, 0, 0, 0, 6, ALGO_TILED, 10001),
            (fr, wp + 4, wp, 0, 0, 6, ALGO_TILED, 10001), (fr, 0, wp + 12, 1, 1, 26, ALGO_NAIVE, 10001),
            (fr, 0, wp, 2, 0, 6, ALGO_TILED, 10001), (fr, 0, wp, 0, 2, 6, ALGO_TILED, 10001), (fr, 0, wp, 0, 0, 7, ALGO_TILED, 10001),
            (fr, 0, wp, 0, 0, 6, 9, 10001), (fr, 0, pv, 0, 0, 6, ALGO_TILED, 10001), (fr, 0, ph, 1, 1, 26, ALGO_NAIVE, 10001),
            (fr, pe, wp, 0, 0, 6, ALGO_TILED, 10001)):
        stats = (ctypes.c_uint64 * 4)(6, 7, 8, 9)
        rc = lib.vp_extrema(ctx._h, ctypes.byref(frame), V(d or None), V(v or None), kind, scale, 5, conn, algo, stats)
        assert rc == code and list(stats) == [6, 7, 8, 9], (kind, scale, conn, algo, rc)
        unchanged()
    assert lib.vp_reconstruct(None, ctypes.byref(fr), None, V(wp), V(wp), 0, 6, ALGO_TILED, None) == 10001
    assert lib.vp_extrema(None, ctypes.byref(fr), None, V(wp), 0, 0, 0, 6, ALGO_TILED, None) == 10001
    h = np.zeros(n ** 3, np.uint32)
    for call in (lambda: ctx.reconstruct_host(slab, h, h), lambda: ctx.extrema_host(slab, h)):
        with pytest.raises(capi.VPError) as e:
            call()
        assert e.value.code == 10002
    for call in (lambda: ctx.reconstruct_host(fr, h, h, None, 5), lambda: ctx.reconstruct_host(fr, h, h, want=(False, False)),
                 lambda: ctx.extrema_host(fr, h, None, 0, 3), lambda: ctx.extrema_host(fr, h, want=(False,) * 4)):
        with pytest.raises(capi.VPError) as e:
            call()
        assert e.value.code == 10001
    unchanged()
    # the result of one feature may go into the other without a copy: they write different buffers
    again = ctx.reconstruct(fr, eres[1], eres[0], 0, capi.REC_DILATION, 6, ALGO_TILED)
    assert again[:2] == (n ** 3, 0)                                 # H under V is H


def test_timing_keys(engine):
    n = 64
    fr = _frame(n)
    F, G, _ = R.case("seams")
    f, g = _dev(engine, F), _dev(engine, G)
    ctx = engine.ctx
    every = list(capi.EVERY_PROF_KEY)

    def keys(fn):
        ctx.prof_reset()
        ctx.prof_enable(True)
        fn()
        ctx.prof_enable(False)
        return {k: v["launches"] for k, v in ctx.prof().items()}
    tiled = keys(lambda: ctx.reconstruct(fr, f.data_ptr(), g.data_ptr(), 0, capi.REC_DILATION, 26, ALGO_TILED))
    assert set(tiled) == {"md_fill", "md_split", "md_scan", "md_brick"}, tiled
    assert tiled["md_fill"] == 1 and tiled["md_split"] == 1 and tiled["md_brick"] >= 1
    assert tiled["md_scan"] == tiled["md_brick"] + 1                # a list in front of every round and the empty one that ends the loop
    naive = keys(lambda: ctx.reconstruct(fr, f.data_ptr(), g.data_ptr(), 0, capi.REC_DILATION, 26, ALGO_NAIVE))
    assert set(naive) == {"md_fill", "md_split", "md_naive"}, naive
    assert naive["md_fill"] == 1 and naive["md_split"] == 1 and naive["md_naive"] >= 8 and naive["md_naive"] % 8 == 0
    ext = keys(lambda: ctx.extrema(fr, g.data_ptr(), 0, capi.EXT_MAXIMA, capi.EXT_LINEAR, 2, 6, ALGO_TILED))
    assert set(ext) == {"md_fill", "md_split", "md_scan", "md_brick"}, ext
    assert ext["md_fill"] == 4 and ext["md_split"] == 3             # two shifts and two R0 launches; two final launches and the ballot
    assert ext["md_scan"] == ext["md_brick"] + 2
    assert list(capi.EVERY_PROF_KEY) == every and capi.lib().vp_abi_version() == 6


def test_naive_rounds_cross_the_flag_ring_twice(engine):
    """NAIVE with face steps on the comb: a front gains about a voxel per round against the order of the launch, so the rounds fill at least
    three batches of eight (csrc/round_ring.h) -- both halves of the flag ring are reused; the result is the reference's"""
    ctx = engine.ctx
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        _check(engine, "comb", R.DILATION, 6, ALGO_NAIVE)
    finally:
        ctx.prof_enable(False)
    launches = ctx.prof()["md_naive"]["launches"]
    assert launches >= 3 * 8 and launches % 8 == 0, launches


# ---- 9: the largest side ---------------------------------------------------------------------------------------------------------------------------
N = 1024
PLACES = {"far corner": None, "unaligned": (949, 953, 957)}


def _offset(place, m):
    return PLACES[place] or (N - m,) * 3


def _done(engine):
    engine.ctx.release()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("place", sorted(PLACES))
def test_reconstruction_of_an_embedded_case_at_n_1024(engine, place, algo):
    """R spans 4 GiB: a 32-bit index anywhere shows.  Outside the box F = G = 0: walls, so the small reference holds as it is."""
    name, conn = "gate +x+y+z", 26
    F, G, _ = R.case(name)
    m = G.shape[0]
    o = _offset(place, m)
    exp, estats = R.expected(name, R.DILATION, conn)
    f, g = E.embed(F, N, o, engine.device), E.embed(G, N, o, engine.device)
    rec = None
    try:
        rec, stats = engine.reconstruct(Frame.make(N, 1.0, np.zeros(3, np.float32)), f, g, None, capi.REC_DILATION, conn, algo)
        engine.sync()
        assert stats == (N ** 3,) + estats[1:], (stats, estats)
        assert np.array_equal(E.box(rec, N, m, o), exp)
        assert int(torch.count_nonzero(rec)) == int(np.count_nonzero(exp))
    finally:
        del rec, f, g
        _done(engine)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("place", sorted(PLACES))
def test_extrema_of_an_embedded_case_at_n_1024(engine, place, algo):
    mask, d2 = R.three_balls()
    m, conn = 64, 6
    o = _offset(place, m)
    V, H, Eb, estats = R.extrema_expected("balls", R.MAXIMA, 8, conn)
    v, d = E.embed(d2, N, o, engine.device), E.embed(mask, N, o, engine.device)
    out = None
    try:
        out = engine.extrema(Frame.make(N, 1.0, np.zeros(3, np.float32)), v, d, capi.EXT_MAXIMA, capi.EXT_SQRT16, 8, conn, algo)
        engine.sync()
        assert out[3] == estats, (out[3], estats)
        assert np.array_equal(E.box(out[0], N, m, o), V) and np.array_equal(E.box(out[1], N, m, o), H)
        assert int(torch.count_nonzero(out[0])) == int(np.count_nonzero(V)) and int(torch.count_nonzero(out[1])) == int(np.count_nonzero(H))
        assert np.array_equal(E.box_bits(out[2], N, m, o), Eb) and int(torch.count_nonzero(out[2])) == E.nonzero_words(Eb, o)
    finally:
        del out, v, d
        _done(engine)


# ---- 10: the CLI ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["bunny.obj", "bimba.obj"])
@pytest.mark.parametrize("arg", ["h:0.5", "h:1.5:2:26"])
def test_cli_device_equals_host(tmp_path, mesh, arg):
    """NAIVE (-t 1) and TILED (-t 2) against SEQUENTIAL (-t 0): the two lines, the labels and the cut grid"""
    from cuda_mesh_voxelization_amd import build, mesh as M
    cli = build.build_cli()
    n = 64
    dumps, lines = {}, {}
    for t in ("2", "1", "0"):
        d = tmp_path / ("t" + t)
        d.mkdir()
        p = subprocess.run([cli, M.asset(mesh), "-n", str(n), "-t", t, "--watershed", arg, "-d", str(d / "x")], capture_output=True, text=True,
                           timeout=900, cwd=str(d))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert "Extrema]: " in p.stdout
        lines[t] = [ln for ln in p.stdout.splitlines() if ln.startswith(("extrema:", "watershed:"))]
        dumps[t] = tuple(np.fromfile(str(d / ("x." + f)), np.uint32) for f in ("grid.u32", "labels.u32"))
    assert len(lines["0"]) == 2 and lines["0"][0].startswith("extrema: n 64, h16 %d, " % (8 if arg == "h:0.5" else 24))
    for t in ("2", "1"):
        assert lines[t] == lines["0"], (t, lines[t], lines["0"])
        for a, b in zip(dumps[t], dumps["0"]):
            assert np.array_equal(a, b), t


# ---- 11: the host entry points -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_host_entry_points(engine, algo):
    F, G, domain = R.case("random 32")
    fr = _frame(32)
    exp, estats = R.expected("random 32", R.EROSION, 26)
    dw = np.ascontiguousarray(R.bool_to_words(domain), np.uint32).reshape(-1)
    for want in ((True, True), (True, False), (False, True)):
        r, s = engine.ctx.reconstruct_host(fr, F, G, dw, R.EROSION, 26, algo, want)
        assert (r is None) == (not want[0]) and (s is None) == (not want[1])
        assert r is None or np.array_equal(r, exp.reshape(-1))
        assert s is None or s == estats
    r, s = engine.ctx.reconstruct_host(fr, F, G, None, R.DILATION, 6, algo)
    ref, rstats = R.reconstruct(F, G, None, R.DILATION, 6)
    assert np.array_equal(r, ref.reshape(-1)) and s == rstats
    values, domain, scale = R.extrema_case("sqrt")
    V, H, Eb, estats = R.extrema_expected("sqrt", R.MINIMA, 700, 26)
    for want in ((True, True, True, True), (False, True, False, False), (False, False, True, True), (True, False, False, False), (False, False, False, True)):
        v, h, e, s = engine.ctx.extrema_host(fr, values, None, R.MINIMA, scale, 700, 26, algo, want)
        assert [x is None for x in (v, h, e, s)] == [not w for w in want]
        assert v is None or np.array_equal(v, V.reshape(-1))
        assert h is None or np.array_equal(h, H.reshape(-1))
        assert e is None or np.array_equal(e, R.bool_to_words(Eb).reshape(-1))
        assert s is None or s == estats


def test_engine_returns_views_of_the_context_buffers(engine):
    F, G, _ = R.case("seams")
    fr = _frame(64)
    rec, stats = engine.reconstruct(fr, _dev(engine, F), _dev(engine, G), None, capi.REC_DILATION, 26)
    pr, rstats, side = engine.ctx.reconstruct_result()
    assert (rec.data_ptr(), stats, side) == (pr, rstats, 64)
    with pytest.raises(capi.VPError) as e:                          # what comes back cannot go in again without a copy
        engine.ctx.reconstruct(fr, pr, pr)
    assert e.value.code == 10001
    scaled, flat, ext, stats = engine.extrema(fr, _dev(engine, G), None, capi.EXT_MAXIMA, capi.EXT_LINEAR, 2, 26)
    pv, ph, pe, estats, side = engine.ctx.extrema_result()
    assert (scaled.data_ptr(), flat.data_ptr(), ext.data_ptr(), stats, side) == (pv, ph, pe, estats, 64)
    with pytest.raises(capi.VPError) as e:
        engine.ctx.extrema(fr, ph)
    assert e.value.code == 10001
