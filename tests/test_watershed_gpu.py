"""Seeded watershed and influence zones on the GPU (vp_watershed*, csrc/watershed.hip) against the numpy restatement of
tests/watershed_ref.py, byte for byte (labels, cut grid) and statistics included, NAIVE and TILED x both connectivities: the two-ball
cases, markers on every kind of block seam, interfaces along a seam plane and across a block corner, the snake, the diagonal chain,
random masks with ties everywhere and basins without markers (both quanta, both orders), the extreme labels, an empty mask, no markers,
markers that cover the mask, a side that is no power of two; the limits of the key (P up to 2^32 - 1, a span of 16383, quanta up to
2^32 - 1, the extreme labels, all at once), blocks flooded only through a seam, the comb that outlasts the sweep cap; what a context
keeps between calls, refusals (the quantum they name against the reference), timing keys,
vp_watershed_host and Engine.watershed.  Sides 32, 64 and 96; side 1024 is in tests/test_largest_side_gpu.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from cuda_mesh_voxelization_amd import build, capi
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import watershed_ref as R  # noqa: E402
from test_watershed_cpu import cli_expected, cli_run, comb_past_the_sweep_cap  # noqa: E402

pytestmark = pytest.mark.gpu
ALGOS = (ALGO_NAIVE, ALGO_TILED)


def _frame(n):
    return Frame.make(n, 1.0, np.zeros(3, np.float32))


def _dev(engine, a):
    return torch.from_numpy(np.array(a).reshape(-1).view(np.int32)).to(engine.device)


def _last_error():
    return (capi.lib().vp_last_error() or b"").decode("utf-8", "replace")


def _fetch(ctx, n):
    """(W, cut words, stats) of the context's last result, numpy"""
    pl, pc, stats, side = ctx.watershed_result()
    assert pl and pc and side == n
    w, c = np.empty(n ** 3, np.uint32), np.empty(n ** 3 // 32, np.uint32)
    ctx.download(w, pl)
    ctx.download(c, pc)
    return w, c, stats


def _run(engine, mask, markers, priority, order, q, conn, algo, ctx=None):
    """(W, cut words, stats) of one device call"""
    ctx = ctx or engine.ctx
    n = mask.shape[0]
    m, l = _dev(engine, R.bool_to_words(mask)), _dev(engine, markers)
    p = None if priority is None else _dev(engine, priority)
    stats = ctx.watershed(_frame(n), m.data_ptr(), l.data_ptr(), 0 if p is None else p.data_ptr(), order, q, conn, algo)
    w, c, rstats = _fetch(ctx, n)
    assert rstats == stats
    return w, c, stats


def _check(engine, name, conn, algo, ctx=None):
    """a named case of watershed_ref against its shared reference"""
    exp, cut, stats = R.expected(name, conn)
    w, c, s = _run(engine, *R.case(name), conn, algo, ctx)
    bad = w != exp.reshape(-1)
    assert not bad.any(), (name, conn, algo, int(bad.sum()), np.flatnonzero(bad)[:4].tolist())
    assert np.array_equal(c, R.bool_to_words(cut)), (name, conn, algo)
    assert s == stats, (name, conn, algo, s, stats)
    return exp, cut, stats


# ---- 1: every case of the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("conn", R.CONNS)
@pytest.mark.parametrize("name", R.HAND)
def test_hand_cases(engine, name, conn, algo):
    mask = R.case(name)[0]
    exp, cut, stats = _check(engine, name, conn, algo)
    assert not exp[~mask].any()
    if name == "equal balls":
        side = R.two_balls(R.EQUAL_BALLS)[3]
        assert not (mask & (exp != side)).any() and (exp[:, :, 32][mask[:, :, 32]] == 1).all()
    elif name == "diagonal chain":
        assert stats[1] == (32 if conn == 26 else 2)
    elif name == "empty mask":
        assert stats == (0, 0, 0, 0)
    elif name in ("no markers", "markers outside"):
        assert stats[:2] == (0, 0) and stats[2] > 0 and stats[3] == 0 and not exp.any()
    elif name == "markers cover the mask":
        assert np.array_equal(exp, np.where(mask, R.case(name)[1], 0)) and stats[0] == stats[1] == int(mask.sum())
    elif name == "labels 1 and max":
        assert set(np.unique(exp).tolist()) == {0, 1, R.LABEL_MAX}
    elif name.startswith("snake"):
        assert stats[1] == int(mask.sum()) and set(np.unique(exp[mask]).tolist()) == {1, 2}
    elif name.startswith("seams"):
        assert stats[0] == len(R.SEAM_MARKERS) and stats[1] == 64 ** 3


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("conn", R.CONNS)
@pytest.mark.parametrize("name", R.RANDOMS)
def test_random_masks(engine, name, conn, algo):
    mask = R.case(name)[0]
    _, _, stats = _check(engine, name, conn, algo)
    assert 0 < stats[0] <= 12 and stats[0] < stats[1] <= int(mask.sum())
    assert " 0.7 " in name or stats[1] < int(mask.sum())             # the sparse masks have components that no marker reaches


# ---- 1b: the limits of the key, gates on block seams, the sweep cap --------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("conn", R.CONNS)
@pytest.mark.parametrize("name", R.WIDES + R.QUANTA)
def test_priorities_ranks_and_labels_at_their_limits(engine, name, conn, algo):
    """P up to 2^32 - 1, a level span of exactly 16383 with both ends in M (or a quantum of 2^31 and more), labels 1, 2, 2^20 - 2 and
    2^20 - 1 flooding at once: every field of the key full at the same time.  What each case reaches is asserted without a GPU in
    tests/test_watershed_cpu.py::test_limit_cases_reach_the_limits"""
    mask, markers, P, order, q = R.case(name)
    exp, _, stats = _check(engine, name, conn, algo)
    level = P.astype(np.int64)[mask] // q
    assert int(level.max()) - int(level.min()) == (R.MAX_SPAN - 1 if name in R.WIDES else 1)
    assert stats[0] == 12 and stats[1] > 20000 and stats[2] == len(np.unique(level))
    assert set(np.unique(exp[mask]).tolist()) - {0} == set(R.EXTREME_LABELS)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("conn", R.CONNS)
@pytest.mark.parametrize("order", R.ORDERS)
def test_adding_a_constant_to_the_field_changes_nothing(engine, order, conn, algo):
    """the case whose presence bits wrap in the middle of the bitmap against its copy moved down to first = 0, which does not wrap"""
    name = R.wide_name(1, R.SECOND_WRAP + R.MAX_SPAN - 1, 4096, order)
    mask, markers, P, _, q = R.case(name)
    exp, cut, stats = R.expected(name, conn)
    w, c, s = _run(engine, mask, markers, P - np.uint32(R.SECOND_WRAP), order, q, conn, algo)
    assert np.array_equal(w, exp.reshape(-1)) and np.array_equal(c, R.bool_to_words(cut)) and s == stats


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("conn", R.CONNS)
@pytest.mark.parametrize("name", R.GATE_CASES)
def test_gates_on_block_seams(engine, name, conn, algo):
    """a full block B whose own level ran before any source touched it, next to a block A (and C) flooded at a level that no voxel of B
    has: B is on no first list of ws_first, TILED reaches it only through the flags that A's changed seam voxels raise.  With two fronts
    the reference decides where B is split, so the arrival times behind the seam count, not only that the flood came through"""
    mask, markers, P, order, q = R.case(name)
    exp, _, stats = _check(engine, name, conn, algo)
    if name.startswith("two fronts"):
        b = R.TWO_FRONTS[name.split()[2]][1]
        labels, counts = np.unique(exp[R.block_box(b)], return_counts=True)
        assert labels.tolist() == [4, 9] and counts.min() > 2000 and stats[:3] == (2, 24576, 2) and stats[3] > 0
        return
    b = R.GATES[" ".join(name.split()[1:-1])]
    lo, hi = np.unique(P[R.block_box(b)]), np.unique(P[R.block_box(R.GATE_A)])
    assert len(lo) == len(hi) == 1 and (lo[0] < hi[0] if order == R.ASCENDING else lo[0] > hi[0])   # [lo, hi] of B never meets A's level
    if sum(abs(u - v) for u, v in zip(R.GATE_A, b)) == 1 or conn == 26:
        assert stats == (1, 16384, 2, 0) and (exp[R.block_box(b)] == 9).all()
    else:
        assert stats == (1, 8192, 2, 0) and not exp[R.block_box(b)].any()   # no face step leads across an edge or a corner


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("conn", R.CONNS)
@pytest.mark.parametrize("name", R.COMBS)
def test_comb_inside_one_block_exceeds_the_sweep_cap(engine, name, conn, algo):
    """270 face steps inside one block, 240 of them across x rows -- one sweep each: ws_relax stops at kWsSweeps and the block re-lists
    itself several times per level; in the flood, three levels end while it does"""
    mask, start, sweeps, cap = comb_past_the_sweep_cap()            # fails with the advice to build a longer maze once the cap has caught up
    assert np.array_equal(mask, R.case(name)[0]) and _block_count(mask) == 1
    exp, _, stats = _check(engine, name, conn, algo)
    assert stats == (1, 271, 3 if name == "comb flood" else 1, 0) and (exp[mask] == 7).all()
    if algo == ALGO_TILED and conn == 6 and name == "comb zones":   # a sweep carries a key one x row on: the block ran ceil(240 / cap) times at least
        ctx = engine.ctx
        ctx.prof_reset()
        ctx.prof_enable(True)
        try:
            _run(engine, *R.case(name), conn, algo)
        finally:
            ctx.prof_enable(False)
        assert ctx.prof()["md_brick"]["launches"] >= -(-sweeps // cap) > 2


def _block_count(mask):
    idx = np.argwhere(mask)
    return len(set(map(tuple, np.stack([idx[:, 2] // 32, idx[:, 1] // 16, idx[:, 0] // 16], axis=1).tolist())))


# ---- 2: what a context keeps ------------------------------------------------------------------------------------------------------------------
def test_context_history_and_release(engine):
    runs = (("seams flood", 26, ALGO_TILED), ("snake flood", 6, ALGO_NAIVE), ("not a power of two", 6, ALGO_TILED),
            ("interface along a seam", 26, ALGO_TILED), (R.wide_name(3, R.TOP, 256, R.DESCENDING), 26, ALGO_TILED), ("unequal balls", 6, ALGO_NAIVE),
            ("empty mask", 6, ALGO_TILED), (R.wide_name(1 << 18, R.TOP, 4096, R.ASCENDING), 6, ALGO_NAIVE), ("gate edge xy asc", 26, ALGO_TILED))
    ctx = capi.Context(0)
    try:
        assert ctx.watershed_result() == (0, 0, (0, 0, 0, 0), 0)
        for name, conn, algo in runs:                               # n = 64, 32, 96, 32, 32, 64, 32, 32, 64 on one context: a smaller side after a larger
            _check(engine, name, conn, algo, ctx)
        ctx.release()
        assert ctx.watershed_result() == (0, 0, (0, 0, 0, 0), 0)
        _check(engine, "diagonal chain", 26, ALGO_TILED, ctx)
    finally:
        ctx.close()


# ---- 3: refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_result_untouched(engine):
    n = 32
    fr = _frame(n)
    name = "random 32 0.7 3 1 q1 asc"
    before = _run(engine, *R.case(name), 6, ALGO_TILED)
    pl, pc, rstats, side = result = engine.ctx.watershed_result()
    buf = torch.zeros(fr.voxels + 64, dtype=torch.int32, device=engine.device)
    wp = buf.data_ptr()
    slab = Frame.make(64, 1.0, np.zeros(3, np.float32), 0, 32)
    big = Frame.make(1056, 1.0, np.zeros(3, np.float32))
    lib = capi.lib()
    A, D, T, N = R.ASCENDING, R.DESCENDING, ALGO_TILED, ALGO_NAIVE

    def refused(frame, m, l, p, order, q, conn, algo, code):
        stats = (ctypes.c_uint64 * 4)(6, 7, 8, 9)
        rc = lib.vp_watershed(engine.ctx._h, ctypes.byref(frame), ctypes.c_void_p(m or None), ctypes.c_void_p(l or None), ctypes.c_void_p(p or None),
                              order, q, conn, algo, stats)
        assert rc == code, (order, q, conn, algo, rc)
        assert list(stats) == [6, 7, 8, 9]
        assert engine.ctx.watershed_result() == result
        w, c, st = _fetch(engine.ctx, n)
        assert np.array_equal(w, before[0]) and np.array_equal(c, before[1]) and st == before[2]

    for args in ((slab, wp, wp, wp, A, 1, 6, T, 10002), (big, wp, wp, wp, A, 1, 6, T, 10002),
                 (fr, 0, wp, wp, A, 1, 6, T, 10001), (fr, wp, 0, wp, A, 1, 6, N, 10001),                      # null mask / markers
                 (fr, wp + 4, wp, wp, A, 1, 6, T, 10001), (fr, wp, wp + 8, wp, D, 1, 26, N, 10001), (fr, wp, wp, wp + 4, D, 1, 26, T, 10001),
                 (fr, wp, wp, wp, 2, 1, 6, T, 10001), (fr, wp, wp, wp, -1, 1, 6, N, 10001),                      # order
                 (fr, wp, wp, wp, A, 0, 6, T, 10001),                                                             # quantum
                 (fr, wp, wp, wp, A, 1, 18, T, 10001), (fr, wp, wp, 0, A, 1, 0, N, 10001),                       # connectivity
                 (fr, wp, wp, wp, A, 1, 6, 0, 10001), (fr, wp, wp, 0, A, 1, 26, 3, 10001),                       # algo
                 (fr, pc, wp, wp, A, 1, 6, T, 10001), (fr, wp, pl, wp, A, 1, 6, N, 10001), (fr, wp, wp, pl, D, 1, 6, T, 10001),
                 (fr, wp, pl, 0, A, 1, 26, T, 10001)):                                                            # the last result as an input
        refused(*args)
    assert lib.vp_watershed(None, ctypes.byref(fr), ctypes.c_void_p(wp), ctypes.c_void_p(wp), None, A, 1, 6, T, None) == 10001
    assert lib.vp_watershed(engine.ctx._h, None, ctypes.c_void_p(wp), ctypes.c_void_p(wp), None, A, 1, 6, T, None) == 10001

    # what only the data show: the pre-pass finds it before a result buffer is written
    full = _dev(engine, np.full(fr.words, 0xFFFFFFFF, np.uint32))
    L = np.zeros(n ** 3, np.uint32)
    L[5], L[77] = 1, R.LABEL_MAX + 1
    P = np.zeros(n ** 3, np.uint32)
    P[9], P[100] = 1000, 1000 + R.MAX_SPAN
    ok_markers, bad_markers = _dev(engine, np.where(L > R.LABEL_MAX, R.LABEL_MAX, L)), _dev(engine, L)
    wide, wide3 = _dev(engine, P), _dev(engine, P * 3)
    for algo in ALGOS:
        refused(fr, full.data_ptr(), bad_markers.data_ptr(), 0, A, 1, 6, algo, 10001)                           # label 2^20
        assert "VP_WS_LABEL_MAX" in _last_error()
        refused(fr, full.data_ptr(), ok_markers.data_ptr(), wide.data_ptr(), A, 1, 6, algo, 10001)               # span 16384
        assert "quantum that fits is 2" in _last_error()
        refused(fr, full.data_ptr(), ok_markers.data_ptr(), wide3.data_ptr(), D, 3, 6, algo, 10001)
        assert "quantum that fits is 4" in _last_error()
    # the whole range of uint32 in M, and more (lowest P, highest P, quantum): the quantum named is the one the reference finds
    everything = np.ones(n ** 3, bool)
    assert R.fitting_quantum(np.array([0, R.TOP], np.uint32), np.ones(2, bool), 1) == 262144
    for k, (lo, hi, q) in enumerate(((0, R.TOP, 1), (0, R.TOP, 262143), (1000, 1000 + 5 * R.MAX_SPAN + 3, 2), (7, 0xFFFFFFF0, 1000),
                                     (1 << 31, R.TOP, 1), (R.TOP - 3 * R.MAX_SPAN, R.TOP, 2), (16383, 2 * 16384, 1), (3, R.TOP - 1, 262143))):
        Q = np.full(n ** 3, lo, np.uint32)
        Q[(7 * k + 3) % 50::50] = hi
        fits = R.fitting_quantum(Q, everything, q)
        assert fits > q and (hi // fits - lo // fits) < R.MAX_SPAN <= (hi // (fits - 1) - lo // (fits - 1))
        field = _dev(engine, Q)
        for algo, order in ((T, A), (N, D)):
            refused(fr, full.data_ptr(), ok_markers.data_ptr(), field.data_ptr(), order, q, 26 if k % 2 else 6, algo, 10001)
            found = re.search(r"the levels span (\d+), VP_WS_MAX_SPAN = 16384: the smallest quantum that fits is (\d+)$", _last_error())
            assert found and int(found.group(2)) == fits and int(found.group(1)) == hi // q - lo // q + 1, (lo, hi, q, fits, _last_error())
    # ... outside the mask neither counts
    hole = np.full(fr.words, 0xFFFFFFFF, np.uint32)
    hole[77 // 32] &= ~np.uint32(1 << (77 % 32))
    hole[100 // 32] &= ~np.uint32(1 << (100 % 32))
    P[9] = 0
    holed, outside = _dev(engine, hole), _dev(engine, P)
    s = engine.ctx.watershed(fr, holed.data_ptr(), bad_markers.data_ptr(), outside.data_ptr(), A, 1, 6, ALGO_TILED)
    assert s == (1, n ** 3 - 2, 1, 0)
    # the bounds themselves are served: label 2^20 - 1, span 16383
    P[100] = R.MAX_SPAN - 1
    widest = _dev(engine, P)
    served = np.where(L > R.LABEL_MAX, R.LABEL_MAX, L).reshape(n, n, n), P.reshape(n, n, n)
    for order, conn in ((D, 6), (A, 26)):
        W, cut, stats = R.watershed(np.ones((n,) * 3, bool), served[0], served[1], order, 1, conn)
        assert stats[:3] == (2, n ** 3, 2) and set(np.unique(W).tolist()) == {1, R.LABEL_MAX}
        for algo in ALGOS:
            s = engine.ctx.watershed(fr, full.data_ptr(), ok_markers.data_ptr(), widest.data_ptr(), order, 1, conn, algo)
            w, c, rs = _fetch(engine.ctx, n)
            assert np.array_equal(w, W.reshape(-1)) and np.array_equal(c, R.bool_to_words(cut)) and s == rs == stats, (order, conn, algo, s, stats)
    h = np.zeros(fr.words, np.uint32)
    hv = np.zeros(fr.voxels, np.uint32)
    for frame, order, q, conn, algo, code in ((slab, A, 1, 6, T, 10002), (fr, 5, 1, 6, T, 10001), (fr, A, 0, 6, T, 10001), (fr, A, 1, 7, T, 10001),
                                              (fr, A, 1, 6, 9, 10001)):
        with pytest.raises(capi.VPError) as e:
            engine.ctx.watershed_host(frame, h, hv, hv, order, q, conn, algo)
        assert e.value.code == code
    with pytest.raises(capi.VPError) as e:
        engine.ctx.watershed_host(fr, h, hv, None, A, 1, 6, T, want=(False, False, False))
    assert e.value.code == 10001
    # without a priority field order and quantum are not looked at
    assert engine.ctx.watershed(fr, full.data_ptr(), ok_markers.data_ptr(), 0, 9, 0, 6, ALGO_TILED)[2] == 1


# ---- 4: timing keys -----------------------------------------------------------------------------------------------------------------------------
def test_timing_keys(engine):
    name = "unequal balls"
    mask, markers, P, order, q = R.case(name)
    m, l, p = _dev(engine, R.bool_to_words(mask)), _dev(engine, markers), _dev(engine, P)
    ctx, fr = engine.ctx, _frame(64)
    every = list(capi.EVERY_PROF_KEY)
    levels = R.expected(name, 6)[2][2]

    def keys(fn):
        ctx.prof_reset()
        ctx.prof_enable(True)
        fn()
        ctx.prof_enable(False)
        return {k: v["launches"] for k, v in ctx.prof().items()}
    tiled = keys(lambda: ctx.watershed(fr, m.data_ptr(), l.data_ptr(), p.data_ptr(), order, q, 6, ALGO_TILED))
    assert set(tiled) == {"md_fill", "md_split", "md_scan", "md_brick"}, tiled
    assert tiled["md_fill"] == 1 and tiled["md_split"] == 1 and tiled["md_brick"] >= levels
    assert tiled["md_scan"] == tiled["md_brick"] + 2 * levels       # per level the first flags, a list in front of every round and the empty one
    naive = keys(lambda: ctx.watershed(fr, m.data_ptr(), l.data_ptr(), p.data_ptr(), order, q, 6, ALGO_NAIVE))
    assert set(naive) == {"md_fill", "md_split", "md_naive"}, naive
    assert naive["md_fill"] == 1 and naive["md_split"] == 1 and naive["md_naive"] >= levels
    assert list(capi.EVERY_PROF_KEY) == every and capi.lib().vp_abi_version() == 6


def test_naive_rounds_cross_the_flag_ring_twice(engine):
    """NAIVE, conn 6, one level: the serpentine of tests/geodesic_ref.py at n = 32 as an influence-zone mask with a single marker at its
    start.  The rounds of the level fill at least three batches of eight (csrc/round_ring.h) -- both halves of the flag ring are reused"""
    import geodesic_ref as G
    mask, start = G.case("serpentine 32")
    markers = start.astype(np.uint32)
    exp, cut, stats = R.watershed(mask, markers, None, R.DESCENDING, 1, 6)
    assert stats[2] == 1 and np.array_equal(exp != 0, mask)
    ctx = engine.ctx
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        w, c, s = _run(engine, mask, markers, None, R.DESCENDING, 1, 6, ALGO_NAIVE)
    finally:
        ctx.prof_enable(False)
    assert np.array_equal(w, exp.reshape(-1)) and np.array_equal(c, R.bool_to_words(cut)) and s == stats
    launches = ctx.prof()["md_naive"]["launches"]
    assert launches >= 3 * 8 and launches % 8 == 0, launches


# ---- 5: vp_watershed_host and the engine ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", R.CONNS)
def test_host_entry_point(engine, conn):
    every = ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (True, False, False), (False, False, True))
    for name, algo, wants in (("snake flood", ALGO_TILED, every), ("interface along a seam", ALGO_NAIVE, every),
                              (R.wide_name(3, R.TOP, 4096, R.DESCENDING), ALGO_TILED, every[:1]), ("quantum %d asc" % R.TOP, ALGO_NAIVE, every[:1]),
                              ("gate corner ++ desc", ALGO_TILED, every[:1]), ("two fronts y asc", ALGO_NAIVE, every[:1])):
        mask, markers, P, order, q = R.case(name)
        exp, cut, stats = R.expected(name, conn)
        for want in wants:
            w, c, s = engine.ctx.watershed_host(_frame(mask.shape[0]), R.bool_to_words(mask), markers.reshape(-1), None if P is None else P.reshape(-1),
                                                order, q, conn, algo, want)
            assert (w is None) == (not want[0]) and (c is None) == (not want[1]) and (s is None) == (not want[2])
            assert w is None or np.array_equal(w, exp.reshape(-1))
            assert c is None or np.array_equal(c, R.bool_to_words(cut))
            assert s is None or s == stats


def test_engine_returns_views_of_the_context_buffers(engine):
    name = "unequal balls swapped"
    mask, markers, P, order, q = R.case(name)
    fr = _frame(64)
    m = _dev(engine, R.bool_to_words(mask))
    labels, cut, stats = engine.watershed(fr, m, _dev(engine, markers), _dev(engine, P), order, q, capi.CONN_26)
    pl, pc, rstats, side = engine.ctx.watershed_result()
    assert (labels.data_ptr(), cut.data_ptr(), stats, side) == (pl, pc, rstats, 64)
    exp, ecut, estats = R.expected(name, 26)
    engine.sync()
    assert np.array_equal(labels.cpu().numpy().view(np.uint32), exp.reshape(-1)) and stats == estats
    assert np.array_equal(engine.words_to_numpy(cut), R.bool_to_words(ecut))
    with pytest.raises(capi.VPError) as e:                          # what comes back cannot go in again without a copy
        engine.ctx.watershed(fr, cut.data_ptr(), labels.data_ptr())
    assert e.value.code == 10001
    # the labels as markers of their own mask: nothing is left to flood, and the cut grid is the same again
    again = engine.watershed(fr, m, labels.clone(), None, connectivity=capi.CONN_26)
    assert again[2] == (estats[1], estats[1], 1, estats[3])
    assert np.array_equal(engine.words_to_numpy(again[1]), R.bool_to_words(ecut))
    # the cut grid separates the parts: its components carry one label each
    lab = torch.zeros(fr.voxels, dtype=torch.int32, device=engine.device)
    k = engine.ctx.components_label(fr, again[1].clone().data_ptr(), lab.data_ptr(), capi.CONN_26)
    assert k == 2


# ---- 6: the CLI ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_device_equals_host(tmp_path):
    cli = build.build_cli()
    _, vox, _ = cli_run(cli, tmp_path, "plain", "bunny.obj", 64, "2", [])
    W, cut, count, line = cli_expected(vox, 2, 1, 6)
    assert count == 4
    for t in ("2", "1", "0"):
        out, grid, labels = cli_run(cli, tmp_path, "t" + t, "bunny.obj", 64, t, ["--watershed", "2"])
        assert [ln for ln in out.splitlines() if ln.startswith("watershed:")] == [line], t
        assert np.array_equal(labels, W.reshape(-1)) and np.array_equal(grid, cut), t
        assert "Watershed]: " in out
