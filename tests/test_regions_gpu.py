"""Region analysis on the GPU (vp_regions*, csrc/regions.hip) against the numpy restatement of tests/regions_ref.py, table and statistics
byte for byte, NAIVE and TILED, with and without a value field: the hand cases, a label over every kind of block seam and a block corner,
voxels on all six grid faces, random labels (K = 5 with ignored labels; K = 4000 where the label slots of a block overflow), values over the
full uint32 range, one label over the whole 96^3 and 128^3 grids with every value 0xFFFFFFFF (at 128 sum x^2 and sum xy pass 2^32), count = 0,
every label above K, an empty volume; agreement with vp_components_*, vp_skeleton and vp_watershed; what a context keeps between calls,
refusals, timing keys, vp_regions_host, Engine.regions and `vpcli --regions`.  Sides 32, 64, 96 and 128; side 1024 is in
tests/test_largest_side_gpu.py, every kind of seam at every phase in tests/test_phases_gpu.py.

The issue asks, for W of the watershed's "equal balls" case, for equal V and equal contact of both labels.  The contact counts are equal; the
volumes cannot be: vp_watershed gives the voxels ON the symmetry plane x = 32 to label 1 (tests/test_watershed_gpu.py pins that), so
V(1) = V(2) + 293, the 293 voxels of that plane, which are also the 293 contact faces.  The test asserts exactly that."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from cuda_mesh_voxelization_amd import build, capi
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_ref as R  # noqa: E402
import skeleton_ref  # noqa: E402
import watershed_ref  # noqa: E402
from fill_ref import bool_to_words  # noqa: E402
from test_regions_cpu import cli_check, cli_run  # noqa: E402

pytestmark = pytest.mark.gpu
ALGOS = (ALGO_NAIVE, ALGO_TILED)


def _frame(n):
    return Frame.make(n, 1.0, np.zeros(3, np.float32))


def _dev(engine, a):
    return torch.from_numpy(np.array(a).reshape(-1).view(np.int32)).to(engine.device)


def _fetch(ctx, n, count):
    """(table, stats) of the context's last result, numpy"""
    pt, k, stats, side = ctx.regions_result()
    assert k == count and side == n and bool(pt) == (count != 0)
    t = np.empty((count, 26), np.uint64)
    if count:
        ctx.download(t, pt)
    return t, stats


def _run(engine, W, K, values, algo, ctx=None):
    """(table, stats) of one device call"""
    ctx = ctx or engine.ctx
    n = W.shape[0]
    w = _dev(engine, W)
    v = None if values is None else _dev(engine, values)
    stats = ctx.regions(_frame(n), w.data_ptr(), K, 0 if v is None else v.data_ptr(), algo)
    t, rstats = _fetch(ctx, n, K)
    assert rstats == stats
    return t, stats


def _check(engine, name, with_values, algo, ctx=None):
    """a named case of regions_ref against its shared reference"""
    T, stats = R.expected(name, with_values)
    W, K = R.case(name)
    t, s = _run(engine, W, K, R.values_of(name) if with_values else None, algo, ctx)
    bad = np.argwhere(t != T)
    assert len(bad) == 0, (name, with_values, algo, len(bad), [(int(a), int(b), int(t[a, b]), int(T[a, b])) for a, b in bad[:6]])
    assert s == stats, (name, with_values, algo, s, stats)
    return T, stats


# ---- 1: every case of the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("with_values", (False, True))
@pytest.mark.parametrize("name", R.CASES)
def test_cases(engine, name, with_values, algo):
    T, stats = _check(engine, name, with_values, algo)
    if name in ("voxel", "corner_voxel", "far_corner_voxel"):
        assert [int(t) for t in T[0, 16:22]] == [2, 2, 2, 0, 8, 12] and int(R.euler(T)[0]) == 1
    elif name in ("ball", "shell", "torus"):
        assert int(R.euler(T)[0]) == {"ball": 1, "shell": 2, "torus": 0}[name]
    elif name == "halves":
        assert T[0, 19] == T[1, 19] == stats[3] and list(R.euler(T)) == [1, 1]
    elif name == "seams":
        assert [int(t) for t in T[0, 1:7]] == [3, 3, 5, 40, 19, 19] and stats[3] > 0
    elif name.startswith("faces"):
        n = R.case(name)[0].shape[0]
        assert [int(t) for t in T[0, 1:7]] == [0, 0, 0, n - 1, n - 1, n - 1] and int(T[2, 0]) == 2
    elif name == "random5":
        assert stats[2] > 0 and stats[1] == 5
    elif name == "random4000":
        assert stats[1] > 3900                                      # thousands of labels in every block: the 16 slots cannot hold them
    elif name == "whole96":
        assert stats == (96 ** 3, 1, 0, 0) and (not with_values or int(T[0, 22]) == 96 ** 3 * 0xFFFFFFFF)
    elif name == "whole128":                                        # the smallest side whose sums pass 2^32: every block's share must carry
        assert stats == (128 ** 3, 1, 0, 0) and [int(t) for t in T[0, 10:16]] == [11319377920] * 3 + [8456241152] * 3
    elif name == "above":
        assert stats == (0, 0, 32 ** 3, 0) and not T.any()
    elif name == "empty":
        assert stats == (0, 0, 0, 0) and not T.any()
    elif name == "count0":
        assert T.shape == (0, 26) and stats[:2] == (0, 0) and stats[2] > 0


# ---- 2: agreement with the rest of the library ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_components_sizes_first_voxels_and_euler_under_thinning(engine, algo):
    ctx, fr = engine.ctx, _frame(64)
    rng = np.random.default_rng(5)
    vox = R.torus(64, (20, 20, 20), 10.0, 3.5) | R.shell(64, (44, 44, 40), 100, 36) | R.ball(64, (44, 14, 16), 40) | (rng.random((64, 64, 64)) < 0.01)
    words = _dev(engine, bool_to_words(vox))
    labels = torch.zeros(fr.voxels, dtype=torch.int32, device=engine.device)
    K = ctx.components_label(fr, words.data_ptr(), labels.data_ptr(), capi.CONN_26)
    sizes = torch.zeros(K, dtype=torch.int32, device=engine.device)
    ctx.components_sizes(fr, labels.data_ptr(), K, sizes.data_ptr())
    ctx.regions(fr, labels.data_ptr(), K, 0, algo)
    t, stats = _fetch(ctx, 64, K)
    assert np.array_equal(t[:, 0], sizes.cpu().numpy().view(np.uint32).astype(np.uint64))
    assert K > 3 and (np.diff(t[:, 25].astype(np.int64)) > 0).all()          # components are numbered by their lowest voxel
    assert stats == (int(vox.sum()), K, 0, 0)
    chi = int(R.euler(t).sum())
    assert chi == skeleton_ref.euler(vox)
    # the homotopy kernel keeps the topology: the same sum over the components of the thinned grid
    ctx.skeleton(fr, words.data_ptr(), capi.SKEL_KERNEL)
    ps, left, side = ctx.skeleton_result()
    assert ps and side == 64
    K2 = ctx.components_label(fr, ps, labels.data_ptr(), capi.CONN_26)
    ctx.regions(fr, labels.data_ptr(), K2, 0, algo)
    t2, stats2 = _fetch(ctx, 64, K2)
    assert K2 == K and int(R.euler(t2).sum()) == chi and stats2[0] == left[0] < stats[0]


@pytest.mark.parametrize("algo", ALGOS)
def test_watershed_equal_balls(engine, algo):
    """see the module docstring: equal contact, and V(1) - V(2) = the voxels of the symmetry plane, which label 1 gets"""
    mask, markers, P, order, q = watershed_ref.case("equal balls")
    fr = _frame(64)
    labels, _, _ = engine.watershed(fr, _dev(engine, bool_to_words(mask)), _dev(engine, markers), _dev(engine, P), order, q, capi.CONN_6)
    table, stats = engine.regions(fr, labels, 2, None, algo)
    engine.sync()
    t = table.cpu().numpy().view(np.uint64)
    plane = int(mask[:, :, 32].sum())
    assert t[0, 19] == t[1, 19] == stats[3] == plane and int(t[0, 0]) - int(t[1, 0]) == plane
    assert stats[:3] == (int(mask.sum()), 2, 0) and list(R.euler(t)) == [1, 1]
    assert np.array_equal(t, R.regions(watershed_ref.expected("equal balls", 6)[0], 2)[0])


# ---- 3: what a context keeps ------------------------------------------------------------------------------------------------------------------
def test_context_history_and_release(engine):
    ctx = capi.Context(0)
    try:
        assert ctx.regions_result() == (0, 0, (0, 0, 0, 0), 0)
        _check(engine, "blobs", True, ALGO_TILED, ctx)
        first = ctx.regions_result()[0]
        _check(engine, "blobs", False, ALGO_NAIVE, ctx)
        assert ctx.regions_result()[0] == first                     # the same size again: the table stays where it is
        for name, with_values, algo in (("random4000", True, ALGO_TILED), ("blobs96", False, ALGO_TILED), ("voxel", True, ALGO_NAIVE),
                                        ("count0", False, ALGO_TILED), ("seams", True, ALGO_TILED)):
            _check(engine, name, with_values, algo, ctx)             # sides 32, 96, 32, 32, 64; K = 4000, 7, 1, 0, 2 on one context
        ctx.release()
        assert ctx.regions_result() == (0, 0, (0, 0, 0, 0), 0)
        _check(engine, "halves", True, ALGO_TILED, ctx)
    finally:
        ctx.close()


# ---- 4: refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_result_untouched(engine):
    n = 32
    fr = _frame(n)
    W, K = R.case("random5")
    before = _run(engine, W, K, R.values_of("random5"), ALGO_TILED)
    pt, k, rstats, side = result = engine.ctx.regions_result()
    buf = torch.zeros(fr.voxels + 64, dtype=torch.int32, device=engine.device)
    wp = buf.data_ptr()
    slab = Frame.make(64, 1.0, np.zeros(3, np.float32), 0, 32)
    big = Frame.make(1056, 1.0, np.zeros(3, np.float32))
    lib = capi.lib()
    T, N = ALGO_TILED, ALGO_NAIVE

    def refused(frame, l, count, v, algo, code):
        stats = (ctypes.c_uint64 * 4)(6, 7, 8, 9)
        rc = lib.vp_regions(engine.ctx._h, ctypes.byref(frame), ctypes.c_void_p(l or None), count, ctypes.c_void_p(v or None), algo, stats)
        assert rc == code, (count, algo, rc)
        assert list(stats) == [6, 7, 8, 9]
        assert engine.ctx.regions_result() == result
        t, st = _fetch(engine.ctx, n, K)
        assert np.array_equal(t, before[0]) and st == before[1]

    for args in ((slab, wp, 3, 0, T, 10002), (big, wp, 3, wp, N, 10002),
                 (fr, 0, 3, wp, T, 10001),                                                  # null labels
                 (fr, wp + 4, 3, 0, T, 10001), (fr, wp, 3, wp + 8, N, 10001),              # alignment
                 (fr, wp, R.REGIONS_MAX + 1, 0, T, 10001), (fr, wp, 0xFFFFFFFF, wp, N, 10001),
                 (fr, wp, 3, 0, 0, 10001), (fr, wp, 3, wp, 3, 10001),                      # algo
                 (fr, pt, 3, 0, T, 10001), (fr, wp, 3, pt, N, 10001)):                     # the context's table as an input
        refused(*args)
    refused(fr, wp, R.REGIONS_MAX + 1, 0, T, 10001)
    assert "minsize" in (lib.vp_last_error() or b"").decode()
    assert lib.vp_regions(None, ctypes.byref(fr), ctypes.c_void_p(wp), 3, None, T, None) == 10001
    assert lib.vp_regions(engine.ctx._h, None, ctypes.c_void_p(wp), 3, None, T, None) == 10001
    hv = np.zeros(fr.voxels, np.uint32)
    for frame, count, algo, code in ((slab, 3, T, 10002), (fr, R.REGIONS_MAX + 1, T, 10001), (fr, 3, 9, 10001)):
        with pytest.raises(capi.VPError) as e:
            engine.ctx.regions_host(frame, hv, count, None, algo)
        assert e.value.code == code
    with pytest.raises(capi.VPError) as e:
        engine.ctx.regions_host(fr, hv, 3, None, T, want=(False, False))
    assert e.value.code == 10001
    # the bound itself is served
    t, stats = engine.ctx.regions_host(fr, np.ascontiguousarray(W).reshape(-1), R.REGIONS_MAX, None, T)
    full = R.regions(W, 8)[0]
    assert t.shape == (R.REGIONS_MAX, 26) and np.array_equal(t[:8], full) and not t[8:].any() and stats[2] == 0


# ---- 5: timing keys -----------------------------------------------------------------------------------------------------------------------------
def test_timing_keys(engine):
    W, K = R.case("blobs")
    w, v = _dev(engine, W), _dev(engine, R.values_of("blobs"))
    ctx, fr = engine.ctx, _frame(64)
    every = list(capi.EVERY_PROF_KEY)

    def keys(fn):
        ctx.prof_reset()
        ctx.prof_enable(True)
        fn()
        ctx.prof_enable(False)
        return {k: v["launches"] for k, v in ctx.prof().items()}
    assert keys(lambda: ctx.regions(fr, w.data_ptr(), K, v.data_ptr(), ALGO_TILED)) == {"md_fill": 1, "md_brick": 1, "md_split": 1}
    assert keys(lambda: ctx.regions(fr, w.data_ptr(), K, 0, ALGO_NAIVE)) == {"md_fill": 1, "md_naive": 1, "md_split": 1}
    assert keys(lambda: ctx.regions(fr, w.data_ptr(), 0, 0, ALGO_TILED)) == {"md_brick": 1}     # no table: nothing to clear or to finish
    assert list(capi.EVERY_PROF_KEY) == every and capi.lib().vp_abi_version() == 6


# ---- 6: vp_regions_host and the engine -----------------------------------------------------------------------------------------------------------
def test_host_entry_point(engine):
    for name, algo, with_values in (("seams", ALGO_TILED, True), ("random5", ALGO_NAIVE, False), ("count0", ALGO_TILED, False)):
        W, K = R.case(name)
        T, stats = R.expected(name, with_values)
        for want in ((True, True), (False, True), (True, False)):
            t, s = engine.ctx.regions_host(_frame(W.shape[0]), np.ascontiguousarray(W).reshape(-1), K,
                                           R.values_of(name).reshape(-1) if with_values else None, algo, want)
            assert (t is None) == (not want[0]) and (s is None) == (not want[1])
            assert t is None or np.array_equal(t, T)
            assert s is None or s == stats


def test_engine_returns_a_view_of_the_context_table(engine):
    W, K = R.case("blobs")
    fr = _frame(64)
    labels, values = _dev(engine, W), _dev(engine, R.values_of("blobs"))
    table, stats = engine.regions(fr, labels, K, values)
    pt, k, rstats, side = engine.ctx.regions_result()
    assert (table.data_ptr(), tuple(table.shape), stats, side, k) == (pt, (K, 26), rstats, 64, K) and table.dtype == torch.int64
    T, estats = R.expected("blobs", True)
    engine.sync()
    assert np.array_equal(table.cpu().numpy().view(np.uint64), T) and stats == estats
    with pytest.raises(capi.VPError) as e:                          # what comes back cannot go in again without a copy
        engine.ctx.regions(fr, table.data_ptr(), K)
    assert e.value.code == 10001
    rt = capi.region_table(table.cpu().numpy(), fr)
    assert list(rt["voxels"]) == [int(v) for v in T[:, 0]] and list(rt["euler"]) == list(R.euler(T))
    empty, stats0 = engine.regions(fr, labels, 0)
    assert tuple(empty.shape) == (0, 26) and stats0 == (0, 0, int((W > 0).sum()), 0)


# ---- 7: the CLI ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_device_equals_host(tmp_path):
    cli = build.build_cli()
    for t, name in (("2", "tiled"), ("1", "naive")):
        out, vox, table, d = cli_run(cli, tmp_path, "t" + t, "bunny.obj", 64, t, ["--fill", "--watershed", "2", "--regions", "6", "-o", "thing.obj"])
        T, count = cli_check(out, vox, table, str(d / "out" / ("thing_%s_regions.csv" % name)), 6, 64)
        assert count >= 4 and "Regions]: " in out
