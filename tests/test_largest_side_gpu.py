"""vp_regions, vp_geodesic and vp_watershed at the largest side they document, n = 1024: 131,072 blocks (kMaxBlocksPerThread of
block_list.h filled exactly), the last block (31, 63, 63), voxel indices up to 2^30 - 1, table words that need 64 bits.  No reference runs
at 2^30 voxels; the three operations are exactly translation-equivariant, so a small case of the references is embedded ON THE DEVICE at
two offsets -- the far corner, block-aligned, and (949, 953, 957), across word and block seams away from the faces -- and the result is the
small reference moved by the rules of tests/embed.py, which tests/test_embed_cpu.py proves on the CPU.  NAIVE and TILED, every metric and
connectivity, byte for byte.

Nothing of n^3 values comes to the host: the sub-box that holds the case is compared with the reference, and torch.count_nonzero on the
whole volume and on the whole bit grid shows that nothing else was written; tables and statistics are compared whole.  Every test frees
its tensors and releases the context (a watershed holds about 20 GB)."""
import os
import sys

import numpy as np
import pytest
import torch

from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed as E  # noqa: E402
import geodesic_ref as G  # noqa: E402
import regions_ref as R  # noqa: E402
import watershed_ref as WS  # noqa: E402

pytestmark = pytest.mark.gpu
ALGOS = (ALGO_NAIVE, ALGO_TILED)
N = 1024
PLACES = ("far corner", "unaligned")


def _offset(place, m):
    return (N - m,) * 3 if place == "far corner" else (949, 953, 957)


def _frame():
    return Frame.make(N, 1.0, np.zeros(3, np.float32))


def _done(engine):
    engine.ctx.release()
    torch.cuda.empty_cache()


def _table(engine, labels, K, values, algo):
    table, stats = engine.regions(_frame(), labels, K, values, algo)
    engine.sync()
    t = table.cpu().numpy().view(np.uint64)
    del table
    return t, stats


def _same_table(t, exp, what):
    bad = np.argwhere(t != exp)
    assert t.shape == exp.shape and len(bad) == 0, (what, len(bad), [(int(a), int(b), int(t[a, b]), int(exp[a, b])) for a, b in bad[:6]])


# ---- regions -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("name", ("seams", "random4000"))
def test_regions_of_an_embedded_case(engine, name, place, algo):
    """with values; random4000 overflows the label slots of its blocks, so the runs that go to the table directly are moved too.  Both hold
    only a few voxels per block and label: the shifted words that pass 2^32 are test_regions_of_the_last_block's"""
    W, K = R.case(name)
    m = W.shape[0]
    o = _offset(place, m)
    T, stats = R.expected(name, True)
    exp = E.shift_regions(T, o, m, N)
    labels, values = E.embed(W, N, o, engine.device), E.embed(R.values_of(name), N, o, engine.device)
    try:
        assert int(torch.count_nonzero(labels)) == int(np.count_nonzero(W))
        t, s = _table(engine, labels, K, values, algo)
        _same_table(t, exp, (name, place, algo))
        assert s == stats
        if name == "random4000":                                    # it fills its own grid: at the far corner the last voxel of the large one
            assert [int(v) for v in exp[:, 4:7].max(0)] == [c + m - 1 for c in o]
    finally:
        del labels, values
        _done(engine)


@pytest.mark.parametrize("algo", ALGOS)
def test_regions_of_the_last_block(engine, algo):
    """label 1 on the whole block (31, 63, 63), every value 0xFFFFFFFF, against the closed form: V X^2 = 8192 * 992^2 is the largest term a
    slot is ever shifted by, sum x^2 = 8.3e9 and the three mixed sums pass 2^32"""
    x0, y0, z0 = N - 32, N - 16, N - 16
    exp, stats = E.full_block_table(x0, y0, z0, N, 0xFFFFFFFF)
    assert int(exp[0, 10]) > 1 << 32 and int(exp[0, 25]) + 31 + 15 * N * (N + 1) == N ** 3 - 1
    labels = torch.zeros((N, N, N), dtype=torch.int32, device=engine.device)
    labels[z0:, y0:, x0:] = 1
    values = torch.zeros((N, N, N), dtype=torch.int32, device=engine.device)
    values[z0:, y0:, x0:] = -1
    try:
        t, s = _table(engine, labels.view(-1), 1, values.view(-1), algo)
        _same_table(t, exp, ("last block", algo))
        assert s == stats
    finally:
        del labels, values
        _done(engine)


# ---- geodesic ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("metric", G.METRICS)
@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("name", ("contact corner", "torus two seeds"))
def test_geodesic_of_an_embedded_case(engine, name, place, metric, algo):
    mask, seeds = G.case(name)
    m = mask.shape[0]
    o = _offset(place, m)
    exp, reach, stats = G.expected(name, metric)
    dm, ds = E.embed(mask, N, o, engine.device), E.embed(seeds, N, o, engine.device)
    dist = rch = None
    try:
        dist, rch, s = engine.geodesic(_frame(), dm, ds, metric, algo)
        engine.sync()
        assert s == E.shift_geodesic_stats(stats, o, m, N), (s, stats)
        got = E.box(dist, N, m, o)
        bad = got != exp
        assert not bad.any(), (name, place, metric, algo, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        assert int(torch.count_nonzero(dist != -1)) == stats[1] == int(reach.sum())       # VP_GEO_NONE everywhere else
        assert np.array_equal(E.box_bits(rch, N, m, o), reach)
        assert int(torch.count_nonzero(rch)) == E.nonzero_words(reach, o)
    finally:
        del dist, rch, dm, ds
        _done(engine)


# ---- watershed -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("conn", WS.CONNS)
@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("name", ("interface along a seam", "labels 1 and max"))
def test_watershed_of_an_embedded_case(engine, name, place, conn, algo):
    """zones on a mask that fills its own small grid -- after the move its faces meet label 0, as watershed_ref.cut_of treats the outside --
    and a flood of four levels with a priority field and the largest label"""
    mask, markers, P, order, q = WS.case(name)
    m = mask.shape[0]
    o = _offset(place, m)
    exp, cut, stats = WS.expected(name, conn)
    dm, dl = E.embed(mask, N, o, engine.device), E.embed(markers, N, o, engine.device)
    dp = None if P is None else E.embed(P, N, o, engine.device)
    labels = dcut = None
    try:
        labels, dcut, s = engine.watershed(_frame(), dm, dl, dp, order, q, conn, algo)
        engine.sync()
        assert s == stats, (s, stats)
        got = E.box(labels, N, m, o)
        bad = got != exp
        assert not bad.any(), (name, place, conn, algo, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        assert int(torch.count_nonzero(labels)) == stats[1] == int(np.count_nonzero(exp))
        assert np.array_equal(E.box_bits(dcut, N, m, o), cut)
        assert int(torch.count_nonzero(dcut)) == E.nonzero_words(cut, o)
    finally:
        del labels, dcut, dm, dl, dp
        _done(engine)
