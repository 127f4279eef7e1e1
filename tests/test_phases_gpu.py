"""Seam phases at side 64: the named seam cases of the regions, geodesic and watershed tests sit at hand-picked positions; here one small
piece per feature (tests/embed.py: phase_piece -- two labels in contact, two boxes that touch at a corner, two overlapping balls with a
priority field; side 24, its voxels inside one 12-voxel box) is moved to eight placements, so that it crosses the x word seam alone, a y
seam alone, z seams alone, two edges, a block corner (for the geodesic piece the corner contact lies ON the block corner) and ends on the
last voxel of the grid on every axis (tests/test_embed_cpu.py checks that each placement crosses what it names).  The expected result
is the plain reference run on the embedded volume itself; NAIVE and TILED, every metric and connectivity, byte for byte."""
import functools
import os
import sys

import numpy as np
import pytest

from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed as E  # noqa: E402
import geodesic_ref as G  # noqa: E402
import regions_ref as R  # noqa: E402
import test_geodesic_gpu as TG  # noqa: E402
import test_regions_gpu as TR  # noqa: E402
import test_watershed_gpu as TW  # noqa: E402
import watershed_ref as WS  # noqa: E402

pytestmark = pytest.mark.gpu
ALGOS = (ALGO_NAIVE, ALGO_TILED)
PLACES = tuple(E.PHASE_OFFSETS)
N = E.PHASE_GRID


@functools.lru_cache(maxsize=None)
def _placed(feature, place):
    """the arrays of the feature's piece at a placement (other settings pass through), read-only"""
    out = tuple(E.embed(a, N, E.PHASE_OFFSETS[place]) if isinstance(a, np.ndarray) else a for a in E.phase_piece(feature))
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _expected(feature, place, mode):
    """the reference on the embedded volume, computed once per placement and metric / connectivity"""
    if feature == "regions":
        W, K, values = _placed(feature, place)
        return R.regions(W, K, values if mode else None)
    if feature == "geodesic":
        return G.geodesic(*_placed(feature, place), mode)
    return WS.watershed(*_placed(feature, place), mode)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("with_values", (False, True))
@pytest.mark.parametrize("place", PLACES)
def test_regions(engine, place, with_values, algo):
    W, K, values = _placed("regions", place)
    T, stats = _expected("regions", place, with_values)
    t, s = TR._run(engine, W, K, values if with_values else None, algo)
    bad = np.argwhere(t != T)
    assert len(bad) == 0, (place, algo, [(int(a), int(b), int(t[a, b]), int(T[a, b])) for a, b in bad[:6]])
    assert s == stats and stats[1] == 2 and stats[3] > 0


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("metric", G.METRICS)
@pytest.mark.parametrize("place", PLACES)
def test_geodesic(engine, place, metric, algo):
    mask, seeds = _placed("geodesic", place)
    exp, reach, stats = _expected("geodesic", place, metric)
    d, r, s = TG._run(engine, mask, seeds, metric, algo)
    bad = d != exp.reshape(-1)
    assert not bad.any(), (place, metric, algo, int(bad.sum()), np.flatnonzero(bad)[:4].tolist())
    assert np.array_equal(r, G.bool_to_words(reach)) and s == stats
    assert stats[1] == (216 if metric == G.GEO_6 else 432)          # no face step crosses the corner


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("conn", WS.CONNS)
@pytest.mark.parametrize("place", PLACES)
def test_watershed(engine, place, conn, algo):
    mask, markers, P, order, q = _placed("watershed", place)
    exp, cut, stats = _expected("watershed", place, conn)
    w, c, s = TW._run(engine, mask, markers, P, order, q, conn, algo)
    bad = w != exp.reshape(-1)
    assert not bad.any(), (place, conn, algo, int(bad.sum()), np.flatnonzero(bad)[:4].tolist())
    assert np.array_equal(c, WS.bool_to_words(cut)) and s == stats
    assert stats[:2] == (2, int(mask.sum())) and stats[2] > 1 and 0 < stats[3] < stats[1]
