"""The translation rules of tests/embed.py against the plain references, without a GPU: a case of regions_ref, geodesic_ref and
watershed_ref embedded at an offset in a larger grid gives, by the reference run on the embedded volume itself, exactly the moved small
result -- table, statistics, distances, labels and cut grids.  Also the device form of embed() (run on the CPU device of torch) against
the numpy form, the closed form of a whole block, the placements of tests/test_phases_gpu.py, and capi.region_table under a translation
to the far corner of a grid of side 1024.  tests/test_largest_side_gpu.py rests on these rules where no reference can run."""
import os
import sys

import numpy as np
import pytest

from cuda_mesh_voxelization_amd import capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed as E  # noqa: E402
import geodesic_ref as G  # noqa: E402
import regions_ref as R  # noqa: E402
import watershed_ref as WS  # noqa: E402
from fill_ref import bool_to_words  # noqa: E402

OFFSETS = ((32, 32, 32), (13, 7, 21))                              # block-aligned; across word and block seams on every axis


# ---- regions -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("name", ("seams", "faces", "random5", "blobs", "halves"))
def test_regions_table_moves_with_the_volume(name, offset):
    W, K = R.case(name)
    m = W.shape[0]
    n = m + 32
    T, stats = R.expected(name, True)
    got, gstats = R.regions(E.embed(W, n, offset), K, E.embed(R.values_of(name), n, offset))
    exp = E.shift_regions(T, offset, m, n)
    assert np.array_equal(got, exp), (name, offset, np.argwhere(got != exp)[:6].tolist())
    assert gstats == stats
    assert (exp[:, 0] == T[:, 0]).all() and np.array_equal(exp[:, 16:25], T[:, 16:25]) and not exp[T[:, 0] == 0].any()


def test_a_whole_block_by_closed_form():
    """the block at (32, 16, 32) of a grid of side 64 -- every term of the closed form against the reference -- and the largest shifted
    word of the far-corner block at side 1024, which is what the 64-bit arithmetic of the kernel is for"""
    W = np.zeros((64, 64, 64), np.uint32)
    W[32:48, 16:32, 32:64] = 1
    values = np.full(W.shape, 0xFFFFFFFF, np.uint32)
    T, stats = R.regions(W, 1, values)
    exp, estats = E.full_block_table(32, 16, 32, 64, 0xFFFFFFFF)
    assert np.array_equal(T, exp) and stats == estats
    assert np.array_equal(R.regions(W, 1)[0], E.full_block_table(32, 16, 32, 64)[0])
    far, _ = E.full_block_table(992, 1008, 1008, 1024, 0xFFFFFFFF)
    assert int(far[0, 10]) > 8192 * 992 * 992 > 1 << 32 and int(far[0, 13]) > 1 << 32 and int(far[0, 25]) == 1024 ** 3 - 1 - 15 * 1024 * 1025 - 31
    assert np.array_equal(far, E.shift_regions(E.full_block_table(0, 0, 0, 32, 0xFFFFFFFF)[0], (992, 1008, 1008), 32, 1024))


def test_whole128_needs_64_bits():
    T, stats = R.expected("whole128", True)
    assert int(T[0, 10]) == 11319377920 > 1 << 32 and int(T[0, 13]) == 8456241152 > 1 << 32
    assert int(T[0, 22]) == 128 ** 3 * 0xFFFFFFFF and stats == (128 ** 3, 1, 0, 0)
    assert np.array_equal(T[0, 10:16], np.array([11319377920] * 3 + [8456241152] * 3, np.uint64))


# ---- geodesic ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("metric", G.METRICS)
@pytest.mark.parametrize("name", ("contact corner", "torus two seeds"))
def test_geodesic_moves_with_the_mask(name, metric, offset):
    mask, seeds = G.case(name)
    m = mask.shape[0]
    n = m + 32
    dist, reach, stats = G.expected(name, metric)
    d, r, s = G.geodesic(E.embed(mask, n, offset), E.embed(seeds, n, offset), metric)
    assert np.array_equal(d, E.embed(dist, n, offset, fill=G.NONE)) and np.array_equal(r, E.embed(reach, n, offset))
    assert s == E.shift_geodesic_stats(stats, offset, m, n) and s[:3] == stats[:3]
    assert d.reshape(-1)[s[3]] == stats[2]


def test_geodesic_statistics_of_nothing_reached_stay_zero():
    assert E.shift_geodesic_stats((0, 0, 0, 0), (5, 6, 7), 32, 64) == (0, 0, 0, 0)
    assert E.relinearise(1 + 32 * (2 + 32 * 3), (5, 6, 7), 32, 64) == 6 + 64 * (8 + 64 * 10)


# ---- watershed -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("conn", WS.CONNS)
@pytest.mark.parametrize("name", ("interface along a seam", "labels 1 and max"))
def test_watershed_moves_with_the_mask(name, conn, offset):
    """zones on a mask that fills its own grid (its faces meet label 0 after the move, as cut_of treats the outside) and a flood with a
    priority field"""
    mask, markers, P, order, q = WS.case(name)
    m = mask.shape[0]
    n = m + 32
    W, cut, stats = WS.expected(name, conn)
    w, c, s = WS.watershed(E.embed(mask, n, offset), E.embed(markers, n, offset), None if P is None else E.embed(P, n, offset), order, q, conn)
    assert np.array_equal(w, E.embed(W, n, offset)) and np.array_equal(c, E.embed(cut, n, offset)) and s == stats


# ---- embed() on a device ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", ((32, 16, 16), (13, 7, 21), (40, 40, 40), (31, 0, 5)))
def test_device_form_equals_the_numpy_form(offset):
    rng = np.random.default_rng(3)
    vol = rng.integers(0, 1 << 32, (24, 24, 24), dtype=np.uint64).astype(np.uint32)
    bits = rng.random((24, 24, 24)) < 0.4
    n = 64
    t = E.embed(vol, n, offset, "cpu")
    assert t.shape == (n ** 3,) and np.array_equal(t.numpy().view(np.uint32), E.embed(vol, n, offset).reshape(-1))
    assert np.array_equal(E.box(t, n, 24, offset), vol)
    t = E.embed(vol, n, offset, "cpu", fill=0xFFFFFFFF)
    assert np.array_equal(t.numpy().view(np.uint32), E.embed(vol, n, offset, fill=0xFFFFFFFF).reshape(-1))
    w = E.embed(bits, n, offset, "cpu")
    assert w.shape == (n ** 3 // 32,) and np.array_equal(w.numpy().view(np.uint32), bool_to_words(E.embed(bits, n, offset)))
    assert np.array_equal(E.box_bits(w, n, 24, offset), bits)
    assert E.nonzero_words(bits, offset) == int(np.count_nonzero(w.numpy()))


# ---- the placements of test_phases_gpu.py ----------------------------------------------------------------------------------------------
def test_phase_placements_cross_what_they_name():
    for feature in ("regions", "geodesic", "watershed"):
        piece = E.phase_piece(feature)[0]
        at = np.argwhere(piece != 0)
        assert piece.shape == (E.PHASE_SIDE,) * 3 and at.min(0).tolist() == [E.PHASE_LO] * 3 and at.max(0).tolist() == [E.PHASE_HI] * 3, feature
    assert len(E.PHASE_OFFSETS) == 8 and set(E.PHASE_OFFSETS) == set(E.PHASE_CROSSINGS)
    for name, offset in E.PHASE_OFFSETS.items():
        assert E.phase_crossings(offset) == E.PHASE_CROSSINGS[name], name
        assert all(0 <= o and o + E.PHASE_SIDE <= E.PHASE_GRID for o in offset)
    crossed = list(E.PHASE_CROSSINGS.values())
    assert ((31,), (), ()) in crossed                                                              # the x word seam alone
    assert {c[1:] for c in crossed if c[0] == ()} >= {((15,), ()), ((), (31,)), ((), (47,))}      # a y seam alone, z seams alone
    assert any(sum(bool(a) for a in c) == 2 for c in crossed) and any(all(c) for c in crossed)    # an edge, a block corner
    assert [o + E.PHASE_HI for o in E.PHASE_OFFSETS["last voxels"]] == [E.PHASE_GRID - 1] * 3
    W, K, _ = E.phase_piece("regions")
    T, stats = R.regions(W, K)
    assert stats[3] > 0 and T[0, 19] == T[1, 19] == stats[3]                                       # two labels in contact
    mask, seeds = E.phase_piece("geodesic")
    assert [G.geodesic(mask, seeds, metric)[2][1] for metric in G.METRICS] == [216, 432, 432]      # only a diagonal step crosses the corner


# ---- capi.region_table under a translation ---------------------------------------------------------------------------------------------
def test_region_table_at_the_far_corner_of_1024():
    """the raw table of "blobs" moved to (960, 960, 960) in a grid of side 1024: the shape quantities are those at the origin, the
    positions move by the offset times the voxel size"""
    vs, origin, o = 0.37, (-3.0, 5.5, 100.25), (960, 960, 960)
    T, _ = R.expected("blobs", True)
    near = capi.region_table(T, capi.Frame.make(64, vs, origin))
    far = capi.region_table(E.shift_regions(T, o, 64, 1024), capi.Frame.make(1024, vs, origin))
    for field in ("label", "voxels", "volume", "surface", "contact_area", "sphericity", "euler", "value_mean", "value_min", "value_max"):
        assert np.array_equal(far[field], near[field]), field
    # region_table re-centres the second moments about the middle of the box in exact int64 arithmetic; the middle moves by the offset, so
    # the integers that reach float64 are the same at both placements.  Measured: the largest relative difference of a covariance entry
    # is 0.0 (every entry is bit-identical), so ten times that figure asks for equality -- also of what is derived from the covariance
    assert np.array_equal(far["covariance"], near["covariance"])
    assert np.array_equal(far["eigenvalues"], near["eigenvalues"]) and np.array_equal(far["radii"], near["radii"])
    shift = np.array(o, np.float64) * np.float64(np.float32(vs))
    for field in ("centroid", "box_min", "box_max"):                # a division, a product and two sums, each rounded once, at both placements
        assert np.allclose(far[field], near[field] + shift, rtol=16 * np.finfo(np.float64).eps, atol=0), field
    assert np.array_equal(far["first"], near["first"] + np.array(o))
