"""The whole-row form of the fused JFA start (jfa_first_two.hip: jfa_first_two_rows; powers of two from 128 to 1024, 4-byte ids).

Every case compares ctx.jfa_window_first_two -- passes k = n/2 and k = n/4 in one launch from the border mask -- id for id over ALL voxels
with jfa_init + jfa_pass(n/2) + jfa_pass(n/4) of the one-thread-per-voxel kernel (ALGO_NAIVE: the reference's scan order, strict '<'), as
test_gpu_parity.py::test_jfa_every_pass_ids_tiled_equals_naive does.  n = 128 and 256: one and two border words per x segment.

The kernel answers a lattice (the 64 voxels of one residue class x, y, z mod n/4) of no border voxel with "none", of one with that voxel,
and evaluates only the lattices of two or more; the cases place border voxels so that every class, the tie order inside a contested
lattice and the rounds of a tile with more contested lattices than its patch buffer holds are all met."""
import numpy as np
import pytest
import torch

import float_frames as FF
from cuda_mesh_voxelization_amd import mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame, Window

pytestmark = pytest.mark.gpu

PATCH_LATTICES = 24          # mirrors kRowsPatchLattices of jfa_first_two.hip: contested lattices a tile evaluates per round
SIZES = (128, 256)
DYADIC = (0.03125, (0.25, -1.0, 3.5))


def _points(n, pts):
    occ = np.zeros((n, n, n), bool)                                   # z, y, x
    for x, y, z in pts:
        occ[z, y, x] = True
    return FF.pack(occ)


def _random(n, density, seed):
    rng = np.random.default_rng([n, seed])
    return FF.pack(rng.random((n, n, n)) < density)


def _lattice_counts(border_words, n):
    """border voxels per lattice, indexed [rz, ry, rx]"""
    k = n // 4
    return FF.unpack(border_words, n).reshape(4, k, 4, k, 4, k).sum(axis=(0, 2, 4))


def _check(engine, n, words, frame=DYADIC, tag=""):
    """first two passes from the mask == the naive sequence, every voxel; returns the border words (numpy)"""
    vs, origin = frame
    fr = Frame.make(n, vs, origin)
    ctx = engine.ctx
    assert ctx.jfa_id_bytes(fr) == 4 and ctx.jfa_can_fuse_first_two(fr, ALGO_TILED)
    g = engine.to_device(words, np.uint32)
    border = torch.empty(fr.words, dtype=torch.int32, device=engine.device)
    ctx.surface(fr, g.data_ptr(), None, None, border.data_ptr())
    a = torch.empty(fr.voxels, dtype=torch.int32, device=engine.device)
    b = torch.empty_like(a)
    ctx.jfa_init(fr, g.data_ptr(), None, None, a.data_ptr())
    ctx.jfa_pass(fr, n // 2, a.data_ptr(), None, None, b.data_ptr(), ALGO_NAIVE)
    ctx.jfa_pass(fr, n // 4, b.data_ptr(), None, None, a.data_ptr(), ALGO_NAIVE)
    wbytes = ctx.jfa_window_bytes(fr, n)
    assert wbytes == fr.voxels * 4
    t = torch.full((wbytes,), 0xA5, dtype=torch.uint8, device=engine.device)       # no valid id: a voxel left unwritten shows
    ctx.jfa_window_first_two(fr, border.data_ptr(), Window.make(t.data_ptr(), wbytes, n, 0))
    engine.sync()
    got = t.view(torch.int32)
    bad = int((got != a).sum().item())
    assert bad == 0, (n, tag, "%d of %d ids differ" % (bad, fr.voxels))
    return engine.words_to_numpy(border)


@pytest.mark.parametrize("n", SIZES)
def test_empty_grid(engine, n):
    bw = _check(engine, n, np.zeros(n * n * n // 32, np.uint32), tag="empty")
    assert not bw.any()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("where", ["corner", "far corner", "interior"])
def test_single_voxel(engine, n, where):
    p = {"corner": (0, 0, 0), "far corner": (n - 1, n - 1, n - 1), "interior": (n // 4 + 5, n // 2 + 3, 3 * n // 4 - 2)}[where]
    bw = _check(engine, n, _points(n, [p]), tag=where)
    assert int(_lattice_counts(bw, n).sum()) == 1


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shift", [(2, 0, 0), (0, 2, 0), (0, 0, 2), (2, 2, 0), (2, 2, 2), (1, 0, 0), (3, 0, 0), (1, 1, 1), (1, 0, 3)])
def test_two_voxels_in_one_lattice_with_equidistant_planes(engine, n, shift):
    """Two seeds of one lattice, `shift` chain positions apart.  In the dyadic frame every distance is exact: with a shift of two along an
    axis the whole planes of the chain positions between them are equidistant from both (pass n/4 decides them by scan order, and a voxel
    that already holds one of the two keeps it: own state first); an odd shift makes the ties of pass n/2."""
    k = n // 4
    p = (k // 2 + 1, 3, k - 1)
    q = tuple(c + s * k for c, s in zip(p, shift))
    bw = _check(engine, n, _points(n, [p, q]), tag=shift)
    lat = _lattice_counts(bw, n)
    assert int((lat == 2).sum()) == 1 and int(lat.sum()) == 2


@pytest.mark.parametrize("n", SIZES)
def test_two_voxels_in_different_lattices_of_one_tile(engine, n):
    k = n // 4
    bw = _check(engine, n, _points(n, [(5, 7, 9), (6 + k, 7 + 2 * k, 9)]), tag="two lattices")
    lat = _lattice_counts(bw, n)
    assert int((lat[9, 7] == 1).sum()) == 2 and int(lat.sum()) == 2


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("frame", ["dyadic", "far", "collapsed"])
def test_sparse_grid_has_every_lattice_class(engine, n, frame):
    """density 0.01: none / one / more = 52 / 34 / 14 % of the lattices expected; each class at least 10 %"""
    fr = DYADIC if frame == "dyadic" else FF.check_band(frame, n)[:2]
    bw = _check(engine, n, _random(n, 0.01, 1), frame=fr, tag=frame)
    lat = _lattice_counts(bw, n)
    for share in ((lat == 0).mean(), (lat == 1).mean(), (lat >= 2).mean()):
        assert share >= 0.10, ((lat == 0).mean(), (lat == 1).mean(), (lat >= 2).mean())


@pytest.mark.parametrize("n", SIZES)
def test_medium_density_straddles_the_patch_capacity(engine, n):
    """density 0.03: about 58 % of a tile's lattices are contested, so the tiles of one grid end below, at and above the capacity"""
    bw = _check(engine, n, _random(n, 0.03, 2), tag="0.03")
    per_tile = (_lattice_counts(bw, n) >= 2).sum(axis=2)
    if n == 128:
        assert per_tile.min() < PATCH_LATTICES < per_tile.max()
    else:
        assert per_tile.max() > PATCH_LATTICES


@pytest.mark.parametrize("n", SIZES)
def test_noise_every_tile_exceeds_the_patch_buffer(engine, n):
    """density 0.5: every lattice is contested, and a tile has k = n/4 of them: more than the patch buffer holds, at both sizes"""
    assert n // 4 > PATCH_LATTICES
    bw = _check(engine, n, _random(n, 0.5, 3), tag="noise")
    assert (_lattice_counts(bw, n) >= 2).all()


@pytest.mark.parametrize("n", SIZES)
def test_full_grid(engine, n):
    """every voxel set: the border is the six faces of the grid"""
    bw = _check(engine, n, np.full(n * n * n // 32, 0xFFFFFFFF, np.uint32), tag="full")
    b = FF.unpack(bw, n)
    assert b[0].all() and b[:, 0].all() and b[:, :, 0].all() and b[-1].all() and not b[1:-1, 1:-1, 1:-1].any()


def test_bunny_256(engine):
    n = 256
    xyz, tri = M.import_mesh(M.asset("bunny.obj"))
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    g = engine.voxelize(fr, dx, dt)
    engine.sync()
    bw = _check(engine, n, engine.words_to_numpy(g), frame=(vs, origin), tag="bunny")
    assert (_lattice_counts(bw, n) >= 2).any()


def test_whole_jfa_tiled_equals_naive_256(engine):
    """vp_jfa end to end on the sparse grid: the sdf of ALGO_TILED (which starts with the fused two passes) bit for bit that of ALGO_NAIVE"""
    n = 256
    fr = Frame.make(n, *DYADIC)
    g = engine.to_device(_random(n, 0.01, 1), np.uint32)
    tiled = engine.jfa(fr, g, algo=ALGO_TILED).clone()
    naive = engine.jfa(fr, g, algo=ALGO_NAIVE)
    engine.sync()
    assert torch.equal(tiled.view(torch.int32), naive.view(torch.int32))
