"""The float kernels in frames that round and lie far from the origin (tests/float_frames.py): the solid voxelizer and every JFA route
against the oracle, the mesh distance in all its forms against the numpy restatement -- on all voxels, bit for bit.  The other GPU tests
run these kernels in dyadic frames near the origin or in the frame of an asset that sits at the origin, where float32 is exact or nearly
so; here the voxel size is 0.037, the origins reach 6e5 (neighbouring columns share one float32 position) and the meshes are translated
until one ulp of a coordinate is up to two voxels."""
import gc
import math
import os
import sys

import numpy as np
import pytest
import torch

from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame
from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float_frames as FF  # noqa: E402
import meshdist_ref as R  # noqa: E402
from test_gpu_parity import _assert_sdf_equal, _run_with_hooks  # noqa: E402
from test_meshdist_cpu import SLIVER_BAND, SLIVER_XYZ, TRI  # noqa: E402
from test_meshdist_gpu import _check_all_forms  # noqa: E402
from test_slab_gpu import _run_slabs  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
ALGOS = (ALGO_TILED, ALGO_NAIVE)
FRAMES5 = ("near", "mid", "far", "collapsed", "far_x1000")
LEVELS4 = tuple(FF.LEVELS)
TESTS = os.path.dirname(os.path.abspath(__file__))


def _frame(n, name):
    vs, o, _ = FF.check_band(name, n)
    return Frame.make(n, vs, tuple(float(v) for v in o)), vs, o


def _cuts(n):
    return sorted({0, n} | {c for c in (8, 40, 136) if c < n})


# ---- solid voxelizer -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES5)
@pytest.mark.parametrize("n", [96, 128, 160, 256])
def test_voxelize_soup(engine, n, frame):
    """96 / 160: rows of 3 / 5 words, one word per lane in the fill; 128: the 16-byte fill.  Whole grid, the slabs cut at z = 8, 40 and
    136, and accumulate twice = empty: both algorithms against the oracle's scanline"""
    fr, vs, o = _frame(n, frame)
    xyz, tri = FF.soup(n, 1, vs, o)
    exp = O.voxelize(xyz, tri, n, vs, o)
    assert 0 < O.popcount(exp) < n ** 3
    dx, dt = engine.mesh_to_device(xyz, tri)
    pw = n * n // 32
    for algo in ALGOS:
        got = engine.words_to_numpy(engine.voxelize(fr, dx, dt, algo=algo))
        assert np.array_equal(got, exp), (n, frame, algo, int(np.count_nonzero(got != exp)))
        for z0, z1 in zip(_cuts(n)[:-1], _cuts(n)[1:]):
            part = engine.words_to_numpy(engine.voxelize(fr.slab(z0, z1), dx, dt, algo=algo))
            assert np.array_equal(part, exp[z0 * pw:z1 * pw]), (n, frame, algo, z0, z1, int(np.count_nonzero(part != exp[z0 * pw:z1 * pw])))
        g = torch.zeros(fr.words, dtype=torch.int32, device=engine.device)
        engine.voxelize(fr, dx, dt, out=g, algo=algo, accumulate=True)
        assert np.array_equal(engine.words_to_numpy(g), exp), (n, frame, algo, "accumulate once")
        engine.voxelize(fr, dx, dt, out=g, algo=algo, accumulate=True)
        assert not engine.words_to_numpy(g).any(), (n, frame, algo, "accumulate twice")


@pytest.mark.parametrize("level", LEVELS4)
@pytest.mark.parametrize("name,n", [("bunny.obj", 128), ("d20.obj", 256)])
def test_voxelize_translated_mesh(engine, name, n, level):
    """bunny at 128: the small-triangle path; d20 at 256: the record list and the tile path"""
    xyz, tri, origin, vs = FF.mesh_level(name, n, level)
    fr = Frame.make(n, vs, origin)
    exp = O.voxelize(xyz, tri, n, vs, origin)
    assert 0 < O.popcount(exp) < n ** 3
    dx, dt = engine.mesh_to_device(xyz, tri)
    for algo in ALGOS:
        got = engine.words_to_numpy(engine.voxelize(fr, dx, dt, algo=algo))
        assert np.array_equal(got, exp), (name, n, level, algo, int(np.count_nonzero(got != exp)))


def test_voxelize_translated_d20_through_the_overflow_paths(engine):
    """the d20 half a voxel of ulp away, with a work queue of 7 and a record list of 3 entries (test-hook build, child process)"""
    code = (
        "sys.path.insert(0, %r)\n"
        "import float_frames as FF\n"
        "from cuda_mesh_voxelization_amd.capi import Frame, ALGO_TILED\n"
        "from cuda_mesh_voxelization_amd.pipeline import Engine\n"
        "from oracle import oracle as O\n"
        "eng = Engine(0)\n"
        "xyz, tri, origin, vs = FF.mesh_level('d20.obj', 256, '0.5'); fr = Frame.make(256, vs, origin)\n"
        "dx, dt = eng.mesh_to_device(xyz, tri)\n"
        "exp = O.voxelize(xyz, tri, 256, vs, origin)\n"
        "for rep in range(3):\n"
        "    g = eng.voxelize(fr, dx, dt, algo=ALGO_TILED); eng.sync()\n"
        "    assert np.array_equal(eng.words_to_numpy(g), exp), rep\n"
        "print('ok')\n") % TESTS
    p = _run_with_hooks(code, {"VP_VOX_QUEUE_CAP": "7", "VP_VOX_REC_CAP": "3"})
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.stdout[-500:], p.stderr[-2000:])


# ---- JFA -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", ["near", "far", "collapsed"])
@pytest.mark.parametrize("n", [96, 128, 160, 256])
def test_jfa_every_pass_ids(engine, n, frame):
    """96: the first tile size; 128: starts from the mask; 160: ragged; 256: pair mode and closed tiles at k = n / 8.  In these frames
    rounding decides almost every tie, so "the first minimum in scan order" meets pairs that no integer tie offers"""
    fr, vs, o = _frame(n, frame)
    for kind in FF.GRID_KINDS:
        g = engine.to_device(FF.grid(kind, n), np.uint32)
        done = FF.check_every_pass_ids(engine, fr, g, (n, frame, kind))
        assert done >= len([k for k in (n >> s for s in range(1, 12)) if k >= 1])          # one comparison per pass at the least
    gc.collect(); torch.cuda.empty_cache()


def test_jfa_compact_ids_far(engine):
    """n = 1152 (ids in the 5-byte windows) on a sparse grid in the `far` frame: TILED against NAIVE"""
    gc.collect(); torch.cuda.empty_cache()
    n = 1152
    fr, vs, o = _frame(n, "far")
    rng = np.random.default_rng(n)
    words = (rng.random(fr.words) < 32 * 0.004).astype(np.uint32) << rng.integers(0, 32, fr.words).astype(np.uint32)
    g = engine.to_device(words, np.uint32)
    assert engine.ctx.jfa_id_bytes(fr) == 8 and engine.ctx.jfa_can_fuse_first_two(fr, ALGO_TILED)
    s_t = engine.jfa(fr, g, algo=ALGO_TILED).clone()
    s_n = engine.jfa(fr, g, algo=ALGO_NAIVE)
    engine.sync()
    same = torch.equal(s_t.view(torch.int32), s_n.view(torch.int32))
    bad = 0 if same else int((s_t.view(torch.int32) != s_n.view(torch.int32)).sum().item())
    del s_t, s_n, g
    engine._work = None
    gc.collect(); torch.cuda.empty_cache()
    assert same, (n, bad)


def _bites(frame, words, n, exp_minus):
    """the oracle's own output shows what a collapsed frame does: seeds at distance 0 from voxels that are no border voxels, -0.0 on unset ones"""
    if frame != "collapsed":
        return
    brd = FF.border(words, n).reshape(-1)
    zero = exp_minus == 0
    assert (zero & ~brd).any(), (n, "no zero off the border")
    assert (zero & np.signbit(exp_minus)).any(), (n, "no -0.0")


def _sdf_case(engine, n, frame, kind, algos):
    fr, vs, o = _frame(n, frame)
    words = FF.grid(kind, n)
    g = engine.to_device(words, np.uint32)
    for fill in (-np.inf, np.inf):
        exp = O.jfa(words, n, vs, o, fill=fill)
        assert not np.isnan(exp).any()
        if fill < 0:
            _bites(frame, words, n, exp)
        for algo in algos:
            got = engine.jfa(fr, g, fill=float(fill), algo=algo).cpu().numpy()
            bad = int(np.count_nonzero(got.view(np.uint32) != exp.view(np.uint32)))
            assert bad == 0, (n, frame, kind, fill, algo, bad)
            _assert_sdf_equal(got, exp)


@pytest.mark.parametrize("kind", FF.GRID_KINDS)
@pytest.mark.parametrize("frame", FRAMES5)
@pytest.mark.parametrize("n", [32, 64, 96, 128, 160])
def test_jfa_sdf_matches_oracle(engine, n, frame, kind):
    """32 and 64: the direct kernel; 96, 128, 160: the tile kernels.  Both algorithms, both fill signs"""
    _sdf_case(engine, n, frame, kind, ALGOS)


@pytest.mark.parametrize("kind", ["sparse", "boxes"])
@pytest.mark.parametrize("frame", ["far", "collapsed"])
def test_jfa_sdf_matches_oracle_n256(engine, frame, kind):
    _sdf_case(engine, 256, frame, kind, (ALGO_TILED,))


@pytest.mark.parametrize("level", LEVELS4)
def test_pipeline_on_translated_bunny(engine, level):
    """voxelize, vp_surface, vp_jfa and vp_jfa_start + vp_jfa_run at n = 128 against the oracle.  The border mask is NOT the zero set of the
    sdf here: a seed can lie at distance 0 from a voxel that is no border voxel"""
    name, n = "bunny.obj", 128
    xyz, tri, origin, vs = FF.mesh_level(name, n, level)
    fr = Frame.make(n, vs, origin)
    exp_w = O.voxelize(xyz, tri, n, vs, origin)
    exp_s = O.jfa(exp_w, n, vs, origin)
    assert np.isfinite(exp_s).all()
    exp_b = FF.pack(FF.border(exp_w, n))
    dx, dt = engine.mesh_to_device(xyz, tri)
    for algo in ALGOS:
        g = engine.voxelize(fr, dx, dt, algo=algo)
        assert np.array_equal(engine.words_to_numpy(g), exp_w), (level, algo)
        assert np.array_equal(engine.words_to_numpy(engine.surface(fr, g)), exp_b), (level, algo)
        got = engine.jfa(fr, g, algo=algo).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), exp_s.view(np.uint32)), (level, algo, int(np.count_nonzero(got.view(np.uint32) != exp_s.view(np.uint32))))
        _assert_sdf_equal(got, exp_s)
        out = torch.full((fr.voxels,), 7.0, dtype=torch.float32, device=engine.device)
        engine.ctx.jfa_start(fr, g.data_ptr(), None, 0, algo)
        engine.ctx.jfa_run(fr, g.data_ptr(), -math.inf, out.data_ptr(), None, 0, algo)
        engine.sync()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), exp_s.view(np.uint32)), (level, algo, "start + run")


def test_slab_routes_on_translated_bunny(engine):
    """two slabs at n = 128, the bunny half a voxel of ulp away: vp_surface with the neighbour's boundary plane as halo, and the hybrid
    window pipeline, equal the whole grid (which equals the oracle)"""
    name, n, world = "bunny.obj", 128, 2
    xyz, tri, origin, vs = FF.mesh_level(name, n, "0.5")
    fr = Frame.make(n, vs, origin)
    exp_w = O.voxelize(xyz, tri, n, vs, origin)
    exp_s = O.jfa(exp_w, n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    g = engine.voxelize(fr, dx, dt)
    assert np.array_equal(engine.words_to_numpy(g), exp_w)
    whole = engine.words_to_numpy(engine.surface(fr, g)).copy()
    assert np.array_equal(whole, FF.pack(FF.border(exp_w, n)))
    pw = n * n // 32
    parts = []
    for z0, z1 in ((0, n // 2), (n // 2, n)):
        sf = fr.slab(z0, z1)
        out = torch.empty(sf.words, dtype=torch.int32, device=engine.device)
        below = g[(z0 - 1) * pw:z0 * pw] if z0 > 0 else None
        above = g[z1 * pw:(z1 + 1) * pw] if z1 < n else None
        engine.ctx.surface(sf, g[z0 * pw:z1 * pw].data_ptr(), below.data_ptr() if below is not None else None,
                           above.data_ptr() if above is not None else None, out.data_ptr())
        parts.append(engine.words_to_numpy(out).copy())
    assert np.array_equal(np.concatenate(parts), whole)
    words, sdf = _run_slabs(world, fr, xyz, tri, ALGO_TILED, kind="hybrid")
    assert np.array_equal(words, exp_w)
    assert np.array_equal(sdf.view(np.uint32), exp_s.view(np.uint32)), int(np.count_nonzero(sdf.view(np.uint32) != exp_s.view(np.uint32)))


# ---- mesh distance ---------------------------------------------------------------------------------------------------------
MD_LEVELS = ("2^-10", "2^-4", "0.5", "x1000")


@pytest.mark.parametrize("level", MD_LEVELS)
@pytest.mark.parametrize("name,n", [("d20.obj", 32), ("torus.obj", 32), ("sphere.obj", 32), ("d20.obj", 64)])
def test_mesh_distance_translated(engine, name, n, level):
    """bands 1, 3 and 32, signed by the voxelized grid of the same translated mesh and unsigned: NAIVE, TILED, the host form and the numpy
    restatement.  The largest coordinate M is 2^13 .. 2^22 voxels here, so the grown box (2^-19 M t) and the plane bound (2^-16 M) are
    up to several voxels wide and each form culls another set of pairs"""
    xyz, tri, origin, vs = FF.mesh_level(name, n, level)
    fr = Frame.make(n, vs, origin)
    words = O.voxelize(xyz, tri, n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    assert np.array_equal(engine.words_to_numpy(engine.voxelize(fr, dx, dt)), words)
    bits = FF.unpack(words, n).reshape(-1)
    assert bits.any() and not bits.all()
    for band in (1, 3, 32):
        exp_d, exp_i = _check_all_forms(engine, xyz, tri, fr, n, vs, origin, band, words, (name, n, level, band))
        assert np.array_equal((exp_d >> 31) == 0, bits)
        un_d, un_i = _check_all_forms(engine, xyz, tri, fr, n, vs, origin, band, None, (name, n, level, band, "unsigned"))
        assert not (un_d >> 31).any() and np.array_equal(un_i, exp_i)
        assert (exp_i != R.NONE).any()


def test_mesh_distance_translated_mesh_that_leaves_the_frame(engine):
    name, n = "d20.obj", 64
    xyz, tri, origin, vs = FF.mesh_level(name, n, "0.5", scale=1.3)
    lo, hi = origin, origin + F(n) * vs
    assert (xyz.min(0) < lo).all() and (xyz.max(0) > hi).all()
    fr = Frame.make(n, vs, origin)
    _, exp_i = _check_all_forms(engine, xyz, tri, fr, n, vs, origin, 3, None, (name, n, "clipped, translated"))
    near = (exp_i != R.NONE).reshape(n, n, n)
    for face in (near[0], near[-1], near[:, 0], near[:, -1], near[:, :, 0], near[:, :, -1]):
        assert face.any()


def test_mesh_distance_translated_hand_cases(engine):
    """the sliver and the fan of test_hand_cases, moved by (81100.3, -40990.7, 6500.1) with the frame: vs = 1, origin = T"""
    n = 32
    T = np.array(FF.GRID_FRAMES["far"][1], np.float64)
    origin, vs = T.astype(F), F(1.0)
    fr = Frame.make(n, vs, origin)
    hub = np.array([10.5, 10.5, 10.5])
    fan_xyz = np.array([hub] + [hub + np.array([4 * np.cos(k * np.pi / 3), 4 * np.sin(k * np.pi / 3), -3.0]) for k in range(6)])
    fan = np.array([[0, 1 + k, 1 + (k + 1) % 6] for k in (3, 4, 5, 0, 1, 2)], np.uint32)
    for tag, xyz0, tri, band in (("sliver", SLIVER_XYZ, TRI, SLIVER_BAND), ("fan", fan_xyz, fan, 6)):
        xyz = FF.translate(xyz0, T)
        _, exp_i = _check_all_forms(engine, xyz, tri, fr, n, vs, origin, band, None, (tag, "translated"))
        assert (exp_i != R.NONE).any(), tag


@pytest.mark.parametrize("level", ["2^-4", "0.5"])
def test_mesh_distance_translated_bunny_lists(engine, level, capsys):
    """bunny at n = 128, band 3: TILED against NAIVE on the device; the (triangle, brick) pairs listed, beside the untranslated figure, are
    printed (the grown box lengthens the lists: DESIGN.md section 15 records the figures)"""
    from cuda_mesh_voxelization_amd import mesh as M
    name, n, band = "bunny.obj", 128, 3
    xyz0, tri0 = M.import_mesh(M.asset(name))
    o0, vs0 = M.frame([xyz0], n)
    dx0, dt0 = engine.mesh_to_device(xyz0, tri0)
    engine.mesh_distance(Frame.make(n, vs0, o0), dx0, dt0, band, algo=ALGO_TILED)
    engine.sync()
    base = engine.ctx.mesh_distance_list_entries()
    xyz, tri, origin, vs = FF.mesh_level(name, n, level)
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    grid = engine.voxelize(fr, dx, dt)
    td, ti = engine.mesh_distance(fr, dx, dt, band, sign_words=grid, want_nearest=True, algo=ALGO_TILED)
    engine.sync()
    listed = engine.ctx.mesh_distance_list_entries()
    nd, ni = engine.mesh_distance(fr, dx, dt, band, sign_words=grid, want_nearest=True, algo=ALGO_NAIVE)
    engine.sync()
    with capsys.disabled():
        print("\n[mesh distance lists] bunny n = 128 band 3: %d pairs at the origin, %d at level %s (x %.2f)" % (base, listed, level, listed / max(base, 1)))
    assert int((td.view(torch.int32) != nd.view(torch.int32)).sum()) == 0 and int((ti != ni).sum()) == 0
    assert int((ti != -1).sum()) > n * n
