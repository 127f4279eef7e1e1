"""The mesh distance field on the GPU (vp_mesh_distance): hand cases and the small meshes against the numpy restatement of
tests/meshdist_ref.py -- both algorithms and the host form, bit for bit including signs and -0.0, the nearest faces equal; the bands 1, 3
and 32; a fine mesh (many LDS batches per brick) against NAIVE and the sequential host path; large triangles at n = 512 compared on the
device; a mesh that leaves the frame through all six faces; the sign; refusals; the state shared with the rest of the context; the z ranges
of a capped list; the CLI."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cuda_mesh_voxelization_amd import build, capi, mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshdist_ref as R  # noqa: E402
from test_meshdist_cpu import SLIVER_BAND, SLIVER_XYZ, TRI, TRI_XYZ, _build_check  # noqa: E402

pytestmark = pytest.mark.gpu

ALGOS = (ALGO_NAIVE, ALGO_TILED)
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cli():
    return build.build_cli()


@functools.lru_cache(maxsize=None)
def _case(name, n, scale=1.0):
    """(xyz, tri, origin, vs, frame): the frame is that of the unscaled mesh; scale > 1 pushes the mesh out of it about its centre"""
    xyz, tri = M.import_mesh(M.asset(name))
    origin, vs = M.frame([xyz], n)
    if scale != 1.0:
        mid = ((xyz.max(0) + xyz.min(0)) * F(0.5)).astype(F)
        xyz = ((xyz - mid) * F(scale) + mid).astype(F)
    return xyz, tri, origin, vs, Frame.make(n, vs, origin)


def _run(engine, fr, dx, dt, band, sign, algo):
    """(dist2 as uint32, nearest as uint32), numpy"""
    d, i = engine.mesh_distance(fr, dx, dt, band, sign_words=sign, want_nearest=True, algo=algo)
    engine.sync()
    return d.cpu().numpy().view(np.uint32), i.cpu().numpy().view(np.uint32)


def _check_all_forms(engine, xyz, tri, fr, n, vs, origin, band, sign_np, tag):
    """NAIVE, TILED and the host form against the numpy restatement"""
    xyz, tri = np.ascontiguousarray(xyz, F).reshape(-1, 3), np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    exp_d, exp_i = R.mesh_distance_f32(xyz, tri, n, vs, origin, band, sign_np)
    exp_d = exp_d.view(np.uint32)
    dx, dt = engine.mesh_to_device(xyz, tri)
    sign = None if sign_np is None else torch.from_numpy(sign_np.view(np.int32)).to(engine.device)
    for algo in ALGOS:
        got_d, got_i = _run(engine, fr, dx, dt, band, sign, algo)
        assert np.array_equal(got_d, exp_d), (tag, algo, int((got_d != exp_d).sum()), np.argwhere(got_d != exp_d)[:4].tolist())
        assert np.array_equal(got_i, exp_i), (tag, algo, int((got_i != exp_i).sum()), np.argwhere(got_i != exp_i)[:4].tolist())
        only_d = engine.mesh_distance(fr, dx, dt, band, sign_words=sign, algo=algo)                  # d_nearest = NULL
        engine.sync()
        assert np.array_equal(only_d.cpu().numpy().view(np.uint32), exp_d), (tag, algo)
        host_d, host_i = engine.ctx.mesh_distance_host(fr, xyz, tri, band, sign_np, True, algo)
        assert np.array_equal(host_d.view(np.uint32), exp_d) and np.array_equal(host_i, exp_i), (tag, algo, "host")
    return exp_d, exp_i


def test_hand_cases(engine):
    n = 32
    vs, origin = F(1.0), np.zeros(3, F)
    fr = Frame.make(n, vs, origin)
    unset = np.zeros(n ** 3 // 32, np.uint32)
    some = np.zeros(n ** 3 // 32, np.uint32)
    some[5] = 0x80000001
    bad_xyz = np.concatenate([TRI_XYZ, [[np.nan, 1, 1], [np.inf, 2, 2], [20.5, 20.5, 20.5], [22.5, 22.5, 22.5], [21.5, 21.5, 21.5]]]).astype(F)
    bad = np.array([[0, 1, 9], [0, 3, 2], [4, 1, 2], [5, 6, 7], [5, 5, 6], [0, 1, 2]], np.uint32)
    hub = np.array([10.5, 10.5, 10.5], F)
    fan_xyz = np.array([hub] + [hub + np.array([4 * np.cos(k * np.pi / 3), 4 * np.sin(k * np.pi / 3), -3.0], F) for k in range(6)], F)
    fan = np.array([[0, 1 + k, 1 + (k + 1) % 6] for k in (3, 4, 5, 0, 1, 2)], np.uint32)
    cases = [
        ("one triangle, band 8", TRI_XYZ, TRI, 8, None),
        ("zeros on unset voxels", TRI_XYZ, TRI, 2, unset),
        ("band edge", TRI_XYZ, TRI, 2, some),
        ("nothing contributes but the last", bad_xyz, bad, 3, None),
        ("nothing contributes", bad_xyz, bad[:5], 3, unset),
        ("no triangles", np.zeros((0, 3), F), np.zeros((0, 3), np.uint32), 2, some),
        ("no triangles, unsigned", np.zeros((0, 3), F), np.zeros((0, 3), np.uint32), 32, None),
        ("wholly outside", TRI_XYZ + F(100.0), TRI, 2, None),
        ("partly outside", TRI_XYZ + np.array([-8.0, 0, 0], F), TRI, 2, None),
        ("outside, within the band of x = 0", TRI_XYZ + np.array([-13.5, 0, 0], F), TRI, 2, None),
        ("fan around one vertex", fan_xyz, fan, 6, None),
        ("the same triangle three times", TRI_XYZ, np.concatenate([TRI, TRI, TRI]), 6, None),
        ("sliver: face region with mixed signs", SLIVER_XYZ, TRI, SLIVER_BAND, None),
    ]
    for tag, xyz, tri, band, sign in cases:
        exp_d, exp_i = _check_all_forms(engine, xyz, tri, fr, n, vs, origin, band, sign, tag)
        if tag == "zeros on unset voxels":
            assert exp_d.reshape(n, n, n)[4, 4, 4] == 0x80000000                                   # -0.0 came through
        if tag == "the same triangle three times":
            assert set(np.unique(exp_i)) == {0, R.NONE}


@pytest.mark.parametrize("name,n", [("d20.obj", 32), ("torus.obj", 32), ("sphere.obj", 32), ("d20.obj", 64), ("d20.obj", 96)])
def test_meshes_against_the_numpy_restatement(engine, name, n):
    """n = 96: rows of three words, 12 bricks per side"""
    xyz, tri, origin, vs, fr = _case(name, n)
    dx, dt = engine.mesh_to_device(xyz, tri)
    grid = engine.voxelize(fr, dx, dt)
    engine.sync()
    words = engine.words_to_numpy(grid).copy().view(np.uint32)
    exp_d, _ = _check_all_forms(engine, xyz, tri, fr, n, vs, origin, 3, words, (name, n))
    # the sign bits are the grid's bits, everywhere
    bits = np.unpackbits(words.view(np.uint8), bitorder="little").astype(bool)
    assert np.array_equal((exp_d >> 31) == 0, bits) and bits.any() and not bits.all()
    if n == 32:
        un_d, _ = _check_all_forms(engine, xyz, tri, fr, n, vs, origin, 3, None, (name, n, "unsigned"))
        assert not (un_d >> 31).any()


@pytest.mark.parametrize("band", [1, 3, 32])
def test_bands(engine, band):
    """32: every brick has a list and every list is long; 1: most bricks are left to the streaming fill"""
    name, n = "d20.obj", 64
    xyz, tri, origin, vs, fr = _case(name, n)
    _, exp_i = _check_all_forms(engine, xyz, tri, fr, n, vs, origin, band, None, (name, n, band))
    inside = float((exp_i != R.NONE).mean())
    assert inside > 0.99 if band == 32 else inside < (0.2 if band == 1 else 0.5)


def test_fine_mesh_tiled_naive_and_sequential(engine, tmp_path):
    """bunny at n = 128: every triangle is far smaller than a voxel, the lists of the bricks run to many LDS batches.  TILED, NAIVE and
    VOX::MeshDistance<SEQUENTIAL> (tests/cpp/meshdist_check.cpp, signed by the sequential solid grid): field and nearest faces, bit for bit"""
    name, n, band = "bunny.obj", 128, 3
    xyz, tri, origin, vs, fr = _case(name, n)
    dx, dt = engine.mesh_to_device(xyz, tri)
    grid = engine.voxelize(fr, dx, dt)
    td, ti = engine.mesh_distance(fr, dx, dt, band, sign_words=grid, want_nearest=True, algo=ALGO_TILED)
    assert engine.ctx.mesh_distance_list_entries() > 64 * 2 * (n // 8) ** 2                      # far more pairs than bricks: long lists
    nd, ni = engine.mesh_distance(fr, dx, dt, band, sign_words=grid, want_nearest=True, algo=ALGO_NAIVE)
    engine.sync()
    assert int((td.view(torch.int32) != nd.view(torch.int32)).sum()) == 0 and int((ti != ni).sum()) == 0
    assert int((ti != -1).sum()) > n * n
    exe = _build_check(tmp_path)
    prefix = str(tmp_path / "bunny")
    subprocess.run([exe, M.asset(name), str(n), str(band), "1", "0", prefix], check=True, timeout=900, capture_output=True)
    seq_d, seq_i = np.fromfile(prefix + ".seq.dist.f32", np.uint32), np.fromfile(prefix + ".seq.near.u32", np.uint32)
    got_d, got_i = td.cpu().numpy().view(np.uint32), ti.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_d, seq_d), int((got_d != seq_d).sum())
    assert np.array_equal(got_i, seq_i), int((got_i != seq_i).sum())


def test_large_triangles_at_a_large_side(engine):
    """d20 at n = 512: twenty triangles of a few hundred voxels each; only a mismatch count comes back"""
    name, n, band = "d20.obj", 512, 2
    xyz, tri, origin, vs, fr = _case(name, n)
    dx, dt = engine.mesh_to_device(xyz, tri)
    grid = engine.voxelize(fr, dx, dt)
    td, ti = engine.mesh_distance(fr, dx, dt, band, sign_words=grid, want_nearest=True, algo=ALGO_TILED)
    nd, ni = engine.mesh_distance(fr, dx, dt, band, sign_words=grid, want_nearest=True, algo=ALGO_NAIVE)
    engine.sync()
    assert torch.equal(td.view(torch.int32), nd.view(torch.int32)) and torch.equal(ti, ni)
    listed = int((ti != -1).sum())
    assert 0 < listed < n ** 3 // 8
    del td, ti, nd, ni
    engine.ctx.release()
    torch.cuda.empty_cache()


def test_mesh_that_leaves_the_frame_through_all_six_faces(engine):
    name, n = "d20.obj", 64
    xyz, tri, origin, vs, fr = _case(name, n, 1.3)
    lo, hi = origin, origin + F(n) * vs
    assert (xyz.min(0) < lo).all() and (xyz.max(0) > hi).all()
    _, exp_i = _check_all_forms(engine, xyz, tri, fr, n, vs, origin, 3, None, (name, n, "clipped"))
    near = (exp_i != R.NONE).reshape(n, n, n)
    for face in (near[0], near[-1], near[:, 0], near[:, -1], near[:, :, 0], near[:, :, -1]):
        assert face.any()


def _raw(ctx_h, fr, dx, nverts, dt, ntris, sign, band, dist, near, algo):
    vp = capi._vp
    return capi.lib().vp_mesh_distance(ctx_h, None if fr is None else capi.ctypes.byref(fr), vp(dx), nverts, vp(dt), ntris, vp(sign), band,
                                       vp(dist), vp(near), algo)


def test_refusals_leave_the_outputs_untouched(engine):
    name, n = "d20.obj", 64
    xyz, tri, origin, vs, fr = _case(name, n)
    dx, dt = engine.mesh_to_device(xyz, tri)
    grid = engine.voxelize(fr, dx, dt)
    inputs = (grid.clone(), dx.clone(), dt.clone())
    pool = torch.full((2 * fr.voxels + 8,), 7, dtype=torch.int32, device=engine.device)
    sentinel = pool.clone()
    dist, near = pool.data_ptr(), pool.data_ptr() + 4 * fr.voxels
    h = engine.ctx._h
    args = dict(ctx_h=h, fr=fr, dx=dx.data_ptr(), nverts=dx.shape[0], dt=dt.data_ptr(), ntris=dt.shape[0], sign=grid.data_ptr(), band=2,
                dist=dist, near=near, algo=ALGO_TILED)
    assert _raw(**args) == 0                                                                     # the arguments are good ...
    engine.sync()
    pool.copy_(sentinel)                                                                         # ... and every change below is refused
    INVALID, UNSUPPORTED = 10001, 10002
    for change, code in [(dict(fr=fr.slab(8, n)), UNSUPPORTED), (dict(fr=Frame.make(2048, vs, origin)), UNSUPPORTED),
                         (dict(band=0), INVALID), (dict(band=33), INVALID), (dict(algo=0), INVALID), (dict(algo=3), INVALID),
                         (dict(dist=dist + 4), INVALID), (dict(near=near + 8), INVALID), (dict(sign=grid.data_ptr() + 4), INVALID),
                         (dict(dx=dx.data_ptr() + 4), INVALID),
                         (dict(near=dist), INVALID), (dict(near=dist + 4 * fr.voxels - 16), INVALID),     # the outputs overlap each other
                         (dict(dist=grid.data_ptr()), INVALID), (dict(near=dx.data_ptr()), INVALID), (dict(dist=dt.data_ptr()), INVALID),
                         (dict(ctx_h=None), INVALID), (dict(fr=None), INVALID), (dict(dist=0), INVALID),
                         (dict(dx=0), INVALID), (dict(dt=0), INVALID), (dict(nverts=0), INVALID)]:
        for algo in ALGOS if "algo" not in change else (None,):
            a = dict(args, **change)
            if algo is not None:
                a["algo"] = algo
            assert _raw(**a) == code, (change, algo)
    engine.sync()
    assert torch.equal(pool, sentinel)
    assert torch.equal(grid, inputs[0]) and torch.equal(dx, inputs[1]) and torch.equal(dt, inputs[2])
    hd = np.full(fr.voxels, 7, np.float32)
    for bad_fr, band, algo, code in ((fr.slab(8, n), 2, ALGO_TILED, UNSUPPORTED), (fr, 0, ALGO_TILED, INVALID), (fr, 2, 5, INVALID)):
        rc = capi.lib().vp_mesh_distance_host(h, capi.ctypes.byref(bad_fr), xyz.ctypes.data_as(capi._vp), xyz.shape[0], tri.ctypes.data_as(capi._vp),
                                              tri.shape[0], None, band, hd.ctypes.data_as(capi._vp), None, algo)
        assert rc == code
    assert (hd == 7).all()


def test_state_shared_with_the_rest_of_the_context(engine):
    n = 32
    xyz, tri, origin, vs, fr = _case("torus.obj", n)
    dx, dt = engine.mesh_to_device(xyz, tri)
    grid = engine.voxelize(fr, dx, dt)
    jfa0 = engine.jfa(fr, grid).clone()
    edt0 = engine.edt_sdf(fr, grid).clone()
    small = engine.mesh_to_device(*_case("d20.obj", n)[:2])
    first = {algo: [t.clone() for t in engine.mesh_distance(fr, *small, 3, sign_words=grid, want_nearest=True, algo=algo)] for algo in ALGOS}
    # a larger mesh on the same context: the records, scans and lists grow
    exp_d, exp_i = R.mesh_distance_f32(xyz, tri, n, vs, origin, 3, engine.words_to_numpy(grid).copy().view(np.uint32))
    for algo in ALGOS:
        got_d, got_i = _run(engine, fr, dx, dt, 3, grid, algo)
        assert np.array_equal(got_d, exp_d.view(np.uint32)) and np.array_equal(got_i, exp_i), algo
    assert torch.equal(engine.jfa(fr, grid), jfa0) and torch.equal(engine.edt_sdf(fr, grid), edt0)
    # a pending vp_jfa_start is dropped by an output that lands on its grid, and only by that
    sdf = torch.empty(fr.voxels, dtype=torch.float32, device=engine.device)
    vol = torch.zeros(fr.voxels, dtype=torch.int32, device=engine.device)
    g = vol[:fr.words]
    g.copy_(grid)
    engine.ctx.jfa_start(fr, g.data_ptr(), None, 0, ALGO_TILED)
    engine.mesh_distance(fr, dx, dt, 2)
    engine.ctx.jfa_run(fr, g.data_ptr(), -math.inf, sdf.data_ptr(), None, 0, ALGO_TILED)
    engine.sync()
    assert torch.equal(sdf, jfa0)
    g.copy_(grid)
    engine.ctx.jfa_start(fr, g.data_ptr(), None, 0, ALGO_TILED)
    engine.mesh_distance(fr, dx, dt, 2, out=vol.view(torch.float32))
    with pytest.raises(capi.VPError) as e:
        engine.ctx.jfa_run(fr, g.data_ptr(), -math.inf, sdf.data_ptr(), None, 0, ALGO_TILED)
    assert e.value.code == 10001
    # release, then again
    engine.sync()
    engine.ctx.release()
    for algo in ALGOS:
        again = engine.mesh_distance(fr, *small, 3, sign_words=grid, want_nearest=True, algo=algo)
        engine.sync()
        assert torch.equal(again[0].view(torch.int32), first[algo][0].view(torch.int32)) and torch.equal(again[1], first[algo][1]), algo
    assert torch.equal(first[ALGO_NAIVE][0].view(torch.int32), first[ALGO_TILED][0].view(torch.int32))
    assert torch.equal(engine.jfa(fr, grid), jfa0) and torch.equal(engine.edt_sdf(fr, grid), edt0)


def test_timing_keys(engine):
    n = 64
    xyz, tri, origin, vs, fr = _case("torus.obj", n)
    dx, dt = engine.mesh_to_device(xyz, tri)
    ctx = engine.ctx

    def keys(fn):
        ctx.prof_reset()
        ctx.prof_enable(True)
        fn()
        ctx.prof_enable(False)
        return {k: v["launches"] for k, v in ctx.prof().items()}
    assert keys(lambda: engine.mesh_distance(fr, dx, dt, 2)) == {"md_setup": 1, "md_scan": 2, "md_count": 1, "md_write": 1, "md_brick": 1, "md_fill": 1}
    assert keys(lambda: engine.mesh_distance(fr, dx, dt, 2, algo=ALGO_NAIVE)) == {"md_prefill": 1, "md_naive": 1, "md_split": 1}
    assert keys(lambda: engine.mesh_distance(fr, dx[:0], dt[:0], 2)) == {"md_fill": 1}
    ctx.prof_select(["md_brick"])
    assert keys(lambda: engine.mesh_distance(fr, dx, dt, 2)) == {"md_brick": 1}
    ctx.prof_select(None)
    for i, name in enumerate(capi.HEADER_PROF_KEYS):
        assert capi.lib().vp_prof_name(i).decode() == name


def test_a_capped_list_runs_in_z_ranges_of_bricks():
    """the test-hook build with a list cap of a few thousand entries: the grid runs in many z ranges and gives the same bytes"""
    code = (
        "import torch\n"
        "from cuda_mesh_voxelization_amd import mesh as M\n"
        "from cuda_mesh_voxelization_amd.capi import Frame, ALGO_TILED, ALGO_NAIVE\n"
        "from cuda_mesh_voxelization_amd.pipeline import Engine\n"
        "eng = Engine(0)\n"
        "for name, n, band in (('torus.obj', 64, 3), ('d20.obj', 96, 32)):\n"
        "    xyz, tri = M.import_mesh(M.asset(name)); origin, vs = M.frame([xyz], n); fr = Frame.make(n, vs, origin)\n"
        "    dx, dt = eng.mesh_to_device(xyz, tri)\n"
        "    a = eng.mesh_distance(fr, dx, dt, band, want_nearest=True, algo=ALGO_TILED)\n"
        "    b = eng.mesh_distance(fr, dx, dt, band, want_nearest=True, algo=ALGO_NAIVE)\n"
        "    eng.sync(); assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]), (name, n)\n"
        "    print(name, eng.ctx.prof().get('md_brick', {}).get('launches'))\n"
        "print('ok')\n")
    build.build_lib(hooks=True)
    pre = "import sys\nsys.path.insert(0, %r)\n" % ROOT
    launches = {}
    for cap in ("1", "3000"):
        p = subprocess.run([sys.executable, "-c", pre + code.replace("eng = Engine(0)\n", "eng = Engine(0); eng.ctx.prof_enable(True)\n")],
                           capture_output=True, text=True, timeout=900, env=dict(os.environ, VPHIP_LIB=capi.HOOKS_LIB_PATH, VP_MESHDIST_LIST_CAP=cap))
        assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (cap, p.stdout[-500:], p.stderr[-2000:])
        launches[cap] = [int(line.split()[1]) for line in p.stdout.strip().splitlines()[:-1]]
    assert launches["1"][0] > 1 and launches["3000"][0] > 1                                      # several ranges did run: one md_brick launch each


def test_cli_device_equals_host(cli, tmp_path):
    n = 64
    mesh = M.asset("torus.obj")
    dumps = {}
    for t in ("2", "0"):
        d = tmp_path / ("t" + t)
        d.mkdir()
        p = subprocess.run([cli, mesh, "-n", str(n), "-t", t, "-s", "--mesh-sdf", "2", "-d", str(d / "x")] + (["-e"] if t == "2" else []),
                           capture_output=True, text=True, timeout=900, cwd=str(d))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert "MeshDistance" in p.stdout
        dumps[t] = (open(str(d / "x.grid.u32"), "rb").read(), open(str(d / "x.sdf.f32"), "rb").read())
    assert dumps["2"] == dumps["0"] and len(dumps["0"][1]) == 4 * n ** 3
    assert os.path.getsize(str(tmp_path / "t2" / "out" / "sdf_tiled_out.obj")) > 0
    p = subprocess.run([cli, mesh, M.asset("d20.obj"), "-n", "32", "-t", "2", "-s", "--mesh-sdf", "2"], capture_output=True, text=True,
                       timeout=300, cwd=str(tmp_path))
    assert p.returncode != 0 and "single mesh" in p.stdout + p.stderr
