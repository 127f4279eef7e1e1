"""Conservative surface voxelization on the GPU (vp_voxelize_conservative): TILED and NAIVE against the host restatement
(`vpcli -t 3 --conservative`, vplib/src/cvox.cpp) and the numpy restatement of tests/test_conservative_cpu.py, word for word; slabs,
accumulate (OR), triangle order, invalid triangles, empty meshes, the record-list fallback, refusals, the state it shares with the rest of
the context, and the CLI composition (CSG, sdf, exports) on its grids."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cuda_mesh_voxelization_amd import build, capi, mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame
from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_conservative_cpu import cvox_numpy, open_sphere, soup  # noqa: E402
from test_export import _check_file, _check_sdf_files  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    return build.build_cli()


def _gpu(engine, fr, xyz, tri, algo, out=None, accumulate=False):
    dx, dt = engine.mesh_to_device(xyz, tri)
    g = engine.voxelize_conservative(fr, dx, dt, out=out, algo=algo, accumulate=accumulate)
    engine.sync()
    return engine.words_to_numpy(g).copy()


def _host(cli, path, n, tmp_path):
    prefix = str(tmp_path / "host")
    p = subprocess.run([cli, path, "-n", str(n), "-t", "3", "--conservative", "-d", prefix], capture_output=True, text=True,
                       timeout=1800, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return np.fromfile(prefix + ".grid.u32", np.uint32)


def _frame(xyz, n):
    origin, vs = M.frame([xyz], n)
    return Frame.make(n, vs, origin), origin, vs


def grid_soup(seed=11, count=12):
    """triangles with corners anywhere in the unit cube (most span a large part of the grid) plus the cube's corners"""
    rng = np.random.default_rng(seed)
    xyz = np.concatenate([np.array([[0, 0, 0], [1, 1, 1]], np.float32), rng.random((3 * count, 3)).astype(np.float32)])
    tri = (np.arange(3 * count).reshape(-1, 3) + 2).astype(np.uint32)
    return xyz, tri


@pytest.mark.parametrize("name", ["d20.obj", "torus.obj", "sphere.obj", "bunny.obj", "bimba.obj"])
def test_tiled_and_naive_equal_the_host_path(engine, cli, tmp_path, name):
    xyz, tri = M.import_mesh(M.asset(name))
    for n in (32, 64, 96, 128, 256, 512):
        fr, _, _ = _frame(xyz, n)
        exp = _host(cli, M.asset(name), n, tmp_path)
        assert exp.any()
        for algo in (ALGO_TILED, ALGO_NAIVE):
            got = _gpu(engine, fr, xyz, tri, algo)
            assert np.array_equal(got, exp), (name, n, algo, int(np.count_nonzero(got != exp)))


@pytest.mark.parametrize("n", [512, 1024])
def test_bunny24_equals_the_host_path(engine, cli, tmp_path, n):
    path = str(tmp_path / "bunny24.obj")
    M.export_obj(path, *M.bunny(24))
    xyz, tri = M.import_mesh(path)
    assert tri.shape[0] == 1348128
    fr, _, _ = _frame(xyz, n)
    exp = _host(cli, path, n, tmp_path)
    for algo in (ALGO_TILED, ALGO_NAIVE):
        assert np.array_equal(_gpu(engine, fr, xyz, tri, algo), exp), (n, algo)


@pytest.mark.parametrize("n", [1024, 2048])
def test_large_triangles_tiled_equals_naive(engine, n):
    for label, (xyz, tri) in (("d20", M.import_mesh(M.asset("d20.obj"))), ("grid_soup", grid_soup())):
        fr, _, _ = _frame(xyz, n)
        a = _gpu(engine, fr, xyz, tri, ALGO_TILED)
        b = _gpu(engine, fr, xyz, tri, ALGO_NAIVE)
        assert a.any() and np.array_equal(a, b), (label, n, int(np.count_nonzero(a != b)))
        del a, b
        torch.cuda.empty_cache()


def test_numpy_restatement_on_the_device(engine):
    for label, (xyz, tri) in (("soup", soup()), ("open_sphere", open_sphere()), ("grid_soup", grid_soup())):
        for n in (32, 64):
            fr, origin, vs = _frame(xyz, n)
            exp = cvox_numpy(xyz, tri, n, vs, origin)
            for algo in (ALGO_TILED, ALGO_NAIVE):
                assert np.array_equal(_gpu(engine, fr, xyz, tri, algo), exp), (label, n, algo)


def test_hand_cases_on_the_device(engine):
    fr = Frame.make(32, 1.0, (0, 0, 0))
    tri = np.array([[0, 1, 2]], np.uint32)
    for v in ([[1, 1, 3.5], [6, 1, 3.5], [1, 6, 3.5]], [[1, 1, 3], [6, 1, 3], [1, 6, 3]], [[-10, 1, 1], [-9, 1, 1], [-10, 2, 1]],
              [[1, 1, 1], [2, 2, 2], [3, 3, 3]]):
        xyz = np.asarray(v, np.float32)
        exp = cvox_numpy(xyz, tri, 32, 1.0, (0, 0, 0))
        for algo in (ALGO_TILED, ALGO_NAIVE):
            assert np.array_equal(_gpu(engine, fr, xyz, tri, algo), exp), (v, algo)


def test_slabs_are_planes_of_the_whole_grid(engine):
    for name, n, cuts in (("sphere.obj", 128, (0, 40, 48, 128)), ("d20.obj", 256, (0, 8, 136, 256)), ("torus.obj", 96, (0, 96))):
        xyz, tri = M.import_mesh(M.asset(name))
        fr, _, _ = _frame(xyz, n)
        plane = n * n // 32
        for algo in (ALGO_TILED, ALGO_NAIVE):
            whole = _gpu(engine, fr, xyz, tri, algo)
            for z0, z1 in zip(cuts[:-1], cuts[1:]):
                got = _gpu(engine, fr.slab(z0, z1), xyz, tri, algo)
                assert np.array_equal(got, whole[z0 * plane:z1 * plane]), (name, z0, z1, algo)


def test_accumulate_is_a_union(engine):
    xyz, tri = M.import_mesh(M.asset("sphere.obj"))
    fr, _, _ = _frame(xyz, 128)
    dx = engine.to_device(xyz, np.float32)
    for algo in (ALGO_TILED, ALGO_NAIVE):
        whole = _gpu(engine, fr, xyz, tri, algo)
        g = engine.new_grid(fr)
        g.fill_(-1)                                                   # overwrite: the garbage goes
        engine.voxelize_conservative(fr, dx, engine.to_device(tri[0::2], np.uint32), out=g, algo=algo)
        engine.voxelize_conservative(fr, dx, engine.to_device(tri[1::2], np.uint32), out=g, algo=algo, accumulate=True)
        engine.sync()
        assert np.array_equal(engine.words_to_numpy(g), whole)
        pre = np.random.default_rng(5).integers(0, 2 ** 32, fr.words, dtype=np.uint64).astype(np.uint32)
        pre[::3] = 0
        g = engine.to_device(pre, np.uint32)
        engine.voxelize_conservative(fr, dx, engine.to_device(tri, np.uint32), out=g, algo=algo, accumulate=True)
        engine.sync()
        assert np.array_equal(engine.words_to_numpy(g), pre | whole)


def test_triangle_order_does_not_matter(engine):
    for name, n in (("bunny.obj", 256), ("d20.obj", 128)):
        xyz, tri = M.import_mesh(M.asset(name))
        fr, _, _ = _frame(xyz, n)
        perm = np.random.default_rng(9).permutation(tri.shape[0])
        for algo in (ALGO_TILED, ALGO_NAIVE):                          # (corner order is part of the float contract: e0, e1, nrm)
            assert np.array_equal(_gpu(engine, fr, xyz, tri, algo), _gpu(engine, fr, xyz, tri[perm], algo)), (name, algo)


def test_invalid_triangles_contribute_nothing(engine):
    xyz, tri = soup()
    xyz = np.concatenate([xyz, np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf]], np.float32)])
    k = xyz.shape[0]
    bad = np.array([[k - 3, 0, 1], [2, k - 2, 3], [4, 5, k - 1], [0, 1, k], [k + 7, 2, 3], [0, 2 ** 31, 1]], np.uint32)
    tri2 = np.concatenate([tri[:5], bad, tri[5:]]).astype(np.uint32)
    fr, origin, vs = _frame(xyz[np.isfinite(xyz).all(axis=1)], 64)
    exp = cvox_numpy(xyz, tri2, 64, vs, origin)
    assert np.array_equal(exp, cvox_numpy(xyz, tri, 64, vs, origin))
    for algo in (ALGO_TILED, ALGO_NAIVE):
        assert np.array_equal(_gpu(engine, fr, xyz, tri2, algo), exp), algo


def test_empty_mesh(engine):
    fr = Frame.make(64, 0.1, (0, 0, 0))
    dx = engine.to_device(np.zeros((3, 3), np.float32), np.float32)
    dt = engine.to_device(np.zeros((0, 3), np.uint32), np.uint32)
    for algo in (ALGO_TILED, ALGO_NAIVE):
        g = engine.new_grid(fr)
        g.fill_(7)
        engine.ctx.voxelize_conservative(fr, g.data_ptr(), dx.data_ptr(), 3, dt.data_ptr(), 0, algo, True)
        engine.sync()
        assert (engine.words_to_numpy(g) == 7).all()
        engine.ctx.voxelize_conservative(fr, g.data_ptr(), dx.data_ptr(), 3, dt.data_ptr(), 0, algo, False)
        engine.sync()
        assert not engine.words_to_numpy(g).any()


def test_record_list_overflow_path():
    """The large-triangle list is sized from what earlier calls counted; a large triangle that finds it full is walked by its setup
    thread.  VP_CVOX_REC_CAP (hooks build) forces lists of 0 / 3 / 7 entries: same bits as NAIVE."""
    code = (
        "from cuda_mesh_voxelization_amd import mesh as M\n"
        "from cuda_mesh_voxelization_amd.capi import Frame, ALGO_TILED, ALGO_NAIVE\n"
        "from cuda_mesh_voxelization_amd.pipeline import Engine\n"
        "eng = Engine(0)\n"
        "for name, n in (('d20.obj', 256), ('sphere.obj', 128), ('bunny.obj', 64)):\n"
        "    xyz, tri = M.import_mesh(M.asset(name)); origin, vs = M.frame([xyz], n); fr = Frame.make(n, vs, origin)\n"
        "    dx, dt = eng.mesh_to_device(xyz, tri)\n"
        "    a = eng.voxelize_conservative(fr, dx, dt, algo=ALGO_TILED); b = eng.voxelize_conservative(fr, dx, dt, algo=ALGO_NAIVE)\n"
        "    eng.sync(); assert np.array_equal(eng.words_to_numpy(a), eng.words_to_numpy(b)), (name, n)\n"
        "print('ok')\n")
    build.build_lib(hooks=True)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pre = "import sys, numpy as np\nsys.path.insert(0, %r)\n" % root
    for cap in ("0", "3", "7"):
        p = subprocess.run([sys.executable, "-c", pre + code], capture_output=True, text=True, timeout=900,
                           env=dict(os.environ, VPHIP_LIB=capi.HOOKS_LIB_PATH, VP_CVOX_REC_CAP=cap))
        assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (cap, p.stdout[-500:], p.stderr[-2000:])


def test_refusals_leave_the_buffer_untouched(engine):
    xyz, tri = M.import_mesh(M.asset("d20.obj"))
    fr, _, _ = _frame(xyz, 64)
    dx, dt = engine.mesh_to_device(xyz, tri)
    g = torch.full((fr.words + 4,), 5, dtype=torch.int32, device=engine.device)
    ctx = engine.ctx
    calls = [
        lambda: ctx.voxelize_conservative(fr, 0, dx.data_ptr(), dx.shape[0], dt.data_ptr(), dt.shape[0]),
        lambda: ctx.voxelize_conservative(fr, g.data_ptr(), 0, dx.shape[0], dt.data_ptr(), dt.shape[0]),
        lambda: ctx.voxelize_conservative(fr, g.data_ptr() + 4, dx.data_ptr(), dx.shape[0], dt.data_ptr(), dt.shape[0]),
        lambda: ctx.voxelize_conservative(fr, g.data_ptr(), dx.data_ptr(), dx.shape[0], dt.data_ptr(), dt.shape[0], algo=3),
        lambda: ctx.voxelize_conservative(Frame.make(48, fr.voxel_size, fr.origin), g.data_ptr(), dx.data_ptr(), dx.shape[0],
                                          dt.data_ptr(), dt.shape[0]),
        lambda: ctx.voxelize_conservative(fr.slab(4, 64), g.data_ptr(), dx.data_ptr(), dx.shape[0], dt.data_ptr(), dt.shape[0]),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(capi.VPError):
            call()
        engine.sync()
        assert (g.cpu().numpy() == 5).all(), i


def test_jfa_start_is_dropped_by_a_conservative_write(engine):
    xyz, tri = M.import_mesh(M.asset("bunny.obj"))
    fr, _, _ = _frame(xyz, 128)
    dx, dt = engine.mesh_to_device(xyz, tri)
    g = engine.voxelize(fr, dx, dt)
    out = torch.empty(fr.voxels, dtype=torch.float32, device=engine.device)
    for algo in (ALGO_TILED, ALGO_NAIVE):
        engine.ctx.jfa_start(fr, g.data_ptr(), None, 0, algo)
        engine.voxelize_conservative(fr, dx, dt, out=g, accumulate=True)
        with pytest.raises(capi.VPError) as e:
            engine.ctx.jfa_run(fr, g.data_ptr(), -math.inf, out.data_ptr(), None, 0, algo)
        assert e.value.code == 10001
    engine.ctx.jfa_start(fr, g.data_ptr(), None, 0, ALGO_TILED)      # a fresh start serves the run
    engine.ctx.jfa_run(fr, g.data_ptr(), -math.inf, out.data_ptr(), None, 0, ALGO_TILED)
    engine.sync()


def test_solid_state_is_not_touched(engine):
    """solid, conservative, solid on one context: the solid grids are identical and the repeated solid job still leaves its list
    kernels out (the conservative path keeps counts of its own)"""
    ctx = capi.Context(0)
    try:
        ctx.set_stream(torch.cuda.current_stream(engine.device).cuda_stream, external=True)
        xyz, tri = M.import_mesh(M.asset("bunny.obj"))
        fr, origin, vs = _frame(xyz, 256)
        dx, dt = engine.mesh_to_device(xyz, tri)
        g = engine.new_grid(fr)
        c = engine.new_grid(fr)
        lists = {"vox_scan", "vox_scatter", "vox_tile"}

        def solid(prof=False):
            if prof:
                ctx.prof_reset(); ctx.prof_enable(True)
            ctx.voxelize(fr, g.data_ptr(), dx.data_ptr(), dx.shape[0], dt.data_ptr(), dt.shape[0], ALGO_TILED, False)
            ctx.sync()
            keys = set()
            if prof:
                ctx.prof_enable(False); keys = set(ctx.prof())
            return engine.words_to_numpy(g).copy(), keys

        first, _ = solid()
        solid()
        _, keys = solid(prof=True)
        assert "vox_setup" in keys and not (lists & keys)
        for algo in (ALGO_TILED, ALGO_NAIVE):
            ctx.voxelize_conservative(fr, c.data_ptr(), dx.data_ptr(), dx.shape[0], dt.data_ptr(), dt.shape[0], algo, False)
            ctx.sync()
            again, keys = solid(prof=True)
            assert np.array_equal(again, first) and "vox_setup" in keys and not (lists & keys), algo
        assert np.array_equal(first, O.voxelize(xyz, tri, 256, vs, origin))
    finally:
        ctx.close()


def test_cli_composition(cli, tmp_path):
    n = 64
    meshes = [M.asset("bimba.obj"), M.asset("bunny.obj")]
    dumps = {}
    for t in (2, 0):
        d = tmp_path / ("t%d" % t)
        d.mkdir()
        p = subprocess.run([cli] + meshes + ["-n", str(n), "-t", str(t), "--conservative", "-p", "1", "-s", "-e", "-d", str(d / "x")],
                           capture_output=True, text=True, cwd=str(d), timeout=900)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        dumps[t] = (np.fromfile(str(d / "x.grid.u32"), np.uint32), np.fromfile(str(d / "x.sdf.f32"), np.float32))
    (gw, gs), (hw, hs) = dumps[2], dumps[0]
    assert np.array_equal(gw, hw) and np.array_equal(gs.view(np.uint32), hs.view(np.uint32))
    xyz = [M.import_mesh(m)[0] for m in meshes]
    origin, vs = O.frame(xyz, n)
    exp_w = np.zeros_like(gw)
    for m in meshes:
        exp_w |= cvox_numpy(*M.import_mesh(m), n, vs, origin)
    assert np.array_equal(gw, exp_w)
    sdf = O.jfa(gw, n, vs, origin)
    assert np.array_equal(gs.view(np.uint32), sdf.view(np.uint32))
    out = tmp_path / "t2" / "out"
    _check_file(str(out / "csg_vox_tiled_out.obj"), *O.grid_to_mesh_compressed(gw, n, vs, origin))
    _check_sdf_files(out, "tiled", O.grid_to_mesh_cubes(gw, sdf, n, vs, origin), O.grid_to_point_cloud(gw, sdf, n, vs, origin))
