"""Outputs of the REFERENCE ITSELF, recorded in tests/golden/reference_outputs.json by tests/golden/make_reference_outputs.py, which runs the
record_* functions below on oracle/_ref (oracle/Makefile, target _ref: the reference's mesh/mesh_io.cpp, mesh/grid_to_mesh.cpp, csg/sequential.cpp,
grid/voxels_grid.cu and bounding_box.h behind oracle/ref_driver.cpp, built where the reference tree is at hand).  What they pin:

  * the OBJ importer (ImportMesh) and the frame of a run (CalculateBoundingBox as apps/cli/main.cpp:65-87 uses it)   -> mesh.py, the oracle, vpcli
  * CSG::Compute<SEQUENTIAL> for the three operators                                                              -> the oracle, the golden table's CSG rows, the GPU kernel
  * VoxelsGridToMeshCompressed / VoxelsGridToMesh / VoxelsGridToPointCloud + ExportMesh                         -> oracle_export.c and the files vpcli -e / -s -e writes
  * the bit layout of VoxelsGrid (the exporters and CSG read the product's words through the reference's own Voxel() / Word())

The voxelizer and the JFA of the reference do NOT build (vox.h needs <cub/cub.cuh>; jfa/sequential.cpp allocates with cudaMalloc): those two
stay pinned to the survey table (tests/golden/PROVENANCE.md).  Every test compares with the recorded outputs, so none of them needs the
reference tree or oracle/_ref."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from cuda_mesh_voxelization_amd import build, mesh as M
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_outputs.json")
ASSETS = ["d20.obj", "torus.obj", "sphere.obj", "bunny.obj", "bimba.obj"]
FRAMES = [(["d20.obj"], 32), (["bunny.obj"], 64), (["bimba.obj", "bunny.obj"], 64), (["sphere.obj", "torus.obj"], 48), (["bimba.obj", "bunny.obj"], 512)]
CSG_OPS = [1, 2, 3]
EXPORTS = [("d20.obj", 32), ("torus.obj", 32), ("sphere.obj", 48)]
CLI_EXPORTS = [("d20.obj", 32), ("torus.obj", 32)]
CLI_TYPES = [(0, "sequential"), (3, "openmp")]
GPU_EXPORTS = [("torus.obj", 32), ("bunny.obj", 128)]
MISC_ARGS = ["misc", "/a/b/c.obj", "plain.obj", "dir/"]
ASSERT_MSG = "Number of GPUs must be 1..64"


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cli():
    return build.build_cli()


def _body(path):
    """an OBJ file without its comment lines (the two exporters sign their files differently)"""
    return [ln for ln in open(path) if not ln.startswith("#")]


def _digest(obj):
    return hashlib.sha256(json.dumps(obj).encode()).hexdigest()[:32]


def _bits(a):
    return [int(x) for x in np.asarray(a, np.float32).reshape(-1).view(np.uint32)]


def _write_bunny_x3(path):
    """the refined bunny of the benchmark, written as an OBJ with nine significant digits"""
    xyz, tri = M.bunny(3)
    with open(path, "w") as f:
        f.write("# Vertices: %d\n# Faces: %d\n" % (xyz.shape[0], tri.shape[0]))
        for v in xyz:
            f.write("v %.9g %.9g %.9g\n" % tuple(float(c) for c in v))
        f.write("vn 0 0 1\n")
        for t in tri:
            f.write("f %d//1 %d//1 %d//1\n" % tuple(int(i) + 1 for i in t))
    return xyz, tri


def _grids(n):
    """the bimba / bunny grids of the golden table's CSG rows at n, in the frame of both"""
    a_xyz, a_tri = M.import_mesh(M.asset("bimba.obj"))
    b_xyz, b_tri = M.import_mesh(M.asset("bunny.obj"))
    origin, vs = O.frame([a_xyz, b_xyz], n)
    return O.voxelize(a_xyz, a_tri, n, vs, origin), O.voxelize(b_xyz, b_tri, n, vs, origin)


def _noise(seed, n):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2**32, n * n * n // 32, dtype=np.uint32), rng.integers(0, 2**32, n * n * n // 32, dtype=np.uint32)


def _parse(path):
    """an exported OBJ as [vertex coordinate strings, colour strings, face indices, normal indices]"""
    v, c, f, fn = [], [], [], []
    for ln in open(path):
        p = ln.split()
        if ln.startswith("v "):
            v.append(p[1:4]); c.append(p[4:7])
        elif ln.startswith("f "):
            q = [t.split("//") for t in p[1:4]]
            f.append([int(t[0]) - 1 for t in q]); fn.append([int(t[1]) - 1 for t in q])
    return [v, c, f, fn]


def _cli_dump(cli, tmp_path, name, n, t):
    """`vpcli <mesh> -n n -t t -s -e -d`: the directory of the three exported files, the product's grid and sdf"""
    p = subprocess.run([cli, M.asset(name), "-n", str(n), "-t", str(t), "-s", "-e", "-d", str(tmp_path / "d")], capture_output=True, text=True, cwd=tmp_path, timeout=900)
    assert p.returncode == 0, p.stdout + p.stderr
    return tmp_path / "out", np.fromfile(str(tmp_path / "d.grid.u32"), np.uint32), np.fromfile(str(tmp_path / "d.sdf.f32"), np.float32)


# ---------------------------------------------------------------------------------------------- what the reference's own code outputs
# (run by tests/golden/make_reference_outputs.py on oracle/_ref; each returns the JSON value the tests below compare with)
def record_import(name, workdir):
    rx, rt = O.ref_import(M.asset(name), workdir)
    return [O.fnv(rx), O.fnv(rt), int(rx.shape[0]), int(rt.shape[0])]


def record_import_bunny_x3(workdir):
    path = os.path.join(workdir, "bunny_x3.obj")
    _write_bunny_x3(path)
    rx, rt = O.ref_import(path, workdir)
    return [O.fnv(rx), O.fnv(rt)]


def record_frame(names, n):
    ro, rv = O.ref_frame([M.asset(a) for a in names], n)
    return _bits(ro) + _bits(rv)


def record_csg(op, workdir):
    a, b = _grids(64)
    x, y = _noise(op, 32)
    return [O.fnv(O.ref_csg(a, b, 64, op, workdir)), O.fnv(O.ref_csg(x, y, 32, op, workdir))]


def record_gpu_csg(op, workdir):
    a, b = _noise(10 + op, 64)
    return O.fnv(O.ref_csg(a, b, 64, op, workdir))


def record_exports(name, n, workdir):
    xyz, tri = M.import_mesh(M.asset(name))
    origin, vs = O.frame([xyz], n)
    words = O.voxelize(xyz, tri, n, vs, origin)
    sdf = O.jfa(words, n, vs, origin)
    return [_digest(_parse(p)) for p in O.ref_export(words, sdf, n, vs, origin, workdir)]


def record_cli_exports(cli, tmp_path, name, n, t):
    """the reference's exporters run on the grid and sdf `vpcli -t t` dumps: digests of the three files without their comment lines"""
    _, words, sdf = _cli_dump(cli, tmp_path, name, n, t)
    ro, rv = O.ref_frame([M.asset(name)], n)
    return [_digest(_body(p)) for p in O.ref_export(words, sdf, n, rv, ro, str(tmp_path))]


def record_vector_ops(workdir):
    p = _pairs(7)
    p.tofile(os.path.join(workdir, "pairs.f32"))
    out = []
    for cmd in ("distance", "vec"):
        O._ref(cmd, os.path.join(workdir, "pairs.f32"), os.path.join(workdir, "ref_%s.f32" % cmd))
        out.append(O.fnv(np.fromfile(os.path.join(workdir, "ref_%s.f32" % cmd), np.float32)))
    return out


def record_helpers():
    r = subprocess.run([O.build_ref(), "assert", ASSERT_MSG], capture_output=True, text=True)
    return {"misc": O._ref(*MISC_ARGS), "profile": O._ref("profile", "TiledJFA::Processing"), "assert_rc": r.returncode, "assert_stdout": r.stdout}


# ---------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("name", ASSETS)
def test_import_is_the_references_import(golden, name):
    xyz, tri = M.import_mesh(M.asset(name))
    assert [O.fnv(xyz), O.fnv(tri), int(xyz.shape[0]), int(tri.shape[0])] == golden["import"][name]


def test_import_of_the_generated_benchmark_mesh(golden, tmp_path):
    """the refined bunny of the benchmark, written as an OBJ with nine significant digits and read back by the reference's importer: the floats
    the product voxelizes are the floats the reference would read"""
    path = str(tmp_path / "bunny_x3.obj")
    xyz, tri = _write_bunny_x3(path)
    assert [O.fnv(xyz), O.fnv(tri.astype(np.uint32))] == golden["import_bunny_x3"]
    mx, mt = M.import_mesh(path)
    assert [O.fnv(mx), O.fnv(mt)] == golden["import_bunny_x3"]


@pytest.mark.parametrize("names,n", FRAMES)
def test_frame_is_the_references_frame(golden, names, n):
    """origin = minima of the bounding box of ALL meshes, voxel size = its longest side / n (apps/cli/main.cpp:65-87; bounding_box.h:22-61 with
    its else-if): the reference's code, the oracle's restatement and the harness's mesh.frame give the same four floats"""
    want = golden["frame"]["%s@%d" % ("+".join(names), n)]
    meshes = [M.import_mesh(M.asset(a))[0] for a in names]
    for o, v in (O.frame(meshes, n), M.frame(meshes, n)):
        assert _bits(o) + _bits(v) == want


@pytest.mark.parametrize("op", CSG_OPS)
def test_csg_is_the_references_csg(golden, op):
    """CSG::Compute<SEQUENTIAL> of the reference on the two grids of the golden table's bimba / bunny rows at n = 64: equal to the oracle word
    for word, and its hash IS the golden row's (tests/golden/survey_table.json) -- the table's CSG column re-derived from the reference itself"""
    n = 64
    ref_grid, ref_noise = golden["csg"][str(op)]
    a, b = _grids(n)
    want = a.copy()
    O.csg(want, b.copy(), op)
    assert O.fnv(want) == ref_grid
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "survey_table.json")))["rows"]
    row = [r for r in rows if r["meshes"] == ["bimba.obj", "bunny.obj"] and r["n"] == n and r["op"] == op][0]
    assert [int(np.unpackbits(want.view(np.uint8)).sum()), O.fnv(want)] == row["csg"][:2]
    x, y = _noise(op, 32)                                            # and on noise (every word pattern)
    O.csg(x, y, op)
    assert O.fnv(x) == ref_noise


@pytest.mark.parametrize("name,n", EXPORTS)
def test_oracle_exporters_are_the_references_exporters(golden, name, n):
    """oracle/oracle_export.c (the restatements the GPU-side tests use) against the files the reference's own exporters write: vertex lines
    `v x y z r g b` and face lines `f a//n b//n c//n`, all three exports"""
    xyz, tri = M.import_mesh(M.asset(name))
    origin, vs = O.frame([xyz], n)
    words = O.voxelize(xyz, tri, n, vs, origin)
    sdf = O.jfa(words, n, vs, origin)
    fmt = lambda a: [["%.6f" % float(x) for x in row] for row in a]
    col = lambda rgb: [["%.6f" % float(np.float32(x) / np.float32(255.0)) for x in row] for row in rgb]
    idx = lambda a: np.asarray(a, np.uint32).reshape(-1, 3).tolist()
    co, fa, no = O.grid_to_mesh_compressed(words, n, vs, origin)
    comp = [fmt(co), [["1.000000"] * 3 for _ in range(len(co))], idx(fa), idx(no)]
    co, rgb, fa, no = O.grid_to_mesh_cubes(words, sdf, n, vs, origin)
    cubes = [fmt(co), col(rgb), idx(fa), idx(no)]
    co, rgb = O.grid_to_point_cloud(words, sdf, n, vs, origin)
    points = [fmt(co), col(rgb), [], []]
    assert [_digest(comp), _digest(cubes), _digest(points)] == golden["exports"]["%s@%d" % (name, n)]


@pytest.mark.parametrize("t,typename", CLI_TYPES)
@pytest.mark.parametrize("name,n", CLI_EXPORTS)
def test_cli_exports_are_the_references_files(golden, cli, tmp_path, name, n, t, typename):
    """`vpcli <mesh> -n n -t 0|3 -s -e` against the reference's exporters run on the product's grid and sdf (the -d dump): every line of the
    three OBJ files but the comment header"""
    out, _, _ = _cli_dump(cli, tmp_path, name, n, t)
    got = [_digest(_body(out / ("%s_%s" % (typename, name)))), _digest(_body(out / ("sdf_%s_out.obj" % typename))),
           _digest(_body(out / ("sdf_point_cloud_%s_out.obj" % typename)))]
    assert got == golden["cli_exports"]["%s@%d" % (name, n)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", GPU_EXPORTS)
def test_cli_gpu_exports_are_the_references_files(golden, cli, tmp_path, name, n):
    """-t 2: grid from the HIP voxelizer, sdf from the HIP JFA, the walk over the grid from vp_extract -- the three files against the reference's
    exporters run on the grid and sdf of the CPU path (which the GPU path equals bit for bit)"""
    out, _, _ = _cli_dump(cli, tmp_path, name, n, 2)
    got = [_digest(_body(out / ("tiled_%s" % name))), _digest(_body(out / "sdf_tiled_out.obj")), _digest(_body(out / "sdf_point_cloud_tiled_out.obj"))]
    assert got == golden["cli_exports"]["%s@%d" % (name, n)]


@pytest.mark.gpu
@pytest.mark.parametrize("op", CSG_OPS)
def test_gpu_csg_is_the_references_csg(golden, engine, op):
    """vp_csg (csg_words) against CSG::Compute<SEQUENTIAL> of the reference on noise"""
    a, b = _noise(10 + op, 64)
    da, db = engine.to_device(a, np.uint32), engine.to_device(b, np.uint32)
    engine.csg(da, db, op)
    engine.sync()
    assert O.fnv(engine.words_to_numpy(da)) == golden["gpu_csg"][str(op)]


# ---------------------------------------------------------------------------------------------- header-level functions of the mirror
@pytest.fixture(scope="module")
def host_api_check(tmp_path_factory):
    """tests/cpp/host_api_check.cpp: the same commands answered by THIS repository's vplib mirror"""
    exe = str(tmp_path_factory.mktemp("cpp") / "host_api_check")
    pkg = os.path.join(ROOT, "cuda_mesh_voxelization_amd")
    build.build_lib()
    srcs = [os.path.join(pkg, "vplib", "src", f) for f in sorted(os.listdir(os.path.join(pkg, "vplib", "src"))) if f.endswith(".cpp")]
    subprocess.check_call(["g++", "-std=c++23", "-O2", "-ffp-contract=off", "-fopenmp", "-I", os.path.join(pkg, "vplib", "include"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "host_api_check.cpp")] + srcs + ["-o", exe, "-L", pkg, "-lvphip", "-Wl,-rpath," + pkg])
    return exe


def _pairs(seed, m=20000):
    """pairs of positions as the JFA sees them: grid corners o + i vs of random frames (incl. far origins: cancellation), and free floats"""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    o = ((rng.random(3) - 0.5) * 200).astype(f32)
    vs = f32(10.0 ** rng.uniform(-3, 0))
    i, j = rng.integers(0, 2048, (m, 3)), rng.integers(0, 2048, (m, 3))
    grid = np.concatenate([o + i.astype(f32) * vs, o + j.astype(f32) * vs], 1).astype(f32)
    free = ((rng.random((m, 6)) - 0.5) * 10.0 ** rng.uniform(-3, 3, (m, 1))).astype(f32)
    return np.concatenate([grid, free], 0)


def test_distance_and_vector_ops_are_the_references(golden, tmp_path, host_api_check):
    """JFA::CalculateDistance (jfa/jfa.h:19-20) and Vec3::Cross / Dot (mesh/mesh.h:114-126): the reference's header functions, this
    repository's mirror and the float32 expression the numpy test backend uses -- bit for bit on 40,000 pairs (grid corners of random
    frames, where the subtraction cancels, and free floats over six decades)"""
    p = _pairs(7)
    p.tofile(str(tmp_path / "pairs.f32"))
    for (cmd, width), want in zip((("distance", 1), ("vec", 4)), golden["vector_ops"]):
        subprocess.check_call([host_api_check, cmd, str(tmp_path / "pairs.f32"), str(tmp_path / ("own_%s.f32" % cmd))])
        own = np.fromfile(str(tmp_path / ("own_%s.f32" % cmd)), np.float32)
        assert own.size == p.shape[0] * width and O.fnv(own) == want, cmd
    a, b = p[:, :3], p[:, 3:]
    d = b - a
    want = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])                   # float32 throughout, no contraction
    assert O.fnv(want.astype(np.float32)) == golden["vector_ops"][0]


def test_helpers_timer_grammar_and_assert_line_are_the_references(golden, host_api_check):
    """GetTypesString / NextPow2 / GetFilename (proc_utils.h:11-40); the `[Label]: <ms> ms` line of a Profiling scope (profiling.h:8-26: what
    scripts/benchmarks.py parses); the `[file:line] CPU Assert: message` line and exit code of cpuAssert (debug_utils.h:52-64)"""
    import re
    ref = golden["helpers"]
    assert ref["misc"] == subprocess.run([host_api_check] + MISC_ARGS, capture_output=True, text=True).stdout
    line = re.compile(r"^\[TiledJFA::Processing\]: \d+\.\d{6} ms\n$")
    assert line.match(ref["profile"])
    assert line.match(subprocess.run([host_api_check, "profile", "TiledJFA::Processing"], capture_output=True, text=True).stdout)
    m = subprocess.run([host_api_check, "assert", ASSERT_MSG], capture_output=True, text=True)
    shape = re.compile(r"^\[[^\]:]+:\d+\] CPU Assert: Number of GPUs must be 1\.\.64$")
    assert ref["assert_rc"] == m.returncode == 255 and shape.match(ref["assert_stdout"]) and shape.match(m.stdout)
