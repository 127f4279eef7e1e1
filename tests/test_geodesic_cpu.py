"""Geodesic distance without a GPU: the numpy restatement of tests/geodesic_ref.py against scipy's Dijkstra on the explicit graph, against
the closed forms on the full grid and against scipy.ndimage.label for the reach grid; the host restatement of vplib/src/geodesic.cpp
through the C++ API on both word types, on every case of the GPU tests, and through `vpcli --geodesic`, byte for byte and statistics
included; the refusals of the CLI; the header's prototypes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.ndimage
import scipy.sparse
import scipy.sparse.csgraph

from cuda_mesh_voxelization_amd import build, capi, mesh as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geodesic_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference itself ----------------------------------------------------------------------------------------------------------
def dijkstra(mask, seeds, metric):
    """D by scipy on the explicit graph: one directed edge per allowed step between two voxels of the mask"""
    n = mask.shape[0]
    idx = np.arange(n ** 3).reshape(n, n, n)
    rows, cols, vals = [], [], []
    for (dx, dy, dz), w in R.steps(metric):
        src = tuple(slice(max(0, -d), n - max(0, d)) for d in (dz, dy, dx))
        dst = tuple(slice(max(0, d), n - max(0, -d)) for d in (dz, dy, dx))
        both = mask[src] & mask[dst]
        rows.append(idx[src][both])
        cols.append(idx[dst][both])
        vals.append(np.full(int(both.sum()), w, np.float64))
    g = scipy.sparse.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n ** 3, n ** 3))
    used = np.flatnonzero((seeds & mask).reshape(-1))
    d = scipy.sparse.csgraph.dijkstra(g, directed=True, indices=used, min_only=True)
    out = np.full(n ** 3, R.NONE, np.uint32)
    out[np.isfinite(d)] = d[np.isfinite(d)].astype(np.uint32)
    return out.reshape(n, n, n)


@pytest.mark.parametrize("metric", R.METRICS)
def test_reference_equals_dijkstra(metric):
    mask = R.random_grid(32, 0.6, 1)
    seeds = R.random_grid(32, 0.0005, 2)
    assert 5 <= int((seeds & mask).sum()) <= 20
    d, reach, stats = R.geodesic(mask, seeds, metric)
    assert np.array_equal(d, dijkstra(mask, seeds, metric))
    assert stats[0] == int((seeds & mask).sum()) and stats[1] == int(reach.sum())
    assert (d[~mask] == R.NONE).all() and (d[seeds & mask] == 0).all()


@pytest.mark.parametrize("metric", R.METRICS)
def test_reference_on_a_sparse_mask_leaves_voxels_unreached(metric):
    mask, seeds = R.case("random sparse")
    assert (seeds & mask).any()
    d, reach, stats = R.expected("random sparse", metric)
    assert np.array_equal(d, dijkstra(mask, seeds, metric))
    assert (d[mask] == R.NONE).any() and 0 < stats[1] < int(mask.sum())


@pytest.mark.parametrize("metric", R.METRICS)
def test_closed_form_on_the_full_grid(metric):
    for corner in (0, 1):
        d, reach, stats = R.expected("full 32 %d" % corner, metric)
        assert np.array_equal(d, R.closed_form(32, metric, corner))
        top = {R.GEO_6: 93, R.GEO_26: 31, R.GEO_CHAMFER: 155}[metric]
        assert stats[:3] == (1, 32768, top) and reach.all()
    # the farthest voxel is the opposite corner for the metrics with one; GEO_26 reads 31 on three whole faces, the lowest index wins
    assert R.expected("full 32 0", metric)[2][3] == (31 if metric == R.GEO_26 else 32767)
    assert R.expected("full 32 1", metric)[2][3] == 0


def test_serpentine_values():
    for n in (32, 64):
        for metric in R.METRICS:
            stats = R.expected("serpentine %d" % n, metric)[2]
            assert stats[:3] == (1, R.SERPENTINE_VOXELS[n], R.SERPENTINE_MAX[n][metric])


def label_reach(mask, seeds, metric):
    """the union of the components of the mask that hold a used seed"""
    structure = scipy.ndimage.generate_binary_structure(3, 1 if metric == R.GEO_6 else 3)
    labels, _ = scipy.ndimage.label(mask, structure)
    hit = np.unique(labels[seeds & mask])
    return np.isin(labels, hit[hit != 0])


@pytest.mark.parametrize("metric", R.METRICS)
def test_reach_is_the_components_that_touch_a_seed(metric):
    a, b = R.two_balls()
    assert scipy.ndimage.label(a | b, scipy.ndimage.generate_binary_structure(3, 1))[1] == 2
    for name in ("two balls", "random sparse", "contact corner", "seeds partly inside"):
        mask, seeds = R.case(name)
        assert np.array_equal(R.expected(name, metric)[1], label_reach(mask, seeds, metric)), name
    assert np.array_equal(R.expected("two balls", R.GEO_6)[1], a)


def test_seeds_and_emptiness():
    for metric in R.METRICS:
        d, reach, stats = R.expected("seeds outside", metric)
        assert stats == (0, 0, 0, 0) and not reach.any() and (d == R.NONE).all()
        mask, _ = R.case("seeds equal mask")
        d, reach, stats = R.expected("seeds equal mask", metric)
        assert (d[mask] == 0).all() and np.array_equal(reach, mask)
        assert stats == (int(mask.sum()), int(mask.sum()), 0, int(np.flatnonzero(mask.reshape(-1))[0]))


# ---- the C++ host form ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    pkg = os.path.dirname(capi.LIB_PATH)
    build.build_lib()
    srcs = [os.path.join(pkg, "vplib", "src", f) for f in sorted(os.listdir(os.path.join(pkg, "vplib", "src"))) if f.endswith(".cpp")]
    exe = str(tmp_path_factory.mktemp("geodesic") / "geodesic_check")
    subprocess.check_call(["g++", "-std=c++23", "-O2", "-ffp-contract=off", "-fopenmp",
                           "-I", os.path.join(pkg, "vplib", "include"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "geodesic_check.cpp")] + srcs + ["-o", exe, "-L", pkg, "-lvphip", "-Wl,-rpath," + pkg])
    return exe


def run_check(exe, mask, seeds, metric, bits, types, prefix, timeout=900):
    """{tag: (D uint32[n^3], reach words, statistics)} of tests/cpp/geodesic_check.cpp run on two (z, y, x) bool grids"""
    n = mask.shape[0]
    R.bool_to_words(mask).tofile(prefix + ".mask.u32")
    R.bool_to_words(seeds).tofile(prefix + ".seeds.u32")
    p = subprocess.run([exe, prefix + ".mask.u32", prefix + ".seeds.u32", str(n), str(metric), str(bits), types, prefix], check=True,
                       timeout=timeout, capture_output=True, text=True)
    stats = {t: tuple(int(v) for v in rest.split()) for t, rest in re.findall(r"^(seq|omp|naive|tiled) (\d+ \d+ \d+ \d+)$", p.stdout, re.M)}
    tags = {"s": "seq", "o": "omp", "n": "naive", "t": "tiled"}
    return {tags[c]: (np.fromfile("%s.%s.geo.u32" % (prefix, tags[c]), np.uint32), np.fromfile("%s.%s.reach.u32" % (prefix, tags[c]), np.uint32),
                      stats[tags[c]]) for c in types}


@pytest.mark.parametrize("metric", R.METRICS)
def test_host_form_equals_numpy(check_exe, tmp_path, metric):
    prefix = str(tmp_path / "h")
    for k, name in enumerate(R.CASES):
        mask, seeds = R.case(name)
        d, reach, stats = R.expected(name, metric)
        got = run_check(check_exe, mask, seeds, metric, 64 if k % 2 else 32, "so", prefix)
        for tag in ("seq", "omp"):
            assert np.array_equal(got[tag][0], d.reshape(-1)), (name, tag)
            assert np.array_equal(got[tag][1], R.bool_to_words(reach)), (name, tag)
            assert got[tag][2] == stats, (name, tag, got[tag][2], stats)


# ---- the CLI -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    return build.build_cli()


def cli_line(stats, n, total):
    i = stats[3]
    return "geodesic: n %d, seeds %d, reached %d of %d set, max %d at (%d, %d, %d)" % (n, stats[0], stats[1], total, stats[2], i % n, i // n % n, i // (n * n))


def cli_seeds(vox, arg):
    """the seed grid that SEED of --geodesic names on the dumped grid"""
    if arg == "zmin":
        return R.lowest_plane(vox)
    if arg == "zmax":
        return R.highest_plane(vox)
    x, y, z = (int(v) for v in arg.split(","))
    return R.voxel(vox.shape[0], x, y, z)


def first_set_voxel(cli, mesh, n, tmp_path):
    """"X,Y,Z" of a set voxel of what `vpcli mesh -n n -t 0` voxelizes"""
    p = subprocess.run([cli, mesh, "-n", str(n), "-t", "0", "-d", str(tmp_path / "probe")], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    vox = R.words_to_bool(np.fromfile(str(tmp_path / "probe.grid.u32"), np.uint32), n)
    z, y, x = np.argwhere(vox)[len(np.argwhere(vox)) // 2]
    return "%d,%d,%d" % (x, y, z), vox


def seam_box_obj(tmp_path):
    """path of an OBJ whose solid grid at n = 32 has its lowest occupied plane at z = 15, just under a block seam: a box from z = 0.475 to
    0.9 of a unit frame, and at the origin a closed box too small to hold a voxel centre, which only stretches the frame down to z = 0"""
    def box(lo, hi, first):
        v = ["v %r %r %r" % ((hi if k & 1 else lo)[0], (hi if k & 2 else lo)[1], (hi if k & 4 else lo)[2]) for k in range(8)]
        tris = ((1, 3, 4), (1, 4, 2), (5, 6, 8), (5, 8, 7), (1, 2, 6), (1, 6, 5), (3, 7, 8), (3, 8, 4), (1, 5, 7), (1, 7, 3), (2, 4, 8), (2, 8, 6))
        return v, ["f %d %d %d" % tuple(first + i for i in t) for t in tris]
    v1, f1 = box((0.0, 0.0, 0.0), (0.001, 0.001, 0.001), 0)
    v2, f2 = box((0.1, 0.1, 0.475), (1.0, 0.9, 0.9), 8)
    path = str(tmp_path / "seam_box.obj")
    with open(path, "w") as f:
        f.write("\n".join(v1 + v2 + f1 + f2) + "\n")
    return path


def test_cli_zmin_plane_under_a_block_seam(cli, tmp_path):
    mesh = seam_box_obj(tmp_path)
    for t in ("0", "3"):
        d = tmp_path / ("t" + t)
        d.mkdir()
        p = subprocess.run([cli, mesh, "-n", "32", "-t", t, "--geodesic", "zmin:6", "-d", str(d / "x")], capture_output=True, text=True, timeout=600, cwd=str(d))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        vox = R.words_to_bool(np.fromfile(str(d / "x.grid.u32"), np.uint32), 32)
        assert int(np.flatnonzero(vox.any(axis=(1, 2)))[0]) == 15 and vox[16].any()
        exp, reach, stats = R.geodesic(vox, R.lowest_plane(vox), R.GEO_6)
        assert np.array_equal(np.fromfile(str(d / "x.geo.u32"), np.uint32), exp.reshape(-1))
        assert cli_line(stats, 32, int(vox.sum())) + "\n" in p.stdout and stats[1] == int(vox.sum()) > stats[0]


def test_cli_cpu_types_equal_numpy(cli, tmp_path):
    voxel, _ = first_set_voxel(cli, M.asset("d20.obj"), 32, tmp_path)
    for k, (t, mesh, n, seed, metric) in enumerate((("0", "d20.obj", 32, "zmin", None), ("3", "d20.obj", 32, voxel, "6"), ("0", "bunny.obj", 64, "zmax", "26"),
                                                    ("3", "bunny.obj", 64, "zmin", "chamfer"), ("3", "d20.obj", 64, "zmax", "chamfer"),
                                                    ("0", "d20.obj", 64, "zmin", "26"), ("0", "bunny.obj", 32, "zmin", "6"),
                                                    ("3", "bunny.obj", 32, "zmax", None))):
        d = tmp_path / ("run%d" % k)
        d.mkdir()
        arg = seed if metric is None else seed + ":" + metric
        p = subprocess.run([cli, M.asset(mesh), "-n", str(n), "-t", t, "--geodesic", arg, "-d", str(d / "x")],
                           capture_output=True, text=True, timeout=600, cwd=str(d))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        vox = R.words_to_bool(np.fromfile(str(d / "x.grid.u32"), np.uint32), n)
        code = {None: R.GEO_CHAMFER, "6": R.GEO_6, "26": R.GEO_26, "chamfer": R.GEO_CHAMFER}[metric]
        exp, reach, stats = R.geodesic(vox, cli_seeds(vox, seed), code)
        assert stats[1] > stats[0] > 0
        assert np.array_equal(np.fromfile(str(d / "x.geo.u32"), np.uint32), exp.reshape(-1))
        assert np.array_equal(np.fromfile(str(d / "x.reach.u32"), np.uint32), R.bool_to_words(reach))
        assert cli_line(stats, n, int(vox.sum())) + "\n" in p.stdout, p.stdout
        assert re.search(r"^\[\w*Geodesic\]: [0-9.]+ ms$", p.stdout, re.M), p.stdout


def test_cli_runs_on_the_final_grid(cli, tmp_path):
    """after --skeleton-only the distance is measured along the centre line"""
    p = subprocess.run([cli, M.asset("torus.obj"), "-n", "64", "-t", "0", "--skeleton", "curve", "--skeleton-only", "--geodesic", "zmin:26",
                        "-d", str(tmp_path / "x")], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    vox = R.words_to_bool(np.fromfile(str(tmp_path / "x.grid.u32"), np.uint32), 64)
    assert np.array_equal(np.fromfile(str(tmp_path / "x.grid.u32"), np.uint32), np.fromfile(str(tmp_path / "x.skel.u32"), np.uint32))
    exp, reach, stats = R.geodesic(vox, R.lowest_plane(vox), R.GEO_26)
    assert np.array_equal(np.fromfile(str(tmp_path / "x.geo.u32"), np.uint32), exp.reshape(-1))
    assert cli_line(stats, 64, int(vox.sum())) + "\n" in p.stdout and stats[1] == int(vox.sum())


def test_cli_refuses_bad_geodesic_arguments(cli, tmp_path):
    mesh = M.asset("d20.obj")
    voxel, vox = first_set_voxel(cli, mesh, 32, tmp_path)
    z, y, x = np.argwhere(~vox)[0]
    for args in (["--geodesic", "zmin", "-g", "2"], ["--geodesic", "ymin"], ["--geodesic", "zmin:8"], ["--geodesic", "zmin:"], ["--geodesic", ":26"],
                 ["--geodesic", "1,2"], ["--geodesic", "1,2,3,4"], ["--geodesic", "1,,3"], ["--geodesic", "32,0,0"], ["--geodesic", "0,0,99:6"],
                 ["--geodesic", "%d,%d,%d" % (x, y, z)], ["--geodesic"]):
        p = subprocess.run([cli, mesh, "-n", "32", "-t", "0"] + args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert p.returncode != 0, args
    p = subprocess.run([cli, mesh, "-n", "32", "-t", "0", "--geodesic", voxel + ":6"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode == 0 and "geodesic: n 32, seeds 1, " in p.stdout


def test_cli_help_names_the_flag(cli, tmp_path):
    p = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert "--geodesic" in p.stdout + p.stderr
    with open(os.path.join(os.path.dirname(capi.LIB_PATH), "apps", "cli", "main.cpp")) as f:
        assert "--geodesic S[:M]" in f.read()


# ---- the header ----------------------------------------------------------------------------------------------------------------------
def test_prototypes_and_sources():
    with open(os.path.join(ROOT, "include", "vphip.h")) as f:
        header = f.read()
    for proto in ("int vp_geodesic(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_mask, const uint32_t* d_seeds, int metric, int algo,",
                  "int vp_geodesic_result(vp_ctx* ctx, uint32_t** d_dist, uint32_t** d_reach, uint64_t* h_stats",
                  "int vp_geodesic_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_mask, const uint32_t* h_seeds, int metric, int algo,",
                  "enum { VP_GEO_6 = 0, VP_GEO_26 = 1, VP_GEO_CHAMFER = 2 };", "#define VP_GEO_NONE 0xFFFFFFFFu", "#define VP_GEO_MAX 0xFFFFFFFEu",
                  "#define VP_ABI_VERSION 6"):
        assert proto in header, proto
    assert "geodesic.hip" in build.HIP_SOURCES
    assert {"vp_geodesic", "vp_geodesic_result", "vp_geodesic_host"} <= set(capi.SYMBOLS)
    assert (capi.GEO_6, capi.GEO_26, capi.GEO_CHAMFER, capi.GEO_NONE) == (0, 1, 2, 0xFFFFFFFF)
    assert len(capi.HEADER_PROF_KEYS) == 64
