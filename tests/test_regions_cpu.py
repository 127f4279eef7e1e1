"""Region analysis without a GPU: the numpy restatement of tests/regions_ref.py against scipy.ndimage, against the Euler characteristic of
tests/skeleton_ref.py and on the hand cases of the issue; the host restatement of vplib/src/regions.cpp through the C++ API on every case of
the GPU tests, byte for byte and totals included; `vpcli --regions`; capi.region_table against numpy; the header's phrases."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cuda_mesh_voxelization_amd import build, capi, mesh as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_ref  # noqa: E402
import edt_ref  # noqa: E402
import regions_ref as R  # noqa: E402
import skeleton_ref  # noqa: E402
from fill_ref import words_to_bool  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference itself ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("random5", "sparse300", "blobs"))
def test_reference_against_scipy(name):
    from scipy import ndimage
    W, K = R.case(name)
    values = R.values_of(name)
    T, stats = R.expected(name, True)
    L = np.where(W <= K, W, 0).astype(np.int64)
    index = np.arange(1, K + 1)
    some = T[:, 0] > 0
    assert np.array_equal(T[:, 0], ndimage.sum(np.ones(L.shape, np.int64), L, index).astype(np.uint64))
    v = values.astype(np.float64)                                   # exact here: per-label sums stay below 2^53
    assert np.array_equal(T[:, 22][some], ndimage.sum(v, L, index)[some].astype(np.uint64))
    assert np.array_equal(T[:, 23][some], ndimage.minimum(v, L, index)[some].astype(np.uint64))
    assert np.array_equal(T[:, 24][some], ndimage.maximum(v, L, index)[some].astype(np.uint64))
    boxes = ndimage.find_objects(L, K)
    centres = ndimage.center_of_mass(np.ones(L.shape), L, index)
    for k in range(K):
        if not some[k]:
            assert boxes[k] is None and not T[k].any()
            continue
        sz, sy, sx = boxes[k]
        assert tuple(int(t) for t in T[k, 1:7]) == (sx.start, sy.start, sz.start, sx.stop - 1, sy.stop - 1, sz.stop - 1)
        cz, cy, cx = centres[k]
        assert np.allclose(T[k, 7:10].astype(np.float64) / float(T[k, 0]), (cx, cy, cz), rtol=1e-12, atol=1e-12)
        assert int(T[k, 25]) == int(np.flatnonzero(L.reshape(-1) == k + 1)[0])
    assert stats == (int((L != 0).sum()), int(some.sum()), int((W > K).sum()), int(T[:, 19].sum()) // 2)


def test_second_moments_and_faces_by_hand():
    W, K = R.case("random5")
    T, _ = R.expected("random5", False)
    z, y, x = np.indices(W.shape)
    P = np.pad(np.where(W <= K, W, 0), 1)
    for k in (1, 4):
        m = W == k
        sums = [int((a[m] * b[m]).sum()) for a, b in ((x, x), (y, y), (z, z), (x, y), (x, z), (y, z))]
        assert [int(t) for t in T[k - 1, 10:16]] == sums
        faces, contact = [0, 0, 0], 0
        for vz, vy, vx in zip(*np.nonzero(m)):
            for a, (dx, dy, dz) in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
                for s in (-1, 1):
                    other = P[vz + 1 + s * dz, vy + 1 + s * dy, vx + 1 + s * dx]
                    faces[a] += other != k
                    contact += other != k and other != 0
        assert [int(t) for t in T[k - 1, 16:20]] == faces + [contact]
        assert not T[k - 1, 22:25].any()                            # no value field: 0, 0, 0


@pytest.mark.parametrize("name", ("blobs", "random5", "seams", "faces"))
def test_euler_numbers_of_a_26_labelling_add_up(name):
    W, K = R.case(name)
    vox = (W >= 1) & (W <= K)
    labels, count = components_ref.label_bool(vox, 26)
    T, stats = R.regions(labels, count)
    assert int(R.euler(T).sum()) == skeleton_ref.euler(vox) and stats[3] == 0 and stats[1] == count


def test_ball_shell_torus():
    for name, chi in (("ball", 1), ("shell", 2), ("torus", 0)):
        T, stats = R.expected(name, False)
        assert int(R.euler(T)[0]) == chi and stats[1] == 1 and stats[2] == stats[3] == 0, name


def test_halves_of_a_ball():
    T, stats = R.expected("halves", False)
    assert T[0, 19] == T[1, 19] > 0 and T[0, 0] == T[1, 0] and stats[3] == int(T[0, 19])
    assert list(R.euler(T)) == [1, 1]
    assert int(T[0, 4]) == 15 and int(T[1, 1]) == 16


def test_single_voxel_anywhere():
    for name, at in (("voxel", (7, 9, 11)), ("corner_voxel", (0, 0, 0)), ("far_corner_voxel", (31, 31, 31))):
        T, stats = R.expected(name, False)
        x, y, z = at
        assert [int(t) for t in T[0]] == [1, x, y, z, x, y, z, x, y, z, x * x, y * y, z * z, x * y, x * z, y * z, 2, 2, 2, 0, 8, 12, 0, 0, 0,
                                          x + 32 * (y + 32 * z)]
        assert int(R.euler(T)[0]) == 1 and stats == (1, 1, 0, 0)


def test_ignored_labels_and_empty_inputs():
    T, stats = R.expected("above", False)
    assert not T.any() and stats == (0, 0, 32 ** 3, 0)
    T, stats = R.expected("empty", True)
    assert T.shape == (4, 26) and not T.any() and stats == (0, 0, 0, 0)
    T, stats = R.expected("count0", False)
    W, _ = R.case("count0")
    assert T.shape == (0, 26) and stats == (0, 0, int((W > 0).sum()), 0)
    T, stats = R.expected("whole96", True)
    assert int(T[0, 22]) == 96 ** 3 * 0xFFFFFFFF > 2 ** 51 and int(T[0, 20]) == 97 ** 3 and int(R.euler(T)[0]) == 1


# ---- the C++ host form -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    pkg = os.path.dirname(capi.LIB_PATH)
    build.build_lib()
    srcs = [os.path.join(pkg, "vplib", "src", f) for f in sorted(os.listdir(os.path.join(pkg, "vplib", "src"))) if f.endswith(".cpp")]
    exe = str(tmp_path_factory.mktemp("regions") / "regions_check")
    subprocess.check_call(["g++", "-std=c++23", "-O2", "-ffp-contract=off", "-fopenmp",
                           "-I", os.path.join(pkg, "vplib", "include"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "regions_check.cpp")] + srcs + ["-o", exe, "-L", pkg, "-lvphip", "-Wl,-rpath," + pkg])
    return exe


def run_check(exe, W, K, values, types, prefix, timeout=900):
    """the finished process and {tag: (table uint64 (K, 26), (totals, sum of the Euler numbers))} of tests/cpp/regions_check.cpp"""
    np.ascontiguousarray(W, np.uint32).tofile(prefix + ".labels.u32")
    if values is not None:
        np.ascontiguousarray(values, np.uint32).tofile(prefix + ".values.u32")
    p = subprocess.run([exe, prefix + ".labels.u32", "-" if values is None else prefix + ".values.u32", str(W.shape[0]), str(K), types, prefix],
                       timeout=timeout, capture_output=True, text=True)
    if p.returncode != 0:
        return p, {}
    lines = {t: tuple(int(v) for v in rest.split()) for t, rest in re.findall(r"^(seq|omp|naive|tiled) (\d+ \d+ \d+ \d+ -?\d+)$", p.stdout, re.M)}
    tags = {"s": "seq", "o": "omp", "n": "naive", "t": "tiled"}
    return p, {tags[c]: (np.fromfile("%s.%s.table.u64" % (prefix, tags[c]), np.uint64).reshape(-1, 26), lines[tags[c]]) for c in types}


@pytest.mark.parametrize("with_values", (False, True))
def test_host_form_equals_numpy(check_exe, tmp_path, with_values):
    prefix = str(tmp_path / "h")
    for name in R.CASES:
        W, K = R.case(name)
        T, stats = R.expected(name, with_values)
        p, got = run_check(check_exe, W, K, R.values_of(name) if with_values else None, "so", prefix)
        assert p.returncode == 0, (name, p.stdout[-500:] + p.stderr[-500:])
        for tag in ("seq", "omp"):
            assert got[tag][0].shape == T.shape and np.array_equal(got[tag][0], T), (name, tag, np.argwhere(got[tag][0] != T)[:5])
            assert got[tag][1] == stats + (int(R.euler(T).sum()),), (name, tag, got[tag][1], stats)


def test_host_form_on_an_odd_side_and_its_bound(check_exe, tmp_path):
    rng = np.random.default_rng(11)
    W = rng.integers(0, 6, (21, 21, 21), dtype=np.uint32)
    T, stats = R.regions(W, 4)
    p, got = run_check(check_exe, W, 4, None, "so", str(tmp_path / "odd"))
    assert p.returncode == 0 and np.array_equal(got["seq"][0], T) and np.array_equal(got["omp"][0], T) and got["seq"][1][:4] == stats
    p, _ = run_check(check_exe, W, R.REGIONS_MAX + 1, None, "s", str(tmp_path / "odd"))
    assert p.returncode != 0


# ---- the CLI -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    return build.build_cli()


def cli_run(cli, tmp_path, tag, mesh, n, t, args):
    """(stdout, the dumped grid as bool, the dumped table or None, the folder) of one run in a folder of its own"""
    d = tmp_path / tag
    d.mkdir()
    p = subprocess.run([cli, M.asset(mesh), "-n", str(n), "-t", t, "-d", str(d / "x")] + args, capture_output=True, text=True, timeout=600, cwd=str(d))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    table = str(d / "x.regions.u64")
    return (p.stdout, words_to_bool(np.fromfile(str(d / "x.grid.u32"), np.uint32), n),
            np.fromfile(table, np.uint64).reshape(-1, 26) if os.path.exists(table) else None, d)


def cli_check(out, vox, table, csv_path, conn, n):
    """the table, the CSV's integer columns and the printed line against the reference for the grid the run measured"""
    labels, count = components_ref.label_bool(vox, conn)
    d2 = edt_ref.edt_numpy(vox, edt_ref.UNSET)
    T, stats = R.regions(labels, count, d2)
    assert np.array_equal(table, T)
    assert "regions: n %d, labels %d, voxels %d, non-empty %d, ignored %d, interfaces %d, " % ((n, count) + stats) in out, out
    with open(csv_path) as f:
        rows = f.read().strip().split("\n")
    assert rows[0].startswith("label,w0,w1,") and len(rows) == count + 1
    cells = [r.split(",") for r in rows[1:]]
    assert np.array_equal(np.array([[int(c) for c in r[1:27]] for r in cells], np.uint64).reshape(-1, 26), T)
    assert [int(r[0]) for r in cells] == list(range(1, count + 1))
    names = rows[0].split(",")
    assert [int(r[names.index("euler")]) for r in cells] == list(R.euler(T))
    return T, count


def test_cli_cpu_types_equal_numpy(cli, tmp_path):
    for k, (t, mesh, args, conn) in enumerate((("0", "bunny.obj", ["--regions"], 26), ("3", "bimba.obj", ["--regions", "6"], 6),
                                               ("0", "bunny.obj", ["--watershed", "2", "--regions=6"], 6))):
        out, vox, table, d = cli_run(cli, tmp_path, "r%d" % k, mesh, 64, t, args + ["-o", "thing.obj"])
        name = "sequential" if t == "0" else "openmp"
        T, count = cli_check(out, vox, table, str(d / "out" / ("thing_%s_regions.csv" % name)), conn, 64)
        assert count >= (4 if k == 2 else 1)                            # the separated parts of the watershed are measured one by one
        assert int(T[:, 24].max()) > 4                                  # the squared radius of the largest inscribed ball


def test_cli_refuses_bad_regions_arguments(cli, tmp_path):
    mesh = M.asset("d20.obj")
    for args in (["--regions", "-g", "2"], ["--regions=8"], ["--regions="]):
        p = subprocess.run([cli, mesh, "-n", "32", "-t", "0"] + args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert p.returncode != 0, args
    p = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert "--regions" in p.stdout + p.stderr


# ---- the derived quantities ----------------------------------------------------------------------------------------------------------------
def test_region_table_against_numpy():
    fr = capi.Frame.make(64, 0.37, (-3.0, 5.5, 100.25))
    vs, origin = float(fr.voxel_size), np.array([fr.origin[0], fr.origin[1], fr.origin[2]], np.float64)
    W, K = R.case("blobs")
    T, _ = R.expected("blobs", True)
    values = R.values_of("blobs")
    rt = capi.region_table(T, fr)
    assert rt.shape == (K,) and list(rt["label"]) == list(range(1, K + 1))
    for k in range(K):
        zyx = np.argwhere(W == k + 1)
        pts = (zyx[:, ::-1] + 0.5) * vs + origin                     # the voxel centres, (x, y, z)
        r = rt[k]
        assert r["voxels"] == len(pts) and np.isclose(r["volume"], len(pts) * vs ** 3, rtol=1e-12)
        assert np.allclose(r["centroid"], pts.mean(0), rtol=1e-9, atol=0)
        assert np.allclose(r["box_min"], pts.min(0) - vs / 2, rtol=1e-9) and np.allclose(r["box_max"], pts.max(0) + vs / 2, rtol=1e-9)
        centred = pts - pts.mean(0)
        cov = centred.T @ centred / len(pts) + np.eye(3) * vs * vs / 12
        lam = np.linalg.eigvalsh(cov)
        assert np.allclose(r["eigenvalues"], lam, rtol=1e-9, atol=0)
        assert np.allclose(r["covariance"], cov, rtol=1e-9, atol=1e-9 * lam.max())
        assert np.allclose(r["radii"], np.sqrt(5 * lam), rtol=1e-9)
        faces = int(T[k, 16:19].sum())
        assert np.isclose(r["surface"], 2 / 3 * faces * vs * vs, rtol=1e-12) and np.isclose(r["contact_area"], int(T[k, 19]) * vs * vs, rtol=1e-12)
        assert np.isclose(r["sphericity"], np.pi ** (1 / 3) * (6 * r["volume"]) ** (2 / 3) / r["surface"], rtol=1e-12)
        assert r["euler"] == R.euler(T)[k]
        v = values[W == k + 1].astype(np.float64)
        assert np.isclose(r["value_mean"], v.mean(), rtol=1e-9) and r["value_min"] == v.min() and r["value_max"] == v.max()
        assert tuple(r["first"]) == tuple(zyx[0][::-1])
    # a ball in voxel units: the ellipsoid radii are its radius, the Crofton estimate is within a few per cent, the sphericity near 1
    ball = R.ball(64, (32, 31, 30), 20 * 20).astype(np.uint32)
    b = capi.region_table(R.regions(ball, 1)[0], capi.Frame.make(64, 1.0, (0, 0, 0)))[0]
    assert np.allclose(b["radii"], 20, rtol=0.01) and abs(b["surface"] / (4 * np.pi * 400) - 1) < 0.02 and abs(b["sphericity"] - 1) < 0.03
    # an empty label reads zero, nothing is NaN
    e = capi.region_table(np.zeros((2, 26), np.uint64), fr)
    assert not any(np.asarray(e[f]).any() for f in e.dtype.names if f != "label")
    assert capi.region_table(np.zeros((0, 26), np.uint64), fr).shape == (0,)


# ---- the header --------------------------------------------------------------------------------------------------------------------------
def test_prototypes_and_sources():
    with open(os.path.join(ROOT, "include", "vphip.h")) as f:
        header = f.read()
    for phrase in ("int vp_regions(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_labels, uint32_t count, const uint32_t* d_values",
                   "int vp_regions_result(vp_ctx* ctx, uint64_t** d_table, uint32_t* h_count, uint64_t* h_stats",
                   "int vp_regions_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_labels, uint32_t count, const uint32_t* h_values",
                   "#define VP_REGION_WORDS 26", "#define VP_REGIONS_MAX 0xFFFFFu", "#define VP_ABI_VERSION 6",
                   "A VOXEL OUTSIDE THE GRID HAS l = 0", "ALL-ZERO record", "chi = n0 - n1 + n2 - V", "sum x^2 <= 1023^2 * 2^30 < 2^51",
                   "the clear launch under VP_K_MD_FILL, the finishing launch under VP_K_MD_SPLIT, the TILED kernel", "VP_K_MD_BRICK, the NAIVE kernel under VP_K_MD_NAIVE"):
        assert phrase in header, phrase
    assert "regions.hip" in build.HIP_SOURCES
    assert {"vp_regions", "vp_regions_result", "vp_regions_host"} <= set(capi.SYMBOLS)
    assert (capi.REGION_WORDS, capi.REGIONS_MAX) == (R.WORDS, R.REGIONS_MAX) and capi.WS_LABEL_MAX == capi.REGIONS_MAX
    assert len(capi.HEADER_PROF_KEYS) == 64
    pkg = os.path.dirname(capi.LIB_PATH)
    with open(os.path.join(pkg, "csrc", "regions.hip")) as f:
        source = f.read()
    assert "2^51" in source and "2^62" in source and "fits 32 bits" in source      # the bounds are stated where the sums are made
