"""Connected components without a GPU: the numpy restatement of tests/components_ref.py against scipy.ndimage.label and against
hand-written expectations; the host restatement of `vpcli --morph largest / minsize` (-t 0 / -t 3, vplib/src/components.cpp) against the
numpy filter; the place of a filter step inside the list; the list parser; the C++ API on uint32_t and uint64_t grids."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cuda_mesh_voxelization_amd import build, capi, mesh as M
from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from components_ref import (KEEP_LARGEST, MIN_VOXELS, filter_labels, filter_numpy, hand_cases, keep_flags, label_bool, label_numpy,  # noqa: E402
                            sizes_of, structure)
from fill_ref import bool_to_words, fill_numpy, random_grid, words_to_bool  # noqa: E402
from test_conservative_cpu import cvox_numpy  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cli():
    return build.build_cli()


def test_constants_and_symbols_match_the_header():
    assert (capi.CONN_6, capi.CONN_26) == (6, 26)
    assert (capi.COMP_KEEP_LARGEST, capi.COMP_MIN_VOXELS) == (KEEP_LARGEST, MIN_VOXELS) == (0, 1)
    for s in ("vp_components_label", "vp_components_sizes", "vp_components_filter", "vp_components_label_host", "vp_components_filter_host"):
        assert s in capi.SYMBOLS
    header = open(os.path.join(ROOT, "include", "vphip.h")).read()
    enum = header[header.index("VP_K_VOX_SETUP = 0"):header.index("VP_K_COUNT")]
    keys = [t.split("=")[0].strip().lower()[len("vp_k_"):] for t in
            "".join(line.split("/*")[0] for line in enum.splitlines()).split(",") if t.strip()]
    assert len(keys) == len(capi.PROF_KEYS) and capi.PROF_KEYS == capi.KERNELS + capi.COMP_KERNELS
    assert keys[-len(capi.COMP_KERNELS):] == capi.COMP_KERNELS
    assert "VP_CONN_6 = 6, VP_CONN_26 = 26" in header and "VP_COMP_KEEP_LARGEST = 0, VP_COMP_MIN_VOXELS = 1" in header


def test_structures_are_scipys():
    ndimage = pytest.importorskip("scipy.ndimage")
    assert np.array_equal(structure(6), ndimage.generate_binary_structure(3, 1)) and structure(6).sum() == 7
    assert np.array_equal(structure(26), ndimage.generate_binary_structure(3, 3)) and structure(26).sum() == 27


@pytest.mark.parametrize("conn", [6, 26])
def test_label_numpy_equals_scipy_on_random_grids(conn):
    ndimage = pytest.importorskip("scipy.ndimage")
    for n, density, seed in ((32, 0.05, 1), (32, 0.10, 2), (32, 0.31, 3), (32, 0.5, 4), (64, 0.10, 5), (64, 0.20, 6), (64, 0.31, 7)):
        vox = words_to_bool(random_grid(n, density, seed), n)
        exp, k = ndimage.label(vox, structure(conn))
        plain, kp = label_bool(vox, conn)
        assert kp == k and np.array_equal(plain, exp.astype(np.uint32)), (n, density)
        jumped, kj = label_bool(vox, conn, jump=True)
        assert kj == k and np.array_equal(jumped, plain), (n, density)


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("n", [32, 64])
def test_reference_gets_the_hand_cases_right(n, conn):
    names = set()
    for name, vox, k, sizes in hand_cases(n, conn):
        names.add(name)
        labels, got = label_bool(vox, conn, jump=n > 32)
        assert got == k, (n, conn, name, got, k)
        assert np.array_equal(sizes_of(labels, got), sizes), (n, conn, name)
        assert np.array_equal(labels != 0, vox)
    assert {"empty", "full", "eight corners", "pairs by face, edge and corner", "one run across the word edges", "1 0 1 beside 1 1 1",
            "checkerboard", "nested shells", "comb along x", "comb along y", "comb along z", "two interleaved combs", "two equal boxes",
            "six faces"} <= names
    if n > 32:
        assert {"pairs by face, edge and corner across the word edge", "1 0 1 beside 1 1 1 across the word edge"} <= names


def test_filter_reference_rules():
    sizes = np.array([5, 9, 9, 1, 7], np.uint32)
    assert keep_flags(sizes, KEEP_LARGEST, 1).tolist() == [False, True, False, False, False]          # the tie goes to the lower label
    assert keep_flags(sizes, KEEP_LARGEST, 3).tolist() == [False, True, True, False, True]
    assert keep_flags(sizes, KEEP_LARGEST, 16).all()
    assert keep_flags(sizes, MIN_VOXELS, 0).all() and keep_flags(sizes, MIN_VOXELS, 1).all()
    assert keep_flags(sizes, MIN_VOXELS, 7).tolist() == [False, True, True, False, True]
    assert not keep_flags(sizes, MIN_VOXELS, 10).any()
    w = random_grid(32, 0.2, 9)
    out, k, kept = filter_numpy(w, 32, 6, MIN_VOXELS, 1)
    assert np.array_equal(out, w) and kept == O.popcount(w) and k > 100
    out, k, kept = filter_numpy(np.zeros(1024, np.uint32), 32, 26, KEEP_LARGEST, 1)
    assert k == 0 and kept == 0 and not out.any()


def _vpcli(cli, tmp_path, args, tag):
    prefix = str(tmp_path / tag)
    p = subprocess.run([cli] + args + ["-d", prefix], capture_output=True, text=True, timeout=1800, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return np.fromfile(prefix + ".grid.u32", np.uint32), p.stdout


def _debris_scene(tmp_path):
    """the torus and twelve small copies of d20 beside it, in one OBJ"""
    txyz, ttri = M.import_mesh(M.asset("torus.obj"))
    dxyz, dtri = M.import_mesh(M.asset("d20.obj"))
    lo, hi = txyz.min(0), txyz.max(0)
    ext = float((hi - lo).max())
    dunit = (dxyz - (dxyz.min(0) + dxyz.max(0)) / 2) / float((dxyz.max(0) - dxyz.min(0)).max())
    xyz, tri = [txyz], [ttri]
    count = len(txyz)
    for i in range(12):
        c = np.array([lo[0] + ext * (0.1 + 0.16 * (i % 6)), lo[1] + ext * (0.1 + 0.8 * (i // 6)), hi[2] + ext * 0.25], np.float32)
        xyz.append((dunit * ext * (0.04 + 0.005 * i) + c).astype(np.float32))
        tri.append(dtri + count)
        count += len(dxyz)
    xyz, tri = np.concatenate(xyz).astype(np.float32), np.concatenate(tri).astype(np.uint32)
    path = str(tmp_path / "debris.obj")
    M.export_obj(path, xyz, tri)
    return path, xyz, tri


@pytest.mark.parametrize("n", [32, 64])
def test_cli_host_restatement_equals_the_numpy_filter(cli, tmp_path, n):
    path, xyz, tri = _debris_scene(tmp_path)
    xyz, tri = M.import_mesh(path)                             # what the CLI reads back
    origin, vs = O.frame([xyz], n)
    surf = cvox_numpy(xyz, tri, n, vs, origin)
    sizes = {}
    for conn in (6, 26):
        labels, k = label_numpy(surf, n, conn, jump=True)
        sizes[conn] = np.sort(sizes_of(labels, k))
        assert k >= 2, (n, conn, k)                            # the scene has debris at this n
    v = int(sizes[26][-2]) + 1                                 # more than every blob but the largest
    for t in ("0", "3"):
        for item, conn, mode, param in (("largest", 26, KEEP_LARGEST, 1), ("largest:6", 6, KEEP_LARGEST, 1), ("largest:26", 26, KEEP_LARGEST, 1),
                                        ("minsize:%d" % v, 26, MIN_VOXELS, v), ("minsize:%d:6" % v, 6, MIN_VOXELS, v),
                                        ("minsize:2:26", 26, MIN_VOXELS, 2), ("minsize:0", 26, MIN_VOXELS, 0)):
            got, out = _vpcli(cli, tmp_path, [path, "-n", str(n), "-t", t, "--conservative", "--morph", item], "c" + t)
            exp, k, kept = filter_numpy(surf, n, conn, mode, param, jump=True)
            assert np.array_equal(got, exp), (n, t, item, int(np.count_nonzero(got != exp)))
            assert "components: %d, kept: %d voxels" % (k, kept) in out, (item, out[-800:])
            assert "Components]: " in out and " ms" in out.split("Components]: ")[1].splitlines()[0], out[-800:]
    # the repair chain with a filter at its end: the largest blob of the solid
    chain, out = _vpcli(cli, tmp_path, [path, "-n", str(n), "-t", "0", "--conservative", "--morph", "fill,largest"], "chain")
    exp, k, kept = filter_numpy(fill_numpy(surf, n), n, 26, KEEP_LARGEST, 1, jump=True)
    assert np.array_equal(chain, exp) and "components: %d, kept: %d voxels" % (k, kept) in out


def test_the_place_of_a_filter_in_the_list_matters(cli, tmp_path):
    """A closed sphere and a large open plate: the plate has more voxels than the sphere's shell and fewer than its solid, so
    `fill,largest` keeps the solid sphere and `largest,fill` the plate."""
    n = 64
    sxyz, stri = M.import_mesh(M.asset("sphere.obj"))
    c, r = (sxyz.min(0) + sxyz.max(0)) / 2, float((sxyz.max(0) - sxyz.min(0)).max()) / 2
    ball = (sxyz - c) / r * 0.25 + np.array([0.5, 0.5, 0.3])
    plate = np.array([[0, 0, 0.8], [1, 0, 0.8], [1, 1, 0.8], [0, 1, 0.8]], np.float32)
    xyz = np.concatenate([ball, plate]).astype(np.float32)
    tri = np.concatenate([stri, np.array([[0, 1, 2], [0, 2, 3]], np.uint32) + len(ball)]).astype(np.uint32)
    path = str(tmp_path / "scene.obj")
    M.export_obj(path, xyz, tri)
    xyz, tri = M.import_mesh(path)
    origin, vs = O.frame([xyz], n)
    surf = cvox_numpy(xyz, tri, n, vs, origin)
    labels, k = label_numpy(surf, n, 26, jump=True)
    shell, sheet = (int(s) for s in sizes_of(labels, k))       # the sphere lies below the plate: label 1
    solid = fill_numpy(surf, n)
    ls, ks = label_numpy(solid, n, 26, jump=True)
    assert k == 2 and ks == 2 and shell < sheet < int(sizes_of(ls, ks)[0]), (k, ks, shell, sheet)
    args = [path, "-n", str(n), "-t", "0", "--conservative", "--morph"]
    a, _ = _vpcli(cli, tmp_path, args + ["fill,largest"], "a")
    b, _ = _vpcli(cli, tmp_path, args + ["largest,fill"], "b")
    assert np.array_equal(a, filter_labels(ls, ks, KEEP_LARGEST, 1)[0])
    assert np.array_equal(b, fill_numpy(filter_labels(labels, k, KEEP_LARGEST, 1)[0], n))
    assert not np.array_equal(a, b)
    assert O.popcount(b) == sheet and O.popcount(a) == int(sizes_of(ls, ks)[0])


@pytest.mark.parametrize("bad", ["largest:18", "minsize", "minsize:", "minsize:-1", "largest:6:6", "largest:", "minsize:5:18", "minsize:5:6:6",
                                 "largestx", "minsize:4294967296", "largest,", "minsize:1x"])
def test_cli_refuses_malformed_steps(cli, tmp_path, bad):
    p = subprocess.run([cli, M.asset("d20.obj"), "-n", "32", "-t", "0", "--morph=" + bad], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    assert p.returncode != 0, bad
    assert "--morph" in p.stdout + p.stderr


def test_cli_refuses_several_gpus_and_documents_the_steps(cli, tmp_path):
    p = subprocess.run([cli, M.asset("d20.obj"), "-n", "32", "-t", "2", "--morph", "largest", "-g", "2"], capture_output=True, text=True,
                       timeout=300, cwd=str(tmp_path))
    assert p.returncode != 0
    assert "--morph runs on one device" in p.stdout + p.stderr
    h = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert h.returncode == 0 and "largest[:C]" in h.stdout and "minsize:V[:C]" in h.stdout


def _hash_voxels(n, density):
    i = np.arange(n ** 3, dtype=np.uint32)
    with np.errstate(over="ignore"):
        h = i * np.uint32(2654435761)
        h ^= h >> np.uint32(15)
        h *= np.uint32(2246822519)
    return ((h >> np.uint32(24)) < density).reshape(n, n, n)


def test_cpp_api_on_uint32_and_uint64_grids(tmp_path):
    build.build_lib()
    pkg = os.path.join(ROOT, "cuda_mesh_voxelization_amd")
    srcs = [os.path.join(pkg, "vplib", "src", f) for f in sorted(os.listdir(os.path.join(pkg, "vplib", "src"))) if f.endswith(".cpp")]
    exe = str(tmp_path / "components_check")
    subprocess.check_call(["g++", "-std=c++23", "-O2", "-ffp-contract=off", "-fopenmp",
                           "-I", os.path.join(pkg, "vplib", "include"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "components_check.cpp")] + srcs + ["-o", exe, "-L", pkg, "-lvphip", "-Wl,-rpath," + pkg])
    for n, density in ((32, 40), (64, 70)):
        out = subprocess.run([exe, str(n), str(density), "0"], capture_output=True, text=True, timeout=600, check=True).stdout
        got = {}
        for line in out.strip().splitlines():
            tag, conn, what, k, kept, h = line.split()
            got[(tag, int(conn), what)] = (int(k), int(kept), h)
        words = bool_to_words(_hash_voxels(n, density))
        for conn in (6, 26):
            labels, k = label_numpy(words, n, conn, jump=True)
            exp = {"label": (k, 0, O.fnv(labels))}
            for what, mode, param in (("largest2", KEEP_LARGEST, 2), ("min3", MIN_VOXELS, 3)):
                w, kept = filter_labels(labels, k, mode, param)
                exp[what] = (k, kept, O.fnv(w))
            assert k > 50                                      # many components at these densities: the order of the labels is tested
            for tag in ("seq32", "seq64", "omp32", "omp64"):
                for what in exp:
                    assert got[(tag, conn, what)] == exp[what], (n, conn, tag, what)
