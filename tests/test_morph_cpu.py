"""Ball morphology without a GPU: the two numpy restatements of tests/morph_ref.py against each other, against scipy.ndimage and against
hand-written expectations; the algebra the border convention buys (adjunction: open / close idempotent, close extensive, open
anti-extensive); the shell-with-a-hole repair dilate -> fill -> erode and the trap fill(close); the host restatement of
`vpcli --morph` (-t 0 / -t 3, vplib/src/morph.cpp) against the numpy pipeline; the list parser; uint64_t grids."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cuda_mesh_voxelization_amd import build, capi, mesh as M
from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fill_ref import fill_numpy  # noqa: E402
from morph_ref import (CLOSE, DILATE, ERODE, OPEN, ball, bool_to_words, hand_cases, morph_bool, morph_bool_sep, morph_numpy,  # noqa: E402
                       morph_numpy_sep, random_grid, shell_with_hole, words_to_bool)
from test_conservative_cpu import cvox_numpy  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cli():
    return build.build_cli()


def test_constants_match_the_header():
    assert (capi.MORPH_DILATE, capi.MORPH_ERODE, capi.MORPH_OPEN, capi.MORPH_CLOSE) == (DILATE, ERODE, OPEN, CLOSE) == (0, 1, 2, 3)
    assert "vp_morph" in capi.SYMBOLS and "vp_morph_host" in capi.SYMBOLS
    assert capi.KERNELS[-2:] == ["morph", "morph_naive"]


def test_ball_sizes():
    assert [int(ball(r).sum()) for r in (1, 2, 3, 4, 8, 16)] == [7, 33, 123, 257, 2109, 17077]


def _random_cases(n, radii):
    for r in radii:
        for density in (0.001, 0.02, 0.2, 0.5):
            yield r, density, words_to_bool(random_grid(n, density, 100 * n + 10 * r + int(1000 * density)), n)


@pytest.mark.parametrize("n,radii", [(32, (1, 2, 3, 4, 5)), (64, (1, 2, 3, 4, 5))])
def test_brute_equals_separable(n, radii):
    for r, density, v in _random_cases(n, radii):
        d = morph_bool(v, DILATE, r)
        assert np.array_equal(d, morph_bool_sep(v, DILATE, r)), (n, r, density)
        e = morph_bool(~v, ERODE, r)
        assert np.array_equal(e, morph_bool_sep(~v, ERODE, r)), (n, r, density)
        assert np.array_equal(e, ~d)


@pytest.mark.parametrize("n,radii", [(32, (1, 2, 3, 4, 5)), (64, (1, 2, 3, 4, 5))])
def test_brute_equals_separable_equals_scipy(n, radii):
    """With test_brute_equals_separable (which needs no scipy): brute == separable == scipy."""
    ndimage = pytest.importorskip("scipy.ndimage")
    for r, density, v in _random_cases(n, radii):
        assert np.array_equal(morph_bool_sep(v, DILATE, r), ndimage.binary_dilation(v, structure=ball(r), border_value=0)), (n, r, density)
        assert np.array_equal(morph_bool_sep(~v, ERODE, r), ndimage.binary_erosion(~v, structure=ball(r), border_value=1)), (n, r, density)


@pytest.mark.parametrize("n", [32, 64, 96])
def test_references_get_the_hand_cases_right(n):
    for r in (1, 2, 3, 5):
        names = set()
        for name, op, vox, exp in hand_cases(n, r):
            names.add(name)
            assert np.array_equal(morph_bool_sep(vox, op, r), exp), (n, r, name)
            if r <= 3:
                assert np.array_equal(morph_bool(vox, op, r), exp), (n, r, name)
        assert {"single voxel middle", "single voxel corner", "single voxel x=31", "single voxel x=n-1", "erode full", "dilate empty",
                "erode thin box"} <= names
    v = words_to_bool(random_grid(n, 0.3, n), n)
    for op in (DILATE, ERODE, OPEN, CLOSE):
        assert np.array_equal(morph_bool_sep(v, op, 0), v)


def test_algebra_on_random_grids():
    for n, density, seed in ((32, 0.05, 1), (32, 0.5, 2), (64, 0.9, 3)):
        v = words_to_bool(random_grid(n, density, seed), n)
        for r in (1, 2, 3):
            c, o = morph_bool_sep(v, CLOSE, r), morph_bool_sep(v, OPEN, r)
            assert not (v & ~c).any() and not (o & ~v).any(), (n, r)
            assert np.array_equal(morph_bool_sep(c, CLOSE, r), c) and np.array_equal(morph_bool_sep(o, OPEN, r), o), (n, r)
            assert np.array_equal(morph_bool_sep(v, ERODE, r), ~morph_bool_sep(~v, DILATE, r))


def _repair(shell, R):
    n = shell.shape[0]
    d = morph_bool_sep(shell, DILATE, R)
    f = words_to_bool(fill_numpy(bool_to_words(d), n), n)
    return morph_bool_sep(f, ERODE, R)


@pytest.mark.parametrize("k,R", [(2, 1), (3, 2), (4, 2), (5, 3), (6, 3)])
def test_dilate_fill_erode_repairs_a_shell_with_a_hole(k, R):
    n = 64
    shell, full = shell_with_hole(n, k)
    w = bool_to_words(shell)
    assert np.array_equal(fill_numpy(w, n), w)               # the fill alone leaks through the hole
    got = _repair(shell, R)
    assert not (got & ~full).any()                           # nothing outside the box
    missing = int((full & ~got).sum())
    print("k=%d R=%d dimple %d voxels (cap %d)" % (k, R, missing, k * k * R))
    assert missing <= k * k * R                              # a shallow dimple behind the hole: a cap, not a measurement
    assert got[n // 2, n // 2, n // 2 - 8]


@pytest.mark.parametrize("k,R", [(7, 3), (4, 1)])
def test_a_hole_wider_than_the_ball_still_leaks(k, R):
    n = 64
    shell, full = shell_with_hole(n, k)
    got = _repair(shell, R)
    assert not got[n // 2, n // 2, n // 2 - 8]               # the cavity was not filled
    assert int((full & ~got).sum()) > full.sum() // 2


def test_fill_after_close_leaks():
    """the documented trap: the erosion inside close re-opens the plug from the side before the fill runs"""
    n, k, R = 64, 3, 2
    shell, full = shell_with_hole(n, k)
    c = bool_to_words(morph_bool_sep(shell, CLOSE, R))
    f = words_to_bool(fill_numpy(c, n), n)
    assert np.array_equal(bool_to_words(f), c)
    assert not f[n // 2, n // 2, n // 2 - 8]


def _vpcli(cli, tmp_path, args, tag):
    prefix = str(tmp_path / tag)
    p = subprocess.run([cli] + args + ["-d", prefix], capture_output=True, text=True, timeout=1800, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return np.fromfile(prefix + ".grid.u32", np.uint32), p.stdout


@pytest.mark.parametrize("name", ["torus.obj", "bunny.obj"])
def test_cli_host_restatement_equals_the_numpy_pipeline(cli, tmp_path, name):
    n = 64
    xyz, tri = M.import_mesh(M.asset(name))
    origin, vs = O.frame([xyz], n)
    exp = cvox_numpy(xyz, tri, n, vs, origin)
    exp = morph_numpy(exp, n, DILATE, 2)
    exp = fill_numpy(exp, n)
    exp = morph_numpy(exp, n, ERODE, 2)
    for t in ("0", "3"):
        got, out = _vpcli(cli, tmp_path, [M.asset(name), "-n", str(n), "-t", t, "--conservative", "--morph", "dilate:2,fill,erode:2"], "m" + t)
        assert np.array_equal(got, exp), (name, t, int(np.count_nonzero(got != exp)))
        assert out.count("Morph]: ") == 2 and "Fill]: " in out, out[-1500:]


def test_cli_every_op_equals_the_separable_reference(cli, tmp_path):
    n = 32
    xyz, tri = M.import_mesh(M.asset("bimba.obj"))
    origin, vs = O.frame([xyz], n)
    solid = O.voxelize(xyz, tri, n, vs, origin)
    for t in ("0", "3"):
        for item, op, r in (("dilate:3", DILATE, 3), ("erode:2", ERODE, 2), ("open:2", OPEN, 2), ("close:5", CLOSE, 5), ("dilate:0", DILATE, 0)):
            got, _ = _vpcli(cli, tmp_path, [M.asset("bimba.obj"), "-n", str(n), "-t", t, "--morph=" + item], "op")
            assert np.array_equal(got, morph_numpy_sep(solid, n, op, r)), (t, item)


def test_cli_morph_runs_before_fill(cli, tmp_path):
    """--fill keeps its place after the list wherever it stands on the command line: `--morph close:1 --fill` and `--fill --morph close:1`
    are both fill(close(W)); the other order is spelled inside the list, `--morph fill,close:1` = close(fill(W)).  On a closed mesh the two
    orders of close and fill happen to agree, so the difference between the orders is shown with erode:1, which removes the thin shell."""
    n = 64
    args = [M.asset("torus.obj"), "-n", str(n), "-t", "0", "--conservative"]
    surf, _ = _vpcli(cli, tmp_path, args, "s")
    for item, op in (("close:1", CLOSE), ("erode:1", ERODE)):
        a, _ = _vpcli(cli, tmp_path, args + ["--morph", item, "--fill"], "a")
        b, _ = _vpcli(cli, tmp_path, args + ["--fill", "--morph", item], "b")
        c, _ = _vpcli(cli, tmp_path, args + ["--morph", "fill," + item], "c")
        first = fill_numpy(morph_numpy_sep(surf, n, op, 1), n)
        assert np.array_equal(a, first) and np.array_equal(b, first), item
        assert np.array_equal(c, morph_numpy_sep(fill_numpy(surf, n), n, op, 1)), item
        if op == ERODE:
            assert not np.array_equal(a, c)


@pytest.mark.parametrize("bad", ["dilate", "dilate:", "dilate:33", "dilate:-1", "grow:2", "dilate:2,,erode:2", "dilate:2,", "fill:2", "erode:1x", ""])
def test_cli_refuses_malformed_lists(cli, tmp_path, bad):
    p = subprocess.run([cli, M.asset("d20.obj"), "-n", "32", "-t", "0", "--morph=" + bad], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    assert p.returncode != 0, bad
    assert "--morph" in p.stdout + p.stderr


def test_cli_refuses_several_gpus_and_documents_the_flag(cli, tmp_path):
    p = subprocess.run([cli, M.asset("d20.obj"), "-n", "32", "-t", "2", "--morph", "dilate:1", "-g", "2"], capture_output=True, text=True,
                       timeout=300, cwd=str(tmp_path))
    assert p.returncode != 0
    assert "--morph runs on one device" in p.stdout + p.stderr
    h = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert h.returncode == 0 and "--morph" in h.stdout and "dilate:R" in h.stdout


def test_cpp_host_restatement_on_uint64_grids(tmp_path):
    build.build_lib()
    pkg = os.path.join(ROOT, "cuda_mesh_voxelization_amd")
    srcs = [os.path.join(pkg, "vplib", "src", f) for f in sorted(os.listdir(os.path.join(pkg, "vplib", "src"))) if f.endswith(".cpp")]
    exe = str(tmp_path / "morph_check")
    subprocess.check_call(["g++", "-std=c++23", "-O2", "-ffp-contract=off", "-fopenmp",
                           "-I", os.path.join(pkg, "vplib", "include"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "morph_check.cpp")] + srcs + ["-o", exe, "-L", pkg, "-lvphip", "-Wl,-rpath," + pkg])
    for n, r in ((32, 2), (64, 3)):
        out = subprocess.run([exe, str(n), str(r), "0"], capture_output=True, text=True, timeout=600, check=True).stdout
        got = {}
        for line in out.strip().splitlines():
            tag, op, h = line.split()
            got[(tag, op)] = h
        # the same voxels, rebuilt here with the generator of morph_check.cpp, through the separable reference
        for op in range(4):
            s = np.uint32(12345)
            keep = 3 if op in (0, 3) else 200
            seq = np.empty(n ** 3, np.uint32)
            with np.errstate(over="ignore"):
                for i in range(n ** 3):
                    s = s * np.uint32(1664525) + np.uint32(1013904223)
                    seq[i] = s
            vox = ((seq >> 24) < keep).reshape(n, n, n)
            exp = O.fnv(morph_numpy_sep(bool_to_words(vox), n, op, r))
            for tag in ("seq32", "seq64", "omp32", "omp64"):
                assert got[(tag, "op%d" % op)] == exp, (n, r, op, tag)
