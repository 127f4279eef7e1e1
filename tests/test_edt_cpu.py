"""The exact distance transform without a GPU: the numpy restatement of tests/edt_ref.py against a brute force over the seed list, against
scipy.ndimage, against the ball morphology references and against hand-written expectations; the figures of the golden grid and how far
the oracle's JFA is from them; the host restatement of vplib/src/edt.cpp through the C++ API on both word types and through `vpcli`
(-t 0 / -t 3: --exact-sdf, --morph offset:R / inset:R); the new usage errors."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cuda_mesh_voxelization_amd import build, capi, mesh as M
from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edt_ref as E  # noqa: E402
from fill_ref import fill_numpy  # noqa: E402
from morph_ref import DILATE, ERODE, bool_to_words, morph_bool_sep, random_grid, shell_with_hole, words_to_bool  # noqa: E402
from test_conservative_cpu import cvox_numpy  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bunny_decimated_n64.grid.u32")
MODES = (E.SET, E.UNSET, E.BORDER)
CASES = [(32, 0.001), (32, 0.3), (64, 0.02), (96, 0.0001)]
# seeds, max and sum of the transform of the golden grid, per mode
GOLDEN_TABLE = {E.SET: (52619, 1205, 28537538), E.UNSET: (209525, 211, 1273656), E.BORDER: (13679, 1205, 29333323)}


@pytest.fixture(scope="module")
def cli():
    return build.build_cli()


@pytest.fixture(scope="module")
def refs():
    """the reference transforms of the random grids, computed once: {(n, density, mode): (vox, seeds, D)}"""
    out = {}
    for n, density in CASES:
        vox = words_to_bool(random_grid(n, density, 5), n)
        for mode in MODES:
            s = E.seeds_of(vox, mode)
            out[(n, density, mode)] = (vox, s, E.edt_seeds(s))
    return out


def test_constants_symbols_and_timing_keys_match_the_header():
    assert (capi.EDT_SEEDS_SET, capi.EDT_SEEDS_UNSET, capi.EDT_SEEDS_BORDER) == (E.SET, E.UNSET, E.BORDER) == (0, 1, 2)
    assert capi.EDT_NONE == E.NONE == 0xFFFFFFFF
    for s in ("vp_edt", "vp_edt_sdf", "vp_edt_morph", "vp_edt_host", "vp_edt_sdf_host", "vp_edt_morph_host"):
        assert s in capi.SYMBOLS
    header = open(os.path.join(ROOT, "include", "vphip.h")).read()
    assert "#define VP_ABI_VERSION 6" in header.replace("  ", " ")
    assert "VP_EDT_SEEDS_SET = 0, VP_EDT_SEEDS_UNSET = 1, VP_EDT_SEEDS_BORDER = 2" in header and "#define VP_EDT_NONE 0xFFFFFFFFu" in header
    third = header[header.index("VP_K_EDT_X = VP_K_TOTAL"):header.index("VP_K_END")]
    keys = [t.split("=")[0].strip().lower()[len("vp_k_"):] for t in
            "".join(line.split("/*")[0] for line in third.splitlines()).split(",") if t.strip()]
    assert keys == capi.EDT_KERNELS
    assert capi.EVERY_PROF_KEY == capi.ALL_PROF_KEYS + capi.EDT_KERNELS and len(capi.EVERY_PROF_KEY) <= 64
    assert capi.ALL_PROF_KEYS == capi.KERNELS + capi.COMP_KERNELS + capi.SURFNETS_KERNELS          # the first two enums did not grow
    assert header.index("VP_K_EDT_X = VP_K_TOTAL") > header.index("VP_K_SN_RELAX_NAIVE")
    assert "edt.hip" in build.HIP_SOURCES


@pytest.mark.parametrize("n", [32, 64])
def test_reference_gets_the_hand_cases_right(n):
    names = set()
    for name, mode, vox, exp in E.hand_cases(n):
        names.add(name)
        got = E.edt_numpy(vox, mode)
        assert got.dtype == np.uint32 and np.array_equal(got, exp), (n, name)
    assert {"empty, mode 2", "full, BORDER", "single voxel corner", "single voxel x=31", "two opposite corners", "wall x=31",
            "UNSET on a box on three faces"} <= names


def test_reference_equals_brute_force(refs):
    for density in (0.001, 0.3):
        for mode in MODES:
            vox, s, d = refs[(32, density, mode)]
            assert np.array_equal(d, E.edt_brute(s)), (density, mode)


def test_reference_equals_scipy(refs):
    ndimage = pytest.importorskip("scipy.ndimage")
    for (n, density, mode), (vox, s, d) in refs.items():
        if not s.any():
            assert (d == E.NONE).all()
            continue
        idx = ndimage.distance_transform_edt(~s, return_distances=False, return_indices=True).astype(np.int64)
        grid = np.indices(s.shape).astype(np.int64)
        exact = ((idx - grid) ** 2).sum(0)
        assert np.array_equal(d.astype(np.int64), exact), (n, density, mode)


def test_thresholds_equal_the_ball_morphology(refs):
    for n, density in CASES:
        vox = refs[(n, density, E.SET)][0]
        d_set, d_unset = refs[(n, density, E.SET)][2], refs[(n, density, E.UNSET)][2]
        for r in (3, 32):
            assert np.array_equal(d_set.astype(np.int64) <= r * r, morph_bool_sep(vox, DILATE, r)), (n, density, r)
            assert np.array_equal(d_unset.astype(np.int64) > r * r, morph_bool_sep(vox, ERODE, r)), (n, density, r)
    v = refs[(32, 0.3, E.SET)][0]
    for op in range(4):
        assert np.array_equal(E.morph_edt(v, op, 2), morph_bool_sep(v, op, 2)), op
        assert np.array_equal(E.morph_edt(v, op, 0), v)


def test_golden_grid_figures_and_the_error_of_the_jfa():
    n = 64
    words = np.fromfile(GOLDEN, np.uint32)
    vox = words_to_bool(words, n)
    d = {}
    for mode in MODES:
        s = E.seeds_of(vox, mode)
        d[mode] = E.edt_seeds(s)
        assert (int(s.sum()), int(d[mode].max()), int(d[mode].astype(np.int64).sum())) == GOLDEN_TABLE[mode], mode
    # unit frame: every float the JFA computes is an exact integer
    jfa = O.jfa(words, n, 1.0, np.zeros(3, np.float32)).reshape(n, n, n)
    exact = E.sdf_numpy(vox, 1.0)
    assert np.array_equal(np.signbit(jfa), np.signbit(exact)) and np.array_equal(jfa == 0, exact == 0)
    excess = np.abs(jfa).astype(np.int64) - np.abs(exact).astype(np.int64)
    assert excess.min() == 0                                               # never too small
    assert (int(np.count_nonzero(excess)), int(excess.max())) == (436, 31)
    rnd = random_grid(64, 0.01, 2)
    j = np.abs(O.jfa(rnd, n, 1.0, np.zeros(3, np.float32))).astype(np.int64).reshape(n, n, n)
    e = E.edt_numpy(words_to_bool(rnd, n), E.BORDER).astype(np.int64)
    assert (j >= e).all() and int(np.count_nonzero(j != e)) == 88


def test_sdf_reference_signs_and_fill():
    n = 32
    vox = words_to_bool(random_grid(n, 0.4, 9), n)
    s = E.sdf_numpy(vox, 0.3)
    assert s.dtype == np.float32 and (s[vox] >= 0).all() and (s[~vox] < 0).all()
    assert np.array_equal(s == 0, E.border_mask(vox))
    empty = np.zeros((n, n, n), bool)
    assert (E.sdf_numpy(empty, 0.3) == -np.inf).all() and (E.sdf_numpy(empty, 0.3, np.inf) == np.inf).all()


def _lcg_vox(n, keep):
    """the voxels of tests/cpp/edt_check.cpp"""
    s = np.uint32(12345)
    seq = np.empty(n ** 3, np.uint32)
    with np.errstate(over="ignore"):
        for i in range(n ** 3):
            s = s * np.uint32(1664525) + np.uint32(1013904223)
            seq[i] = s
    return ((seq >> 24) < keep).reshape(n, n, n)


def _pack(vox):
    """bit words of any side (n^3 a multiple of 32)"""
    return np.packbits(np.ascontiguousarray(vox, bool).reshape(-1), bitorder="little").view(np.uint32)


def test_cpp_host_restatement_on_both_word_types(tmp_path):
    build.build_lib()
    pkg = os.path.join(ROOT, "cuda_mesh_voxelization_amd")
    srcs = [os.path.join(pkg, "vplib", "src", f) for f in sorted(os.listdir(os.path.join(pkg, "vplib", "src"))) if f.endswith(".cpp")]
    exe = str(tmp_path / "edt_check")
    subprocess.check_call(["g++", "-std=c++23", "-O2", "-ffp-contract=off", "-fopenmp",
                           "-I", os.path.join(pkg, "vplib", "include"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "edt_check.cpp")] + srcs + ["-o", exe, "-L", pkg, "-lvphip", "-Wl,-rpath," + pkg])
    for n, r in ((32, 2), (40, 3)):                                         # 40: the host restatement serves any side
        out = subprocess.run([exe, str(n), str(r), "0"], capture_output=True, text=True, timeout=600, check=True).stdout
        got = {}
        for line in out.strip().splitlines():
            tag, what, h = line.split()
            got[(tag, what)] = h
        vox = {keep: _lcg_vox(n, keep) for keep in (2, 3, 254, 220)}
        exp = {}
        for mode in MODES:
            exp["edt%d" % mode] = O.fnv(E.edt_numpy(vox[2 if mode == E.SET else 220], mode))
        for op in range(4):
            exp["op%d" % op] = O.fnv(_pack(E.morph_edt(vox[3 if op in (0, 3) else 254], op, r)))
        exp["sdf"] = O.fnv(E.sdf_numpy(vox[220], np.float32(0.75) / np.float32(n)))
        assert len(set(exp.values())) == len(exp)                           # no two cases degenerate into the same result
        for tag in ("seq32", "seq64", "omp32", "omp64"):
            for what, h in exp.items():
                assert got[(tag, what)] == h, (n, r, tag, what)


def _vpcli(cli, tmp_path, args, tag):
    prefix = str(tmp_path / tag)
    p = subprocess.run([cli] + args + ["-d", prefix], capture_output=True, text=True, timeout=1800, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return prefix, p.stdout


def test_cli_exact_sdf_equals_the_reference(cli, tmp_path):
    n = 64
    xyz, tri = M.import_mesh(M.asset("bunny.obj"))
    origin, vs = O.frame([xyz], n)
    words = O.voxelize(xyz, tri, n, vs, origin)
    exp = E.sdf_numpy(words_to_bool(words, n), vs).reshape(-1)
    for t in ("0", "3"):
        prefix, _ = _vpcli(cli, tmp_path, [M.asset("bunny.obj"), "-n", str(n), "-t", t, "-s", "--exact-sdf"], "x" + t)
        assert np.array_equal(np.fromfile(prefix + ".grid.u32", np.uint32), words)
        got = np.fromfile(prefix + ".sdf.f32", np.float32)
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (t, int(np.count_nonzero(got != exp)))
    # the JFA of the same job: the same signs and the same zeros (its magnitudes come from float positions, so they are compared with
    # the exact field in the unit frame only, test_golden_grid_figures_and_the_error_of_the_jfa)
    prefix, _ = _vpcli(cli, tmp_path, [M.asset("bunny.obj"), "-n", str(n), "-t", "0", "-s"], "j")
    jfa = np.fromfile(prefix + ".sdf.f32", np.float32)
    assert np.array_equal(np.signbit(jfa), np.signbit(exp)) and np.array_equal(jfa == 0, exp == 0)
    assert not np.array_equal(jfa, exp)


def test_cli_offset_and_inset_equal_the_reference(cli, tmp_path):
    n = 64
    xyz, tri = M.import_mesh(M.asset("torus.obj"))
    origin, vs = O.frame([xyz], n)
    surf = words_to_bool(cvox_numpy(xyz, tri, n, vs, origin), n)
    exp = E.morph_edt(words_to_bool(fill_numpy(bool_to_words(E.morph_edt(surf, 0, 5)), n), n), 1, 5)
    far = E.morph_edt(surf, 0, 40)
    for t in ("0", "3"):
        prefix, out = _vpcli(cli, tmp_path, [M.asset("torus.obj"), "-n", str(n), "-t", t, "--conservative", "--morph", "offset:5,fill,inset:5"], "m" + t)
        got = np.fromfile(prefix + ".grid.u32", np.uint32)
        assert np.array_equal(got, bool_to_words(exp)), (t, int(np.count_nonzero(got != bool_to_words(exp))))
        assert out.count("MorphExact]: ") == 2 and "Fill]: " in out, out[-1500:]
        prefix, _ = _vpcli(cli, tmp_path, [M.asset("torus.obj"), "-n", str(n), "-t", t, "--conservative", "--morph=offset:40"], "f" + t)
        assert np.array_equal(np.fromfile(prefix + ".grid.u32", np.uint32), bool_to_words(far)), t
    # where both are served, offset:R is dilate:R and inset:R is erode:R
    a, _ = _vpcli(cli, tmp_path, [M.asset("torus.obj"), "-n", str(n), "-t", "0", "--conservative", "--morph", "dilate:7,erode:3"], "a")
    b, _ = _vpcli(cli, tmp_path, [M.asset("torus.obj"), "-n", str(n), "-t", "0", "--conservative", "--morph", "offset:7,inset:3"], "b")
    assert np.array_equal(np.fromfile(a + ".grid.u32", np.uint32), np.fromfile(b + ".grid.u32", np.uint32))


WIDE_HOLE_K = 70        # hole width of the repair below: 60 is still plugged by r = 32 (its centre is 30 voxels from the rim), 70 is not


def test_a_wide_hole_needs_a_radius_above_32():
    """the repair tests/test_edt_gpu.py runs on the device, decided here on the CPU with the separable morphology reference: the shell of
    morph_ref.shell_with_hole(128, 70) leaks through dilate:32 -> fill -> erode:32 and is closed by radius 40.  (At n = 128 the shell
    dilated by 40 covers every grid face, so the closed result is the full grid: outside reads as set for the erosion.)"""
    n, k = 128, WIDE_HOLE_K
    shell, full = shell_with_hole(n, k)

    def repair(r):
        d = morph_bool_sep(shell, DILATE, r)
        f = words_to_bool(fill_numpy(bool_to_words(d), n), n)
        return morph_bool_sep(f, ERODE, r)
    leaking, closed = repair(32), repair(40)
    centre = (n // 2, n // 2, n // 2)
    assert not leaking[centre] and int((full & ~leaking).sum()) > full.sum() // 2          # the cavity was not filled
    assert closed[centre] and not (full & ~closed).any()                                    # the whole box is solid


@pytest.mark.parametrize("args", [["--exact-sdf"], ["-s", "--exact-sdf", "-g", "2", "-t", "2"], ["--morph=offset:65536"], ["--morph=inset:-1"],
                                  ["--morph=offset"], ["--morph=offset:"], ["--morph=inset:1x"], ["--morph=dilate:33"]])
def test_cli_refuses_the_new_usage_errors(cli, tmp_path, args):
    p = subprocess.run([cli, M.asset("d20.obj"), "-n", "32", "-t", "0"] + args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode != 0, args
    assert ("--exact-sdf" if "--exact-sdf" in args else "--morph") in p.stdout + p.stderr


def test_cli_help_names_the_new_flags(cli):
    h = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    assert h.returncode == 0 and "--exact-sdf" in h.stdout and "offset:R" in h.stdout and "inset:R" in h.stdout
