"""Local thickness without a GPU: the numpy restatement of tests/thickness_ref.py against hand-written expectations (a single voxel, the
empty and the full grid, slabs of 1 .. 7 voxels, a ball, a dumbbell), the five facts of the header on random grids and their complements,
the host restatement of vplib/src/thickness.cpp through the C++ API on both word types and through `vpcli --thickness`, bit for bit, and
the header's prototypes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cuda_mesh_voxelization_amd import build, capi, mesh as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thickness_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_cases():
    for k, density in enumerate((0.9, 0.97, 0.995)):
        vox = R.words_to_bool(R.random_grid(32, density, 160 + k), 32)
        yield "random %g" % density, vox
        yield "complement of random %g" % density, ~vox


# ---- hand cases ------------------------------------------------------------------------------------------------------------------
def test_hand_cases():
    for name, rmax, vox, exp in R.hand_cases(32):
        got = R.thickness_numpy(vox, rmax)
        if isinstance(exp, tuple):                                   # the closed form holds away from the walls
            exp, where = exp
            assert np.array_equal(got[where], exp[where]), name
            assert not got[~vox].any(), name
        else:
            assert np.array_equal(got, exp), name


def test_slab_read_out_is_the_half_width_rounded_up_squared():
    """w = 1 .. 7 reads 1, 1, 4, 4, 9, 9, 16: the discrete read-out of a w-voxel wall is 2 ceil(w / 2)"""
    n = 32
    for w, exp in zip(range(1, 8), (1, 1, 4, 4, 9, 9, 16)):
        for lo in (7, 8, 9):
            t2 = R.thickness_numpy(R.slab(n, lo, w, axis=0), 8)
            assert (t2[lo:lo + w, 8:24, 8:24] == exp).all(), (w, lo)
            assert exp == ((w + 1) // 2) ** 2


def test_full_grid_is_bounded_by_the_walls():
    """outside the grid counts as empty: the full 32^3 grid reads 16^2 at its centre at rmax 32, not 32^2, and every ball stays inside"""
    n = 32
    vox = np.ones((n, n, n), bool)
    D = R.capped_radius(vox, 32)
    assert np.array_equal(D, R.wall_radius(n)) and D.max() == 256 and D.min() == 1
    t2 = R.thickness_numpy(vox, 32, D)
    assert t2.max() == 256 and t2[15:17, 15:17, 15:17].min() == 256
    assert t2[0, 0, 0] == 4                                          # the corner voxel: the ball of squared radius 4 around (1, 1, 1), q = 3
    assert (t2 >= D).all()


def test_ball():
    """a ball |p - c|^2 <= 81 at n = 32: its centre carries E = the squared distance to the nearest voxel outside, 82 = 9^2 + 1^2 (the
    smallest sum of three squares above 81), and every voxel of the ball lies inside that open ball"""
    n = 32
    vox = R.ball(n, (16, 16, 16), 81)
    e = R.edt_numpy(vox, R.UNSET)
    assert e[16, 16, 16] == 82
    t2 = R.thickness_numpy(vox, 32)
    assert (t2[vox] == 82).all() and not t2[~vox].any()
    t2 = R.thickness_numpy(vox, 4)
    assert t2[16, 16, 16] == 16 and t2[vox].min() >= 1


def test_dumbbell():
    vox = R.dumbbell()
    for rmax in (4, 8):
        t2 = R.thickness_numpy(vox, rmax)
        assert t2[32, 32, 32] == 4                                   # the rod's centre: the 3 x 3 rod reads 2 ceil(3 / 2) = 4 voxels
        assert t2[32, 32, 16] == rmax * rmax and t2[32, 32, 48] == rmax * rmax
        thin = R.thin_numpy(vox, t2, R.thin2_of_width(6))            # thinner than 6 voxels: T2 < 9
        assert R.thin2_of_width(6) == 9 and int(thin.sum()) == 99
        assert thin[31:34, 31:34, 27:38].all() and int(thin[31:34, 31:34, 27:38].sum()) == 99


def test_thin_width_rule():
    """thin iff 4 T2 < W^2"""
    for w in range(1, 65):
        t = R.thin2_of_width(w)
        assert 4 * (t - 1) < w * w <= 4 * t


# ---- the five facts on random grids and their complements ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def randoms():
    out = []
    for name, vox in random_cases():
        res = {}
        for rmax in (1, 2, 4):
            D = R.capped_radius(vox, rmax)
            res[rmax] = (D, R.thickness_numpy(vox, rmax, D))
        out.append((name, vox, res))
    return out


def test_bounds(randoms):
    for name, vox, res in randoms:
        for rmax, (D, t2) in res.items():
            assert (t2 >= D).all(), (name, rmax)
            assert t2.max() == D.max(), (name, rmax)
            assert np.array_equal(t2 == 0, ~vox), (name, rmax)
            assert D[vox].min() >= 1 and D.max() <= rmax * rmax, (name, rmax)


def test_saturated_region_is_one_more_transform(randoms):
    seen = 0
    for name, vox, res in randoms:
        for rmax, (D, t2) in res.items():
            sat = t2 == rmax * rmax
            assert np.array_equal(sat, R.saturated_by_transform(vox, rmax)), (name, rmax)
            seen += int(sat.any() and not sat[vox].all())
    assert seen >= 3                                                  # grids that are saturated in part


def test_cap_consistency(randoms):
    strict = 0
    for name, vox, res in randoms:
        for r, rr in ((1, 2), (1, 4), (2, 4)):
            small, large = res[r][1].astype(np.int64), res[rr][1].astype(np.int64)
            bound = np.minimum(large, r * r)
            assert (small <= bound).all(), (name, r, rr)
            below = large < r * r
            assert np.array_equal(small[below], large[below]), (name, r, rr)
            strict += int((small < bound).sum())
    assert strict > 0                                                 # the inequality is strict somewhere (a cut-down ball covers less)


def test_opening_lies_below_the_thickness(randoms):
    for name, vox, res in randoms:
        for rmax, (D, t2) in res.items():
            for t in np.unique(D[D > 0]):
                opened = R.edt_seeds(D >= t).astype(np.int64) < t
                assert (t2[opened] >= t).all(), (name, rmax, int(t))


def test_ball_volume_sum_counts_pairs():
    vox = R.words_to_bool(R.random_grid(32, 0.97, 7), 32)
    D = R.capped_radius(vox, 3)
    n = 32
    a = np.arange(-2, 3)
    q = a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2
    exp = sum(int((q < d).sum()) for d in D[D > 0])
    assert R.ball_volume_sum(D) == exp and n == 32


# ---- the host form through the C++ API ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    pkg = os.path.dirname(capi.LIB_PATH)
    build.build_lib()
    srcs = [os.path.join(pkg, "vplib", "src", f) for f in sorted(os.listdir(os.path.join(pkg, "vplib", "src"))) if f.endswith(".cpp")]
    exe = str(tmp_path_factory.mktemp("thickness") / "thickness_check")
    subprocess.check_call(["g++", "-std=c++23", "-O2", "-ffp-contract=off", "-fopenmp",
                           "-I", os.path.join(pkg, "vplib", "include"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "thickness_check.cpp")] + srcs + ["-o", exe, "-L", pkg, "-lvphip", "-Wl,-rpath," + pkg])
    return exe


def run_check(exe, words, n, rmax, thin2, bits, types, prefix, timeout=900):
    np.asarray(words, np.uint32).tofile(prefix + ".in.u32")
    p = subprocess.run([exe, prefix + ".in.u32", str(n), str(rmax), str(thin2), str(bits), types, prefix], check=True, timeout=timeout,
                       capture_output=True, text=True)
    counts = dict(re.findall(r"^(seq|omp|naive|tiled) (\d+)$", p.stdout, re.M))
    tags = {"s": "seq", "o": "omp", "n": "naive", "t": "tiled"}
    return {tags[c]: (np.fromfile("%s.%s.t2.u32" % (prefix, tags[c]), np.uint32), np.fromfile("%s.%s.thin.u32" % (prefix, tags[c]), np.uint32),
                      int(counts[tags[c]])) for c in types}


def test_cpp_host_form_equals_the_restatement_bit_for_bit(check_exe, tmp_path):
    cases = [(name, vox, rmax) for name, rmax, vox, _ in R.hand_cases(32) if "axis=1" not in name and "axis=0" not in name]
    cases += [(name, vox, rmax) for name, vox in random_cases() for rmax in (2, 5)]
    cases += [("full 32", np.ones((32,) * 3, bool), 32), ("dumbbell", R.dumbbell(), 8), ("dumbbell", R.dumbbell(), 16)]
    for k, (name, vox, rmax) in enumerate(cases):
        n = vox.shape[0]
        exp = R.thickness_numpy(vox, rmax)
        thin2 = (0, 1, R.thin2_of_width(min(3, 2 * rmax)), rmax * rmax)[k % 4]
        exp_thin = R.bool_to_words(R.thin_numpy(vox, exp, thin2))
        for bits in (32, 64):
            got = run_check(check_exe, R.bool_to_words(vox), n, rmax, thin2, bits, "so", str(tmp_path / "c"))
            for tag, (t2, thin, count) in got.items():
                assert np.array_equal(t2, exp.reshape(-1)), (name, rmax, bits, tag, int((t2 != exp.reshape(-1)).sum()))
                assert np.array_equal(thin, exp_thin), (name, rmax, thin2, bits, tag)
                assert count == int(R.thin_numpy(vox, exp, thin2).sum()), (name, rmax, thin2, bits, tag)


# ---- the header, the ABI and the build list -----------------------------------------------------------------------------------------
def test_header_prototypes_abi_and_build_list():
    text = open(os.path.join(ROOT, "include", "vphip.h")).read()
    assert re.search(r"#define\s+VP_ABI_VERSION\s+6\b", text)
    flat = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("int vp_thickness(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, uint32_t rmax, uint32_t thin2, int algo, "
            "uint64_t* h_thin_count );") in flat
    assert "int vp_thickness_result(vp_ctx* ctx, uint32_t** d_t2, uint32_t** d_thin, uint32_t* h_n);" in flat
    assert ("int vp_thickness_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_words, uint32_t rmax, uint32_t thin2, int algo, "
            "uint32_t* h_t2, uint32_t* h_thin , uint64_t* h_thin_count );") in flat
    assert "thickness.hip" in build.HIP_SOURCES
    assert {"vp_thickness", "vp_thickness_result", "vp_thickness_host"} <= set(capi.SYMBOLS)
    # no timing key was added: the 64-bit mask of vp_prof_select is full
    assert len(capi.EVERY_PROF_KEY) == 55 and len(capi.HEADER_PROF_KEYS) == 64


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    return build.build_cli()


def test_cli_thickness_dumps_the_restatement(cli, tmp_path):
    n, rmax, width = 64, 8, 3
    exp = None
    for t in ("0", "3"):
        d = tmp_path / ("t" + t)
        d.mkdir()
        p = subprocess.run([cli, M.asset("torus.obj"), "-n", str(n), "-t", t, "--thickness", "%d:%d" % (rmax, width), "-d", str(d / "x")],
                           capture_output=True, text=True, timeout=600, cwd=str(d))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert re.search(r"^\[\w*Thickness\]: [0-9.]+ ms$", p.stdout, re.M), p.stdout
        vox = R.words_to_bool(np.fromfile(str(d / "x.grid.u32"), np.uint32), n)
        assert vox.any()
        if exp is None:
            exp = R.thickness_numpy(vox, rmax)
        got = np.fromfile(str(d / "x.thick.u32"), np.uint32)
        assert np.array_equal(got, exp.reshape(-1)), t
        thin = R.thin_numpy(vox, exp, R.thin2_of_width(width))
        assert np.array_equal(np.fromfile(str(d / "x.thin.u32"), np.uint32), R.bool_to_words(thin)), t
        m = re.search(r"^thickness: rmax 8, set voxels (\d+), min T2 (\d+)$", p.stdout, re.M)
        assert m and int(m.group(1)) == int(vox.sum()) and int(m.group(2)) == int(got[got > 0].min()), p.stdout
        hist = dict((int(a), int(b)) for a, b in re.findall(r" (\d+): (\d+)", re.search(r"^thickness histogram.*$", p.stdout, re.M).group(0)))
        assert hist == {int(v): int(c) for v, c in zip(*np.unique(got[got > 0], return_counts=True))}
        m = re.search(r"^thin voxels \(thinner than 3 voxels, T2 < 3\): (\d+)$", p.stdout, re.M)
        assert m and int(m.group(1)) == int(thin.sum()), p.stdout


def test_cli_thin_only_exports_the_thin_grid(cli, tmp_path):
    n = 64
    p = subprocess.run([cli, M.asset("torus.obj"), "-n", str(n), "-t", "0", "--morph", "erode:1", "--thickness", "8:16", "--thin-only", "-e",
                        "-d", str(tmp_path / "x")], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    grid = np.fromfile(str(tmp_path / "x.grid.u32"), np.uint32)
    assert grid.any() and np.array_equal(grid, np.fromfile(str(tmp_path / "x.thin.u32"), np.uint32))
    thick = np.fromfile(str(tmp_path / "x.thick.u32"), np.uint32)
    assert np.array_equal(R.words_to_bool(grid, n).reshape(-1), (thick > 0) & (thick < 64))
    out = [f for f in os.listdir(str(tmp_path / "out")) if f.startswith("thin_")]
    assert out and os.path.getsize(str(tmp_path / "out" / out[0])) > 0


def test_cli_thickness_usage_errors(cli, tmp_path):
    mesh = M.asset("d20.obj")
    for args in ([mesh, "--thickness", "0"], [mesh, "--thickness", "33"], [mesh, "--thickness", "4:9"], [mesh, "--thickness", "4:0"],
                 [mesh, "--thickness", "x"], [mesh, "--thickness", "4", "--thin-only"], [mesh, "--thin-only"],
                 [mesh, "--thickness", "4:2", "-g", "2"]):
        p = subprocess.run([cli] + args + ["-n", "32", "-t", "0"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert p.returncode != 0, args
