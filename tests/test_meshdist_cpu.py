"""The mesh distance field without a GPU: the numpy float32 restatement of tests/meshdist_ref.py against hand-written expectations (vertex,
edge and face regions, zero distances, triangles that contribute nothing, triangles outside the grid, the band edge, ties), against an
independent float64 distance, and the host restatement of vplib/src/meshdist.cpp through the C++ API and through `vpcli -t 0 -s --mesh-sdf`,
bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cuda_mesh_voxelization_amd import build, capi, mesh as M
from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshdist_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = 2.0 ** -24
# max |D2_f32 - D2_f64| / (u M^2) over d20, torus and sphere at n = 32, band 32, as measured: the float32 walk against
# the float64 projection-and-segments distance.  The assertion allows four times that against other libm / numpy builds.
MEASURED_F32_F64 = 2.254
MESHES = ("d20.obj", "torus.obj", "sphere.obj")


@pytest.fixture(scope="module")
def cli():
    return build.build_cli()


def unit_frame(n):
    """voxel size 1, origin 0: centres at i + 0.5, every hand-case value exact in float32"""
    return F(1.0), np.zeros(3, F)


def field(xyz, tri, n, band, vs=None, origin=None, sign=None):
    if vs is None:
        vs, origin = unit_frame(n)
    d, i = R.mesh_distance_f32(np.asarray(xyz, F), np.asarray(tri, np.uint32), n, vs, origin, band, sign)
    return d.reshape(n, n, n), i.reshape(n, n, n)                   # (z, y, x)


# one right triangle in the plane z = 4.5 with its legs along x and y: a = (4.5, 4.5), b = (12.5, 4.5), c = (4.5, 12.5)
TRI_XYZ = np.array([[4.5, 4.5, 4.5], [12.5, 4.5, 4.5], [4.5, 12.5, 4.5]], F)
TRI = np.array([[0, 1, 2]], np.uint32)


def test_constants_symbols_and_timing_keys_match_the_header():
    assert capi.MESH_NONE == R.NONE == 0xFFFFFFFF
    for s in ("vp_mesh_distance", "vp_mesh_distance_host", "vp_mesh_distance_stats"):
        assert s in capi.SYMBOLS
    header = open(os.path.join(ROOT, "include", "vphip.h")).read()
    assert "#define VP_ABI_VERSION 6" in header.replace("  ", " ") and "#define VP_MESH_NONE 0xFFFFFFFFu" in header
    fourth = header[header.index("VP_K_MD_SETUP = VP_K_END"):header.index("VP_K_ALL")]
    keys = [t.split("=")[0].strip().lower()[len("vp_k_"):] for t in
            "".join(line.split("/*")[0] for line in fourth.splitlines()).split(",") if t.strip()]
    assert keys == capi.MESHDIST_KERNELS
    assert capi.HEADER_PROF_KEYS == capi.EVERY_PROF_KEY + capi.MESHDIST_KERNELS and len(capi.HEADER_PROF_KEYS) <= 64
    assert capi.EVERY_PROF_KEY == capi.ALL_PROF_KEYS + capi.EDT_KERNELS                           # the first three enums did not grow
    assert header.index("VP_K_MD_SETUP = VP_K_END") > header.index("VP_K_EDT_THRESH")
    assert "meshdist.hip" in build.HIP_SOURCES


def test_vertex_edge_and_face_regions_of_one_triangle():
    n, band = 32, 8
    d, i = field(TRI_XYZ, TRI, n, band)
    # the face: above the interior, the distance is the height
    assert d[6, 6, 6] == 4.0 and i[6, 6, 6] == 0                      # centre (6.5, 6.5, 6.5): 2 above the plane
    # vertex a: beyond both legs
    assert d[4, 2, 1] == 3.0 ** 2 + 2.0 ** 2 + 0.0                    # centre (1.5, 2.5, 4.5)
    assert d[2, 3, 3] == 1.0 + 1.0 + 4.0                              # (3.5, 3.5, 2.5)
    # vertices b and c
    assert d[4, 4, 15] == 9.0 and d[4, 15, 4] == 9.0                  # (15.5, 4.5, 4.5), (4.5, 15.5, 4.5)
    # edge ab (y below the leg), edge ac (x left of the leg)
    assert d[4, 2, 8] == 4.0 and d[5, 8, 2] == 4.0 + 1.0
    # edge bc, the hypotenuse x + y = 17: centre (10.5, 10.5, 4.5) is 2 sqrt(2) away
    assert d[4, 10, 10] == 8.0
    # all seven regions occur inside the band
    P = R.centres(n, *unit_frame(n))
    a, b, c = TRI_XYZ
    ab, ac = b - a, c - a
    d1, d2 = (P - a) @ ab, (P - a) @ ac
    d3, d4 = (P - b) @ ab, (P - b) @ ac
    d5, d6 = (P - c) @ ab, (P - c) @ ac
    inband = (d.reshape(-1) < band * band)
    regions = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (d6 >= 0) & (d5 <= d6)]
    for r in regions:
        assert (r & inband).any()
    assert (~regions[0] & ~regions[1] & ~regions[2] & inband).sum() > 100


def test_centres_on_a_vertex_an_edge_and_the_face_read_zero():
    n = 32
    words = np.zeros(n ** 3 // 32, np.uint32)
    d, i = field(TRI_XYZ, TRI, n, 2, sign=words)                       # every voxel unset: zeros are -0.0
    for z, y, x in ((4, 4, 4), (4, 4, 12), (4, 12, 4), (4, 4, 8), (4, 8, 4), (4, 8, 8), (4, 6, 6)):
        assert d[z, y, x] == 0.0 and np.signbit(d[z, y, x]) and i[z, y, x] == 0, (z, y, x)
    du, _ = field(TRI_XYZ, TRI, n, 2)
    assert not np.signbit(du).any() and np.array_equal(np.abs(d), du)
    words[:] = 0xFFFFFFFF
    dp, _ = field(TRI_XYZ, TRI, n, 2, sign=words)
    assert np.array_equal(dp.view(np.uint32), du.view(np.uint32))


def test_triangles_that_contribute_nothing():
    n, band = 32, 3
    xyz = np.concatenate([TRI_XYZ, [[np.nan, 1, 1], [np.inf, 2, 2], [20.5, 20.5, 20.5], [22.5, 22.5, 22.5], [21.5, 21.5, 21.5]]]).astype(F)
    bad = np.array([[0, 1, 9], [0, 3, 2], [4, 1, 2], [5, 6, 7], [5, 5, 6]], np.uint32)     # index, NaN, inf, collinear, repeated vertex
    assert R.valid_triangles(xyz, bad).size == 0
    d, i = field(xyz, bad, n, band)
    assert (d == 9.0).all() and (i == R.NONE).all()
    both = np.concatenate([bad, TRI])
    d2, i2 = field(xyz, both, n, band)
    d1, i1 = field(TRI_XYZ, TRI, n, band)
    assert np.array_equal(d2, d1) and np.array_equal(i2 == R.NONE, i1 == R.NONE) and (i2[i2 != R.NONE] == 5).all()


def test_no_triangles_and_triangles_outside_the_grid():
    n, band = 32, 2
    d, i = field(np.zeros((0, 3), F), np.zeros((0, 3), np.uint32), n, band)
    assert (d == 4.0).all() and (i == R.NONE).all()
    words = np.zeros(n ** 3 // 32, np.uint32)
    words[5] = 0x80000001
    d, _ = field(np.zeros((0, 3), F), np.zeros((0, 3), np.uint32), n, band, sign=words)
    assert (d.reshape(-1)[[160, 191]] == 4.0).all() and (np.delete(d.reshape(-1), [160, 191]) == -4.0).all()
    far = TRI_XYZ + F(100.0)                                            # wholly outside, further than the band
    d, i = field(far, TRI, n, band)
    assert (d == 4.0).all() and (i == R.NONE).all()
    part = TRI_XYZ + np.array([-8.0, 0, 0], F)                          # a = (-3.5, ...): the left part hangs out of the grid
    d, i = field(part, TRI, n, band)
    assert d[4, 4, 0] == 0.0 and d[4, 4, 4] == 0.0 and d[4, 4, 5] == 1.0 and d[5, 6, 0] == 1.0 and i[5, 6, 0] == 0
    near = TRI_XYZ + np.array([-13.5, 0, 0], F)                         # b = (-1, 4.5, 4.5): outside, but within the band of column x = 0
    d, i = field(near, TRI, n, band)
    assert d[4, 4, 0] == 2.25 and i[4, 4, 0] == 0 and d[4, 4, 1] == 4.0 and i[4, 4, 1] == R.NONE


def test_the_band_edge_is_outside_the_band():
    n, band = 32, 2
    d, i = field(TRI_XYZ, TRI, n, band)
    assert d[6, 6, 6] == 4.0 and i[6, 6, 6] == R.NONE                   # exactly B above the face: not within the band
    assert d[4, 4, 14] == 4.0 and i[4, 4, 14] == R.NONE                 # exactly B beyond vertex b
    assert d[5, 6, 6] == 1.0 and i[5, 6, 6] == 0
    d3, i3 = field(TRI_XYZ, TRI, n, 3)
    assert d3[6, 6, 6] == 4.0 and i3[6, 6, 6] == 0


def test_ties_resolve_to_the_lowest_index():
    n, band = 32, 6
    hub = np.array([10.5, 10.5, 10.5], F)
    ring = [hub + np.array([4 * np.cos(k * np.pi / 3), 4 * np.sin(k * np.pi / 3), -3.0], F) for k in range(6)]
    xyz = np.array([hub] + ring, F)
    fan = np.array([[0, 1 + k, 1 + (k + 1) % 6] for k in range(6)], np.uint32)
    fan = np.concatenate([fan[3:], fan[:3]])                             # the order of the list is not the order around the hub
    d, i = field(xyz, fan, n, band)
    assert d[10, 10, 10] == 0.0 and i[10, 10, 10] == 0                  # the hub itself: all six tie
    assert d[13, 10, 10] == 9.0 and i[13, 10, 10] == 0                  # above the apex of the cone: the hub is the closest point of all six
    twice = np.concatenate([TRI, TRI, TRI])
    d, i = field(TRI_XYZ, twice, n, band)
    assert set(np.unique(i)) == {0, R.NONE}
    rev = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1]], np.uint32)          # the same triangle from each vertex: values may differ in the last bit
    d, i = field(TRI_XYZ, rev, n, band)
    assert (i[d < 36.0] <= 2).all()


# a sliver (height about 1e-7 of its length) in the unit frame, as float32 bit patterns: at two centres the walk reaches the face region
# with va, vb, vc of mixed signs, and the face's two clamps change the bits of D2
SLIVER_XYZ = np.array([0x4169480b, 0x4137b223, 0x4173619a, 0x4181a45f, 0x4094949d, 0x40c3dfd0, 0x417b4d29, 0x40d7c137, 0x410e9684],
                      np.uint32).view(F).reshape(3, 3)
SLIVER_BAND = 6


def test_sliver_reaches_the_face_region_with_mixed_signs():
    n = 32
    P = R.centres(n, *unit_frame(n))
    a, b, c = SLIVER_XYZ[0:1], SLIVER_XYZ[1:2], SLIVER_XYZ[2:3]
    assert R.valid_triangles(SLIVER_XYZ, TRI).size == 1
    with np.errstate(all="ignore"):
        clamped, free = R.pair_d2_f32(P, a, b, c)[:, 0], R.pair_d2_f32(P, a, b, c, clamp=False)[:, 0]
    differ = np.nonzero(clamped.view(np.uint32) != free.view(np.uint32))[0]
    assert differ.tolist() == [9517, 9519] and (clamped[differ] < SLIVER_BAND ** 2).all()           # inside the band: the clamps decide bits
    d, i = field(SLIVER_XYZ, TRI, n, SLIVER_BAND)
    assert np.array_equal(d.reshape(-1)[differ], clamped[differ]) and (i.reshape(-1)[differ] == 0).all()
    # q stays a point of the triangle, so the value is never below the true distance -- and for a sliver it can be well above it
    d64, _, _ = R.mesh_distance_f64(SLIVER_XYZ, TRI, n, *unit_frame(n))
    inband = d.reshape(-1) < SLIVER_BAND ** 2
    assert (d.reshape(-1)[inband] >= d64[inband] * (1 - 1e-5)).all()


def _mesh_case(name, n):
    xyz, tri = M.import_mesh(M.asset(name))
    origin, vs = M.frame([xyz], n)
    return xyz, tri, origin, vs


def test_float32_contract_against_an_independent_float64_distance():
    n, band = 32, 32                                                   # band 32 at n = 32: every voxel is within the band
    worst = 0.0
    for name in MESHES:
        xyz, tri, origin, vs = _mesh_case(name, n)
        d32, i32 = R.mesh_distance_f32(xyz, tri, n, vs, origin, band)
        d64, i64, second = R.mesh_distance_f64(xyz, tri, n, vs, origin)
        B2 = float(F(F(band) * vs) * F(F(band) * vs))
        inside = d64 < B2 * (1 - 1e-4)
        assert inside.sum() > 0.5 * n ** 3, name
        Mx = max(float(np.abs(R.centres(n, vs, origin)).max()), float(np.abs(xyz).max()))
        err = np.abs(d32[inside].astype(np.float64) - d64[inside]) / (U * Mx * Mx)
        print("%s: max |D2_f32 - D2_f64| / (u M^2) = %.3f (mean %.4f), M = %g" % (name, err.max(), err.mean(), Mx))
        worst = max(worst, float(err.max()))
        bound = 4 * MEASURED_F32_F64 * U * Mx * Mx
        assert err.max() <= 4 * MEASURED_F32_F64, (name, float(err.max()))
        unique = inside & (second - d64 > bound)                       # the float64 minimum is unique by more than the bound
        assert unique.sum() > 0.2 * inside.sum(), name
        assert np.array_equal(i32[unique].astype(np.int64), i64[unique]), name
    print("worst over the three meshes: %.3f" % worst)
    assert worst >= MEASURED_F32_F64 / 4                                # the recorded figure is the measured one, not a loose cap


def _words(xyz, tri, n, vs, origin):
    return O.voxelize(xyz, tri, n, vs, origin)


def _build_check(tmp_path):
    pkg = os.path.dirname(capi.LIB_PATH)
    build.build_lib()
    srcs = [os.path.join(pkg, "vplib", "src", f) for f in sorted(os.listdir(os.path.join(pkg, "vplib", "src"))) if f.endswith(".cpp")]
    exe = str(tmp_path / "meshdist_check")
    subprocess.check_call(["g++", "-std=c++23", "-O2", "-ffp-contract=off", "-fopenmp",
                           "-I", os.path.join(pkg, "vplib", "include"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "meshdist_check.cpp")] + srcs + ["-o", exe, "-L", pkg, "-lvphip", "-Wl,-rpath," + pkg])
    return exe


CPP_CASES = [("d20.obj", 32), ("torus.obj", 32), ("sphere.obj", 32), ("d20.obj", 64)]


def test_cpp_host_restatement_equals_the_numpy_restatement(tmp_path):
    exe = _build_check(tmp_path)
    band = 2
    for name, n in CPP_CASES:
        xyz, tri, origin, vs = _mesh_case(name, n)
        words = _words(xyz, tri, n, vs, origin)
        for signed in (1, 0):
            prefix = str(tmp_path / ("%s_%d_%d" % (name, n, signed)))
            subprocess.run([exe, M.asset(name), str(n), str(band), str(signed), "0", prefix], check=True, timeout=600, capture_output=True)
            exp_d, exp_i = R.mesh_distance_f32(xyz, tri, n, vs, origin, band, words if signed else None)
            for tag in ("seq", "omp"):
                got_d = np.fromfile(prefix + "." + tag + ".dist.f32", np.uint32)
                got_i = np.fromfile(prefix + "." + tag + ".near.u32", np.uint32)
                assert np.array_equal(got_d, exp_d.view(np.uint32)), (name, n, signed, tag, int((got_d != exp_d.view(np.uint32)).sum()))
                assert np.array_equal(got_i, exp_i), (name, n, signed, tag)
            if signed:
                assert np.signbit(exp_d).any() and (~np.signbit(exp_d)).any()
    # the sliver whose face region needs the clamps, padded by two small triangles in opposite corners that make the frame the unit frame of side 32
    xyz = np.concatenate([SLIVER_XYZ, np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [32, 32, 32], [31, 32, 32], [32, 31, 32]], F)])
    tri = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.uint32)
    obj = str(tmp_path / "sliver.obj")
    with open(obj, "w") as f:
        f.write("".join("v %.9g %.9g %.9g\n" % tuple(v) for v in xyz) + "".join("f %d %d %d\n" % tuple(t + 1) for t in tri))
    rx, rt = M.import_mesh(obj)
    assert np.array_equal(rx.view(np.uint32), xyz.view(np.uint32)) and np.array_equal(rt, tri)
    origin, vs = M.frame([xyz], 32)
    assert vs == 1.0 and not origin.any()
    prefix = str(tmp_path / "sliver")
    subprocess.run([exe, obj, "32", str(SLIVER_BAND), "0", "0", prefix], check=True, timeout=600, capture_output=True)
    exp_d, exp_i = R.mesh_distance_f32(xyz, tri, 32, vs, origin, SLIVER_BAND)
    assert (exp_i[[9517, 9519]] == 0).all()
    for tag in ("seq", "omp"):
        assert np.array_equal(np.fromfile(prefix + "." + tag + ".dist.f32", np.uint32), exp_d.view(np.uint32)), tag
        assert np.array_equal(np.fromfile(prefix + "." + tag + ".near.u32", np.uint32), exp_i), tag


def test_cli_host_equals_the_numpy_restatement(cli, tmp_path):
    band = 2
    for name, n in CPP_CASES:
        xyz, tri, origin, vs = _mesh_case(name, n)
        d = tmp_path / ("%s_%d" % (name, n))
        d.mkdir()
        p = subprocess.run([cli, M.asset(name), "-n", str(n), "-t", "0", "-s", "--mesh-sdf", str(band), "-d", str(d / "x")],
                           capture_output=True, text=True, timeout=600, cwd=str(d))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert "MeshDistance" in p.stdout
        words = np.fromfile(str(d / "x.grid.u32"), np.uint32)
        assert np.array_equal(words, _words(xyz, tri, n, vs, origin))
        exp_d, _ = R.mesh_distance_f32(xyz, tri, n, vs, origin, band, words)
        got = np.fromfile(str(d / "x.sdf.f32"), np.uint32)
        assert np.array_equal(got, exp_d.view(np.uint32)), (name, n, int((got != exp_d.view(np.uint32)).sum()))


def test_cli_usage_errors(cli, tmp_path):
    mesh = M.asset("d20.obj")
    for args in ([mesh, "--mesh-sdf", "2"],                               # without -s
                 [mesh, "-s", "--mesh-sdf", "0"], [mesh, "-s", "--mesh-sdf", "33"], [mesh, "-s", "--mesh-sdf", "x"],
                 [mesh, "-s", "--mesh-sdf", "2", "--exact-sdf"],
                 [mesh, M.asset("torus.obj"), "-s", "--mesh-sdf", "2"],    # two meshes
                 [mesh, "-s", "--mesh-sdf", "2", "-p", "1"]):              # a CSG operation
        p = subprocess.run([cli] + args + ["-n", "32", "-t", "0"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert p.returncode != 0, args
    p = subprocess.run([cli, mesh, M.asset("torus.obj"), "-s", "--mesh-sdf", "2", "-n", "32", "-t", "0"], capture_output=True, text=True,
                       timeout=300, cwd=str(tmp_path))
    assert "single mesh" in p.stdout + p.stderr
