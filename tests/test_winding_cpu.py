"""The generalized winding number without a GPU: the numpy float32 restatement of tests/winding_ref.py against hand-written expectations
(one triangle against the spherical-excess solid angle, a tetrahedron, its inverse, two overlapping cubes, centres on a vertex and in a
face, triangles that contribute nothing, no triangles), against an independent float64 brute force and a float64 ray parity, the far field
against the brute force, what the sign is for (iso-nets of a mesh-distance field signed by it), and the host restatement of
vplib/src/winding.cpp through the C++ API and through `vpcli --winding`, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from cuda_mesh_voxelization_amd import build, capi, mesh as M
from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import winding_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CLOSED = ("d20.obj", "torus.obj", "sphere.obj")
# max |w_f32 - w_f64| at beta = 0 over d20, torus and sphere at n = 32, as measured (5.7e-7, 6.4e-7, 1.13e-6): the
# float32 contract with the library's atan2 polynomial against the float64 brute force with np.arctan2.  The assertion allows four times
# that, the margin of the mesh distance field's float32 against float64.
MEASURED_B0 = 1.14e-6
# max |w_f32(beta) - w_f64| per case as measured; the assertion allows twice the largest of a beta
MEASURED_FAR = {2.0: {"d20.obj": 0.00097, "torus.obj": 0.0266, "sphere.obj": 0.0229, "torus.obj@96": 0.0345, "open": 0.0238},
                3.0: {"d20.obj": 6e-7, "torus.obj": 0.0125, "sphere.obj": 0.0029, "torus.obj@96": 0.0166, "open": 0.0032}}
FAR_BOUND = {b: 2 * max(v.values()) for b, v in MEASURED_FAR.items()}


def bits_of(words):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little").astype(bool)


def unit_frame():
    return F(1.0), np.zeros(3, F)


def mesh_case(name, n):
    xyz, tri = M.import_mesh(M.asset(name))
    origin, vs = M.frame([xyz], n)
    return xyz, tri, origin, vs


def open_sphere():
    """sphere.obj without the triangles whose centroid lies above 0.8 of its z extent"""
    xyz, tri = M.import_mesh(M.asset("sphere.obj"))
    cz = xyz[tri.astype(np.int64)][:, :, 2].astype(np.float64).mean(1)
    zlo, zhi = float(xyz[:, 2].min()), float(xyz[:, 2].max())
    tri = np.ascontiguousarray(tri[~(cz > zlo + 0.8 * (zhi - zlo))])
    origin, vs = M.frame([xyz], 32)
    return xyz, tri, origin, vs


def far_cases():
    for name in CLOSED:
        yield (name,) + mesh_case(name, 32) + (32,)
    yield ("torus.obj@96",) + mesh_case("torus.obj", 96) + (96,)
    yield ("open",) + open_sphere() + (32,)


# ---- hand cases, n = 32, unit frame ----------------------------------------------------------------------------------------------
def box(lo, hi):
    """12 outward counter-clockwise triangles of an axis-aligned box"""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    v = np.array([[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0], [x0, y0, z1], [x1, y0, z1], [x1, y1, z1], [x0, y1, z1]], F)
    t = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [2, 3, 7], [2, 7, 6], [1, 2, 6], [1, 6, 5], [0, 4, 7], [0, 7, 3]],
                 np.uint32)
    return v, t


TETRA_XYZ = np.array([[4.2, 5.1, 6.3], [25.7, 8.4, 7.9], [12.3, 27.6, 9.2], [14.1, 13.8, 26.4]], F)
TETRA = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.uint32)         # outward


def in_tetra(P, v):
    P = P.astype(np.float64)
    v = v.astype(np.float64)
    inside = np.ones(len(P), bool)
    for f, opp in (((0, 2, 1), 3), ((0, 1, 3), 2), ((1, 2, 3), 0), ((2, 0, 3), 1)):
        nrm = np.cross(v[f[1]] - v[f[0]], v[f[2]] - v[f[0]])
        assert nrm @ (v[opp] - v[f[0]]) < 0                        # the face is outward
        inside &= (P - v[f[0]]) @ nrm < 0
    return inside


def solid_angle_excess(p, a, b, c):
    """float64 signed solid angle by the spherical excess (l'Huilier), independent of the Van Oosterom-Strackee form"""
    u = [(q - p) / np.linalg.norm(q - p) for q in (a, b, c)]
    ang = lambda s, t: np.arccos(np.clip(s @ t, -1.0, 1.0))        # noqa: E731
    A, B, C = ang(u[1], u[2]), ang(u[2], u[0]), ang(u[0], u[1])
    s = (A + B + C) / 2
    e = 4 * np.arctan(np.sqrt(max(0.0, np.tan(s / 2) * np.tan((s - A) / 2) * np.tan((s - B) / 2) * np.tan((s - C) / 2))))
    return np.sign(u[0] @ np.cross(u[1], u[2])) * e


def test_symbols_constants_and_sources():
    for s in ("vp_winding", "vp_winding_result", "vp_winding_host"):
        assert s in capi.SYMBOLS
    header = open(os.path.join(ROOT, "include", "vphip.h")).read()
    assert "#define VP_ABI_VERSION 6" in header.replace("  ", " ")
    for k, c in enumerate(R.ATAN_C):
        assert "#define VP_WN_ATAN_C%d %sf" % (k, float(c).hex().replace("0000000p", "p")) in header, k
    assert float(R.PI) == float(F(np.pi)) and float(R.HALF_PI) == float(F(np.pi / 2)) and R.FOUR_PI == 4 * np.pi
    assert "winding.hip" in build.HIP_SOURCES


def test_the_atan2_polynomial_against_numpy():
    rng = np.random.default_rng(17)
    ang, rad = rng.uniform(-np.pi, np.pi, 1 << 20), np.exp(rng.uniform(-20, 20, 1 << 20))
    x, y = (rad * np.cos(ang)).astype(F), (rad * np.sin(ang)).astype(F)
    x[:8] = [1, -1, 0, 0, 1, -1, 1, -1]
    y[:8] = [0, 0, 1, -1, 1, 1, -1, -1]
    err = np.abs(R.atan2w(y, x).astype(np.float64) - np.arctan2(y.astype(np.float64), x.astype(np.float64)))
    print("max |atan2w - arctan2| = %.3e" % err.max())
    assert err.max() <= 4.0e-7                                     # 2.7e-7 measured; float32 pi itself is 8.7e-8 off
    assert R.atan2w(F([0.0]), F([1.0]))[0] == 0.0 and R.atan2w(F([1.0]), F([0.0]))[0] == R.HALF_PI and R.atan2w(F([0.0]), F([-1.0]))[0] == R.PI


def test_one_triangle_against_the_spherical_excess():
    n = 32
    xyz = np.array([[6.2, 7.3, 12.1], [24.9, 9.8, 13.4], [11.6, 25.2, 15.3]], F)
    tri = np.array([[0, 1, 2]], np.uint32)
    w, _ = R.winding_f32(xyz, tri, n, *unit_frame())
    w = w.reshape(n, n, n)
    P = R.centres(n, *unit_frame()).reshape(n, n, n, 3).astype(np.float64)
    a, b, c = xyz.astype(np.float64)
    worst = 0.0
    for z, y, x in ((0, 0, 0), (31, 31, 31), (20, 14, 13), (5, 14, 13), (13, 3, 29), (14, 12, 14), (12, 12, 14)):
        exp = solid_angle_excess(P[z, y, x], a, b, c) / (4 * np.pi)
        worst = max(worst, abs(float(w[z, y, x]) - exp))
        assert abs(float(w[z, y, x]) - exp) <= 4 * MEASURED_B0, (z, y, x, float(w[z, y, x]), exp)
    print("one triangle: max |w - excess / 4 pi| = %.3e" % worst)
    assert w.max() > 0.2 and w.min() < -0.2                         # both sides of the triangle, close to it
    rev, _ = R.winding_f32(xyz, tri[:, ::-1], n, *unit_frame())
    assert np.abs(rev.reshape(n, n, n) + w).max() <= 4 * MEASURED_B0        # the other vertex order rounds differently: not the same bits


def test_closed_tetrahedron_and_its_inverse():
    n = 32
    P = R.centres(n, *unit_frame())
    inside = in_tetra(P, TETRA_XYZ)
    assert 500 < inside.sum() < n ** 3 // 4
    w, words = R.winding_f32(TETRA_XYZ, TETRA, n, *unit_frame())
    assert np.abs(w - inside).max() <= 4 * MEASURED_B0
    assert np.array_equal(bits_of(words), inside)
    wi, wordsi = R.winding_f32(TETRA_XYZ, TETRA[:, ::-1], n, *unit_frame())
    assert np.abs(wi + w).max() <= 4 * MEASURED_B0 and not wordsi.any()
    assert np.abs(wi + inside).max() <= 4 * MEASURED_B0            # -1 inside
    _, neg = R.winding_f32(TETRA_XYZ, TETRA[:, ::-1], n, *unit_frame(), level=-0.5)
    assert np.array_equal(bits_of(neg), ~inside)                    # w >= -0.5: everything but the inverted solid


def test_two_overlapping_cubes_union_and_intersection():
    n = 32
    va, ta = box((4.25, 5.25, 6.25), (20.25, 19.25, 18.25))
    vb, tb = box((12.75, 10.75, 9.75), (27.75, 26.75, 25.75))
    xyz, tri = np.concatenate([va, vb]), np.concatenate([ta, tb + 8])
    P = R.centres(n, *unit_frame()).astype(np.float64)
    ina = ((P > va.min(0)) & (P < va.max(0))).all(1)
    inb = ((P > vb.min(0)) & (P < vb.max(0))).all(1)
    assert (ina & inb).sum() > 100 and (ina & ~inb).sum() > 100 and (inb & ~ina).sum() > 100
    w, union = R.winding_f32(xyz, tri, n, *unit_frame(), level=0.5)
    assert np.abs(w - (ina.astype(int) + inb)).max() <= 8 * MEASURED_B0          # two shells: twice the terms
    assert np.array_equal(bits_of(union), ina | inb)
    _, both = R.winding_f32(xyz, tri, n, *unit_frame(), level=1.5)
    assert np.array_equal(bits_of(both), ina & inb)


def test_centres_on_a_vertex_and_in_a_face_take_the_principal_value():
    n = 32
    v, t = box((4.5, 4.5, 4.5), (20.5, 20.5, 20.5))                 # corners and faces pass through voxel centres
    w, words = R.winding_f32(v, t, n, *unit_frame())
    w = w.reshape(n, n, n)
    assert abs(float(w[4, 4, 4]) - 0.125) <= 4 * MEASURED_B0         # on a vertex: the three far faces subtend pi / 2
    assert abs(float(w[4, 10, 10]) - 0.5) <= 4 * MEASURED_B0         # in the face z = 4.5: the other five subtend 2 pi
    assert abs(float(w[4, 4, 10]) - 0.25) <= 4 * MEASURED_B0         # on an edge
    assert abs(float(w[10, 10, 10]) - 1.0) <= 4 * MEASURED_B0 and abs(float(w[2, 10, 10])) <= 4 * MEASURED_B0
    # the pairs with det == 0 contributed exactly nothing: the same value without the faces through the point
    others = np.array([k for k in range(12) if k not in (0, 1)], np.int64)        # t[0], t[1] = the face z = 4.5
    wo, _ = R.winding_f32(v, t[others], n, *unit_frame())
    assert wo.reshape(n, n, n)[4, 10, 10] == w[4, 10, 10]


def test_triangles_that_contribute_nothing_and_the_empty_mesh():
    n = 32
    xyz = np.concatenate([TETRA_XYZ, [[np.nan, 1, 1], [np.inf, 2, 2], [20.5, 20.5, 20.5], [22.5, 22.5, 22.5], [21.5, 21.5, 21.5]]]).astype(F)
    bad = np.array([[0, 1, 9], [0, 4, 2], [5, 1, 2], [6, 7, 8], [6, 6, 7]], np.uint32)      # index, NaN, inf, collinear, repeated vertex
    assert R.valid_triangles(xyz, bad).size == 0
    w, words = R.winding_f32(xyz, bad, n, *unit_frame())
    assert not w.any() and not np.signbit(w).any() and not words.any()
    mixed = np.concatenate([bad[:2], TETRA[:2], bad[2:], TETRA[2:]])
    w2, words2 = R.winding_f32(xyz, mixed, n, *unit_frame())
    w1, words1 = R.winding_f32(TETRA_XYZ, TETRA, n, *unit_frame())
    assert np.array_equal(w2.view(np.uint32), w1.view(np.uint32)) and np.array_equal(words2, words1)
    w0, words0 = R.winding_f32(np.zeros((0, 3), F), np.zeros((0, 3), np.uint32), n, *unit_frame())
    assert not w0.any() and not words0.any()
    _, all_in = R.winding_f32(np.zeros((0, 3), F), np.zeros((0, 3), np.uint32), n, *unit_frame(), level=0.0)
    assert (all_in == 0xFFFFFFFF).all()                             # w = 0 >= 0 everywhere


def test_the_pyramid_is_uneven_at_96_and_clamps_leaves():
    assert R.level_dims(96) == [12, 6, 3, 2, 1] and R.level_dims(32) == [4, 2, 1] and R.level_dims(1024) == [128, 64, 32, 16, 8, 4, 2, 1]
    xyz, tri, origin, vs = mesh_case("d20.obj", 32)
    rec, off, levels = R.pyramid(xyz * F(3.0), tri, 32, vs, origin)               # scaled out of the frame: every triangle still has a leaf
    assert off[-1] == len(tri) == levels[-1]["count"][0]
    for k in range(1, len(levels)):
        assert levels[k]["count"].sum() == len(tri)


# ---- accuracy ----------------------------------------------------------------------------------------------------------------------
def test_float32_contract_against_the_float64_brute_force_without_far_field():
    worst = 0.0
    for name in CLOSED:
        xyz, tri, origin, vs = mesh_case(name, 32)
        w, _ = R.winding_f32(xyz, tri, 32, vs, origin, 0.0)
        w64 = R.winding_f64(xyz, tri, 32, vs, origin)
        err = float(np.abs(w - w64).max())
        print("%s: beta 0, max |w - w64| = %.3e" % (name, err))
        worst = max(worst, err)
        assert err <= 4 * MEASURED_B0, (name, err)
    assert worst >= MEASURED_B0 / 4                                  # the recorded figure is the measured one, not a loose cap


@pytest.mark.parametrize("beta", [2.0, 3.0])
def test_far_field_against_the_float64_brute_force(beta):
    for label, xyz, tri, origin, vs, n in far_cases():
        w, _ = R.winding_f32(xyz, tri, n, vs, origin, beta)
        w64 = R.winding_f64(xyz, tri, n, vs, origin)
        err = float(np.abs(w - w64).max())
        print("%s: beta %g, max |w - w64| = %.4g (recorded %.4g)" % (label, beta, err, MEASURED_FAR[beta][label]))
        assert err <= FAR_BOUND[beta], (label, beta, err)


def test_inside_bits_without_far_field_against_float64():
    for name in CLOSED:
        xyz, tri, origin, vs = mesh_case(name, 32)
        _, words = R.winding_f32(xyz, tri, 32, vs, origin, 0.0, 0.5)
        parity = R.parity_f64(xyz, tri, 32, vs, origin)
        assert 0 < parity.sum() < parity.size
        assert np.array_equal(bits_of(words), parity), (name, int((bits_of(words) != parity).sum()))
    xyz, tri, origin, vs = open_sphere()
    assert len(tri) == 1028
    _, words = R.winding_f32(xyz, tri, 32, vs, origin, 0.0, 0.5)
    w64 = R.winding_f64(xyz, tri, 32, vs, origin)
    sure = np.abs(w64 - 0.5) > 0.005
    print("open sphere: %.4f %% of the voxels within 0.005 of the level" % (100 * (~sure).mean()))
    assert (~sure).mean() <= 0.001
    assert np.array_equal(bits_of(words)[sure], w64[sure] >= 0.5)


def test_inside_bits_with_far_field_against_float64():
    beta = 2.0
    for label, xyz, tri, origin, vs, n in far_cases():
        _, words = R.winding_f32(xyz, tri, n, vs, origin, beta, 0.5)
        w64 = R.winding_f64(xyz, tri, n, vs, origin)
        sure = np.abs(w64 - 0.5) > FAR_BOUND[beta]
        print("%s: %.3f %% of the voxels within %.3f of the level" % (label, 100 * (~sure).mean(), FAR_BOUND[beta]))
        assert (~sure).mean() <= (0.05 if label == "open" else 0.0), label
        assert np.array_equal(bits_of(words)[sure], w64[sure] >= 0.5), label


# ---- what the sign is for -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere.obj", "d20.obj"])
def test_iso_nets_of_the_mesh_distance_signed_by_the_winding_grid(name):
    import isonets_ref as IR
    import meshdist_ref as MD
    import test_isonets_cpu as TI
    n, margin, band = 32, 4, 4
    xyz, tri = M.import_mesh(M.asset(name))
    lo, side = xyz.min(0), float((xyz.max(0) - xyz.min(0)).max())
    vs = F(side / (n - 2 * margin))
    origin = (lo - margin * vs).astype(F)
    _, words = R.winding_f32(xyz, tri, n, vs, origin, 0.0, 0.5)
    exact = TI.convex_sign_grid(xyz, tri, n, vs, origin)             # float64, centre-exact: the sign of the table in DESIGN.md section 16
    assert np.array_equal(bits_of(words).reshape(n, n, n), exact)
    column = O.voxelize(xyz, tri, n, vs, origin)                     # the reference's column rule
    assert not np.array_equal(column, words)
    worst = {}
    for tag, sign in (("winding", words), ("column rule", column)):
        dist, _ = MD.mesh_distance_f32(xyz, tri, n, vs, origin, band, sign)
        _, p, _, quads = IR.isonets_numpy(np.array(dist).reshape(n, n, n), IR.SIGNED_SQUARE, F(0.0))
        world = origin.astype(np.float64) + p.astype(np.float64) * float(vs)
        err = TI._point_mesh_distance(world, xyz, tri) / float(vs)
        worst[tag] = float(err.max())
        print("%s, iso 0, signed by the %s: V %d, error max %.4f mean %.4f voxels" % (name, tag, len(p), err.max(), err.mean()))
    assert worst["winding"] < worst["column rule"]


# ---- the host form --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    pkg = os.path.dirname(capi.LIB_PATH)
    build.build_lib()
    srcs = [os.path.join(pkg, "vplib", "src", f) for f in sorted(os.listdir(os.path.join(pkg, "vplib", "src"))) if f.endswith(".cpp")]
    exe = str(tmp_path_factory.mktemp("winding") / "winding_check")
    subprocess.check_call(["g++", "-std=c++23", "-O2", "-ffp-contract=off", "-fopenmp",
                           "-I", os.path.join(pkg, "vplib", "include"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "winding_check.cpp")] + srcs + ["-o", exe, "-L", pkg, "-lvphip", "-Wl,-rpath," + pkg])
    return exe


def write_obj(path, xyz, tri):
    with open(path, "w") as f:
        f.write("".join("v %.9g %.9g %.9g\n" % tuple(v) for v in xyz) + "".join("f %d %d %d\n" % tuple(int(i) + 1 for i in t) for t in tri))
    rx, rt = M.import_mesh(path)
    assert np.array_equal(rx.view(np.uint32), np.asarray(xyz, F).view(np.uint32)) and np.array_equal(rt, tri)


def hand_meshes():
    va, ta = box((4.25, 5.25, 6.25), (20.25, 19.25, 18.25))
    vb, tb = box((12.75, 10.75, 9.75), (27.75, 26.75, 25.75))
    vc, tc = box((4.5, 4.5, 4.5), (20.5, 20.5, 20.5))
    degenerate = np.array([[0, 0, 1], [1, 1, 1]], np.uint32)         # repeated vertices: nrm == 0
    return {"triangle": (np.array([[6.2, 7.3, 12.1], [24.9, 9.8, 13.4], [11.6, 25.2, 15.3]], F), np.array([[0, 1, 2]], np.uint32)),
            "tetra": (TETRA_XYZ, TETRA), "inverted": (TETRA_XYZ, np.ascontiguousarray(TETRA[:, ::-1])),
            "cubes": (np.concatenate([va, vb]), np.concatenate([ta, tb + 8])), "on_surface": (vc, tc),
            "with_degenerate": (TETRA_XYZ, np.concatenate([degenerate[:1], TETRA, degenerate[1:]]))}


def run_check(exe, obj, n, beta, level, types, prefix, frame=None, timeout=900):
    args = [exe, obj, str(n), repr(float(beta)), repr(float(level)), types, prefix]
    if frame is not None:
        args += [repr(float(frame[0]))] + [repr(float(v)) for v in frame[1]]
    subprocess.run(args, check=True, timeout=timeout, capture_output=True)
    tags = {"s": "seq", "o": "omp", "n": "naive", "t": "tiled"}
    return {tags[c]: (np.fromfile("%s.%s.w.f32" % (prefix, tags[c]), np.uint32), np.fromfile("%s.%s.grid.u32" % (prefix, tags[c]), np.uint32))
            for c in types}


def test_cpp_host_form_equals_the_restatement_bit_for_bit(check_exe, tmp_path):
    n = 32
    for label, (xyz, tri) in hand_meshes().items():
        obj = str(tmp_path / (label + ".obj"))
        write_obj(obj, xyz, tri)
        for beta, level in ((0.0, 0.5), (2.0, 0.5), (1.0, 1.5)):
            exp_w, exp_g = R.winding_f32(xyz, tri, n, *unit_frame(), beta, level)
            got = run_check(check_exe, obj, n, beta, level, "so", str(tmp_path / label), unit_frame())
            for tag, (gw, gg) in got.items():
                assert np.array_equal(gw, exp_w.view(np.uint32)), (label, beta, tag, int((gw != exp_w.view(np.uint32)).sum()))
                assert np.array_equal(gg, exp_g), (label, beta, level, tag)
    # the empty mesh through the C++ API: an OBJ with vertices and no face
    obj = str(tmp_path / "empty.obj")
    with open(obj, "w") as f:
        f.write("v 0 0 0\nv 1 0 0\nv 0 1 0\n")
    got = run_check(check_exe, obj, n, 2.0, 0.5, "s", str(tmp_path / "empty"), unit_frame())
    assert not got["seq"][0].any() and not got["seq"][1].any()
    xo, to, oo, vo = open_sphere()
    obj = str(tmp_path / "open.obj")
    write_obj(obj, xo, to)
    cases = [(name, M.asset(name)) + mesh_case(name, 32) + (32, (0.0, 2.0, 3.0)) for name in CLOSED]
    cases.append(("torus.obj@96", M.asset("torus.obj")) + mesh_case("torus.obj", 96) + (96, (2.0, 3.0)))
    cases.append(("open", obj, xo, to, oo, vo, 32, (0.0, 2.0, 3.0)))
    for label, path, xyz, tri, origin, vs, n, betas in cases:
        for beta in betas:
            exp_w, exp_g = R.winding_f32(xyz, tri, n, vs, origin, beta, 0.5)
            got = run_check(check_exe, path, n, beta, 0.5, "so" if n == 32 else "o", str(tmp_path / "c"), (vs, origin))
            for tag, (gw, gg) in got.items():
                assert np.array_equal(gw, exp_w.view(np.uint32)), (label, beta, tag, int((gw != exp_w.view(np.uint32)).sum()))
                assert np.array_equal(gg, exp_g), (label, beta, tag)


def test_cpp_sequential_equals_openmp_beyond_32(check_exe, tmp_path):
    """the two host types are one function; the GPU suite uses the parallel one as its reference on larger cases"""
    for name, n, beta in (("torus.obj", 64, 0.0), ("torus.obj", 64, 2.0), ("bimba.obj", 64, 2.0)):
        got = run_check(check_exe, M.asset(name), n, beta, 0.5, "so", str(tmp_path / "c"))
        assert np.array_equal(got["seq"][0], got["omp"][0]) and np.array_equal(got["seq"][1], got["omp"][1]), (name, n, beta)
        assert got["seq"][1].any() and not (got["seq"][1] == 0xFFFFFFFF).all()
    xyz, tri, origin, vs = mesh_case("torus.obj", 64)
    exp_w, exp_g = R.winding_f32(xyz, tri, 64, vs, origin, 2.0, 0.5)
    assert exp_g.any()
    got = run_check(check_exe, M.asset("torus.obj"), 64, 2.0, 0.5, "o", str(tmp_path / "c"))
    assert np.array_equal(got["omp"][0], exp_w.view(np.uint32)) and np.array_equal(got["omp"][1], exp_g)


@pytest.fixture(scope="module")
def cli():
    return build.build_cli()


def test_cli_winding_writes_the_grid_of_the_restatement(cli, tmp_path):
    n = 32
    xyz, tri, origin, vs = mesh_case("torus.obj", n)
    for flag, level, beta in ((["--winding"], 0.5, 2.0), (["--winding", "0.5:0"], 0.5, 0.0), (["--winding", "0.25:3"], 0.25, 3.0)):
        d = tmp_path / ("w%g_%g" % (level, beta))
        d.mkdir()
        p = subprocess.run([cli, M.asset("torus.obj"), "-n", str(n), "-t", "0"] + flag + ["-d", str(d / "x")], capture_output=True, text=True,
                           timeout=600, cwd=str(d))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert "Winding" in p.stdout
        _, exp = R.winding_f32(xyz, tri, n, vs, origin, beta, level)
        assert np.array_equal(np.fromfile(str(d / "x.grid.u32"), np.uint32), exp), flag


def test_cli_winding_followed_by_other_flags_keeps_its_defaults(cli, tmp_path):
    """the value is optional: -e, -s and a bare - or . after --winding are not a LEVEL"""
    n = 32
    xyz, tri, origin, vs = mesh_case("torus.obj", n)
    _, exp = R.winding_f32(xyz, tri, n, vs, origin, 2.0, 0.5)
    for k, flags in enumerate((["--winding", "-e", "-s"], ["--winding", "-s", "--mesh-sdf", "2", "-e"], ["-e", "--winding", "-s", "--exact-sdf"])):
        d = tmp_path / ("f%d" % k)
        d.mkdir()
        p = subprocess.run([cli, M.asset("torus.obj"), "-n", str(n), "-t", "0"] + flags + ["-d", str(d / "x")], capture_output=True, text=True,
                           timeout=600, cwd=str(d))
        assert p.returncode == 0, (flags, p.stdout[-2000:] + p.stderr[-2000:])
        assert np.array_equal(np.fromfile(str(d / "x.grid.u32"), np.uint32), exp), flags
        sdf = np.fromfile(str(d / "x.sdf.f32"), np.float32)
        assert np.array_equal(~np.signbit(sdf), bits_of(exp)), flags                 # the field is signed by the winding grid
        assert os.listdir(str(d / "out")), flags                                      # -e was seen as the export flag
    for bad in ("-", ".", "+", "e"):                                                  # not a value, not a flag: read as a file name that does not exist
        p = subprocess.run([cli, M.asset("torus.obj"), "--winding", bad, "-n", "32", "-t", "0"], capture_output=True, text=True, timeout=300,
                           cwd=str(tmp_path))
        assert p.returncode != 0 and "is not LEVEL" not in p.stdout + p.stderr, bad


def test_cli_winding_usage_errors(cli, tmp_path):
    mesh = M.asset("d20.obj")
    for args in ([mesh, "--winding", "x"], [mesh, "--winding", "0.5:0.5"], [mesh, "--winding", "0.5:65"], [mesh, "--winding", "inf"],
                 [mesh, "--winding", "--conservative"]):
        p = subprocess.run([cli] + args + ["-n", "32", "-t", "0"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert p.returncode != 0, args
