"""Grayscale reconstruction and h-extrema without a GPU: the numpy reference of tests/reconstruct_ref.py against itself (the definition, the
queue form, the plateau definition of the extrema, the integer square root), the figures DESIGN.md section 25 records for the three balls, the
C++ host form (VOX::Reconstruct / VOX::Extrema, SEQUENTIAL and OPENMP) byte for byte, `vpcli --watershed h:H[:Q[:C]]` on the CPU types, and
the header, symbols and sources."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.ndimage as ndi

from cuda_mesh_voxelization_amd import build, capi, mesh as M

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_ref  # noqa: E402
import edt_ref  # noqa: E402
import reconstruct_ref as R  # noqa: E402
import watershed_ref as WS  # noqa: E402
from test_watershed_cpu import cli_expected, cli_run  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference itself ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", R.CONNS)
@pytest.mark.parametrize("mode", R.MODES)
def test_queue_form_equals_the_definition_at_n_32(mode, conn):
    for name in R.CASES:
        F, G, domain = R.case(name)
        if G.shape[0] != 32:
            continue
        r, stats = R.reconstruct(F, G, domain, mode, conn)
        q, qstats = R.expected(name, mode, conn)
        assert np.array_equal(r, q) and stats == qstats, name
        off = np.zeros(G.shape, bool) if domain is None else ~domain
        assert (r[off] == (R.TOP if mode == R.EROSION else 0)).all(), name
        work_r, work_g = R.work(r, mode, domain), R.work(G, mode, domain)
        assert (work_r <= work_g).all() and (work_r >= np.minimum(R.work(F, mode, domain), work_g)).all(), name


def test_duality_and_idempotence_of_the_reference():
    F, G, domain = R.case("random 32")
    for conn in R.CONNS:
        ero, _ = R.reconstruct_queue(F, G, domain, R.EROSION, conn)
        dil, st = R.reconstruct_queue(~F, ~G, domain, R.DILATION, conn)
        assert np.array_equal(ero, ~dil)
        again, ast = R.reconstruct_queue(dil, ~G, domain, R.DILATION, conn)
        assert np.array_equal(again, dil) and ast == (st[0], 0, st[2], st[3])


def test_walls_stop_everything():
    """a work value of 0 inside the domain behaves like "not in the domain": the same field with the walls taken out of the domain"""
    F, G, _ = R.case("comb")
    for conn in R.CONNS:
        a, sa = R.reconstruct(F, G, None, R.DILATION, conn)
        b, sb = R.reconstruct(F, G, G != 0, R.DILATION, conn)
        assert np.array_equal(a, b) and sa[1:] == sb[1:] and sa[0] == 32 ** 3 and sb[0] == int((G != 0).sum())
        assert np.array_equal(a == 5, G == 5) and sa[1] == R.comb_field()[2]


@pytest.mark.parametrize("conn", R.CONNS)
@pytest.mark.parametrize("kind", (R.MAXIMA, R.MINIMA))
def test_extrema_by_plateaus_equal_extrema_by_reconstruction(kind, conn):
    for name, h in (("hills", 0), ("hills", 3), ("hills domain", 0), ("hills domain", 2), ("ends", 0), ("ends", 1), ("balls", 8)):
        values, domain, scale = R.extrema_case(name)
        V, H, E, stats = R.extrema_expected(name, kind, h, conn)
        assert np.array_equal(E, R.extrema_plateaus(values, domain, kind, scale, h, conn)), (name, h)
        assert stats[1] == int(E.sum()) and (h != 0 or (stats[3] == 0 and np.array_equal(H[E], V[E])))
    values, domain, scale = R.extrema_case("hills")
    by_definition = R.extrema(values, domain, kind, scale, 2, conn, rec=R.reconstruct)
    for a, b in zip(by_definition, R.extrema_expected("hills", kind, 2, conn)):
        assert np.array_equal(a, b)


def test_isqrt16_is_exact():
    rng = np.random.default_rng(5)
    sample = np.r_[np.array([0, 1, 2, 3, 255, 256, 257, 2 ** 31, R.TOP - 1, R.TOP], np.uint64), rng.integers(0, 2 ** 32, 20000, dtype=np.uint64),
                   np.arange(1, 3000, dtype=np.uint64) ** 2 // 256, (np.arange(1, 3000, dtype=np.uint64) ** 2 + 255) // 256].astype(np.uint32)
    got = R.isqrt16(sample)
    assert got.tolist() == [math.isqrt(int(v) << 8) for v in sample]
    assert [R.isqrt16_python(v) for v in (0, 1, R.TOP)] == [0, 16, 1048575]
    assert R.isqrt16(np.array([197], np.uint32))[0] == 224          # the largest D^2 of the three balls, in sixteenths of a voxel


# ---- the three balls of DESIGN.md section 25 -------------------------------------------------------------------------------------------------
def test_three_balls_inset_never_finds_three_parts():
    mask, d2 = R.three_balls()
    assert int(mask.sum()) == R.THREE_BALLS_VOXELS and int(d2.max()) == R.THREE_BALLS_MAX_D2
    assert np.array_equal(d2, np.where(mask, WS.inside_d2(mask), 0))
    counts = tuple(components_ref.label_bool(np.array(edt_ref.morph_edt(mask, 1, r)), 6)[1] for r in range(1, 9))
    assert counts == R.THREE_BALLS_INSETS and 3 not in counts


@pytest.mark.parametrize("conn", R.CONNS)
def test_three_balls_extended_maxima_find_them(conn):
    mask, d2 = R.three_balls()
    for h, (markers, voxels) in R.THREE_BALLS_MAXIMA.items():
        V, H, E, stats = R.extrema(d2, mask, R.MAXIMA, R.SQRT16, h, conn)
        assert ndi.label(E, structure=R.footprint(conn))[1] == markers, (h, conn)
        assert voxels is None or (int(E.sum()) == voxels == stats[1]), (h, conn, int(E.sum()))
        assert stats[0] == R.THREE_BALLS_VOXELS and stats[2] == 224 - h


@pytest.mark.parametrize("conn", R.CONNS)
def test_three_balls_watershed_from_the_h_8_markers(conn):
    mask, d2 = R.three_balls()
    V, H, E, _ = R.extrema_expected("balls", R.MAXIMA, 8, conn)
    markers, count = components_ref.label_bool(E, conn)
    assert count == 3
    W, cut, stats = WS.watershed(mask, markers, V, WS.DESCENDING, 1, conn)
    assert sorted(int(W[c[2], c[1], c[0]]) for c, _ in R.THREE_BALLS) == [1, 2, 3]       # three labels, one per ball centre
    assert stats[1] == R.THREE_BALLS_VOXELS and set(np.unique(W[mask]).tolist()) == {1, 2, 3}


# ---- the C++ host form ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    pkg = os.path.dirname(capi.LIB_PATH)
    build.build_lib()
    srcs = [os.path.join(pkg, "vplib", "src", f) for f in sorted(os.listdir(os.path.join(pkg, "vplib", "src"))) if f.endswith(".cpp")]
    exe = str(tmp_path_factory.mktemp("reconstruct") / "reconstruct_check")
    subprocess.check_call(["g++", "-std=c++23", "-O2", "-ffp-contract=off", "-fopenmp",
                           "-I", os.path.join(pkg, "vplib", "include"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "reconstruct_check.cpp")] + srcs + ["-o", exe, "-L", pkg, "-lvphip", "-Wl,-rpath," + pkg])
    return exe


TAGS = {"s": "seq", "o": "omp", "n": "naive", "t": "tiled"}


def _stats(stdout):
    return {t: tuple(int(v) for v in rest.split()) for t, rest in re.findall(r"^(seq|omp|naive|tiled) (\d+ \d+ \d+ \d+)$", stdout, re.M)}


def _domain_file(domain, prefix):
    if domain is None:
        return "-"
    R.bool_to_words(domain).tofile(prefix + ".domain.u32")
    return prefix + ".domain.u32"


def run_rec(exe, F, G, domain, mode, conn, bits, types, prefix, timeout=900):
    """{tag: (R uint32[n^3], statistics)} of tests/cpp/reconstruct_check.cpp"""
    np.ascontiguousarray(F, np.uint32).tofile(prefix + ".marker.u32")
    np.ascontiguousarray(G, np.uint32).tofile(prefix + ".mask.u32")
    p = subprocess.run([exe, "rec", _domain_file(domain, prefix), prefix + ".marker.u32", prefix + ".mask.u32", str(G.shape[0]), str(mode), str(conn),
                        str(bits), types, prefix], check=True, timeout=timeout, capture_output=True, text=True)
    stats = _stats(p.stdout)
    return {TAGS[c]: (np.fromfile("%s.%s.rec.u32" % (prefix, TAGS[c]), np.uint32), stats[TAGS[c]]) for c in types}


def run_ext(exe, values, domain, kind, scale, h, conn, bits, types, prefix, timeout=900):
    """{tag: (V, H, E words, statistics)}"""
    np.ascontiguousarray(values, np.uint32).tofile(prefix + ".values.u32")
    p = subprocess.run([exe, "ext", _domain_file(domain, prefix), prefix + ".values.u32", str(values.shape[0]), str(kind), str(scale), str(h), str(conn),
                        str(bits), types, prefix], check=True, timeout=timeout, capture_output=True, text=True)
    stats = _stats(p.stdout)
    return {TAGS[c]: tuple(np.fromfile("%s.%s.%s.u32" % (prefix, TAGS[c], f), np.uint32) for f in ("scaled", "flat", "ext")) + (stats[TAGS[c]],)
            for c in types}


@pytest.mark.parametrize("conn", R.CONNS)
@pytest.mark.parametrize("mode", R.MODES)
def test_host_form_equals_numpy(check_exe, tmp_path, mode, conn):
    prefix = str(tmp_path / "h")
    for k, name in enumerate(R.CASES):
        F, G, domain = R.case(name)
        exp, stats = R.expected(name, mode, conn)
        got = run_rec(check_exe, F, G, domain, mode, conn, 64 if k % 2 else 32, "so", prefix)
        for tag in ("seq", "omp"):
            assert np.array_equal(got[tag][0], exp.reshape(-1)), (name, tag)
            assert got[tag][1] == stats, (name, tag, got[tag][1], stats)


@pytest.mark.parametrize("conn", R.CONNS)
@pytest.mark.parametrize("kind", (R.MAXIMA, R.MINIMA))
def test_host_extrema_equal_numpy(check_exe, tmp_path, kind, conn):
    prefix = str(tmp_path / "e")
    for k, (name, h) in enumerate((("hills", 0), ("hills", 3), ("hills domain", 2), ("ends", 0), ("ends", 1), ("ends", R.TOP), ("sqrt", 1 << 12), ("balls", 8))):
        values, domain, scale = R.extrema_case(name)
        V, H, E, stats = R.extrema_expected(name, kind, h, conn)
        got = run_ext(check_exe, values, domain, kind, scale, h, conn, 64 if k % 2 else 32, "so", prefix)
        for tag in ("seq", "omp"):
            v, hh, e, s = got[tag]
            assert np.array_equal(v, V.reshape(-1)) and np.array_equal(hh, H.reshape(-1)), (name, h, tag)
            assert np.array_equal(e, R.bool_to_words(E)), (name, h, tag)
            assert s == stats, (name, h, tag, s, stats)


# ---- the CLI -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    return build.build_cli()


def cli_chain(vox, h16, q, conn):
    """(W, cut, the two lines `vpcli --watershed h:...` prints) for the grid `vox` it starts from, by the numpy chain"""
    n = vox.shape[0]
    d2 = edt_ref.edt_numpy(vox, edt_ref.UNSET)
    V, H, E, stats = R.extrema(d2, vox, R.MAXIMA, R.SQRT16, h16, conn)
    markers, count = components_ref.label_bool(E, conn)
    W, cut, st = WS.watershed(vox, markers, V, WS.DESCENDING, q, conn)
    return W, cut, count, ("extrema: n %d, h16 %d, maxima voxels %d, markers %d" % (n, h16, stats[1], count),
                           "watershed: n %d, markers %d, marker voxels %d, labelled %d, levels %d, cut %d" % (n, count, st[0], st[1], st[2], st[3]))


CLI_RUNS = (("bunny.obj", "h:0.5", 8, 1, 6), ("bimba.obj", "h:1.5:2:26", 24, 2, 26))


def test_cli_cpu_types_equal_the_numpy_chain(cli, tmp_path):
    for k, (mesh, arg, h16, q, conn) in enumerate(CLI_RUNS):
        _, vox, none = cli_run(cli, tmp_path, "plain%d" % k, mesh, 64, "0", [])
        W, cut, count, lines = cli_chain(vox, h16, q, conn)
        assert none is None and count >= 2 and int(W.max()) == count
        for t in ("0", "3"):                                        # SEQUENTIAL, OPENMP
            out, grid, labels = cli_run(cli, tmp_path, "split%d_%s" % (k, t), mesh, 64, t, ["--watershed", arg])
            assert "\n".join(lines) + "\n" in out, (out, lines)   # the extrema line right in front of the watershed line
            assert np.array_equal(labels, W.reshape(-1)) and np.array_equal(grid, cut)
            assert re.search(r"^\[\w*Extrema\]: [0-9.]+ ms$", out, re.M), out


def test_cli_numeric_form_is_as_before(cli, tmp_path):
    _, vox, _ = cli_run(cli, tmp_path, "plain", "bunny.obj", 64, "0", [])
    out, grid, labels = cli_run(cli, tmp_path, "split", "bunny.obj", 64, "0", ["--watershed", "2:3:26"])
    W, cut, count, line = cli_expected(vox, 2, 3, 26)
    assert line + "\n" in out and "extrema:" not in out and "Extrema" not in out
    assert np.array_equal(labels, W.reshape(-1)) and np.array_equal(grid, cut)


def test_cli_refuses_malformed_depths(cli, tmp_path):
    mesh = M.asset("d20.obj")
    for arg in ("h:", "h", "h:x", "h:-1", "h:1024", "h:1e2", "h:1.5.2", "h:.", "h:1:0", "h:1:1:8", "h:1:1:6:1", "h:1:", "H:1", "h:1,5", "h: 1", "h:+1"):
        p = subprocess.run([cli, mesh, "-n", "32", "-t", "0", "--watershed", arg], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert p.returncode != 0, arg
    p = subprocess.run([cli, mesh, "-n", "32", "-t", "0", "--watershed", "h:1", "-g", "2"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode != 0
    for arg, h16 in (("h:0", 0), ("h:1023", 16368), ("h:0.03", 0), ("h:0.04", 1), ("h:.5", 8), ("h:2.", 32)):
        p = subprocess.run([cli, mesh, "-n", "32", "-t", "0", "--watershed", arg], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert p.returncode == 0 and "extrema: n 32, h16 %d, " % h16 in p.stdout, (arg, p.stdout[-600:], p.stderr[-600:])
    p = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert "h:H[:Q[:C]]" in p.stdout + p.stderr


# ---- the header --------------------------------------------------------------------------------------------------------------------------------
def test_prototypes_and_sources():
    with open(os.path.join(ROOT, "include", "vphip.h")) as f:
        header = f.read()
    for proto in ("int vp_reconstruct(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_domain",
                  "const uint32_t* d_marker, const uint32_t* d_mask, int mode, int connectivity, int algo",
                  "int vp_reconstruct_result(vp_ctx* ctx, uint32_t** d_field, uint64_t* h_stats",
                  "int vp_reconstruct_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_domain",
                  "int vp_extrema(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_domain",
                  "int vp_extrema_result(vp_ctx* ctx, uint32_t** d_scaled, uint32_t** d_flat, uint32_t** d_extrema, uint64_t* h_stats",
                  "int vp_extrema_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_domain",
                  "enum { VP_REC_DILATION = 0, VP_REC_EROSION = 1 };", "enum { VP_EXT_MAXIMA = 0, VP_EXT_MINIMA = 1 };",
                  "enum { VP_EXT_LINEAR = 0, VP_EXT_SQRT16 = 1 };", "#define VP_ABI_VERSION 6"):
        assert proto in header, proto
    assert "reconstruct.hip" in build.HIP_SOURCES
    assert {"vp_reconstruct", "vp_reconstruct_result", "vp_reconstruct_host", "vp_extrema", "vp_extrema_result", "vp_extrema_host"} <= set(capi.SYMBOLS)
    assert (capi.REC_DILATION, capi.REC_EROSION, capi.EXT_MAXIMA, capi.EXT_MINIMA, capi.EXT_LINEAR, capi.EXT_SQRT16) == (0, 1, 0, 1, 0, 1)
    assert len(capi.HEADER_PROF_KEYS) == 64                         # no new timing key
    import ctx_history
    outputs = ctx_history.header_device_outputs()                   # every result is context-owned: no caller-addressed device output
    assert not [name for name in outputs if name.startswith(("vp_reconstruct", "vp_extrema"))]
    pkg = os.path.dirname(capi.LIB_PATH)
    with open(os.path.join(pkg, "csrc", "reconstruct.hip")) as f:
        src = f.read()
    assert re.search(r"^constexpr uint32_t kRecSweeps = \d+;", src, re.M)
    for shared in ("stage_halo(", "store_lowered(", "block_seen_by(", "block_raise(", "list_active(", "run_rounds(", "store_ballot(", "wg_sum_256("):
        assert shared in src, shared
    assert "atomicMin" not in src and "atomicCAS" not in src and "atomicExch" not in src      # no atomics on R
    with open(os.path.join(pkg, "csrc", "vp_internal.h")) as f:
        internal = f.read()
    assert "struct Rc : vp::OwnedResult" in internal and "struct Ex : vp::OwnedResult" in internal and "f(rc); f(ex);" in internal
