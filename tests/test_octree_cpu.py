"""The sparse voxel octree without a GPU: the numpy restatement of tests/octree_ref.py against the facts of the header (include/vphip.h,
vp_octree), its invariants on random grids and on the oracle's solids, the C++ host form (vplib/src/octree.cpp) SEQUENTIAL == OPENMP ==
numpy byte for byte on both word types, Octree::Test, the validators (vp_octree_validate_host, Octree::Validate through ReadOctree)
against one mutated word per kind of corruption, the .svo file, `vpcli --octree`, and the header's prototypes."""
import glob
import json
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from cuda_mesh_voxelization_amd import build, capi, mesh as M
from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import octree_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "octree_counts.json")
HEADER_BYTES = 8 + 16 + 16 + 44 + 44


def counts(vox):
    nodes, lo, fl = R.build_numpy(vox)
    return R.counts_of(lo, vox.shape[0]), nodes, lo, fl


def hold_invariants(vox, nodes, lo, fl, tag):
    n = vox.shape[0]
    P, L = R.geometry(n)
    assert R.validate_numpy(nodes, n) is None, (tag, R.validate_numpy(nodes, n))
    valid, full = nodes[:, 0] & 0xFF, (nodes[:, 0] >> 8) & 0xFF
    assert not (nodes[:, 0] >> 16).any() and not (full & ~valid).any(), tag
    mixed = valid & ~full
    kids = np.array([bin(int(m)).count("1") for m in mixed], np.int64)
    # the children of the nodes are consecutive: every child index is the running sum, which starts behind the root
    has = kids > 0
    assert np.array_equal(nodes[has, 1].astype(np.int64), (1 + np.cumsum(kids) - kids)[has]) and not nodes[~has, 1].any(), tag
    assert 1 + int(kids.sum()) == len(nodes) == int(lo[L]) and (lo[L:] == lo[L]).all() and lo[0] == 0 and lo[1] == 1, tag
    assert R.popcount_from_full_leaves(fl, n) == int(vox.sum()), tag
    assert np.array_equal(R.expand_numpy(nodes, n), vox), tag
    # Morton order strictly ascending per level: rebuild the cell coordinates by a walk and compare the codes
    level = [(0, 0, 0, 0)]
    for l in range(L):
        codes = R.morton([c[3] for c in level], [c[2] for c in level], [c[1] for c in level])
        assert [c[0] for c in level] == list(range(int(lo[l]), int(lo[l + 1]))) and (np.diff(codes.astype(np.int64)) > 0).all(), (tag, l)
        nxt = []
        for node, z, y, x in level:
            rank = 0
            for c in range(8):
                if (int(mixed[node]) >> c) & 1:
                    nxt.append((int(nodes[node, 1]) + rank, 2 * z + (c >> 2), 2 * y + ((c >> 1) & 1), 2 * x + (c & 1)))
                    rank += 1
        level = nxt
    assert not level


# ---- the facts of the contract --------------------------------------------------------------------------------------------------------
def test_empty_and_full_grids():
    for n in (32, 64, 96):
        c, nodes, lo, fl = counts(np.zeros((n,) * 3, bool))
        assert c == [1] + [0] * (len(c) - 1) and nodes.tolist() == [[0, 0]] and not fl.any()
    for n in (32, 64):
        c, nodes, lo, fl = counts(np.ones((n,) * 3, bool))
        assert nodes.tolist() == [[0xFFFF, 0]] and fl[0] == 8 and not fl[1:].any()
    c, nodes, lo, fl = counts(np.ones((96,) * 3, bool))
    assert c == [1, 7, 0, 0, 0, 0, 0]
    assert nodes[0].tolist() == [0xFF | (1 << 8), 1]                # child 0 of the root is the full 64^3 cube, the other seven straddle the edge
    for k in range(1, 8):
        assert nodes[k, 1] == 0 and (nodes[k, 0] & 0xFF) == (nodes[k, 0] >> 8) and 0 < (nodes[k, 0] & 0xFF) < 0xFF
    assert R.popcount_from_full_leaves(fl, 96) == 96 ** 3


def test_hand_counts():
    assert counts(R.single(64, 31, 0, 17))[0] == [1, 1, 1, 1, 1, 1]
    assert counts(R.box(64, 8, 40))[0] == [1, 8, 26, 0, 0, 0]
    c = counts(R.ball(96, (48, 48, 48), 1600))[0]
    assert c == [1, 8, 26, 113, 391, 1384, 3769] and sum(c) == 5692
    c = counts(R.ball(128, (64, 64, 64), 2500))[0]
    assert c == [1, 8, 56, 176, 668, 2245, 5884] and sum(c) == 9038


def test_the_tree_of_a_grid_placed_in_a_larger_frame_with_the_same_p_is_identical():
    vox = R.ball(96, (48, 48, 48), 1600)
    a, b = R.build_numpy(vox), R.build_numpy(R.embed(vox, 128))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(R.expand_numpy(a[0], 128), R.embed(vox, 128))


def random_cases():
    for k, density in enumerate((0.03, 0.5, 0.97)):
        vox = R.random_bool(32, density, 170 + k)
        yield "random %g at 32" % density, vox
        yield "complement of random %g at 32" % density, ~vox
    yield "random 0.5 at 64", R.random_bool(64, 0.5, 64)
    yield "box at 64", R.box(64, 8, 40)
    yield "random 0.97 at 96", R.random_bool(96, 0.97, 96)
    yield "ball at 96", R.ball(96, (48, 48, 48), 1600)
    yield "full 96", np.ones((96,) * 3, bool)
    yield "random 0.9 at 160", R.random_bool(160, 0.9, 160)
    yield "shell of a ball at 160", R.ball(160, (80, 70, 90), 4900) & ~R.ball(160, (80, 70, 90), 4000)


@pytest.fixture(scope="module")
def cases():
    return [(tag, vox) + R.build_numpy(vox) for tag, vox in random_cases()]


def test_round_trip_and_invariants(cases):
    seen = set()
    for tag, vox, nodes, lo, fl in cases:
        hold_invariants(vox, nodes, lo, fl, tag)
        key = nodes.tobytes()
        assert key not in seen, tag                                   # build is injective: different grids, different bytes
        seen.add(key)


def test_point_query(cases):
    tag, vox, nodes, lo, fl = cases[1]
    n = vox.shape[0]
    got = np.array([[[R.query_numpy(nodes, n, x, y, z) for x in range(n)] for y in range(n)] for z in range(0, n, 5)])
    assert np.array_equal(got, vox[::5])


# ---- the C++ host form ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def octree_exe(tmp_path_factory):
    pkg = os.path.dirname(capi.LIB_PATH)
    build.build_lib()
    srcs = [os.path.join(pkg, "vplib", "src", f) for f in sorted(os.listdir(os.path.join(pkg, "vplib", "src"))) if f.endswith(".cpp")]
    exe = str(tmp_path_factory.mktemp("octree") / "octree_check")
    subprocess.check_call(["g++", "-std=c++23", "-O2", "-ffp-contract=off", "-fopenmp",
                           "-I", os.path.join(pkg, "vplib", "include"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "octree_check.cpp")] + srcs + ["-o", exe, "-L", pkg, "-lvphip", "-Wl,-rpath," + pkg])
    return exe


def read_svo(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"VPSVO1\0\0"
    n, P, L, m = struct.unpack_from("<4I", raw, 8)
    frame = struct.unpack_from("<4f", raw, 24)
    lo = np.frombuffer(raw, np.uint32, 11, 40)
    fl = np.frombuffer(raw, np.uint32, 11, 84)
    assert len(raw) == HEADER_BYTES + 8 * m
    return dict(n=n, P=P, L=L, M=m, frame=frame, lo=lo, fl=fl, nodes=np.frombuffer(raw, np.uint32, 2 * m, HEADER_BYTES).reshape(m, 2))


def run_build(exe, words, n, bits, types, prefix, timeout=900):
    np.asarray(words, np.uint32).tofile(prefix + ".in.u32")
    p = subprocess.run([exe, "build", prefix + ".in.u32", str(n), str(bits), types, prefix], check=True, timeout=timeout, capture_output=True,
                       text=True)
    tags = {"s": "seq", "o": "omp", "n": "naive", "t": "tiled"}
    found = dict(re.findall(r"^(seq|omp|naive|tiled) (\d+)$", p.stdout, re.M))
    out = {}
    for c in types:
        tree = read_svo("%s.%s.svo" % (prefix, tags[c]))
        assert tree["M"] == int(found[tags[c]])
        out[tags[c]] = (tree, np.fromfile("%s.%s.grid.u32" % (prefix, tags[c]), np.uint32))
    return out


def same_tree(tree, n, nodes, lo, fl):
    P, L = R.geometry(n)
    return ((tree["n"], tree["P"], tree["L"], tree["M"]) == (n, P, L, len(nodes)) and np.array_equal(tree["nodes"], nodes)
            and np.array_equal(tree["lo"], lo) and np.array_equal(tree["fl"], fl))


def test_cpp_host_form_equals_the_restatement_byte_for_byte(octree_exe, cases, tmp_path):
    for tag, vox, nodes, lo, fl in cases:
        n = vox.shape[0]
        words = R.bool_to_words(vox)
        for bits in (32, 64):
            got = run_build(octree_exe, words, n, bits, "so", str(tmp_path / "c"))
            for name, (tree, back) in got.items():
                assert same_tree(tree, n, nodes, lo, fl), (tag, bits, name)
                assert tree["frame"] == (0.5, 1.0, -2.0, 3.0), (tag, bits, name)
                assert np.array_equal(back, words), (tag, bits, name)
    assert open(str(tmp_path / "c.seq.svo"), "rb").read() == open(str(tmp_path / "c.omp.svo"), "rb").read()


@pytest.fixture(scope="module")
def assets():
    out = {}
    for name in ("bunny", "torus"):
        xyz, tri = M.import_mesh(M.asset(name + ".obj"))
        for n in (64, 96, 128):
            origin, vs = O.frame([xyz], n)
            out["%s %d" % (name, n)] = (n, np.asarray(O.voxelize(xyz, tri, n, vs, origin), np.uint32).reshape(-1))
    return out


def test_asset_grids_host_form_and_recorded_counts(octree_exe, assets, tmp_path):
    golden = json.load(open(GOLDEN))
    assert golden["bunny 64"] == [1, 8, 42, 165, 628, 1711] and golden["bunny 128"] == [1, 8, 42, 183, 722, 2578, 7106]
    assert sorted(golden) == sorted(assets)
    for key, (n, words) in assets.items():
        vox = R.words_to_bool(words, n)
        nodes, lo, fl = R.build_numpy(vox)
        assert R.counts_of(lo, n) == golden[key], key
        assert R.validate_numpy(nodes, n) is None and np.array_equal(R.expand_numpy(nodes, n), vox), key
        assert R.popcount_from_full_leaves(fl, n) == int(vox.sum()), key
        for name, (tree, back) in run_build(octree_exe, words, n, 32, "so", str(tmp_path / "a")).items():
            assert same_tree(tree, n, nodes, lo, fl) and np.array_equal(back, words), (key, name)


def test_octree_test_on_every_voxel_at_32_and_on_random_voxels_at_128(octree_exe, assets, tmp_path):
    vox = R.random_bool(32, 0.5, 7)
    prefix = str(tmp_path / "q")
    run_build(octree_exe, R.bool_to_words(vox), 32, 32, "s", prefix)
    subprocess.run([octree_exe, "read", prefix + ".seq.svo", "s", prefix, "all"], check=True, timeout=300)
    assert np.array_equal(np.fromfile(prefix + ".test.u32", np.uint32), R.bool_to_words(vox))
    n, words = assets["bunny 128"]
    vox = R.words_to_bool(words, n)
    run_build(octree_exe, words, n, 32, "o", prefix)
    pts = np.random.default_rng(128).integers(0, n, (100000, 3), dtype=np.uint32)
    pts[:4] = [[n, 0, 0], [0, n, 0], [0, 0, 1 << 20], [n - 1, n - 1, n - 1]]       # outside the grid: unset
    pts.tofile(prefix + ".pts.u32")
    subprocess.run([octree_exe, "read", prefix + ".omp.svo", "s", prefix, prefix + ".pts.u32"], check=True, timeout=300)
    got = np.fromfile(prefix + ".test.u8", np.uint8).astype(bool)
    inside = (pts < n).all(axis=1)
    exp = np.zeros(len(pts), bool)
    exp[inside] = vox[pts[inside, 2], pts[inside, 1], pts[inside, 0]]
    assert np.array_equal(got, exp) and exp.any() and not exp.all()
    assert np.array_equal(np.fromfile(prefix + ".grid.u32", np.uint32), words)


# ---- the validators: one mutated word per kind of corruption ----------------------------------------------------------------------------
def corruptions(nodes, lo, n):
    """(what, mutated copy): `nodes` is the tree of the ball at 96, which has nodes of every kind"""
    P, L = R.geometry(n)
    def mutated(i, j, value):
        m = nodes.copy()
        m[i, j] = value
        return m
    inner = int(lo[2])                                                  # a level-2 node
    with_kids = next(i for i in range(inner, len(nodes)) if nodes[i, 1])
    last = len(nodes) - 1                                               # a level L - 1 node: its children are voxels
    some_full = next(i for i in range(1, len(nodes)) if (nodes[i, 0] >> 8) & 0xFF)
    yield "upper bits", mutated(inner, 0, int(nodes[inner, 0]) | 0x10000)
    yield "full outside valid", mutated(last, 0, int(nodes[last, 0]) | 0xFF00)
    yield "child one too far", mutated(with_kids, 1, int(nodes[with_kids, 1]) + 1)
    yield "child one too near", mutated(with_kids, 1, int(nodes[with_kids, 1]) - 1)
    yield "child out of range", mutated(with_kids, 1, len(nodes) + 5)
    yield "child where there is none", mutated(last, 1, 1)
    yield "child missing", mutated(with_kids, 1, 0)
    yield "a mixed voxel", mutated(last, 0, int(nodes[last, 0]) & 0xFF)
    yield "an empty stored cell", mutated(some_full, 0, 0)
    yield "a full stored cell", mutated(last, 0, 0xFFFF)
    full_bit = 0x100 << next(c for c in range(8) if (int(nodes[some_full, 0]) >> (8 + c)) & 1)
    yield "a full child turned mixed: one stored child more than there are nodes", mutated(some_full, 0, int(nodes[some_full, 0]) & ~full_bit)
    yield "one node short", nodes[:-1].copy()
    yield "one node more", np.vstack([nodes, nodes[-1:]])


def test_validators_reject_each_kind_of_corruption(octree_exe, tmp_path):
    n = 96
    vox = R.ball(n, (48, 48, 48), 1600)
    vox[64:, :8, :8] = True                                              # a full cell at the grid's edge
    nodes, lo, fl = R.build_numpy(vox)
    assert R.validate_numpy(nodes, n) is None
    assert capi.lib().vp_octree_validate_host(nodes.ctypes.data_as(capi.ctypes.c_void_p), len(nodes), n) == 0
    prefix = str(tmp_path / "v")
    run_build(octree_exe, R.bool_to_words(vox), n, 32, "s", prefix)
    good = open(prefix + ".seq.svo", "rb").read()
    p = subprocess.run([octree_exe, "read", prefix + ".seq.svo", "s", prefix], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "n 96 nodes %d" % len(nodes) in p.stdout
    seen = 0
    for what, bad in corruptions(nodes, lo, n):
        if np.array_equal(bad, nodes):
            continue
        seen += 1
        bad = np.ascontiguousarray(bad, np.uint32)
        assert R.validate_numpy(bad, n) is not None, what
        assert capi.lib().vp_octree_validate_host(bad.ctypes.data_as(capi.ctypes.c_void_p), len(bad), n) == 10001, what
        head = bytearray(good[:HEADER_BYTES])
        struct.pack_into("<I", head, 20, len(bad))
        open(prefix + ".bad.svo", "wb").write(bytes(head) + bad.tobytes())
        p = subprocess.run([octree_exe, "read", prefix + ".bad.svo", "s", prefix], capture_output=True, text=True, timeout=300)
        assert p.returncode == 4 and "rejected: " in p.stdout, (what, p.returncode, p.stdout)
    assert seen >= 13
    # a full child that pokes out of the grid, and nothing else wrong: in the tree of the full 96^3 grid node 1 is the cell x = 64 .. 127,
    # whose children with x = 64 .. 95 are full; one more full child at x = 96 .. 127 lies outside
    full96 = R.build_numpy(np.ones((n,) * 3, bool))[0]
    assert full96[1].tolist() == [0x5555, 0] and R.validate_numpy(full96, n) is None
    full96[1, 0] = 0x5757
    assert R.validate_numpy(full96, n) == "a full child outside the grid"
    assert capi.lib().vp_octree_validate_host(full96.ctypes.data_as(capi.ctypes.c_void_p), len(full96), n) == 10001
    assert b"pokes out of the grid" in capi.lib().vp_last_error()
    # the file itself: a wrong magic, a truncated file, a count that does not belong to the size, summaries that do not belong to the records
    for what, raw in (("magic", b"VPSVO2\0\0" + good[8:]), ("truncated", good[:-4]), ("count", good[:20] + struct.pack("<I", len(nodes) - 1) + good[24:]),
                      ("side", good[:8] + struct.pack("<I", 160) + good[12:]), ("level_offset", good[:44] + struct.pack("<I", 2) + good[48:]),
                      ("full_leaves", good[:84] + struct.pack("<I", 9) + good[88:]), ("short header", good[:30])):
        open(prefix + ".bad.svo", "wb").write(raw)
        p = subprocess.run([octree_exe, "read", prefix + ".bad.svo", "s", prefix], capture_output=True, text=True, timeout=300)
        assert p.returncode == 4 and "rejected: " in p.stdout, (what, p.returncode, p.stdout)
    for args in ((None, 1, 32), (nodes, 0, n), (nodes, len(nodes), 100), (nodes, len(nodes), 2048), (nodes, 1 << 28, n)):
        ptr = args[0].ctypes.data_as(capi.ctypes.c_void_p) if args[0] is not None else None
        assert capi.lib().vp_octree_validate_host(ptr, args[1], args[2]) == 10001, args[1:]


# ---- the header, the ABI and the build list ---------------------------------------------------------------------------------------------
def test_header_prototypes_abi_and_build_list():
    text = open(os.path.join(ROOT, "include", "vphip.h")).read()
    assert re.search(r"#define\s+VP_ABI_VERSION\s+6\b", text)
    flat = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "int vp_octree(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_words, int algo, uint64_t* h_nodes );" in flat
    assert ("int vp_octree_result(vp_ctx* ctx, uint32_t** d_nodes, uint64_t* h_nodes, uint32_t* h_level_offset , uint32_t* h_full_leaves , "
            "uint32_t* h_n);") in flat
    assert "int vp_octree_expand(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_nodes, uint64_t nodes, int algo);" in flat
    assert "int vp_octree_expand_result(vp_ctx* ctx, uint32_t** d_words, uint32_t* h_n);" in flat
    assert "int vp_octree_validate_host(const uint32_t* h_nodes, uint64_t nodes, uint32_t n);" in flat
    assert "int vp_octree_host(" in flat and "int vp_octree_expand_host(" in flat
    assert "octree.hip" in build.HIP_SOURCES
    assert {"vp_octree", "vp_octree_result", "vp_octree_expand", "vp_octree_expand_result", "vp_octree_host", "vp_octree_expand_host", "vp_octree_validate_host"} <= set(capi.SYMBOLS)
    # no timing key was added: the 64-bit mask of vp_prof_select is full
    assert len(capi.EVERY_PROF_KEY) == 55 and len(capi.HEADER_PROF_KEYS) == 64


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    return build.build_cli()


def test_cli_octree_round_trips_to_the_grid_dump(cli, octree_exe, tmp_path):
    n = 64
    files = {}
    for t, args in (("0", []), ("3", []), ("0m", ["--morph", "dilate:2,fill,erode:2"])):
        d = tmp_path / ("t" + t)
        d.mkdir()
        p = subprocess.run([cli, M.asset("bunny.obj"), "-n", str(n), "-t", t[0], "--octree", "-d", str(d / "x")] + args, capture_output=True,
                           text=True, timeout=600, cwd=str(d))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        assert re.search(r"^\[\w*Octree\]: [0-9.]+ ms$", p.stdout, re.M), p.stdout
        svo = glob.glob(str(d / "out" / "*.svo"))
        assert [os.path.basename(s) for s in svo] == ["out_%s_out.svo" % ("sequential" if t[0] == "0" else "openmp")], svo
        tree = read_svo(svo[0])
        words = np.fromfile(str(d / "x.grid.u32"), np.uint32)
        nodes, lo, fl = R.build_numpy(R.words_to_bool(words, n))
        assert same_tree(tree, n, nodes, lo, fl), t
        m = re.search(r"^octree: n 64, P 64, nodes (\d+), per level \[([0-9, ]+)\], (\d+) bytes, grid 32768 bytes, ratio ([0-9.]+), ", p.stdout, re.M)
        assert m and int(m.group(1)) == len(nodes) and [int(v) for v in m.group(2).split(",")] == R.counts_of(lo, n), p.stdout
        assert int(m.group(3)) == 8 * len(nodes) and abs(float(m.group(4)) - 32768 / (8 * len(nodes))) < 0.006
        q = subprocess.run([octree_exe, "read", svo[0], "s", str(d / "back")], capture_output=True, text=True, timeout=300)
        assert q.returncode == 0, q.stdout
        assert np.array_equal(np.fromfile(str(d / "back.grid.u32"), np.uint32), words)
        files[t] = open(svo[0], "rb").read()
    assert files["0"] == files["3"] and files["0m"] != files["0"]


def test_cli_octree_refusals(cli, tmp_path):
    mesh = M.asset("d20.obj")
    for args in (["-n", "48", "--octree"], ["-n", "32", "--octree", "-g", "2"], ["-n", "2048", "--octree"]):
        p = subprocess.run([cli, mesh, "-t", "0"] + args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert p.returncode != 0, args
