"""Seeded watershed without a GPU: the numpy restatement of tests/watershed_ref.py against its literal form, against the geodesic
reference (zones), against the component labels, on the two-ball cases of the issue and on hand-made flood orders; what the cases at the
limits of the key reach (priorities up to 2^32 - 1, rank 16383, the extreme labels, gates on block seams, the comb past the sweep cap
of watershed.hip); the cut grid; the
host restatement of vplib/src/watershed.cpp through the C++ API on both word types, on every case of the GPU tests, byte for byte and
statistics included, and its refusals; `vpcli --watershed`; the header's prototypes."""
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
import geodesic_ref  # noqa: E402
import watershed_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference itself ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", R.CONNS)
def test_reference_equals_its_literal_form(conn):
    """the index-list form starts a level from the neighbours of the voxels whose level it is: the same bytes as the definition"""
    for name in R.CASES:
        m, L, P, order, q = R.case(name)
        if not R.has_literal(name):                                 # a side above 32, or thousands of levels: minutes
            continue
        W, cut, stats = R.watershed_literal(m, L, P, order, q, conn)
        e = R.expected(name, conn)
        assert np.array_equal(W, e[0]) and np.array_equal(cut, e[1]) and stats == e[2], (name, conn)
    # every gate, quantum and comb, and the four wide cases of 256 levels
    assert all(R.has_literal(name) for name in R.GATE_CASES + R.QUANTA + R.COMBS)
    assert [name for name in R.WIDES if R.has_literal(name)] == [R.wide_name(q, R.TOP, 256, o) for q in (1, 3) for o in R.ORDERS]


# ---- the limits of the key ---------------------------------------------------------------------------------------------------------------
def levels_of(name):
    """(first level, last level, q) over M"""
    m, _, P, _, q = R.case(name)
    level = P.astype(np.int64)[m] // q
    return int(level.min()), int(level.max()), q


def test_limit_cases_reach_the_limits():
    """what the wide cases are for, as caps on the cases and not as measurements"""
    wraps = beyond = 0
    for name in R.WIDES + R.QUANTA:
        m, L, P, order, q = R.case(name)
        first, last, _ = levels_of(name)
        wraps += first % R.MAX_SPAN + (last - first) >= R.MAX_SPAN  # the index into the presence bitmap wraps
        beyond += last * q + q - 1 >= 1 << 32                       # the top of the last level's range of P lies beyond uint32
        rank, levels = R.ranks(m, P, order, q)
        for conn in R.CONNS:
            W, _, stats = R.expected(name, conn)
            assert stats[0] == 12 and stats[1] > 20000 and stats[2] == levels, (name, conn, stats)   # far more labelled than markers
            assert set(np.unique(W[m]).tolist()) - {0} == set(R.EXTREME_LABELS), (name, conn)
        assert set(np.unique(L[m]).tolist()) == {0} | set(R.EXTREME_LABELS)
        if name in R.WIDES:
            assert last - first == R.MAX_SPAN - 1 and {0, R.MAX_SPAN - 1} <= set(rank[m].tolist()), name
            assert last == int(name.split()[2][3:]) // q, name
        else:
            assert (first, last, levels) == (0, 1, 2) and int(P[m].max()) == R.TOP and int(P[m].min()) == 0, name
    assert wraps >= 6 and beyond >= 8, (wraps, beyond)
    # every rank value: the case that asks for all 16384 levels holds as many as the mask lets it, far above 2^13
    most = R.expected(R.wide_name(1, R.TOP, R.MAX_SPAN, R.ASCENDING), 6)[2][2]
    assert most > 12000, most
    assert [levels_of(R.wide_name(3, R.TOP, 256, o))[0] for o in R.ORDERS] == [0x55555555 - (R.MAX_SPAN - 1)] * 2
    assert R.fitting_quantum(np.array([0, R.TOP], np.uint32), np.ones(2, bool), 1) == 1 << 18


def test_a_short_rank_field_cannot_pass():
    """the reference with the rank cut to 13 bits differs from the true one on thousands of voxels of a wide case"""
    name = R.wide_name(1, R.TOP, 256, R.DESCENDING)
    m, L, P, order, q = R.case(name)
    first, last, _ = levels_of(name)
    cut_rank = (first + ((last - P.astype(np.int64)) & 0x1FFF)).astype(np.uint32)   # ascending over the cut ranks = descending with 13 bits
    W = R.watershed(m, L, cut_rank, R.ASCENDING, 1, 6)[0]
    assert int((W != R.expected(name, 6)[0]).sum()) > 1000


@pytest.mark.parametrize("conn", R.CONNS)
def test_adding_a_constant_to_the_field_changes_nothing(conn):
    """the wrap far from the top equals its copy moved down to first = 0"""
    for order in R.ORDERS:
        name = R.wide_name(1, R.SECOND_WRAP + R.MAX_SPAN - 1, 4096, order)
        m, L, P, _, q = R.case(name)
        moved = R.watershed(m, L, P - np.uint32(R.SECOND_WRAP), order, q, conn)
        e = R.expected(name, conn)
        assert int(P[m].min()) == R.SECOND_WRAP and np.array_equal(moved[0], e[0]) and np.array_equal(moved[1], e[1]) and moved[2] == e[2]


def in_block(W, b):
    return W[R.block_box(b)]


@pytest.mark.parametrize("conn", R.CONNS)
def test_gates_flood_a_block_at_a_level_it_does_not_hold(conn):
    for name in R.GATE_CASES:
        m, L, P, order, q = R.case(name)
        W, cut, stats = R.expected(name, conn)
        if name.startswith("two fronts"):
            a, b, c = R.TWO_FRONTS[name.split()[2]]
            assert (in_block(W, a) == 9).sum() > 7000 and (in_block(W, c) == 4).sum() > 7000 and stats[:3] == (2, 24576, 2) and stats[3] > 0
            both = np.unique(in_block(W, b), return_counts=True)
            assert both[0].tolist() == [4, 9] and both[1].min() > 2000, (name, both)   # B is split between the two fronts
            continue
        b = R.GATES[" ".join(name.split()[1:-1])]
        steps = sum(abs(u - v) for u, v in zip(R.GATE_A, b))
        assert (in_block(W, R.GATE_A) == 9).all()
        lo, hi = int(in_block(P, b).min()), int(in_block(P, R.GATE_A).min())
        assert lo == int(in_block(P, b).max()) and (lo < hi if order == R.ASCENDING else lo > hi)   # B's own level runs first, without a source
        if steps == 1 or conn == 26:
            assert stats == (1, 16384, 2, 0) and (in_block(W, b) == 9).all(), (name, conn, stats)
        else:
            assert stats == (1, 8192, 2, 0) and not in_block(W, b).any(), (name, conn, stats)
    assert sorted(sum(abs(u - v) for u, v in zip(R.GATE_A, b)) for b in R.GATES.values()) == [1] * 5 + [2] * 3 + [3] * 2


def comb_past_the_sweep_cap():
    """(mask, start, the sweeps the comb needs, kWsSweeps of watershed.hip), after the check that the first exceeds the second; shared with
    tests/test_watershed_gpu.py"""
    with open(os.path.join(os.path.dirname(capi.LIB_PATH), "csrc", "watershed.hip")) as f:
        cap = int(re.search(r"^constexpr uint32_t kWsSweeps = (\d+);", f.read(), re.M).group(1))
    mask, start, steps = geodesic_ref.comb()
    assert steps == 270 and int(mask.sum()) == 271
    # the 30 steps along x between two corridors cost no sweep of their own (a sweep walks a whole x row): count the 240 along y only
    assert steps - 30 > cap, "kWsSweeps has caught up with the comb: build a longer maze inside one block for the comb cases"
    return mask, start, steps - 30, cap


def test_the_comb_outlasts_the_sweep_cap():
    """the comb lies inside one block and a sweep of ws_relax carries a key one row on: its face steps must exceed the sweeps of one launch,
    so that the block stops at the cap and re-lists itself"""
    mask, start, _, _ = comb_past_the_sweep_cap()
    idx = np.argwhere(mask)
    assert idx[:, 2].max() < 32 and idx[:, 1].max() < 16 and idx[:, 0].max() < 16   # one block
    for conn in R.CONNS:
        assert R.expected("comb zones", conn)[2] == (1, 271, 1, 0) and R.expected("comb flood", conn)[2] == (1, 271, 3, 0)
    P = R.case("comb flood")[2]
    d = geodesic_ref.geodesic(mask, start, geodesic_ref.GEO_6)[0]
    assert sorted(set(P[mask].tolist())) == [0, 1, 2] and int(P[mask][np.argsort(d[mask])][-1]) == 2   # 0, 1, 2 along the path: every level ends in the block that is still re-listing itself


@pytest.mark.parametrize("conn", R.CONNS)
def test_zones_against_the_geodesic_reference(conn):
    """W(v) = the smallest label among the markers at the least geodesic distance, 0 where none arrives: the hop metric and the label tie,
    without sharing code"""
    metric = geodesic_ref.GEO_6 if conn == 6 else geodesic_ref.GEO_26
    rng = np.random.default_rng(5)
    mask = rng.random((32, 32, 32)) < (0.45 if conn == 6 else 0.25)
    L = np.zeros(mask.shape, np.uint32)
    L.reshape(-1)[rng.choice(32 ** 3, 14, replace=False)] = rng.integers(1, 6, 14)   # several voxels and blobs per label, some outside M
    W, cut, stats = R.watershed(mask, L, None, conn=conn)
    best = np.full(mask.shape, np.int64(geodesic_ref.NONE))
    want = np.zeros(mask.shape, np.uint32)
    for k in sorted(set(L[mask & (L != 0)].tolist())):
        d = geodesic_ref.geodesic(mask, L == k, metric)[0].astype(np.int64)
        closer = d < best                                           # ascending labels and a strict test: the smaller label keeps a tie
        want[closer] = k
        best[closer] = d[closer]
    assert np.array_equal(W, want)
    assert (W[mask] == 0).any() and len(np.unique(W)) >= 4 and stats[1] == int((want != 0).sum())


@pytest.mark.parametrize("conn", R.CONNS)
def test_component_labels_as_markers_come_back(conn):
    mask = R._random(32, 0.3, 3, 4)[0]
    labels, k = components_ref.label_bool(mask, conn)
    assert 2 < k <= R.LABEL_MAX
    for P in (None, R._random(32, 0.3, 255, 4)[2]):
        W, cut, stats = R.watershed(mask, labels, P, R.ASCENDING, 3, conn)
        assert np.array_equal(W, labels) and np.array_equal(cut, mask)
        assert stats[0] == stats[1] == int(mask.sum()) and stats[3] == 0


def off_side(W, mask, side):
    return int((mask & (W != side)).sum())


@pytest.mark.parametrize("conn", R.CONNS)
def test_two_equal_balls_split_on_their_symmetry_plane(conn):
    mask, L, P, side = R.two_balls(R.EQUAL_BALLS)
    assert np.array_equal(P, edt_ref.edt_numpy(mask, edt_ref.UNSET)) and int(mask.sum()) == 21733
    W = R.expected("equal balls", conn)[0]
    assert off_side(W, mask, side) == 0                             # not one voxel off the plane x = 32 ...
    assert (side[:, :, 32] == 1).all() and (W[:, :, 32][mask[:, :, 32]] == 1).all() and mask[:, :, 32].any()   # ... which goes to label 1


# measured with this reference: the voxels off the radical plane's side, connectivity -> (labels as given, labels swapped)
UNEQUAL_OFF = {6: (28, 43), 26: (49, 26)}


@pytest.mark.parametrize("conn", R.CONNS)
def test_two_unequal_balls_split_near_their_radical_plane(conn):
    for swapped in (False, True):
        mask, L, P, side = R.two_balls(R.UNEQUAL_BALLS, swapped)
        assert int(mask.sum()) == 18174
        W = R.expected("unequal balls swapped" if swapped else "unequal balls", conn)[0]
        off = off_side(W, mask, side)
        print("unequal balls, connectivity %d, swapped %d: %d voxels off the radical plane's side" % (conn, swapped, off))
        assert off <= 181                                           # 1 % of |M|
        assert off == UNEQUAL_OFF[conn][swapped]


# ---- flood order -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", R.CONNS)
def test_ascending_equals_descending_on_the_mirrored_field(conn):
    m, L, P = R._random(32, 0.7, 255, 21)
    top = int(P[m].max())
    mirrored = np.where(m, top - P.astype(np.int64), 0).astype(np.uint32)
    a = R.watershed(m, L, P, R.ASCENDING, 1, conn)
    d = R.watershed(m, L, mirrored, R.DESCENDING, 1, conn)
    assert np.array_equal(a[0], d[0]) and np.array_equal(a[1], d[1]) and a[2] == d[2]
    assert not np.array_equal(a[0], R.watershed(m, L, P, R.DESCENDING, 1, conn)[0])


@pytest.mark.parametrize("conn", R.CONNS)
def test_a_constant_field_equals_zones(conn):
    m, L, _ = R._random(32, 0.7, 3, 22)
    zones = R.watershed(m, L, None, conn=conn)
    for order, q in ((R.ASCENDING, 1), (R.DESCENDING, 5)):
        flat = R.watershed(m, L, np.full(m.shape, 77, np.uint32), order, q, conn)
        assert np.array_equal(flat[0], zones[0]) and np.array_equal(flat[1], zones[1]) and flat[2] == zones[2]
    coarse = R.watershed(m, L, R._random(32, 0.7, 255, 22)[2], R.ASCENDING, 256, conn)   # every level in one quantum
    assert np.array_equal(coarse[0], zones[0]) and coarse[2] == zones[2]


def corridor():
    """(mask, markers, P) at n = 32, a corridor along x at y = z = 5: marker 1 at x = 2, marker 2 at x = 28, a basin without a marker at
    x = 11 .. 19 behind a pass of height 5 at x = 10 and one of height 3 at x = 20; a second component without a marker; a marker outside M"""
    m = np.zeros((32, 32, 32), bool)
    m[5, 5, 2:29] = True
    P = np.zeros(m.shape, np.uint32)
    P[5, 5, 3:10] = 2
    P[5, 5, 10] = 5
    P[5, 5, 11:20] = 1
    P[5, 5, 20] = 3
    P[5, 5, 21:28] = 2
    m[20, 20, 3:9] = True                                           # no marker here
    L = R.marker_volume(32, [((2, 5, 5), 1), ((28, 5, 5), 2), ((15, 6, 5), 9)])   # label 9 lies outside M, next to the basin
    return m, L, P


@pytest.mark.parametrize("conn", R.CONNS)
def test_basins_components_and_markers_outside(conn):
    m, L, P = corridor()
    W, cut, stats = R.watershed(m, L, P, R.ASCENDING, 1, conn)
    row = W[5, 5]
    # the basin is reached over its lower pass, at level 3, by label 2; the higher pass is then won by the basin's side: its source
    # (x = 11, level 1) lies earlier in flood order than the other one (x = 9, level 2)
    assert (row[2:10] == 1).all() and (row[10:29] == 2).all()
    assert not W[20].any() and not (W == 9).any() and stats == (2, 27, 5, 1)
    # without the priority field the corridor is split half way, the tie going to the smaller label
    Z = R.watershed(m, L, None, conn=conn)[0][5, 5]
    assert (Z[2:16] == 1).all() and (Z[16:29] == 2).all()


# ---- the cut grid ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", R.CONNS)
def test_cut_grid_separates_the_labels(conn):
    for name in ("unequal balls", "seams flood", "random 64 0.7 255 1 q1 asc", "not a power of two"):
        W, cut, stats = R.expected(name, conn)
        n = W.shape[0]
        inside = np.where(cut, W, 0)
        p = np.pad(inside, 1)
        for dx, dy, dz in R.offsets(conn):
            other = p[1 + dz:1 + dz + n, 1 + dy:1 + dy + n, 1 + dx:1 + dx + n]
            assert not ((inside != 0) & (other != 0) & (inside != other)).any(), (name, conn)
        assert stats[3] == stats[1] - int(cut.sum()) > 0 and not (cut & (W == 0)).any()
        assert np.array_equal(cut & (W == W.max()), W == W.max())     # one-sided: the largest label loses nothing


# ---- the C++ host form -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    pkg = os.path.dirname(capi.LIB_PATH)
    build.build_lib()
    srcs = [os.path.join(pkg, "vplib", "src", f) for f in sorted(os.listdir(os.path.join(pkg, "vplib", "src"))) if f.endswith(".cpp")]
    exe = str(tmp_path_factory.mktemp("watershed") / "watershed_check")
    subprocess.check_call(["g++", "-std=c++23", "-O2", "-ffp-contract=off", "-fopenmp",
                           "-I", os.path.join(pkg, "vplib", "include"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "watershed_check.cpp")] + srcs + ["-o", exe, "-L", pkg, "-lvphip", "-Wl,-rpath," + pkg])
    return exe


def run_check(exe, mask, markers, priority, order, q, conn, bits, types, prefix, timeout=900):
    """the finished process and {tag: (W uint32[n^3], cut words, statistics)} of tests/cpp/watershed_check.cpp"""
    n = mask.shape[0]
    R.bool_to_words(mask).tofile(prefix + ".mask.u32")
    np.ascontiguousarray(markers, np.uint32).tofile(prefix + ".markers.u32")
    if priority is not None:
        np.ascontiguousarray(priority, np.uint32).tofile(prefix + ".priority.u32")
    p = subprocess.run([exe, prefix + ".mask.u32", prefix + ".markers.u32", "-" if priority is None else prefix + ".priority.u32", str(n), str(order),
                        str(q), str(conn), str(bits), types, prefix], timeout=timeout, capture_output=True, text=True)
    if p.returncode != 0:
        return p, {}
    stats = {t: tuple(int(v) for v in rest.split()) for t, rest in re.findall(r"^(seq|omp|naive|tiled) (\d+ \d+ \d+ \d+)$", p.stdout, re.M)}
    tags = {"s": "seq", "o": "omp", "n": "naive", "t": "tiled"}
    return p, {tags[c]: (np.fromfile("%s.%s.labels.u32" % (prefix, tags[c]), np.uint32), np.fromfile("%s.%s.cut.u32" % (prefix, tags[c]), np.uint32),
                         stats[tags[c]]) for c in types}


@pytest.mark.parametrize("conn", R.CONNS)
def test_host_form_equals_numpy(check_exe, tmp_path, conn):
    prefix = str(tmp_path / "h")
    for k, name in enumerate(R.CASES):
        mask, markers, P, order, q = R.case(name)
        W, cut, stats = R.expected(name, conn)
        for bits in ((32, 64) if name in R.LIMITS else (64 if k % 2 else 32,)):   # the cases at the limits of the key on both word types
            p, got = run_check(check_exe, mask, markers, P, order, q, conn, bits, "so", prefix)
            assert p.returncode == 0, (name, bits, p.stdout[-500:] + p.stderr[-500:])
            for tag in ("seq", "omp"):
                assert np.array_equal(got[tag][0], W.reshape(-1)), (name, bits, tag)
                assert np.array_equal(got[tag][1], R.bool_to_words(cut)), (name, bits, tag)
                assert got[tag][2] == stats, (name, bits, tag, got[tag][2], stats)


def test_host_form_on_the_hand_made_orders(check_exe, tmp_path):
    m, L, P = corridor()
    for conn in R.CONNS:
        for priority, order in ((P, R.ASCENDING), (None, R.DESCENDING)):
            W, cut, stats = R.watershed(m, L, priority, order, 1, conn)
            p, got = run_check(check_exe, m, L, priority, order, 1, conn, 32, "s", str(tmp_path / "c"))
            assert p.returncode == 0
            assert np.array_equal(got["seq"][0], W.reshape(-1)) and np.array_equal(got["seq"][1], R.bool_to_words(cut)) and got["seq"][2] == stats


def test_host_form_bounds(check_exe, tmp_path):
    """span 16384 refused, 16383 served; label 2^20 refused, 2^20 - 1 served; quantum 0 refused; what lies outside the mask does not count"""
    prefix = str(tmp_path / "b")
    m = np.zeros((32, 32, 32), bool)
    m[3, 3, 2:12] = True
    P = np.zeros(m.shape, np.uint32)
    L = R.marker_volume(32, [((2, 3, 3), 1), ((11, 3, 3), R.LABEL_MAX)])

    def served(markers, priority, order=R.DESCENDING, q=1):
        p, got = run_check(check_exe, m, markers, priority, order, q, 6, 32, "s", prefix)
        if p.returncode == 0:
            W, cut, stats = R.watershed(m, markers, priority, order, q, 6)
            assert np.array_equal(got["seq"][0], W.reshape(-1)) and got["seq"][2] == stats
        return p.returncode == 0

    P[3, 3, 5], P[3, 3, 6] = 1000, 1000 + R.MAX_SPAN - 1
    P[3, 3, 2:5] = P[3, 3, 7:12] = 1000
    assert served(L, P)                                             # span 16383, labels 1 and 2^20 - 1
    P[3, 3, 6] += 1
    assert not served(L, P) and R.fitting_quantum(P, m, 1) == 2     # span 16384
    assert served(L, P, q=2) and served(L, P, R.ASCENDING, 3)
    assert not served(L, P, q=0)
    assert served(L, None, 7, 0)                                    # zones: order and quantum are not looked at
    big = L.copy()
    big[3, 3, 11] = R.LABEL_MAX + 1
    assert not served(big, None)
    big[3, 3, 11], big[9, 9, 9] = R.LABEL_MAX, R.LABEL_MAX + 1      # outside the mask: ignored
    P[3, 3, 6], P[9, 9, 9] = 1000, 0xFFFFFFFF
    assert served(big, P)


# ---- the CLI -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    return build.build_cli()


def cli_expected(vox, radius, q, conn):
    """(W, cut, the line `vpcli --watershed` prints) for the grid `vox` it starts from"""
    d2 = edt_ref.edt_numpy(vox, edt_ref.UNSET)
    markers, count = components_ref.label_bool(d2.astype(np.int64) > radius * radius, conn)
    W, cut, st = R.watershed(vox, markers, d2, R.DESCENDING, q, conn)
    n = vox.shape[0]
    return W, cut, count, "watershed: n %d, markers %d, marker voxels %d, labelled %d, levels %d, cut %d" % (n, count, st[0], st[1], st[2], st[3])


def cli_run(cli, tmp_path, tag, mesh, n, t, args):
    """(stdout, the dumped grid as bool, the dumped labels or None) of one run in a folder of its own"""
    d = tmp_path / tag
    d.mkdir()
    p = subprocess.run([cli, M.asset(mesh), "-n", str(n), "-t", t, "-d", str(d / "x")] + args, capture_output=True, text=True, timeout=600, cwd=str(d))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    labels = str(d / "x.labels.u32")
    return p.stdout, R.words_to_bool(np.fromfile(str(d / "x.grid.u32"), np.uint32), n), np.fromfile(labels, np.uint32) if os.path.exists(labels) else None


def test_cli_cpu_types_equal_numpy(cli, tmp_path):
    for k, (t, mesh, arg, radius, q, conn) in enumerate((("0", "bunny.obj", "2", 2, 1, 6), ("3", "bunny.obj", "4:4:26", 4, 4, 26),
                                                         ("3", "bimba.obj", "3:1", 3, 1, 6), ("0", "bimba.obj", "2:7:26", 2, 7, 26))):
        _, vox, none = cli_run(cli, tmp_path, "plain%d" % k, mesh, 64, t, [])
        out, grid, labels = cli_run(cli, tmp_path, "split%d" % k, mesh, 64, t, ["--watershed", arg])
        W, cut, count, line = cli_expected(vox, radius, q, conn)
        assert none is None and line + "\n" in out, (out, line)
        assert np.array_equal(labels, W.reshape(-1)) and np.array_equal(grid, cut)           # the cut grid replaced the working grid
        assert re.search(r"^\[\w*Watershed\]: [0-9.]+ ms$", out, re.M), out
        assert count >= (2 if k != 3 else 1) and int(W.max()) == count


def test_cli_later_steps_act_on_the_separated_parts(cli, tmp_path):
    """--fill comes before, the exports and --geodesic after: the labels file of -e, and a geodesic reach that stops at the cut"""
    _, vox, _ = cli_run(cli, tmp_path, "plain", "bunny.obj", 64, "0", ["--fill"])
    out, grid, labels = cli_run(cli, tmp_path, "split", "bunny.obj", 64, "0", ["--fill", "--watershed", "2", "-e", "--geodesic", "zmax:6"])
    W, cut, count, line = cli_expected(vox, 2, 1, 6)
    assert line + "\n" in out and count == 4 and np.array_equal(grid, cut)
    raw = np.fromfile(str(tmp_path / "split" / "out" / "bunny_sequential_labels.raw"), np.uint32)
    assert np.array_equal(raw, W.reshape(-1)) and np.array_equal(labels, raw)
    reach = R.words_to_bool(np.fromfile(str(tmp_path / "split" / "x.reach.u32"), np.uint32), 64)
    top = np.unique(W[reach])
    assert reach.any() and len(top) == 1 and int((W == top[0]).sum()) > int(reach.sum()) > 0    # one part, less what the cut took from it


def test_cli_refuses_bad_watershed_arguments(cli, tmp_path):
    mesh = M.asset("d20.obj")
    for args in (["--watershed", "2", "-g", "2"], ["--watershed", "0"], ["--watershed", "x"], ["--watershed", "2:0"], ["--watershed", "2:1:8"],
                 ["--watershed", "2:1:6:1"], ["--watershed", ":2"], ["--watershed", "70000"], ["--watershed", "2:"], ["--watershed"]):
        p = subprocess.run([cli, mesh, "-n", "32", "-t", "0"] + args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert p.returncode != 0, args
    p = subprocess.run([cli, mesh, "-n", "32", "-t", "0", "--watershed", "40"], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode == 0 and "watershed: n 32, markers 0, marker voxels 0, labelled 0, " in p.stdout    # eroded away: nothing is labelled
    p = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert "--watershed" in p.stdout + p.stderr


# ---- the header --------------------------------------------------------------------------------------------------------------------------
def test_prototypes_and_sources():
    with open(os.path.join(ROOT, "include", "vphip.h")) as f:
        header = f.read()
    for proto in ("int vp_watershed(vp_ctx* ctx, const vp_frame* f, const uint32_t* d_mask, const uint32_t* d_markers, const uint32_t* d_priority",
                  "int vp_watershed_result(vp_ctx* ctx, uint32_t** d_labels, uint32_t** d_cut, uint64_t* h_stats",
                  "int vp_watershed_host(vp_ctx* ctx, const vp_frame* f, const uint32_t* h_mask, const uint32_t* h_markers, const uint32_t* h_priority",
                  "enum { VP_WS_ASCENDING = 0, VP_WS_DESCENDING = 1 };", "#define VP_WS_LABEL_MAX 0xFFFFFu", "#define VP_WS_MAX_SPAN 16384u",
                  "#define VP_ABI_VERSION 6"):
        assert proto in header, proto
    assert "watershed.hip" in build.HIP_SOURCES
    assert {"vp_watershed", "vp_watershed_result", "vp_watershed_host"} <= set(capi.SYMBOLS)
    assert (capi.WS_ASCENDING, capi.WS_DESCENDING, capi.WS_LABEL_MAX, capi.WS_MAX_SPAN) == (0, 1, R.LABEL_MAX, R.MAX_SPAN)
    assert len(capi.HEADER_PROF_KEYS) == 64
    pkg = os.path.dirname(capi.LIB_PATH)
    with open(os.path.join(pkg, "csrc", "geodesic.hip")) as f:      # the neighbour-block rule moved, it was not copied
        assert "block_seen_by(" in f.read()
    with open(os.path.join(pkg, "csrc", "block_list.h")) as f:
        assert f.read().count("uint32_t block_seen_by(") == 1
