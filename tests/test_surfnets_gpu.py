"""Surface nets on the GPU (vp_surfnets_count / vp_surfnets, csrc/surfnets.hip) against the numpy restatement of tests/surfnets_ref.py, bit
for bit: records, quads and the float32 positions viewed as uint32 -- every operation of the contract is one correctly rounded IEEE
operation in a prescribed order.  Each case runs for both algos and for 0, 1 and 8 relaxation steps.  The shapes are the smallest at which
each part can go wrong: n = 32 (one word per voxel row: the 33rd cell of every row and the whole -1 layer), n = 64 (a voxel on either side
of the word edge, the golden bunny grid, a random grid with nearly every cell active: many blocks in the scan, more quads than vertices),
n = 96 (three words per row, 97 cells), n = 128 (a grid repaired through the engine; Q against vp_extract's exposed faces) and n = 1024
(single voxels in the two far corners, expectations by hand: 32-bit overflow in the cell index arithmetic)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cuda_mesh_voxelization_amd import build, capi, mesh as M
from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surfnets_ref as R  # noqa: E402
from fill_ref import bool_to_words, words_to_bool  # noqa: E402
from test_surfnets_cpu import check_exe, run_check  # noqa: E402,F401

pytestmark = pytest.mark.gpu

ALGOS = (ALGO_TILED, ALGO_NAIVE)
ITERS = (0, 1, 8)
INVALID, UNSUPPORTED = 10001, 10002


def _unit_frame(n):
    return Frame.make(n, 1.0 / n, np.zeros(3, np.float32))


def _dev(engine, words):
    return engine.to_device(words, np.uint32)


def _numpy(cells, xyz, quads):
    return cells.cpu().numpy().view(np.uint64), xyz.cpu().numpy(), quads.cpu().numpy().view(np.uint32)


def _sphere96():
    z, y, x = np.mgrid[0:96, 0:96, 0:96]
    return (x - 47.3) ** 2 + (y - 48.1) ** 2 + (z - 46.7) ** 2 < 41.5 ** 2


GRIDS = {
    "32 empty": lambda: np.zeros((32, 32, 32), bool),
    "32 voxel": lambda: R.single_voxel(32, (5, 6, 7)),
    "32 voxel first": lambda: R.single_voxel(32, (0, 0, 0)),
    "32 voxel last": lambda: R.single_voxel(32, (31, 31, 31)),
    "32 full": lambda: np.ones((32, 32, 32), bool),
    "32 sphere": lambda: R.sphere(32),
    "32 torus": R.torus,
    "32 checkerboard": lambda: R.checkerboard(32),
    "32 random 0.1": lambda: R.random_bool(32, 0.1, 11),
    "32 random 0.5": lambda: R.random_bool(32, 0.5, 12),
    "64 voxel x31": lambda: R.single_voxel(64, (31, 3, 4)),
    "64 voxel x32": lambda: R.single_voxel(64, (32, 3, 4)),
    "64 bunny": R.bunny64,
    "64 random 0.5": lambda: R.random_bool(64, 0.5, 13),
    "96 random 0.1": lambda: R.random_bool(96, 0.1, 14),
    "96 sphere": _sphere96,
}


@pytest.fixture(scope="module")
def refs():
    """the restatement, once per grid and shared by every test: name -> (words, n, cells, {iterations: xyz}, quads); never written to"""
    cache = {}

    def get(name):
        if name not in cache:
            vox = GRIDS[name]()
            cells, xyz, quads = R.surfnets_bool(vox, every=ITERS)
            for a in (cells, quads, *xyz.values()):
                a.setflags(write=False)
            cache[name] = (bool_to_words(vox), vox.shape[0], cells, xyz, quads)
        return cache[name]
    return get


def _compare(got, cells, xyz, quads, tag):
    gc, gx, gq = got
    assert gc.shape == cells.shape and gq.shape == quads.shape, (tag, gc.shape, gq.shape, cells.shape, quads.shape)
    assert np.array_equal(gc, cells), (tag, "records", int(np.count_nonzero(gc != cells)))
    assert np.array_equal(gq, quads), (tag, "quads", int(np.count_nonzero(gq != quads)))
    assert np.array_equal(gx.view(np.uint32), xyz.view(np.uint32)), (tag, "positions", int(np.count_nonzero(gx != xyz)))


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", list(GRIDS))
def test_device_equals_the_restatement_bit_for_bit(engine, refs, name, algo):
    words, n, cells, xyz, quads = refs(name)
    fr = _unit_frame(n)
    g = _dev(engine, words)
    assert engine.ctx.surfnets_count(fr, g.data_ptr(), algo) == (len(cells), len(quads))
    for it in ITERS:
        _compare(_numpy(*engine.surface_nets(fr, g, it, algo)), cells, xyz[it], quads, (name, algo, it))


def test_repaired_grid_at_128_and_the_exposed_faces_of_extract(engine):
    n = 128
    xyz, tri = M.bunny_decimated()
    origin, vs = M.frame([xyz], n)
    fr = Frame.make(n, vs, origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    g = engine.voxelize_conservative(fr, dx, dt)
    g = engine.morph(fr, g, capi.MORPH_DILATE, 2)
    g, _ = engine.fill_interior(fr, g)
    g = engine.morph(fr, g, capi.MORPH_ERODE, 2)
    g, k, kept = engine.components_filter(fr, g, capi.COMP_KEEP_LARGEST, 1)
    assert k >= 1 and kept > 10000
    words = engine.words_to_numpy(g).copy()
    cells, ref_xyz, quads = R.surfnets_numpy(words, n, every=ITERS)
    assert R.edge_stats(quads)[0]
    for algo in ALGOS:
        for it in ITERS:
            _compare(_numpy(*engine.surface_nets(fr, g, it, algo)), cells, ref_xyz[it], quads, (algo, it))
    # the same count by different code: the face masks of the exposed-voxel records
    count = engine.ctx.extract_count(fr, g.data_ptr(), capi.EXTRACT_EXPOSED)
    rec = torch.empty(count, dtype=torch.int64, device=engine.device)
    engine.ctx.extract(fr, g.data_ptr(), capi.EXTRACT_EXPOSED, None, rec.data_ptr(), None, count)
    masks = (rec.cpu().numpy().view(np.uint64) >> np.uint64(40)).astype(np.uint8)
    faces = int(np.unpackbits(masks).sum())
    assert faces == len(quads) == R.exposed_faces(words_to_bool(words, n))
    assert engine.ctx.surfnets_count(fr, g.data_ptr(), ALGO_TILED) == (len(cells), faces)


@pytest.mark.parametrize("algo", ALGOS)
def test_far_corners_at_1024_by_hand(engine, algo):
    n = 1024
    fr = _unit_frame(n)
    g = torch.zeros(fr.words, dtype=torch.int32, device=engine.device)
    assert engine.ctx.surfnets_count(fr, g.data_ptr(), algo) == (0, 0)
    cells, xyz, quads = engine.surface_nets(fr, g, 8, algo)
    assert cells.numel() == 0 and tuple(xyz.shape) == (0, 3) and tuple(quads.shape) == (0, 4)
    for v in ((0, 0, 0), (1023, 1023, 1023)):
        word = (v[0] + n * (v[1] + n * v[2])) // 32
        g[word] = 1 if v[0] == 0 else -(1 << 31)                       # bit 0 / bit 31 of the word
        ec, _, eq = R.single_voxel_expectation(n, v)
        # by hand again, without the helper: the first and the last record
        n1 = n + 1
        assert int(ec[0]) == (v[0] + n1 * (v[1] + n1 * v[2])) | (0x80 << 40)
        assert int(ec[7]) == ((v[0] + 1) + n1 * ((v[1] + 1) + n1 * (v[2] + 1))) | (0x01 << 40)
        assert engine.ctx.surfnets_count(fr, g.data_ptr(), algo) == (8, 6)
        for it in ITERS:
            _compare(_numpy(*engine.surface_nets(fr, g, it, algo)), ec, R.single_voxel_relaxed(n, v, it), eq, (v, algo, it))
        g[word] = 0
    del g
    engine.ctx.release()                                               # NAIVE: the index volume is 4 (n+1)^3 bytes
    torch.cuda.empty_cache()


def test_two_runs_and_the_two_algos_give_the_same_bytes(engine, refs):
    words, n, cells, xyz, quads = refs("64 random 0.5")
    fr = _unit_frame(n)
    g = _dev(engine, words)
    runs = [engine.surface_nets(fr, g, 8, algo) for algo in (ALGO_TILED, ALGO_TILED, ALGO_NAIVE, ALGO_NAIVE)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _refused(code, fn):
    with pytest.raises(capi.VPError) as e:
        fn()
    assert e.value.code == code, (e.value.code, code, str(e.value))


def test_write_needs_the_count_of_the_same_grid_and_enough_room(engine, refs):
    words, n, cells, xyz, quads = refs("32 sphere")
    fr = _unit_frame(n)
    ctx = engine.ctx
    g, h = _dev(engine, words), _dev(engine, words)
    V, Q = len(cells), len(quads)
    sent = 0x5A5A5A5A
    dc = torch.full((2 * V,), sent, dtype=torch.int32, device=engine.device)
    dx = torch.full((3 * V,), sent, dtype=torch.int32, device=engine.device)
    dq = torch.full((4 * Q,), sent, dtype=torch.int32, device=engine.device)
    write = lambda grid, algo=ALGO_TILED, it=1, vc=V, qc=Q: ctx.surfnets(fr, grid.data_ptr(), algo, it, dc.data_ptr(), dx.data_ptr(), dq.data_ptr(), vc, qc)  # noqa: E731
    ctx.release()                                                      # whatever an earlier test counted is gone
    _refused(INVALID, lambda: write(g))                                # no count at all
    assert ctx.surfnets_count(fr, g.data_ptr(), ALGO_TILED) == (V, Q)
    _refused(INVALID, lambda: write(h))                                # another buffer with the same contents
    _refused(INVALID, lambda: write(g, ALGO_NAIVE))                    # the other algo
    _refused(INVALID, lambda: write(g, vc=V - 1))                      # short capacities
    _refused(INVALID, lambda: write(g, qc=Q - 1))
    _refused(INVALID, lambda: write(g, vc=0, qc=0))
    _refused(INVALID, lambda: write(g, it=65))
    _refused(INVALID, lambda: write(g, algo=0))
    _refused(INVALID, lambda: ctx.surfnets(fr, g.data_ptr(), ALGO_TILED, 1, 0, dx.data_ptr(), dq.data_ptr(), V, Q))
    _refused(INVALID, lambda: ctx.surfnets(fr, g.data_ptr(), ALGO_TILED, 1, dc.data_ptr(), g.data_ptr(), dq.data_ptr(), V, Q))   # output = grid
    ctx.memset(g.data_ptr(), 0, 64)                                    # the grid is rewritten through the ABI: the count is dropped
    _refused(INVALID, lambda: write(g))
    g.copy_(h)
    assert ctx.surfnets_count(fr, g.data_ptr(), ALGO_TILED) == (V, Q)
    ctx.csg(g.data_ptr(), h.data_ptr(), fr.words, capi.OP_UNION)       # a CSG into the grid, even one that changes nothing
    _refused(INVALID, lambda: write(g))
    engine.sync()
    for t in (dc, dx, dq):
        assert bool((t == sent).all())
    assert ctx.surfnets_count(fr, g.data_ptr(), ALGO_TILED) == (V, Q)
    write(g, it=1, vc=V + 5, qc=Q + 7)                                 # room to spare is fine; the tail stays untouched
    engine.sync()
    _compare((dc.cpu().numpy().view(np.uint64), dx.cpu().numpy().view(np.float32).reshape(-1, 3), dq.cpu().numpy().view(np.uint32).reshape(-1, 4)),
             cells, xyz[1], quads, "after the refusals")


def test_refusals_leave_the_outputs_untouched(engine):
    n = 64
    fr = _unit_frame(n)
    ctx = engine.ctx
    g = _dev(engine, bool_to_words(R.random_bool(n, 0.3, 3)))
    V, Q = ctx.surfnets_count(fr, g.data_ptr(), ALGO_TILED)
    sent = 0x5A5A5A5A
    dc = torch.full((2 * V,), sent, dtype=torch.int32, device=engine.device)
    dx = torch.full((3 * V,), sent, dtype=torch.int32, device=engine.device)
    dq = torch.full((4 * Q,), sent, dtype=torch.int32, device=engine.device)
    slab = Frame.make(n, 1.0 / n, np.zeros(3, np.float32), 0, 32)
    large = Frame.make(2048, 1.0 / 2048, np.zeros(3, np.float32))
    small = Frame.make(48, 1.0 / 48, np.zeros(3, np.float32))
    nv, nq = ctypes.c_uint64(77), ctypes.c_uint64(78)
    for bad in (slab, large, small):
        assert capi.lib().vp_surfnets_count(ctx._h, ctypes.byref(bad), g.data_ptr(), ALGO_TILED, ctypes.byref(nv), ctypes.byref(nq)) == UNSUPPORTED
        _refused(UNSUPPORTED, lambda: ctx.surfnets(bad, g.data_ptr(), ALGO_TILED, 1, dc.data_ptr(), dx.data_ptr(), dq.data_ptr(), V, Q))
    for algo in (0, 3):
        assert capi.lib().vp_surfnets_count(ctx._h, ctypes.byref(fr), g.data_ptr(), algo, ctypes.byref(nv), ctypes.byref(nq)) == INVALID
    assert capi.lib().vp_surfnets_count(ctx._h, ctypes.byref(fr), None, ALGO_TILED, ctypes.byref(nv), ctypes.byref(nq)) == INVALID
    assert capi.lib().vp_surfnets_count(ctx._h, ctypes.byref(fr), g.data_ptr(), ALGO_TILED, None, ctypes.byref(nq)) == INVALID
    assert capi.lib().vp_surfnets_count(ctx._h, ctypes.byref(fr), g.data_ptr(), ALGO_TILED, ctypes.byref(nv), None) == INVALID
    assert (nv.value, nq.value) == (77, 78)
    _refused(INVALID, lambda: ctx.surfnets(fr, g.data_ptr(), ALGO_TILED, 65, dc.data_ptr(), dx.data_ptr(), dq.data_ptr(), V, Q))
    _refused(INVALID, lambda: ctx.surfnets(fr, 0, ALGO_TILED, 1, dc.data_ptr(), dx.data_ptr(), dq.data_ptr(), V, Q))
    engine.sync()
    for t in (dc, dx, dq):
        assert bool((t == sent).all())
    # the host form: the same refusals, host outputs untouched
    h = bool_to_words(R.random_bool(n, 0.3, 3))
    hc, hx, hq = np.full(V, 7, np.uint64), np.full((V, 3), 7, np.float32), np.full((Q, 4), 7, np.uint32)

    def host(frame, it=1, vc=V, qc=Q):
        return capi.lib().vp_surfnets_host(ctx._h, ctypes.byref(frame), h.ctypes.data, it, hc.ctypes.data, hx.ctypes.data, hq.ctypes.data, vc, qc,
                                           ctypes.byref(nv), ctypes.byref(nq))
    assert host(slab) == UNSUPPORTED and host(large) == UNSUPPORTED and host(fr, it=65) == INVALID
    assert host(fr, vc=V - 1) == INVALID and host(fr, qc=Q - 1) == INVALID
    assert (hc == 7).all() and (hx == 7).all() and (hq == 7).all() and (nv.value, nq.value) == (77, 78)


def test_host_form_and_timing_keys(engine, refs):
    words, n, cells, xyz, quads = refs("96 random 0.1")
    fr = _unit_frame(n)
    ctx = engine.ctx
    assert ctx.surfnets_host(fr, words, counts_only=True) == (len(cells), len(quads))
    _compare(ctx.surfnets_host(fr, words, 8), cells, xyz[8], quads, "host form")
    g = _dev(engine, words)
    for algo, keys in ((ALGO_TILED, {"sn_cells", "sn_scan", "sn_verts", "sn_quads", "sn_relax"}),
                       (ALGO_NAIVE, {"sn_cells_naive", "sn_scan", "sn_verts_naive", "sn_quads_naive", "sn_relax_naive"})):
        ctx.prof_reset()
        ctx.prof_enable(True)
        engine.surface_nets(fr, g, 3, algo)
        ctx.prof_enable(False)
        p = ctx.prof()
        assert set(p) == keys, p
        relax = "sn_relax" if algo == ALGO_TILED else "sn_relax_naive"
        assert all(v["launches"] == (3 if k == relax else 1) and v["ms"] > 0.0 for k, v in p.items()), p
    try:
        ctx.prof_select(["sn_quads"])
        ctx.prof_reset()
        ctx.prof_enable(True)
        engine.surface_nets(fr, g, 1, ALGO_TILED)
        ctx.prof_enable(False)
        assert set(ctx.prof()) == {"sn_quads"}
    finally:
        ctx.prof_enable(False); ctx.prof_select(None); ctx.prof_reset()


def test_cli_files_of_host_and_device_are_byte_identical_at_64(tmp_path):
    cli = build.build_cli()
    files = {}
    for t, name in (("0", "sequential"), ("2", "tiled")):
        d = tmp_path / t
        d.mkdir()
        p = subprocess.run([cli, M.asset("bunny.obj"), "-n", "64", "-t", t, "-e", "--surface-nets", "8"], capture_output=True, text=True,
                           timeout=600, cwd=str(d))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        files[t] = open(str(d / "out" / (name + "_bunny.obj")), "rb").read()
    assert len(files["0"]) > 100000 and files["0"] == files["2"]


def test_cpp_api_host_and_device_agree(check_exe, tmp_path, refs):  # noqa: F811
    for name in ("64 bunny", "96 random 0.1"):
        words, n, cells, xyz, quads = refs(name)
        lines, (hc, hx, hq, _) = run_check(check_exe, tmp_path, words_to_bool(words, n), 8, gpu=True)
        assert lines["seq32"] == lines["seq64"] == lines["dev32"] == lines["dev64"], (name, lines)
        _compare((hc, hx, hq), cells, xyz[8], quads, name)
