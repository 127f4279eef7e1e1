"""Iso-surface nets on the GPU (vp_isonets*, csrc/isonets.hip) against the numpy restatement of tests/isonets_ref.py, bit for bit: records,
quads, and the float32 positions and normals viewed as uint32 -- every operation of the contract is one correctly rounded IEEE operation in
a prescribed order.  Each case runs for both algos and for 0, 1 and 8 relaxation steps.  n = 32 (a cell row is one word plus the 33rd cell),
64 and 96 (word boundaries, a side off the powers of two); n = 1024 once per algo with nine lone voxels, expectations by hand (32-bit
overflow in the index arithmetic, a 4 GiB field)."""
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
import isonets_ref as R  # noqa: E402
import surfnets_ref as SR  # noqa: E402
from fill_ref import bool_to_words  # noqa: E402
from test_isonets_cpu import check_exe, mesh_case, run_check  # noqa: E402,F401

pytestmark = pytest.mark.gpu

ALGOS = (ALGO_TILED, ALGO_NAIVE)
ITERS = (0, 1, 8)
INVALID, UNSUPPORTED = 10001, 10002
LIN, SQ = R.LINEAR, R.SIGNED_SQUARE


def _unit_frame(n):
    return Frame.make(n, 1.0 / n, np.zeros(3, np.float32))


def _scaled_sphere(n, squared=False, c=R.SPHERE_C):
    k = n / 32.0
    return R.sphere_field(n, tuple(x * k for x in c), R.SPHERE_R * k, squared)


def _sphere96():
    z, y, x = np.mgrid[0:96, 0:96, 0:96]
    return (x - 47.3) ** 2 + (y - 48.1) ** 2 + (z - 46.7) ** 2 < 41.5 ** 2


# name -> (field, transform, iso)
CASES = {
    "32 sphere 0": lambda: (R.sphere_field(32), LIN, 0.0),
    "32 sphere 0.3": lambda: (R.sphere_field(32), LIN, 0.3),
    "32 sphere -1.7": lambda: (R.sphere_field(32), LIN, -1.7),
    "32 sphere sq 0": lambda: (R.sphere_field(32, squared=True), SQ, 0.0),
    "32 sphere sq 0.3": lambda: (R.sphere_field(32, squared=True), SQ, 0.3),
    "32 sphere sq -1.7": lambda: (R.sphere_field(32, squared=True), SQ, -1.7),
    "32 cut sphere": lambda: (R.sphere_field(32, c=R.CUT_C), LIN, 0.0),
    "32 laced 0": lambda: (R.laced_random_field(32, 2024), LIN, 0.0),
    "32 laced sq 0.25": lambda: (R.laced_random_field(32, 2024), SQ, 0.25),
    "32 laced sq -0.6": lambda: (R.laced_random_field(32, 2024), SQ, -0.6),
    "32 checkerboard inf": lambda: (R.signed_zero_field(SR.checkerboard(32), inf=True), SQ, 0.0),
    "32 torus zeros": lambda: (R.signed_zero_field(SR.torus()), LIN, 0.0),
    "64 sphere sq 0.3": lambda: (_scaled_sphere(64, True), SQ, 0.3),
    "64 cut sphere sq": lambda: (_scaled_sphere(64, True, R.CUT_C), SQ, 0.0),
    "64 laced -0.6": lambda: (R.laced_random_field(64, 2025), LIN, -0.6),
    "64 laced sq 0": lambda: (R.laced_random_field(64, 2025), SQ, 0.0),
    "64 bunny zeros": lambda: (R.signed_zero_field(SR.bunny64()), SQ, 0.0),
    "96 sphere -1.7": lambda: (_scaled_sphere(96), LIN, -1.7),
    "96 sphere sq 0": lambda: (_scaled_sphere(96, True), SQ, 0.0),
    "96 sphere inf": lambda: (R.signed_zero_field(_sphere96(), inf=True), LIN, 0.0),
}


@pytest.fixture(scope="module")
def refs():
    """the restatement, once per case and shared by every test: name -> (field, transform, iso, cells, {iterations: xyz}, normals, quads)"""
    cache = {}

    def get(name):
        if name not in cache:
            field, transform, iso = CASES[name]()
            cells, xyz, nrm, quads = R.isonets_numpy(field, transform, iso, every=ITERS)
            for a in (field, cells, nrm, quads, *xyz.values()):
                a.setflags(write=False)
            cache[name] = (field, transform, iso, cells, xyz, nrm, quads)
        return cache[name]
    return get


def _dev(engine, field):
    return engine.to_device(np.ascontiguousarray(field).reshape(-1), np.float32)


def _numpy(cells, xyz, nrm, quads):
    return (cells.cpu().numpy().view(np.uint64), xyz.cpu().numpy(), None if nrm is None else nrm.cpu().numpy(), quads.cpu().numpy().view(np.uint32))


def _compare(got, cells, xyz, nrm, quads, tag):
    gc, gx, gn, gq = got
    assert gc.shape == cells.shape and gq.shape == quads.shape, (tag, gc.shape, gq.shape, cells.shape, quads.shape)
    assert np.array_equal(gc, cells), (tag, "records", int(np.count_nonzero(gc != cells)))
    assert np.array_equal(gq, quads), (tag, "quads", int(np.count_nonzero(gq != quads)))
    assert np.array_equal(gx.view(np.uint32), xyz.view(np.uint32)), (tag, "positions", int(np.count_nonzero(gx.view(np.uint32) != xyz.view(np.uint32))))
    if nrm is not None:
        assert np.array_equal(gn.view(np.uint32), nrm.view(np.uint32)), (tag, "normals", int(np.count_nonzero(gn.view(np.uint32) != nrm.view(np.uint32))))


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_the_restatement_bit_for_bit(engine, refs, name, algo):
    field, transform, iso, cells, xyz, nrm, quads = refs(name)
    n = field.shape[0]
    fr = _unit_frame(n)
    d = _dev(engine, field)
    assert engine.ctx.isonets(fr, d.data_ptr(), transform, iso, 0, False, algo) == (len(cells), len(quads))
    assert engine.ctx.isonets_result()[2] == 0                          # no normals asked for
    for it in ITERS:
        _compare(_numpy(*engine.iso_nets(fr, d, iso, transform, it, True, algo)), cells, xyz[it], nrm, quads, (name, algo, it))


def test_degenerate_fields_give_the_bytes_of_the_bit_grid_nets(engine):
    for vox, inf in ((SR.bunny64(), False), (SR.checkerboard(32), True), (SR.sphere(32), False)):
        n = vox.shape[0]
        fr = _unit_frame(n)
        g = engine.to_device(bool_to_words(vox), np.uint32)
        d = _dev(engine, R.signed_zero_field(vox, inf))
        for algo in ALGOS:
            bit = engine.surface_nets(fr, g, 8, algo)
            got = engine.iso_nets(fr, d, 0.0, SQ, 8, False, algo)
            assert torch.equal(bit[0], got[0]) and torch.equal(bit[2], got[3])
            assert torch.equal(bit[1].view(torch.int32), got[1].view(torch.int32))


def test_exact_sdf_on_the_device_names_the_grid_it_came_from(engine):
    n = 64
    vox = SR.sphere(n, (31.3, 32.1, 30.7), 20.0 ** 2)
    fr = _unit_frame(n)
    g = engine.to_device(bool_to_words(vox), np.uint32)
    sdf = engine.edt_sdf(fr, g)
    for algo in ALGOS:
        bit = engine.surface_nets(fr, g, 0, algo)
        got = engine.iso_nets(fr, sdf, 0.0, SQ, 0, True, algo)
        assert torch.equal(bit[0], got[0]) and torch.equal(bit[2], got[3])
    cells, xyz, nrm, quads = R.isonets_numpy(sdf.cpu().numpy().reshape(n, n, n), SQ, 0.0)
    _compare(_numpy(*got), cells, xyz, nrm, quads, "edt sdf")


def test_mesh_distance_of_d20_on_the_device_then_iso_nets(engine):
    n = 32
    xyz, tri, vs, origin, sign, field = mesh_case("d20.obj")
    fr = Frame.make(n, float(vs), origin)
    dx, dt = engine.mesh_to_device(xyz, tri)
    s = engine.to_device(bool_to_words(sign), np.uint32)
    dist = engine.mesh_distance(fr, dx, dt, 4, sign_words=s)
    assert np.array_equal(dist.cpu().numpy().view(np.uint32), field.reshape(-1).view(np.uint32))
    for iso_voxels in (0.0, -1.0):
        level = float(np.float32(np.float32(iso_voxels) * vs))
        cells, pos, nrm, quads = R.isonets_numpy(field, SQ, level, 8)
        for algo in ALGOS:
            _compare(_numpy(*engine.iso_nets(fr, dist, level, SQ, 8, True, algo)), cells, pos, nrm, quads, (iso_voxels, algo))


@pytest.mark.parametrize("algo", ALGOS)
def test_lone_voxels_at_1024_by_hand(engine, algo):
    n = 1024
    fr = _unit_frame(n)
    voxels = [(x, y, z) for z in (0, n - 1) for y in (0, n - 1) for x in (0, n - 1)] + [(500, 600, 700)]
    d = torch.full((n ** 3,), -3.0, dtype=torch.float32, device=engine.device)        # 4 GiB, filled on the device
    for x, y, z in voxels:
        d[x + n * (y + n * z)] = 1.0
    ec, ex, en, eq = R.sparse_expectation(n, voxels)
    n1 = n + 1
    assert int(ec[0]) == 0x80 << 40 and int(ec[-1]) == (n1 ** 3 - 1) | (0x01 << 40)   # by hand again: the first and the last record
    assert len(ec) == 72 and len(eq) == 54
    _compare(_numpy(*engine.iso_nets(fr, d, 0.0, LIN, 0, True, algo)), ec, ex, en, eq, algo)
    del d
    engine.ctx.release()                                               # NAIVE: the index volume is 4 (n+1)^3 bytes
    torch.cuda.empty_cache()


def test_two_runs_and_the_two_algos_give_the_same_bytes(engine, refs):
    field, transform, iso = refs("64 laced sq 0")[:3]
    fr = _unit_frame(64)
    d = _dev(engine, field)
    runs = [engine.iso_nets(fr, d, iso, transform, 8, True, algo) for algo in (ALGO_TILED, ALGO_TILED, ALGO_NAIVE, ALGO_NAIVE)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _refused(code, fn):
    with pytest.raises(capi.VPError) as e:
        fn()
    assert e.value.code == code, (e.value.code, code, str(e.value))


def _result(engine):
    """the last build, read through vp_isonets_result"""
    dc, dx, dn, dq, nv, nq = engine.ctx.isonets_result()
    cells, xyz, quads = np.empty(nv, np.uint64), np.empty((nv, 3), np.float32), np.empty((nq, 4), np.uint32)
    nrm = np.empty((nv, 3), np.float32) if dn else None
    for host, ptr in ((cells, dc), (xyz, dx), (nrm, dn), (quads, dq)):
        if host is not None and host.size:
            engine.ctx.download(host, ptr)
    return cells, xyz, nrm, quads


def test_refusals_leave_the_previous_result_readable(engine, refs):
    field, transform, iso, cells, xyz, nrm, quads = refs("32 sphere 0.3")
    fr = _unit_frame(32)
    ctx = engine.ctx
    d = _dev(engine, field)
    assert ctx.isonets(fr, d.data_ptr(), transform, iso, 1, True, ALGO_TILED) == (len(cells), len(quads))
    slab = Frame.make(32, 1.0 / 32, np.zeros(3, np.float32), 0, 16)
    large = Frame.make(2048, 1.0 / 2048, np.zeros(3, np.float32))
    for bad in (slab, large):
        _refused(UNSUPPORTED, lambda: ctx.isonets(bad, d.data_ptr(), transform, iso, 1, True, ALGO_TILED))
    _refused(INVALID, lambda: ctx.isonets(fr, 0, transform, iso, 1, True, ALGO_TILED))
    _refused(INVALID, lambda: ctx.isonets(fr, d.data_ptr() + 4, transform, iso, 1, True, ALGO_TILED))
    _refused(INVALID, lambda: ctx.isonets(fr, d.data_ptr(), 2, iso, 1, True, ALGO_TILED))
    _refused(INVALID, lambda: ctx.isonets(fr, d.data_ptr(), -1, iso, 1, True, ALGO_TILED))
    for algo in (0, 3):
        _refused(INVALID, lambda: ctx.isonets(fr, d.data_ptr(), transform, iso, 1, True, algo))
    for level in (float("nan"), float("inf"), -float("inf")):
        _refused(INVALID, lambda: ctx.isonets(fr, d.data_ptr(), transform, level, 1, True, ALGO_TILED))
    _refused(INVALID, lambda: ctx.isonets(fr, d.data_ptr(), transform, iso, 65, True, ALGO_TILED))
    L = capi.lib()
    assert L.vp_isonets(None, ctypes.byref(fr), d.data_ptr(), transform, iso, 1, 1, ALGO_TILED, None, None) == INVALID
    assert L.vp_isonets(ctx._h, None, d.data_ptr(), transform, iso, 1, 1, ALGO_TILED, None, None) == INVALID
    _compare(_result(engine), cells, xyz[1], nrm, quads, "after the refusals")
    # the host form: the same refusals, a short capacity, host outputs and counts untouched
    nv, nq = ctypes.c_uint64(77), ctypes.c_uint64(78)
    V, Q = len(cells), len(quads)
    hc, hx, hq = np.full(V, 7, np.uint64), np.full((V, 3), 7, np.float32), np.full((Q, 4), 7, np.uint32)
    flat = np.ascontiguousarray(field).reshape(-1)

    def host(frame, it=1, vc=V, qc=Q, tr=transform, level=iso):
        return L.vp_isonets_host(ctx._h, ctypes.byref(frame), flat.ctypes.data, tr, level, it, ALGO_TILED, hc.ctypes.data, hx.ctypes.data, None,
                                 hq.ctypes.data, vc, qc, ctypes.byref(nv), ctypes.byref(nq))
    assert host(slab) == UNSUPPORTED and host(large) == UNSUPPORTED and host(fr, it=65) == INVALID and host(fr, tr=7) == INVALID
    assert host(fr, level=float("nan")) == INVALID
    assert host(fr, vc=V - 1) == INVALID and host(fr, qc=Q - 1) == INVALID
    assert (hc == 7).all() and (hx == 7).all() and (hq == 7).all() and (nv.value, nq.value) == (77, 78)
    assert host(fr) == 0 and (nv.value, nq.value) == (V, Q)
    _compare((hc, hx, None, hq), cells, xyz[1], None, quads, "host form, no normals")


def test_a_pending_surfnets_count_is_dropped(engine, refs):
    field, transform, iso, cells, _, _, quads = refs("32 sphere 0")
    fr = _unit_frame(32)
    ctx = engine.ctx
    vox = SR.sphere(32)
    g = engine.to_device(bool_to_words(vox), np.uint32)
    d = _dev(engine, field)
    for algo in ALGOS:
        V, Q = ctx.surfnets_count(fr, g.data_ptr(), algo)
        assert (V, Q) == (len(cells), len(quads))
        sent = 0x5A5A5A5A
        dc = torch.full((2 * V,), sent, dtype=torch.int32, device=engine.device)
        dx = torch.full((3 * V,), sent, dtype=torch.int32, device=engine.device)
        dq = torch.full((4 * Q,), sent, dtype=torch.int32, device=engine.device)
        ctx.isonets(fr, d.data_ptr(), transform, 0.3, 0, False, algo)
        _refused(INVALID, lambda: ctx.surfnets(fr, g.data_ptr(), algo, 1, dc.data_ptr(), dx.data_ptr(), dq.data_ptr(), V, Q))
        engine.sync()
        for t in (dc, dx, dq):
            assert bool((t == sent).all())
        assert ctx.surfnets_count(fr, g.data_ptr(), algo) == (V, Q)   # a fresh count serves again
        ctx.surfnets(fr, g.data_ptr(), algo, 1, dc.data_ptr(), dx.data_ptr(), dq.data_ptr(), V, Q)
        assert np.array_equal(dc.cpu().numpy().view(np.uint64), SR.surfnets_bool(vox, 0)[0])


def test_release_and_an_empty_field_give_no_mesh(engine, refs):
    field, transform, iso, cells, _, _, quads = refs("32 sphere 0")
    fr = _unit_frame(32)
    ctx = engine.ctx
    d = _dev(engine, field)
    assert ctx.isonets(fr, d.data_ptr(), transform, iso, 0, True, ALGO_TILED) == (len(cells), len(quads))
    res = ctx.isonets_result()
    assert all(res[:4]) and res[4:] == (len(cells), len(quads))
    ctx.release()
    assert ctx.isonets_result() == (0, 0, 0, 0, 0, 0)
    L = capi.lib()
    assert L.vp_isonets_result(ctx._h, None, None, None, None, None, None) == 0       # any argument may be NULL
    empty = torch.full((32 ** 3,), -1.0, dtype=torch.float32, device=engine.device)
    for algo in ALGOS:
        assert ctx.isonets(fr, empty.data_ptr(), LIN, 0.0, 8, True, algo) == (0, 0)
        assert ctx.isonets_result() == (0, 0, 0, 0, 0, 0)
        c, x, m, q = engine.iso_nets(fr, empty, 0.0, LIN, 8, True, algo)
        assert c.numel() == 0 and tuple(x.shape) == (0, 3) and tuple(m.shape) == (0, 3) and tuple(q.shape) == (0, 4)


def test_host_form_engine_and_timing_keys(engine, refs):
    field, transform, iso, cells, xyz, nrm, quads = refs("96 sphere -1.7")
    fr = _unit_frame(96)
    ctx = engine.ctx
    flat = np.ascontiguousarray(field).reshape(-1)
    assert ctx.isonets_host(fr, flat, transform, iso, counts_only=True) == (len(cells), len(quads))
    for algo in ALGOS:
        _compare(ctx.isonets_host(fr, flat, transform, iso, 8, True, algo), cells, xyz[8], nrm, quads, ("host form", algo))
    d = _dev(engine, field)
    for algo, keys in ((ALGO_TILED, {"sn_cells", "sn_scan", "sn_verts", "sn_quads", "sn_relax"}),
                       (ALGO_NAIVE, {"sn_cells_naive", "sn_scan", "sn_verts_naive", "sn_quads_naive", "sn_relax_naive"})):
        try:
            ctx.prof_reset()
            ctx.prof_enable(True)
            engine.iso_nets(fr, d, iso, transform, 3, True, algo)
            ctx.prof_enable(False)
            p = ctx.prof()
        finally:
            ctx.prof_enable(False); ctx.prof_reset()
        assert set(p) == keys, p
        two = {"sn_cells", "sn_verts", "sn_cells_naive", "sn_verts_naive"}          # classification + count, records + placement
        relax = "sn_relax" if algo == ALGO_TILED else "sn_relax_naive"
        assert all(v["launches"] == (3 if k == relax else 2 if k in two else 1) and v["ms"] > 0.0 for k, v in p.items()), p


@pytest.mark.parametrize("flags,level", [(["--mesh-sdf", "3"], "0.37:8"), (["--exact-sdf"], "-0.5"), ([], "0:1")])
def test_cli_files_of_host_and_device_are_byte_identical_at_64(tmp_path, flags, level):
    cli = build.build_cli()
    files = {}
    for t, name in (("0", "sequential"), ("2", "tiled"), ("1", "naive")):
        d = tmp_path / t
        d.mkdir()
        p = subprocess.run([cli, M.asset("bunny.obj"), "-n", "64", "-t", t, "-s", "-e", "--iso-nets", level] + flags, capture_output=True,
                           text=True, timeout=600, cwd=str(d))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        files[t] = open(str(d / "out" / ("iso_" + name + "_out.obj")), "rb").read()
    assert len(files["0"]) > 100000 and files["0"] == files["2"] == files["1"]


def test_cpp_api_host_and_device_agree(check_exe, tmp_path, refs):  # noqa: F811
    for name in ("64 laced sq 0", "96 sphere -1.7", "32 cut sphere"):
        field, transform, iso, cells, xyz, nrm, quads = refs(name)
        lines, (hc, hx, hn, hq, _) = run_check(check_exe, tmp_path, field, transform, iso, 8, gpu=True)
        assert lines["host"] == lines["tiled"] == lines["naive"], (name, lines)
        _compare((hc, hx, hn, hq), cells, xyz[8], nrm, quads, name)
