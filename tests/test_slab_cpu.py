"""Z-slab pipeline (cuda_mesh_voxelization_amd/slab.py) under gloo with world_size 2 and 4 on CPU:
the concatenated slabs must be bit-identical to the single-domain oracle.  The compute backend is the
numpy stand-in of tests/slab_cpu_backend.py; what is under test is the halo plan and the exchange."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, n, asset, op, outdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cuda_mesh_voxelization_amd import mesh as M
        from cuda_mesh_voxelization_amd.capi import Frame
        from cuda_mesh_voxelization_amd.slab import SlabPipeline
        from slab_cpu_backend import CpuSlabBackend
        meshes = [M.import_mesh(M.asset(a)) for a in asset]
        origin, vs = M.frame([m[0] for m in meshes], n)
        fr = Frame.make(n, vs, origin)
        pipe = SlabPipeline(CpuSlabBackend(meshes[0]), fr, rank, world, dist)
        pipe.voxelize(None, None)
        if len(meshes) > 1:
            other = pipe.be.empty_u32(pipe.frame.words)
            pipe.be.mesh_host = meshes[1]
            pipe.voxelize(None, None, out=other)
            pipe.csg(other, op)
        sdf = pipe.jfa()
        np.save(os.path.join(outdir, "words_%d.npy" % rank), pipe.words.numpy().view(np.uint32))
        np.save(os.path.join(outdir, "sdf_%d.npy" % rank), sdf.numpy())
        np.save(os.path.join(outdir, "rx_%d.npy" % rank), np.array([pipe.bytes_received]))
    finally:
        dist.destroy_process_group()


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world,n,assets,op", [(2, 32, ["sphere.obj"], 0), (4, 32, ["torus.obj"], 0),
                                               (2, 64, ["bimba.obj", "bunny.obj"], 1)])
def test_slab_pipeline_matches_single_domain_oracle(tmp_path, world, n, assets, op):
    sys.path.insert(0, ROOT)
    from cuda_mesh_voxelization_amd import mesh as M
    from oracle import oracle as O
    mp.spawn(_worker, args=(world, _free_port(), n, assets, op, str(tmp_path)), nprocs=world, join=True)
    meshes = [M.import_mesh(M.asset(a)) for a in assets]
    origin, vs = M.frame([m[0] for m in meshes], n)
    words = O.voxelize(meshes[0][0], meshes[0][1], n, vs, origin)
    if len(meshes) > 1:
        O.csg(words, O.voxelize(meshes[1][0], meshes[1][1], n, vs, origin), op)
    exp = O.jfa(words, n, vs, origin)
    got_w = np.concatenate([np.load(tmp_path / ("words_%d.npy" % r)) for r in range(world)])
    got_s = np.concatenate([np.load(tmp_path / ("sdf_%d.npy" % r)) for r in range(world)])
    assert np.array_equal(got_w, words)
    assert np.array_equal(got_s.view(np.uint32), exp.view(np.uint32))
    rx = [int(np.load(tmp_path / ("rx_%d.npy" % r))[0]) for r in range(world)]
    assert all(b > 0 for b in rx)


def test_halo_plan_covers_exactly_what_a_pass_reads():
    sys.path.insert(0, ROOT)
    from cuda_mesh_voxelization_amd.slab import halo_plan, slab_range
    for n, world in ((64, 2), (64, 4), (64, 8), (512, 8), (1024, 4)):
        nz = n // world
        k = n // 2
        while k >= 1:
            plan = halo_plan(n, world, k)
            for dst in range(world):
                z0, z1 = slab_range(n, dst, world)
                need = set()
                for z in range(z0, z1):
                    for zz in (z - k, z + k):
                        if 0 <= zz < n and not (z0 <= zz < z1):
                            need.add(zz)
                have = set()
                for s, t, side, g0, g1 in plan:
                    if t != dst:
                        continue
                    assert g0 // nz == s and (g1 - 1) // nz == s          # one owner per piece
                    have.update(range(g0, g1))
                assert have == need, (n, world, k, dst)
            k //= 2
    with pytest.raises(ValueError):
        slab_range(64, 0, 16)          # 4 planes per slab: not a multiple of the 8-row tile


def _ghost_worker(rank, world, port, n, asset, outdir, poison=None):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cuda_mesh_voxelization_amd import mesh as M
        from cuda_mesh_voxelization_amd.capi import Frame
        from cuda_mesh_voxelization_amd.slab import GhostSlabPipeline
        from slab_cpu_backend import CpuSlabBackend
        mesh = M.import_mesh(M.asset(asset))
        origin, vs = M.frame([mesh[0]], n)
        pipe = GhostSlabPipeline(CpuSlabBackend(mesh, poison=poison), Frame.make(n, vs, origin), rank, world)
        pipe.voxelize(None, None)
        sdf = pipe.jfa()
        dist.barrier()
        np.save(os.path.join(outdir, "sdf_%d.npy" % rank), sdf.numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,asset", [(2, 32, "sphere.obj"), (4, 32, "torus.obj")])
def test_ghost_slab_pipeline_matches_single_domain_oracle(tmp_path, world, n, asset):
    sys.path.insert(0, ROOT)
    from cuda_mesh_voxelization_amd import mesh as M
    from oracle import oracle as O
    mp.spawn(_ghost_worker, args=(world, _free_port(), n, asset, str(tmp_path)), nprocs=world, join=True)
    xyz, tri = M.import_mesh(M.asset(asset))
    origin, vs = M.frame([xyz], n)
    exp = O.jfa(O.voxelize(xyz, tri, n, vs, origin), n, vs, origin)
    got = np.concatenate([np.load(tmp_path / ("sdf_%d.npy" % r)) for r in range(world)])
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))


@pytest.mark.parametrize("poison", [0, 777, -1])
def test_ghost_ignores_unproduced_planes(tmp_path, poison):
    """the ghost regions are rounded outwards to the 8-plane tile and the excess planes of a pass read planes the pass
    before it never produced.  Whatever those planes hold -- voxel 0 as a seed, voxel 777, "none" -- the slabs must not change.
    (The first two passes run over the whole grid, so the windows are fully written once; what the rounding planes of the LATER passes
    read is then the output of an earlier pass on the same buffer or this fill.)"""
    sys.path.insert(0, ROOT)
    from cuda_mesh_voxelization_amd import mesh as M
    from oracle import oracle as O
    world, n, asset = 4, 64, "torus.obj"
    mp.spawn(_ghost_worker, args=(world, _free_port(), n, asset, str(tmp_path), poison), nprocs=world, join=True)
    xyz, tri = M.import_mesh(M.asset(asset))
    origin, vs = M.frame([xyz], n)
    exp = O.jfa(O.voxelize(xyz, tri, n, vs, origin), n, vs, origin)
    got = np.concatenate([np.load(tmp_path / ("sdf_%d.npy" % r)) for r in range(world)])
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))


def test_ghost_regions_feed_each_other():
    """Each pass must produce (at least) the slab widened by the reach of all later passes, and what it
    reads there must have been produced by the previous pass.  (Regions are rounded outwards to the
    8-plane tile; the rounding extras may read stale planes -- their values are never consumed.)"""
    sys.path.insert(0, ROOT)
    from cuda_mesh_voxelization_amd.slab import ghost_regions, slab_range
    for n, world in ((64, 2), (64, 8), (512, 8), (512, 4), (1024, 4), (1024, 8)):
        for rank in range(world):
            regs = ghost_regions(n, rank, world)
            z0, z1 = slab_range(n, rank, world)
            assert regs[-1][1:] == (z0, z1) and regs[-1][0] == 1          # last pass = bare slab
            ks = [k for k, _, _ in regs]
            prev_valid = (0, n)                                             # init covers the whole grid
            for i, (k, b0, b1) in enumerate(regs):
                g = sum(ks[i + 1:])
                u0, u1 = max(0, z0 - g), min(n, z1 + g)                    # planes whose values matter
                assert b0 % 8 == 0 and b1 % 8 == 0 and 0 <= b0 <= u0 < u1 <= b1 <= n
                r0, r1 = max(0, u0 - k), min(n, u1 + k)                    # what those planes read
                assert prev_valid[0] <= r0 and r1 <= prev_valid[1], (n, world, rank, k)
                prev_valid = (u0, u1)


def _hybrid_worker(rank, world, port, n, asset, outdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cuda_mesh_voxelization_amd import mesh as M
        from cuda_mesh_voxelization_amd.capi import Frame
        from cuda_mesh_voxelization_amd.slab import HybridSlabPipeline
        from slab_cpu_backend import CpuSlabBackend
        mesh = M.import_mesh(M.asset(asset))
        origin, vs = M.frame([mesh[0]], n)
        pipe = HybridSlabPipeline(CpuSlabBackend(mesh), Frame.make(n, vs, origin), rank, world, dist)
        pipe.voxelize(None, None)
        sdf = pipe.jfa()
        dist.barrier()
        np.save(os.path.join(outdir, "sdf_%d.npy" % rank), sdf.numpy())
        np.save(os.path.join(outdir, "rep_%d.npy" % rank), np.array([pipe.bytes_received, pipe.planes_computed, pipe.window[0], pipe.window[1]]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,asset", [(2, 32, "sphere.obj"), (4, 32, "torus.obj"), (2, 64, "bunny.obj"), (4, 64, "torus.obj")])
def test_hybrid_slab_pipeline_matches_single_domain_oracle(tmp_path, world, n, asset):
    """Ghost planes for the wide passes, p2p halos (sent a pass ahead, under the interior planes) for the narrow ones, id buffers
    that hold only the planes the rank touches: the numpy backend asserts that no pass reads outside that window."""
    sys.path.insert(0, ROOT)
    from cuda_mesh_voxelization_amd import mesh as M
    from cuda_mesh_voxelization_amd.slab import hybrid_plan
    from oracle import oracle as O
    mp.spawn(_hybrid_worker, args=(world, _free_port(), n, asset, str(tmp_path)), nprocs=world, join=True)
    xyz, tri = M.import_mesh(M.asset(asset))
    origin, vs = M.frame([xyz], n)
    exp = O.jfa(O.voxelize(xyz, tri, n, vs, origin), n, vs, origin)
    got = np.concatenate([np.load(tmp_path / ("sdf_%d.npy" % r)) for r in range(world)])
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    nz = n // world
    for r in range(world):
        rx, planes, lo, hi = [int(v) for v in np.load(tmp_path / ("rep_%d.npy" % r))]
        wide, narrow = hybrid_plan(n, r, world)
        sides = (r > 0) + (r < world - 1)
        assert rx == sides * sum(narrow) * n * n * 4                  # k planes per side and narrow pass, nothing else
        assert planes == sum(b1 - b0 for _, b0, b1 in wide) + nz * len(narrow)
        assert 0 <= lo <= r * nz and (r + 1) * nz <= hi <= n


def test_hybrid_plan_feeds_itself():
    """Wide regions: each produces the slab widened by the reach of the later WIDE passes and reads only what the previous one
    produced; the last wide pass leaves exactly the slab; narrow steps are the k <= nz/2 and end with 1; plane-passes per rank lie
    between the ideal n/G per pass and the ghost-plane count."""
    sys.path.insert(0, ROOT)
    from cuda_mesh_voxelization_amd.slab import ghost_regions, hybrid_plan, slab_range
    for n, world in ((64, 2), (64, 8), (512, 4), (512, 8), (1024, 4), (1024, 8), (2048, 8), (96, 2), (96, 4)):
        nz = n // world
        for rank in range(world):
            z0, z1 = slab_range(n, rank, world)
            wide, narrow = hybrid_plan(n, rank, world)
            ks = [k for k, _, _ in wide] + narrow
            assert ks == sorted(ks, reverse=True) and ks[0] == n // 2 and ks[-1] == 1 and len(ks) == len(set(ks))
            assert all(k > nz // 2 for k, _, _ in wide) and all(k <= nz // 2 for k in narrow) and narrow
            assert wide[-1][1:] == (z0, z1)
            valid = (0, n)
            for i, (k, b0, b1) in enumerate(wide):
                g = sum(kk for kk, _, _ in wide[i + 1:])
                u0, u1 = max(0, z0 - g), min(n, z1 + g)
                assert b0 % 8 == 0 and b1 % 8 == 0 and 0 <= b0 <= u0 < u1 <= b1 <= n
                assert valid[0] <= max(0, u0 - k) and min(n, u1 + k) <= valid[1]
                valid = (u0, u1)
            work = sum(b1 - b0 for _, b0, b1 in wide) + nz * len(narrow)
            ghost = sum(b1 - b0 for _, b0, b1 in ghost_regions(n, rank, world))
            assert nz * len(ks) <= work <= ghost
    wide, narrow = hybrid_plan(64, 0, 1)
    assert narrow == [] and [r[1:] for r in wide] == [(0, 64)] * 6


# ---------------------------------------------------------------------------------------------- transposed pipeline
def _transpose_worker(rank, world, port, n, asset, outdir, poison=None, exchange="a2a"):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cuda_mesh_voxelization_amd import mesh as M
        from cuda_mesh_voxelization_amd.capi import Frame
        from cuda_mesh_voxelization_amd.slab import TransposeSlabPipeline
        from slab_cpu_backend import CpuSlabBackend
        mesh = M.import_mesh(M.asset(asset))
        origin, vs = M.frame([mesh[0]], n)
        pipe = TransposeSlabPipeline(CpuSlabBackend(mesh, poison=poison), Frame.make(n, vs, origin), rank, world, dist, exchange=exchange)
        pipe.voxelize(None, None)
        sdf = pipe.jfa()
        dist.barrier()
        np.save(os.path.join(outdir, "sdf_%d.npy" % rank), sdf.numpy())
        np.save(os.path.join(outdir, "rep_%d.npy" % rank), np.array([pipe.bytes_received, pipe.planes_computed if pipe.fallback is None else -1]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n,asset,poison,exchange", [(2, 32, "sphere.obj", None, "a2a"), (4, 64, "torus.obj", None, "a2a"), (2, 64, "bunny.obj", 777, "a2a"),
                                                           (4, 64, "d20.obj", 0, "a2a"), (2, 96, "torus.obj", None, "a2a"),
                                                           (4, 64, "torus.obj", 777, "p2p"), (2, 32, "sphere.obj", None, "p2p")])
def test_transpose_pipeline_matches_single_domain_oracle(tmp_path, world, n, asset, poison, exchange):
    """Planes dealt cyclically for the passes whose step is a multiple of the rank count (the numpy backend asserts that such a pass
    reads nothing but planes of its own rank), ONE all_to_all_single over gloo, the weave into consecutive planes, the remaining passes on
    the widened slab (the backend asserts that no pass reads outside the window).  exchange "p2p": the same planes as one batch of isend /
    irecv, each received straight into its place in the slab window (no send buffer, no staging buffer, no weave).  `poison`: what the planes of a fresh window that
    nobody ever produces hold -- the result must not depend on it.  n = 96: the step sequence 48, 24, 12, 6, 3, 1 leaves the multiples
    of two after four passes."""
    sys.path.insert(0, ROOT)
    from cuda_mesh_voxelization_amd import mesh as M
    from cuda_mesh_voxelization_amd.slab import transpose_plan
    from oracle import oracle as O
    mp.spawn(_transpose_worker, args=(world, _free_port(), n, asset, str(tmp_path), poison, exchange), nprocs=world, join=True)
    xyz, tri = M.import_mesh(M.asset(asset))
    origin, vs = M.frame([xyz], n)
    exp = O.jfa(O.voxelize(xyz, tri, n, vs, origin), n, vs, origin)
    got = np.concatenate([np.load(tmp_path / ("sdf_%d.npy" % r)) for r in range(world)])
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    for r in range(world):
        rx, planes = [int(v) for v in np.load(tmp_path / ("rep_%d.npy" % r))]
        plan = transpose_plan(n, r, world, 0)
        t0, t1 = plan["recv"]
        assert rx == (world - 1) * ((t1 - t0) // world) * n * n * 4          # one exchange: the planes of the widened slab the others hold
        assert planes == (n // world) * len(plan["cyclic"]) + sum(b1 - b0 for _, b0, b1 in plan["regions"])


def test_transpose_plan_feeds_itself():
    """Cyclic steps: multiples of the rank count, from n/2 on, at least two.  Slab regions: as in the ghost plan, each produces the slab
    widened by the reach of the later steps and reads only what the all-to-all delivered or the region before it produced; the window
    holds everything any region reads.  Plane-passes per rank stay within 1.25 x the ideal n / world per pass on power-of-two grids."""
    sys.path.insert(0, ROOT)
    from cuda_mesh_voxelization_amd.slab import cyclic_passes, ghost_regions, slab_range, transpose_plan
    for n, world in ((512, 2), (512, 4), (512, 8), (1024, 2), (1024, 4), (1024, 8), (2048, 8), (2048, 4), (96, 2), (1152, 8), (1280, 8), (288, 4), (256, 16)):
        for rank in range(world):
            plan = transpose_plan(n, rank, world)
            z0, z1 = slab_range(n, rank, world)
            ks = plan["cyclic"] + [k for k, _, _ in plan["regions"]]
            assert ks == [k for k, _, _ in ghost_regions(n, rank, world)] and len(plan["cyclic"]) == cyclic_passes(n, world) >= 2
            assert all(k % world == 0 and n % k == 0 for k in plan["cyclic"]) and plan["regions"][0][0] % world != 0
            t0, t1 = plan["recv"]
            lo, hi = plan["window"]
            g = sum(k for k, _, _ in plan["regions"])
            assert t0 % world == 0 and t1 % world == 0 and 0 <= lo <= t0 <= max(0, z0 - g) and min(n, z1 + g) <= t1 <= hi <= n
            valid = (t0, t1)
            for i, (k, b0, b1) in enumerate(plan["regions"]):
                gi = sum(kk for kk, _, _ in plan["regions"][i + 1:])
                u0, u1 = max(0, z0 - gi), min(n, z1 + gi)                 # planes whose values matter
                assert b0 % 8 == 0 and b1 % 8 == 0 and lo <= b0 <= u0 < u1 <= b1 <= hi
                assert valid[0] <= max(0, u0 - k) and min(n, u1 + k) <= valid[1], (n, world, rank, k)
                assert lo <= max(0, b0 - k) and min(n, b1 + k) <= hi        # what the rounded region reads lies inside the window
                valid = (u0, u1)
            assert plan["regions"][-1] == (1, z0, z1)
            work = (n // world) * len(plan["cyclic"]) + sum(b1 - b0 for _, b0, b1 in plan["regions"])
            if n & (n - 1) == 0 and n // world >= 64:
                assert work <= 1.25 * (n // world) * len(ks), (n, world, work)
    # below the tile kernels, one rank, slabs that are not a multiple of 8 planes, a rank count that is not a power of two
    # (slabs of a multiple of 8 planes make n/4 a multiple of the rank count: where the split is legal at all there are two cyclic passes)
    assert all(transpose_plan(*a) is None for a in ((64, 0, 2), (512, 0, 1), (96, 0, 8), (384, 0, 3)))
    assert cyclic_passes(96, 4) == 3 and cyclic_passes(128, 8) == 4 and cyclic_passes(1024, 8) == 7 and cyclic_passes(160, 4) == 3


def test_plans_equal_the_recorded_ones():
    """The property tests above prove that the plans are VALID; this one that they are the SAME plans: tests/golden/slab_plans.json holds what
    slab.py planned before the planner was shared (ghost_regions, hybrid_plan, the hybrid window with and without the mask start,
    transpose_plan, cyclic_passes and halo_plan of every step) for every split of n in 96, 128, 160, 256, 1152 over 1, 2, 3, 4, 8 ranks that
    slab_range accepts.  A region one tile wider than needed would pass the property tests and cost time."""
    import importlib.util
    import json
    sys.path.insert(0, ROOT)
    from cuda_mesh_voxelization_amd import slab
    spec = importlib.util.spec_from_file_location("make_slab_plans", os.path.join(ROOT, "tests", "golden", "make_slab_plans.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    with open(os.path.join(ROOT, "tests", "golden", "slab_plans.json")) as f:
        want = json.load(f)
    got = G.record(slab)
    assert sorted(got) == sorted(want) and len(got) == 20 and sum(len(v["ranks"]) for v in got.values()) == 65
    for split in want:
        n, world = [int(v) for v in split.split("/")]
        assert got[split]["halo"] == want[split]["halo"], split
        for r in range(world):
            for what in want[split]["ranks"][r]:
                assert got[split]["ranks"][r][what] == want[split]["ranks"][r][what], (split, r, what)
            lo, hi = slab.hybrid_window(n, r, world, False)                      # the planes a rank holds contain its slab
            assert 0 <= lo <= r * (n // world) and (r + 1) * (n // world) <= hi <= n
    assert slab.steps(160) == [80, 40, 20, 10, 5, 2, 1] and slab.steps(1) == []
