"""Frames in which float32 arithmetic rounds, and inputs for them: shared by test_float_frames_gpu.py and test_float_frames_cpu.py.

The bit-for-bit promises (solid voxelizer and JFA against the sequential path, the mesh distance as a minimum over a set) hold for every
frame (n, voxel size, origin).  In a dyadic frame near the origin every position, difference, square and sum is exact, so a reassociated
sum or a table built from a mathematically equal expression cannot change a bit there.  The frames here are not of that kind:

GRID_FRAMES  voxel size 0.037 (not dyadic) at origins of growing size.  granularity() = ulp(|o| + n vs) / vs per axis, in voxels: the
             spacing of the float32 numbers where the voxel positions lie.  `near` < 1e-4, `far` between 0.01 and 0.5, `collapsed` > 1
             on x (neighbouring columns share one position), `far_x1000` = `far` with everything times 1000 (an absolute epsilon that
             suits `far` is a thousand times too small there).  check_band() asserts what a frame's name claims.
mesh_level   the frame of a TRANSLATED mesh, as a georeferenced file gives it: xyz = float32(xyz0 + T), T = (1, -0.83, 0.61) d vs0 2^23,
             so that one ulp of the largest coordinate is about d voxels; LEVELS = d of 2^-10, 2^-4, 0.5 and 2.  "x1000" is the level 2^-4
             with every coordinate times 1000 before the one rounding.
grids        seeded bit-packed occupancies: noise (p = 0.5), sparse (p = 0.004 per voxel), boxes (XORed axis-aligned slabs, bars and boxes:
             equidistant seeds everywhere).
soup         a triangle soup in voxel units (random size classes, slivers, vertices snapped to voxel corners and centres, triangles in
             axis planes, triangles that leave the frame), mapped into the frame in float64 and rounded once.
Everything is computed once per argument tuple and handed out read-only."""
import functools

import numpy as np

F = np.float32

GRID_FRAMES = {
    "near": (F(0.037), (0.25, -1.0, 3.5)),
    "mid": (F(0.037), (811.3, -4099.7, 65.1)),
    "far": (F(0.037), (81100.3, -40990.7, 6500.1)),
    "collapsed": (F(0.037), (600000.3, -150000.7, 40000.1)),
    "far_x1000": (F(37.0), (81100.3e3, -40990.7e3, 6500.1e3)),
}
LEVELS = {"2^-10": 2.0 ** -10, "2^-4": 2.0 ** -4, "0.5": 0.5, "2": 2.0}
DIRECTION = np.array([1.0, -0.83, 0.61])


def grid_frame(name):
    """(vs float32, origin float32[3]) of a named grid frame"""
    vs, o = GRID_FRAMES[name]
    return F(vs), np.array(o, F)


def granularity(n, vs, origin):
    """ulp(|o_axis| + n vs) / vs per axis: the spacing of float32 at the far end of the grid, in voxels"""
    vs, origin = F(vs), np.asarray(origin, F)
    reach = (np.abs(origin.astype(np.float64)) + n * float(vs)).astype(F)
    return np.spacing(reach).astype(np.float64) / float(vs)


def jfa_positions(n, vs, o_axis):
    """the float32 positions of the JFA along one axis, o + (i * vs): what a seed carries and what a voxel measures from"""
    return F(o_axis) + (np.arange(n, dtype=np.int64).astype(F) * F(vs))


def centres(n, vs, o_axis):
    """the float32 voxel centres of the voxelizer and the mesh distance along one axis, o + ((i * vs) + (vs / 2))"""
    return F(o_axis) + ((np.arange(n, dtype=np.int64).astype(F) * F(vs)) + (F(vs) / F(2.0)))


def check_band(name, n):
    """assert that the frame still is what its name says (a later edit cannot quietly make it an exact frame); returns (vs, origin, g)"""
    vs, o = grid_frame(name)
    g = granularity(n, vs, o)
    if name == "near":
        assert (g < 1e-4).all(), (name, n, g)
    elif name == "mid":
        assert (g > 1e-4).all() and (g < 0.05).all(), (name, n, g)
    elif name in ("far", "far_x1000"):
        assert ((g > 0.01) & (g < 0.5)).all(), (name, n, g)
    elif name == "collapsed":
        assert g[0] > 1, (name, n, g)
        assert np.unique(jfa_positions(n, vs, o[0])).size < n and np.unique(centres(n, vs, o[0])).size < n, (name, n)
    else:
        raise KeyError(name)
    # none of them is a frame of exact arithmetic: the positions along x and y are not equally spaced in float32
    for a in range(2):
        steps = np.diff(jfa_positions(n, vs, o[a]).astype(np.float64))
        assert np.unique(steps).size > 1, (name, n, a)
    return vs, o, g


# ---- grids ----------------------------------------------------------------------------------------------------------------
def pack(occ):
    """bool [z, y, x] -> uint32 words, x fastest, bit i of word w = voxel 32 w + i"""
    return np.packbits(np.ascontiguousarray(occ).reshape(-1), bitorder="little").view(np.uint32).copy()


def unpack(words, n, nz=None):
    nz = n if nz is None else nz
    return np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8), bitorder="little")[:nz * n * n].reshape(nz, n, n).astype(bool)


GRID_KINDS = ("noise", "sparse", "boxes")


@functools.lru_cache(maxsize=None)
def grid(kind, n, seed=0):
    """read-only uint32 words of a seeded n^3 occupancy"""
    rng = np.random.default_rng([GRID_KINDS.index(kind), n, seed])
    if kind == "noise":
        occ = rng.random((n, n, n)) < 0.5
    elif kind == "sparse":
        occ = rng.random((n, n, n)) < 0.004
    else:
        occ = np.zeros((n, n, n), bool)
        for _ in range(int(rng.integers(4, 12))):                      # slabs, bars, boxes, single voxels
            lo = rng.integers(0, n, 3)
            ext = np.where(rng.random(3) < 0.4, n, rng.integers(1, max(2, n // 3), 3))
            hi = np.minimum(n, lo + ext)
            lo = np.where(ext == n, 0, lo)
            occ[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] ^= True
        occ[n // 4:n // 2 + 1, n // 4:n // 2 + 3, n // 4:n // 2 + 2] ^= True          # one box with faces across every axis inside the grid
        assert occ.any() and not occ.all()
    w = pack(occ)
    w.setflags(write=False)
    return w


def border(words, n):
    """numpy restatement of the JFA's seeds: set voxels with an unset voxel, or the outside of the grid, among their 26 neighbours"""
    occ = unpack(words, n)
    pad = np.pad(occ, 1)
    full = np.ones_like(occ)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                full &= pad[dz:dz + n, dy:dy + n, dx:dx + n]
    return occ & ~full


def magnitudes(sdf):
    """number of distinct finite |sdf| values"""
    a = np.abs(np.asarray(sdf, F))
    return int(np.unique(a[np.isfinite(a)]).size)


# ---- soups ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def soup_units(n, seed):
    """(T, 3, 3) float64 triangles in voxel units: the families of the dyadic soup test"""
    rng = np.random.default_rng([n, seed])
    tris = []
    for _ in range(400):                                              # random size classes, sub-voxel to grid-spanning
        c = rng.random(3) * n
        tris.append(c + (rng.random((3, 3)) - 0.5) * n * 10.0 ** rng.uniform(-3.2, 0.0))
    for _ in range(100):                                              # slivers
        c = rng.random(3) * n
        d = (rng.random(3) - 0.5) * n * 0.5
        tris.append(np.stack([c, c + d, c + d * 0.5 + (rng.random(3) - 0.5) * 0.01]))
    for _ in range(100):                                              # vertices on voxel corners / centres
        tris.append(rng.integers(0, n, (3, 3)) + rng.choice([0.0, 0.5], (3, 3)))
    for ax in range(3):                                               # inside planes of constant x / y / z
        for _ in range(30):
            v = rng.random((3, 3)) * n
            v[:, ax] = rng.integers(0, n) + rng.choice([0.0, 0.5])
            tris.append(v)
    for _ in range(60):                                               # partly or wholly outside the frame
        c = (rng.random(3) * 1.6 - 0.3) * n
        tris.append(c + (rng.random((3, 3)) - 0.5) * n * 0.8)
    u = np.stack(tris).astype(np.float64)
    u.setflags(write=False)
    return u


def soup(n, seed, vs, origin):
    """(xyz float32 [3T, 3], tri uint32 [T, 3]): the soup mapped into the frame in float64 and rounded once"""
    u = soup_units(n, seed)
    w = (np.asarray(origin, F).astype(np.float64) + u * float(F(vs))).astype(F)
    xyz = np.ascontiguousarray(w.reshape(-1, 3))
    return xyz, np.arange(xyz.shape[0], dtype=np.uint32).reshape(-1, 3)


# ---- translated meshes ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mesh_level(name, n, level, scale=1.0):
    """(xyz, tri, origin, vs) of an asset translated to a level of LEVELS or to "x1000", in the frame of the translated mesh at side n.
    scale != 1 scales the mesh about its centre AFTER the frame is taken (it then leaves the frame)."""
    from cuda_mesh_voxelization_amd import mesh as M
    xyz0, tri = M.import_mesh(M.asset(name))
    _, vs0 = M.frame([xyz0], n)
    d = LEVELS["2^-4"] if level == "x1000" else LEVELS[level]
    T = DIRECTION * d * float(vs0) * 2.0 ** 23
    w = xyz0.astype(np.float64) + T
    if level == "x1000":
        w = w * 1000.0
    xyz = w.astype(F)
    origin, vs = M.frame([xyz], n)
    if scale != 1.0:
        mid = (w.max(0) + w.min(0)) * 0.5
        xyz = ((w - mid) * scale + mid).astype(F)
    xyz.setflags(write=False)
    return xyz, tri, origin, vs


def translate(xyz0, T):
    """float32(xyz0 + T): one rounding"""
    return (np.asarray(xyz0, F).astype(np.float64) + np.asarray(T, np.float64)).astype(F)


# ---- the ids of every JFA pass -------------------------------------------------------------------------------------------
def check_every_pass_ids(engine, fr, g, tag):
    """The body of test_gpu_parity.py::test_jfa_every_pass_ids_tiled_equals_naive for n <= 1024: after every pass k the packed seed ids of
    the tile kernel equal those of the one-thread-per-voxel kernel on the SAME input state, and so do the first pass and the fused first
    two passes in their from-the-border-mask forms.  Returns the number of comparisons made."""
    import torch
    from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Window
    n, ctx = fr.n, engine.ctx
    assert ctx.jfa_id_bytes(fr) == 4
    brd = torch.empty(fr.words, dtype=torch.int32, device=engine.device)
    ctx.surface(fr, g.data_ptr(), None, None, brd.data_ptr())
    wbytes = ctx.jfa_window_bytes(fr, n)
    assert wbytes == fr.voxels * 4
    cur = torch.empty(fr.voxels, dtype=torch.int32, device=engine.device)
    b = torch.empty_like(cur)
    ctx.jfa_init(fr, g.data_ptr(), None, None, cur.data_ptr())
    wa = torch.empty(wbytes, dtype=torch.uint8, device=engine.device)
    W = lambda t: Window.make(t.data_ptr(), t.numel() * t.element_size(), n, 0)
    done = 0

    def same(win, plain, what):
        engine.sync()
        ok = torch.equal(win.view(torch.int32), plain)
        assert ok, (tag, what, int((win.view(torch.int32) != plain).sum().item()))
        return 1

    k = n // 2
    while k >= 1:
        ctx.jfa_pass(fr, k, cur.data_ptr(), None, None, b.data_ptr(), ALGO_NAIVE)
        ctx.jfa_pass(fr, k, cur.data_ptr(), None, None, wa.data_ptr(), ALGO_TILED)
        done += same(wa, b, k)
        if k == n // 2 and ctx.jfa_can_start_from_mask(fr, ALGO_TILED):
            t = torch.empty(wbytes, dtype=torch.uint8, device=engine.device)
            ctx.jfa_window_first_pass(fr, brd.data_ptr(), W(t))
            done += same(t, b, "first pass from the mask")
            del t
        if k == n // 4 and ctx.jfa_can_fuse_first_two(fr, ALGO_TILED):
            t = torch.empty(wbytes, dtype=torch.uint8, device=engine.device)
            ctx.jfa_window_first_two(fr, brd.data_ptr(), W(t))
            done += same(t, b, "passes n/2 + n/4 from the mask")
            del t
        cur, b = b, cur
        k //= 2
    return done
