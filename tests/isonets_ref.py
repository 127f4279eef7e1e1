"""numpy restatement of the iso-surface-nets contract of include/vphip.h (vp_isonets*), written from the contract text: the inside set of
the field, then the surface nets of tests/surfnets_ref.py on that set for records, quads and the relaxation, and float32 arithmetic in the
prescribed order for the positions and normals.  Also the fields and error measures the CPU and GPU tests share."""
import numpy as np

import surfnets_ref as SR

F32 = np.float32
LINEAR, SIGNED_SQUARE = 0, 1
# the twelve edges in the contract's order: axis x, y, z; per axis the lower corners with that axis bit clear, ascending
EDGES = [(axis, c, c | (1 << axis)) for axis in range(3) for c in range(8) if not (c >> axis) & 1]


def field_h(field, transform, iso):
    """h = g - iso, float32, the field's shape"""
    v = np.asarray(field, F32)
    with np.errstate(all="ignore"):
        g = np.copysign(np.sqrt(np.abs(v)), v).astype(F32) if transform == SIGNED_SQUARE else v
        return (g - F32(iso)).astype(F32)


def inside_of(h):
    """+0 .. +inf; -0, negatives and every NaN are outside"""
    return np.ascontiguousarray(h).view(np.uint32) <= np.uint32(0x7F800000)


def corner_values(h, coords):
    """h at the eight corners of the cells (cx, cy, cz) in `coords` [V, 3]; NaN outside the grid: float32 [V, 8]"""
    n = h.shape[0]
    p = np.full((n + 2,) * 3, np.nan, F32)
    p[1:-1, 1:-1, 1:-1] = h
    out = np.empty((len(coords), 8), F32)
    for c in range(8):
        out[:, c] = p[coords[:, 2] + 1 + (c >> 2), coords[:, 1] + 1 + ((c >> 1) & 1), coords[:, 0] + 1 + (c & 1)]
    return out


def positions(hc, inside_c, coords):
    """starting positions [V, 3] from the corner values hc [V, 8] and the corners' inside flags"""
    acc = np.zeros((len(hc), 3), F32)
    m = np.zeros(len(hc), np.int32)
    with np.errstate(all="ignore"):
        for axis, c, d in EDGES:
            cross = inside_c[:, c] != inside_c[:, d]
            t = (hc[:, c] / (hc[:, c] - hc[:, d]).astype(F32)).astype(F32)
            t = np.where((t >= 0) & (t <= 1), t, F32(0.5)).astype(F32)
            m += cross
            for a in range(3):
                term = t if a == axis else np.full(len(hc), F32((c >> a) & 1), F32)
                acc[:, a] = np.where(cross, (acc[:, a] + term).astype(F32), acc[:, a])
        q = (acc / m.astype(F32)[:, None]).astype(F32)
    return ((coords.astype(F32) + F32(0.5)).astype(F32) + q).astype(F32)


def normals_of(hc):
    h = [hc[:, c] for c in range(8)]
    with np.errstate(all="ignore"):
        def d(a, b):
            return (h[a] - h[b]).astype(F32)

        def g4(p0, p1, p2, p3):
            return ((d(*p0) + d(*p1)).astype(F32) + (d(*p2) + d(*p3)).astype(F32)).astype(F32)
        g = np.stack([g4((1, 0), (3, 2), (5, 4), (7, 6)), g4((2, 0), (3, 1), (6, 4), (7, 5)), g4((4, 0), (5, 1), (6, 2), (7, 3))], axis=1)
        sq = (g * g).astype(F32)
        l2 = ((sq[:, 0] + sq[:, 1]).astype(F32) + sq[:, 2]).astype(F32)
        ok = (l2 > 0) & np.isfinite(l2)
        nrm = ((-g) / np.sqrt(l2).astype(F32)[:, None]).astype(F32)
    return np.where(ok[:, None], nrm, F32(0.0)).astype(F32)


def relax(cells, n, xyz, counts):
    """{count: positions} after `count` Jacobi steps of the surface-nets contract, started from xyz"""
    n1 = n + 1
    idx = (cells & np.uint64((1 << 40) - 1)).astype(np.int64)
    mk = (cells >> np.uint64(40)).astype(np.int64)
    coords = SR.cell_coords(cells, n)
    counts = sorted(set(counts))
    out, cur = {}, xyz
    if counts[-1] > 0:
        rank = np.full(n1 ** 3, -1, np.int64)
        rank[idx] = np.arange(len(idx))
        exists = SR.MIXED_TAB[mk]
        deg = exists.sum(1).astype(np.int32)
        step = (-1, 1, -n1, n1, -n1 * n1, n1 * n1)
        nb = [rank[np.where(exists[:, f], idx + step[f], idx)] for f in range(6)]
        assert all((r >= 0).all() for r in nb)
    for it in range(counts[-1] + 1):
        if it in counts:
            out[it] = cur
        if it < counts[-1]:
            cur = SR.relax_step(cur, coords, nb, exists, deg)
    return out


def isonets_numpy(field, transform=LINEAR, iso=0.0, iterations=0, every=None):
    """field float32 [n, n, n] (index z, y, x) -> (cells uint64[V], xyz float32[V, 3], normals float32[V, 3], quads uint32[Q, 4]);
    every = iterable of iteration counts: xyz becomes {count: positions}"""
    n = field.shape[0]
    h = field_h(field, transform, iso)
    ins = inside_of(h)
    cells, _, quads = SR.surfnets_bool(ins, 0)
    coords = SR.cell_coords(cells, n)
    hc = corner_values(h, coords)
    mk = (cells >> np.uint64(40)).astype(np.int64)
    inside_c = ((mk[:, None] >> np.arange(8)) & 1).astype(bool)
    assert np.array_equal(inside_c, inside_of(hc))
    xyz = positions(hc, inside_c, coords)
    nrm = normals_of(hc)
    if len(cells) == 0:
        rel = {it: xyz for it in ([iterations] if every is None else every)}
    else:
        rel = relax(cells, n, xyz, [iterations] if every is None else every)
    return cells, (rel if every is not None else rel[iterations]), nrm, quads


# ---- fields ------------------------------------------------------------------------------------------------
SPHERE_C, SPHERE_R = (15.3, 16.1, 15.7), 10.0
CUT_C = (2.2, 29.4, 15.7)


def sphere_field(n, c=SPHERE_C, r=SPHERE_R, squared=False, scale=1.0):
    """r - |x - c| at the voxel INDEX (the coordinates of surfnets_ref.sphere), + inside; squared: its signed square; scale: world units"""
    z, y, x = np.mgrid[0:n, 0:n, 0:n].astype(np.float64)
    d = (r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)) * scale
    return (np.copysign(d * d, d) if squared else d).astype(F32)


def signed_zero_field(vox, inf=False):
    mag = F32(np.inf) if inf else F32(0.0)
    return np.where(vox, mag, -mag).astype(F32)


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1e-45, -1e-45, 3e38, -3e38], F32)


def laced_random_field(n, seed):
    """uniform in [-1, 1], 5 % of the voxels replaced by +-0, +-inf, +-NaN, +-1e-45, +-3e38"""
    rng = np.random.default_rng(seed)
    f = rng.uniform(-1.0, 1.0, (n, n, n)).astype(F32)
    lace = rng.random((n, n, n)) < 0.05
    f[lace] = SPECIALS[rng.integers(0, len(SPECIALS), int(lace.sum()))]
    return f


def sparse_field(n, voxels, inside_value=1.0, outside_value=-3.0):
    f = np.full((n, n, n), outside_value, F32)
    for x, y, z in voxels:
        f[z, y, x] = inside_value
    return f


def single_voxel_expectation(n, v):
    """h = +1 on voxel v, -3 elsewhere, LINEAR, iso 0: the records and quads of surfnets_ref.single_voxel_expectation; every crossing lies
    1/4 of an edge from the voxel (1/2 where the edge leaves the grid: h = NaN there), the other two coordinates of an edge's point are the
    voxel's: the vertex of the cell that has the voxel as its upper (lower) corner along an axis sits at local (0.75 + 1 + 1) / 3
    ((0.25 + 0 + 0) / 3); every sum is exact, so the order of the additions does not show"""
    cells, _, quads = SR.single_voxel_expectation(n, v)
    xyz = np.empty((8, 3), F32)
    for t in range(8):
        for a in range(3):
            hi = (t >> a) & 1                                   # the cell lies on the + side of the voxel: the voxel is its lower corner
            cell = v[a] - 1 + hi
            if hi:                                              # the far end of the crossing edge is voxel v_a + 1; outside the grid: t = 0.5
                acc = F32(0.25) if v[a] + 1 < n else F32(0.5)
            else:
                acc = F32(F32(F32(0.75) if v[a] >= 1 else F32(0.5)) + F32(2.0))
            xyz[t, a] = F32(F32(F32(cell) + F32(0.5)) + F32(F32(acc) / F32(3.0)))
    return cells, xyz, quads


def sparse_expectation(n, voxels):
    """by hand: sparse_field(n, voxels) at iso 0, LINEAR, for voxels that share no cell (at least two voxels apart): the meshes of
    single_voxel_expectation merged -- vertices by cell index, quads by owner cell, then axis -- and the normals: G_a = -+4 on a cell
    inside the grid, so N_a = +-4 / sqrtf(48) away from the voxel; zero on a cell with a corner outside the grid"""
    low = np.uint64((1 << 40) - 1)
    # (owner vertex t, axis) of the six quads in the order surfnets_ref.single_voxel_expectation lists them
    keys = sorted([(7 - (1 << a), a) for a in range(3)] + [(7, a) for a in range(3)])
    cells, xyz, nrm, owners, rows = [], [], [], [], []
    length = np.sqrt(F32(48.0))
    for k, v in enumerate(voxels):
        c, x, q = single_voxel_expectation(n, v)
        cells.append(c)
        xyz.append(x)
        for t in range(8):
            cut = any(not (0 <= v[a] - 1 + ((t >> a) & 1) < n - 1) for a in range(3))
            nrm.append([F32(0.0) if cut else F32(F32(4.0 if (t >> a) & 1 else -4.0) / length) for a in range(3)])
        for (t, axis), row in zip(keys, q):
            owners.append((int(c[t] & low), axis))
            rows.append(row.astype(np.int64) + 8 * k)
    cells, xyz, nrm = np.concatenate(cells), np.concatenate(xyz), np.array(nrm, F32)
    order = np.argsort(cells & low, kind="stable")
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    qorder = sorted(range(len(rows)), key=lambda i: owners[i])
    quads = rank[np.array(rows)[qorder]].astype(np.uint32)
    return cells[order], xyz[order], nrm[order], quads


# ---- invariants and error measures --------------------------------------------------------------------------
def euler_characteristic(nverts, quads):
    return nverts - SR.edge_stats(quads)[2] + len(quads)


def in_closed_cell(xyz, cells, n):
    c = SR.cell_coords(cells, n).astype(np.float64)
    p = xyz.astype(np.float64)
    return bool(np.isfinite(xyz).all() and (p >= c + 0.5).all() and (p <= c + 1.5).all())


def sphere_error(xyz, iso, c=SPHERE_C, r=SPHERE_R):
    """| distance of a vertex to the sphere's surface - |iso| | in voxels; lattice position p is voxel index p - 0.5"""
    p = xyz.astype(np.float64) - 0.5
    return np.abs((r - np.sqrt(((p - np.array(c)) ** 2).sum(1))) - iso)
