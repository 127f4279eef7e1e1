"""numpy restatement of the surface-nets contract of include/vphip.h (vp_surfnets_*), written from the contract text: whole arrays over the
(n+1)^3 cells, tables over the 256 corner masks, float32 arithmetic in the prescribed order.  Also the grids and the mesh invariants the CPU
and GPU tests share."""
import os

import numpy as np

from fill_ref import bool_to_words, words_to_bool

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

F32 = np.float32
FACES = (0x55, 0xAA, 0x33, 0xCC, 0x0F, 0xF0)          # corners of the faces -x, +x, -y, +y, -z, +z


def _tables():
    """per corner mask: m (crossing edges), S[3] (sums of twice the midpoint coordinates), the three owned edges, the six mixed faces"""
    m = np.zeros(256, np.int32)
    s = np.zeros((256, 3), np.int32)
    own = np.zeros((256, 3), bool)
    mixed = np.zeros((256, 6), bool)
    for mask in range(256):
        bit = [(mask >> c) & 1 for c in range(8)]
        for axis in range(3):
            for c in range(8):
                if (c >> axis) & 1:
                    continue
                if bit[c] == bit[c | (1 << axis)]:
                    continue
                m[mask] += 1
                for a in range(3):
                    s[mask, a] += 1 if a == axis else 2 * ((c >> a) & 1)
            own[mask, axis] = bit[0] != bit[1 << axis]
        for f, fm in enumerate(FACES):
            mixed[mask, f] = (mask & fm) not in (0, fm)
    return m, s, own, mixed


M_TAB, S_TAB, OWN_TAB, MIXED_TAB = _tables()


def corner_masks(vox):
    """(n+1)^3 uint8 corner masks, index [cz+1, cy+1, cx+1]"""
    n = vox.shape[0]
    p = np.zeros((n + 2,) * 3, np.uint8)
    p[1:-1, 1:-1, 1:-1] = vox
    mask = np.zeros((n + 1,) * 3, np.uint8)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        mask |= p[dz:dz + n + 1, dy:dy + n + 1, dx:dx + n + 1] << c
    return mask


def relax_step(xyz, coords, nb, exists, deg):
    acc = np.zeros_like(xyz)
    started = np.zeros(len(xyz), bool)
    for f in range(6):
        val = xyz[nb[f]]
        e = exists[:, f]
        acc = np.where((e & started)[:, None], acc + val, np.where(e[:, None], val, acc)).astype(F32)
        started |= e
    q = (acc / deg[:, None].astype(F32)).astype(F32)
    lo = (coords.astype(F32) + F32(0.5625)).astype(F32)
    hi = (coords.astype(F32) + F32(1.4375)).astype(F32)
    return np.minimum(np.maximum(q, lo), hi).astype(F32)


def surfnets_bool(vox, iterations=0, every=None):
    """(cells uint64[V], xyz float32[V, 3], quads uint32[Q, 4]); every = iterable of iteration counts: xyz becomes {count: positions}"""
    n = vox.shape[0]
    n1 = n + 1
    mask = corner_masks(vox).reshape(-1)
    active = (mask != 0) & (mask != 255)
    idx = np.flatnonzero(active).astype(np.int64)
    mk = mask[idx].astype(np.int64)
    cells = (idx | (mk << 40)).astype(np.uint64)
    coords = np.stack([idx % n1 - 1, (idx // n1) % n1 - 1, idx // (n1 * n1) - 1], axis=1)          # (cx, cy, cz)
    with np.errstate(divide="ignore", invalid="ignore"):
        quot = (S_TAB[mk].astype(F32) / (2 * M_TAB[mk]).astype(F32)[:, None]).astype(F32)
    xyz = ((coords.astype(F32) + F32(0.5)).astype(F32) + quot).astype(F32)
    rank = np.full(n1 ** 3, -1, np.int64)
    rank[idx] = np.arange(len(idx))
    # quads: ordered by owner cell, then axis
    own = OWN_TAB[mask]                                        # [(n+1)^3, 3]
    flat = np.flatnonzero(own.reshape(-1))
    oc, axis = flat // 3, flat % 3
    s1, s2 = n1, n1 * n1
    offs = np.array([[-s1 - s2, -s2, 0, -s1], [-1 - s2, -1, 0, -s2], [-1 - s1, -s1, 0, -1]], np.int64)
    qc = oc[:, None] + offs[axis]
    quads = rank[qc]
    assert (quads >= 0).all()
    upper = (mask[oc] & 1) == 0                                # corner 0 unset: the upper voxel is the set one
    quads[upper] = quads[upper][:, ::-1]
    quads = quads.astype(np.uint32)
    # relaxation
    counts = sorted(set([iterations] if every is None else every))
    out = {}
    if counts and counts[-1] > 0:
        exists = MIXED_TAB[mk]
        deg = exists.sum(1).astype(np.int32)
        step = (-1, 1, -s1, s1, -s2, s2)
        nb = []
        for f in range(6):
            r = rank[np.where(exists[:, f], idx + step[f], idx)]
            assert (r >= 0).all()
            nb.append(r)
    cur = xyz
    for it in range((counts[-1] if counts else 0) + 1):
        if it in counts:
            out[it] = cur
        if it < counts[-1]:
            cur = relax_step(cur, coords, nb, exists, deg)
    return cells, (out if every is not None else out[iterations]), quads


def surfnets_numpy(words, n, iterations=0, every=None):
    return surfnets_bool(words_to_bool(words, n), iterations, every)


# ---- grids -------------------------------------------------------------------------------------------------
def single_voxel(n, v):
    vox = np.zeros((n, n, n), bool)
    vox[v[2], v[1], v[0]] = True
    return vox


def sphere(n, c=(15.3, 16.1, 15.7), r2=100.0):
    z, y, x = np.mgrid[0:n, 0:n, 0:n]
    return (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 < r2


def torus(n=32):
    z, y, x = np.mgrid[0:n, 0:n, 0:n]
    return (np.sqrt((x - 15.5) ** 2 + (y - 15.5) ** 2) - 9) ** 2 + (z - 15.5) ** 2 < 12


def checkerboard(n):
    z, y, x = np.mgrid[0:n, 0:n, 0:n]
    return (x + y + z) % 2 == 0


def random_bool(n, density, seed):
    return np.random.default_rng(seed).random((n, n, n)) < density


def bunny64():
    return words_to_bool(np.fromfile(os.path.join(GOLDEN, "bunny_decimated_n64.grid.u32"), np.uint32), 64)


def single_voxel_expectation(n, v):
    """by hand: the eight cells around voxel v, their masks (the voxel is corner 7 - t of cell t), positions and the six quads"""
    n1 = n + 1
    cells, xyz = [], []
    for t in range(8):
        dx, dy, dz = t & 1, (t >> 1) & 1, t >> 2
        cx, cy, cz = v[0] - 1 + dx, v[1] - 1 + dy, v[2] - 1 + dz
        corner = (1 - dx) + 2 * (1 - dy) + 4 * (1 - dz)                 # where the voxel sits in this cell
        cells.append(((cx + 1) + n1 * ((cy + 1) + n1 * (cz + 1))) | ((1 << corner) << 40))
        # three crossing edges leave the corner: S_a = 1 (own axis) + 2 * 2 * corner_a ... m = 3, S_a = 1 + 4 corner_a: 1/6 or 5/6
        xyz.append([F32(F32(c) + F32(0.5)) + (F32(5.0) / F32(6.0) if hi == 0 else F32(1.0) / F32(6.0))
                    for c, hi in ((cx, dx), (cy, dy), (cz, dz))])
    cells = np.array(cells, np.uint64)
    xyz = np.array(xyz, F32)
    # vertex t = cell (dx, dy, dz) around the voxel; quads by owner cell, then axis.  The owner of the pair (v - e_a, v) is the cell with
    # corner 0 = v - e_a: t = 7 without bit a, upper voxel set -> reversed; the owner of (v, v + e_a) is t = 7, lower voxel set.
    def cell_at(i, j, k):            # t of the cell whose corner 0 is voxel v + (i, j, k) - 1 ... offsets relative to t = 7
        return (1 + i) + 2 * (1 + j) + 4 * (1 + k)
    quads = {}
    for axis in range(3):
        for upper in (True, False):
            o = [0, 0, 0]
            if upper:
                o[axis] = -1
            i, j, k = o
            if axis == 0:
                q = [cell_at(i, j - 1, k - 1), cell_at(i, j, k - 1), cell_at(i, j, k), cell_at(i, j - 1, k)]
            elif axis == 1:
                q = [cell_at(i - 1, j, k - 1), cell_at(i - 1, j, k), cell_at(i, j, k), cell_at(i, j, k - 1)]
            else:
                q = [cell_at(i - 1, j - 1, k), cell_at(i, j - 1, k), cell_at(i, j, k), cell_at(i - 1, j, k)]
            quads[(cell_at(i, j, k), axis)] = q[::-1] if upper else q
    quads = np.array([quads[key] for key in sorted(quads)], np.uint32)
    return cells, xyz, quads


def single_voxel_relaxed(n, v, iterations):
    """positions of the eight vertices around one voxel after `iterations` steps, by hand: vertex t = (dx, dy, dz) has exactly the three
    neighbours t ^ 1, t ^ 2, t ^ 4 -- across +a where d_a = 0, across -a where d_a = 1 -- which the order -x, +x, -y, +y, -z, +z visits
    as x, y, z; (first + second) + third, one division by 3, the clamp"""
    _, xyz, _ = single_voxel_expectation(n, v)
    for _ in range(iterations):
        new = np.empty_like(xyz)
        for t in range(8):
            cell = [v[a] - 1 + ((t >> a) & 1) for a in range(3)]
            for a in range(3):
                acc = F32(F32(xyz[t ^ 1, a] + xyz[t ^ 2, a]) + xyz[t ^ 4, a])
                q = F32(acc / F32(3.0))
                new[t, a] = min(max(q, F32(F32(cell[a]) + F32(0.5625))), F32(F32(cell[a]) + F32(1.4375)))
        xyz = new
    return xyz


# ---- invariants ---------------------------------------------------------------------------------------------
def exposed_faces(vox):
    """(set, unset) face pairs counted directly; the outside of the grid is unset"""
    p = np.pad(vox, 1)
    return int(sum(np.count_nonzero(np.diff(p.astype(np.int8), axis=a)) for a in range(3)))


def edge_stats(quads):
    """(directed edges balanced?, {multiplicity: undirected edges}, undirected edge count)"""
    a = quads.astype(np.int64)
    b = np.roll(a, -1, axis=1)
    big = np.int64(1) << 32
    fwd = np.sort((a * big + b).reshape(-1))
    bwd = np.sort((b * big + a).reshape(-1))
    und = (np.minimum(a, b) * big + np.maximum(a, b)).reshape(-1)
    _, mult = np.unique(und, return_counts=True)
    vals, cnt = np.unique(mult, return_counts=True)
    return bool(np.array_equal(fwd, bwd)), dict(zip(vals.tolist(), cnt.tolist())), len(mult)


def signed_volume(xyz, quads):
    p = xyz.astype(np.float64)
    vol = 0.0
    for t in ((0, 1, 2), (0, 2, 3)):
        a, b, c = (p[quads[:, i]] for i in t)
        vol += np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0
    return vol


def cell_coords(cells, n):
    idx = (cells & np.uint64((1 << 40) - 1)).astype(np.int64)
    n1 = n + 1
    return np.stack([idx % n1 - 1, (idx // n1) % n1 - 1, idx // (n1 * n1) - 1], axis=1)
