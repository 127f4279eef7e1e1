"""Exact reference for conservative voxelization (include/vphip.h, vp_voxelize_conservative): a voxel is set iff its CLOSED box
overlaps the CLOSED triangle.  A helper module of the tests, not collected by pytest.

Coordinates are integers H in units of a half voxel, relative to the frame's origin: world = origin + H * vs / 2, and voxel i spans
H in [2 i, 2 i + 2].  Vertices on voxel corners are even, on voxel centres odd.  In a dyadic frame (vs = 2^-k, origin a multiple of
vs / 2) every world coordinate is an exact float32, and exact_budget() checks that every intermediate of the contract's float32
formula is exact too.  Where it is, the formula must equal sat_overlap(), the separating-axis test in int64.

  sat_overlap        exact union grid of closed boxes vs closed triangles (13 axes, int64), batched by candidate-box shape
  overlap_f64        the same test in float64 with boxes shrunk or grown by a margin (for frames where float32 is not exact)
  exact_budget       asserts |every intermediate of the float32 formula| < 2^24 in its natural unit
  families()         seeded generators of awkward triangles, in a local cell [0, 2 E]^3
  pack()             one triangle per cell of a lattice, >= 2 empty voxels between candidate boxes: the union is a disjoint union
"""
import numpy as np

F = np.float32
LIMIT = 1 << 24


# ---- the separating-axis test, batched -----------------------------------------------------------------------------------
def _cand(V, scale):
    """candidate voxel range of each triangle: [floor(min / scale) - 1, floor(max / scale) + 1] per axis (a superset of the boxes a
    closed triangle touches, also for boxes grown by up to half a voxel)"""
    lo = np.floor(V.min(axis=1) / scale).astype(np.int64) - 1
    hi = np.floor(V.max(axis=1) / scale).astype(np.int64) + 1
    return lo, hi


def _sat_block(V, lo, shape, scale, offset, half):
    """mask [T, sz, sy, sx]: box (centre scale * idx + offset, half-size half) overlaps triangle V [T, 3, 3] (closed sets).
    Box normals are 1-D tests, e_i x axis are 2-D tests (their component on that axis is zero), the triangle normal is 3-D."""
    sx, sy, sz = shape
    cx = scale * (lo[:, 0:1] + np.arange(sx)) + offset                      # [T, sx]
    cy = scale * (lo[:, 1:2] + np.arange(sy)) + offset
    cz = scale * (lo[:, 2:3] + np.arange(sz)) + offset
    vmin, vmax = V.min(axis=1), V.max(axis=1)
    bx = (cx >= vmin[:, 0:1] - half) & (cx <= vmax[:, 0:1] + half)
    by = (cy >= vmin[:, 1:2] - half) & (cy <= vmax[:, 1:2] + half)
    bz = (cz >= vmin[:, 2:3] - half) & (cz <= vmax[:, 2:3] + half)
    ok = bz[:, :, None, None] & by[:, None, :, None] & bx[:, None, None, :]
    e = [V[:, 1] - V[:, 0], V[:, 2] - V[:, 1], V[:, 0] - V[:, 2]]

    def proj(ax):                                                           # min / max of the vertices on axis ax [T, 3]
        p = np.einsum("tkc,tc->tk", V, ax)
        return p.min(axis=1), p.max(axis=1)

    def within(pc, ax, nd):                                                 # pc: centre projection, nd extra dims to broadcast
        pmin, pmax = proj(ax)
        r = half * np.abs(ax).sum(axis=1)
        sh = (-1,) + (1,) * nd
        return (pc >= (pmin - r).reshape(sh)) & (pc <= (pmax + r).reshape(sh))

    zero = np.zeros(len(V), V.dtype)
    for ei in e:
        # ei x X = (0, ez, -ey): centre projection ez cy - ey cz, over (z, y)
        ax = np.stack([zero, ei[:, 2], -ei[:, 1]], axis=1)
        pc = ei[:, 2, None, None] * cy[:, None, :] - ei[:, 1, None, None] * cz[:, :, None]
        ok &= within(pc, ax, 2)[:, :, :, None]
        # ei x Y = (-ez, 0, ex): -ez cx + ex cz, over (z, x)
        ax = np.stack([-ei[:, 2], zero, ei[:, 0]], axis=1)
        pc = -ei[:, 2, None, None] * cx[:, None, :] + ei[:, 0, None, None] * cz[:, :, None]
        ok &= within(pc, ax, 2)[:, :, None, :]
        # ei x Z = (ey, -ex, 0): ey cx - ex cy, over (y, x)
        ax = np.stack([ei[:, 1], -ei[:, 0], zero], axis=1)
        pc = ei[:, 1, None, None] * cx[:, None, :] - ei[:, 0, None, None] * cy[:, :, None]
        ok &= within(pc, ax, 2)[:, None, :, :]
    nrm = np.cross(e[0], e[1])
    pc = (nrm[:, 0, None, None, None] * cx[:, None, None, :] + nrm[:, 1, None, None, None] * cy[:, None, :, None]
          + nrm[:, 2, None, None, None] * cz[:, :, None, None])
    ok &= within(pc, nrm, 3)
    return ok


def _union(V, scale, offset, half, n, z0, z1, chunk=1 << 22):
    """union over the triangles of _sat_block, scattered into bits [z1 - z0, n, n] (voxels outside the frame dropped)"""
    bits = np.zeros((z1 - z0, n, n), bool)
    if len(V) == 0:
        return bits
    lo, hi = _cand(V, scale)
    shapes = hi - lo + 1
    uniq, inv = np.unique(shapes, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    for g, shape in enumerate(uniq):
        ids = np.nonzero(inv == g)[0]
        step = max(1, chunk // int(np.prod(shape)))
        for s in range(0, len(ids), step):
            t = ids[s:s + step]
            m = _sat_block(V[t], lo[t], tuple(int(x) for x in shape), scale, offset, half)
            k, z, y, x = np.nonzero(m)
            x = x + lo[t[k], 0]
            y = y + lo[t[k], 1]
            z = z + lo[t[k], 2]
            keep = (x >= 0) & (x < n) & (y >= 0) & (y < n) & (z >= z0) & (z < z1)
            bits[z[keep] - z0, y[keep], x[keep]] = True
    return bits


def sat_overlap(H, n, z0=0, z1=None):
    """exact union grid [z1 - z0, n, n] (bool, [z][y][x]) of the closed unit boxes that overlap the closed triangles H [T, 3, 3]
    (int64 half-voxel coordinates relative to the origin); triangles with a zero normal are the caller's to drop"""
    z1 = n if z1 is None else z1
    H = np.asarray(H, np.int64).reshape(-1, 3, 3)
    return _union(H, 2, 1, 1, n, z0, z1)


def overlap_f64(xyz, vs, origin, n, margin, z0=0, z1=None):
    """union grid of the boxes grown by `margin` voxels on every side (margin < 0: shrunk) that overlap the float64 triangles
    xyz [T, 3, 3] (world coordinates), in float64"""
    z1 = n if z1 is None else z1
    u = (np.asarray(xyz, np.float64).reshape(-1, 3, 3) - np.asarray(origin, np.float64)) / float(vs)
    return _union(u, 1.0, 0.5, 0.5 + margin, n, z0, z1)


def to_words(bits):
    return np.packbits(np.asarray(bits, bool).reshape(-1), bitorder="little").view(np.uint32)


# ---- float32 exactness of the contract's formula -------------------------------------------------------------------------
def nonzero_normal(H):
    H = np.asarray(H, np.int64)
    return np.cross(H[:, 1] - H[:, 0], H[:, 2] - H[:, 1]).any(axis=1)


def world(H, vs, origin):
    """float32 world coordinates of H; asserts the conversion is exact"""
    w64 = np.asarray(origin, np.float64) + np.asarray(H, np.float64) * (float(vs) / 2)
    w = w64.astype(F)
    assert np.array_equal(w.astype(np.float64), w64), "coordinates not exact in float32"
    return w


def exact_budget(H, vs, origin, n):
    """Asserts that every intermediate of the float32 formula of the contract is exact for these triangles in this frame, at every
    voxel the implementations evaluate it (the bounding box +- 2 voxels): each one, as an integer multiple of its natural unit,
    is below 2^24 in magnitude.  Units: q = vs / 2, halved away while every input stays a multiple (coordinates q, normal q^2,
    plane sums q^3, edge terms q^2).  Returns the largest magnitude found, as a fraction of 2^24."""
    H = np.asarray(H, np.int64).reshape(-1, 3, 3)
    q = float(vs) / 2
    O = np.asarray(origin, np.float64) / q
    assert np.array_equal(O, np.round(O)), "origin must be a multiple of vs / 2"
    assert 2.0 ** np.round(np.log2(float(vs))) == float(vs), "vs must be a power of two"
    O = O.astype(np.int64)
    W = H + O                                                       # world / q
    lo = np.floor(H.min(axis=1) / 2).astype(np.int64) - 2           # voxel range evaluated (numpy restatement: +- 2)
    hi = np.floor(H.max(axis=1) / 2).astype(np.int64) + 2
    lo = np.maximum(lo, 0)
    hi = np.minimum(hi, n - 1)
    VS = 2
    # common power of two of every input (coordinates, origin, vs): divide it out, so whole-voxel inputs are judged in voxels
    g = np.full(len(H), 1, np.int64)
    allin = np.concatenate([W.reshape(len(H), 9), np.broadcast_to(O, (len(H), 3)), np.full((len(H), 1), VS)], axis=1)
    odd = (allin % 2 != 0).any(axis=1)
    g[~odd] = 2
    W = W // g[:, None, None]
    vs_u = VS // g                                                   # [T]
    O_u = O[None, :] // g[:, None]
    worst = np.zeros(len(H), np.int64)

    def take(*xs):
        for x in xs:
            a = np.abs(np.asarray(x))
            worst[:] = np.maximum(worst, a.reshape(len(H), -1).max(axis=1))

    v = [W[:, 0], W[:, 1], W[:, 2]]
    take(W)
    e = [v[1] - v[0], v[2] - v[1], v[0] - v[2]]
    take(*e)
    a, b = e[0], e[1]
    prods = [a[:, 1] * b[:, 2], a[:, 2] * b[:, 1], a[:, 2] * b[:, 0], a[:, 0] * b[:, 2], a[:, 0] * b[:, 1], a[:, 1] * b[:, 0]]
    take(*prods)
    nrm = np.stack([prods[0] - prods[1], prods[2] - prods[3], prods[4] - prods[5]], axis=1)
    take(nrm)
    c = np.where(nrm > 0, vs_u[:, None], 0)
    cc = vs_u[:, None] - c
    for corner in (c, cc):
        d = corner - v[0]
        take(d)
        terms = nrm * d
        take(terms)
        take(terms[:, 0] + terms[:, 1], terms.sum(axis=1))
    d1 = (nrm * (c - v[0])).sum(axis=1)
    d2 = (nrm * (cc - v[0])).sum(axis=1)
    # corners p = O + idx * vs at the ends of the evaluated range (every sum below is linear in p: extremes at the ends)
    P = [O_u[:, None, :] + np.stack([lo, hi], axis=1) * vs_u[:, None, None]]   # [T, 2, 3]
    P = P[0]
    take(P, P + vs_u[:, None, None])
    for ix in (0, 1):
        for iy in (0, 1):
            for iz in (0, 1):
                p = np.stack([P[:, ix, 0], P[:, iy, 1], P[:, iz, 2]], axis=1)
                t3 = nrm * p
                t = t3.sum(axis=1)
                take(t3, t3[:, 0] + t3[:, 1], t, t + d1, t + d2)
                for qd in range(3):
                    U, Vv, S = qd, (qd + 1) % 3, (qd + 2) % 3
                    sg = np.where(nrm[:, S] >= 0, 1, -1)
                    for i in range(3):
                        nu, nv = -e[i][:, Vv] * sg, e[i][:, U] * sg
                        a1, a2 = nu * v[i][:, U], nv * v[i][:, Vv]
                        de0 = -(a1 + a2)
                        de1 = de0 + np.maximum(0, vs_u * nu)
                        de = de1 + np.maximum(0, vs_u * nv)
                        take(a1, a2, de0, vs_u * nu, vs_u * nv, de1, de)
                        l1, l2 = nu * p[:, U], nv * p[:, Vv]
                        take(l1, l2, l1 + l2, (l1 + l2) + de)
    m = int(worst.max()) if len(H) else 0
    assert m < LIMIT, "float32 not exact: an intermediate reaches %d >= 2^24" % m
    return m / LIMIT


# ---- generators (half-voxel integer coordinates in a local cell [0, 2 E]^3) ------------------------------------------------
def _ri(rng, lo, hi, size):
    return rng.integers(lo, hi + 1, size)


def _even(rng, E, size):
    return 2 * _ri(rng, 0, E, size)


def gen_random(rng, T, E):
    return _ri(rng, 0, 2 * E, (T, 3, 3))


def gen_face_plane(rng, T, E):
    """in a voxel-face plane (one coordinate the same even value on all three vertices)"""
    v = gen_random(rng, T, E)
    ax = _ri(rng, 0, 2, T)
    v[np.arange(T), :, ax] = _even(rng, E, T)[:, None]
    return v


def gen_voxel_edges(rng, T, E):
    """one edge along a voxel edge line (two coordinates equal and even), and one along a diagonal through voxel corners"""
    v = gen_random(rng, T, E)
    v[:, 0] = _even(rng, E, (T, 3))
    ax = _ri(rng, 0, 2, T)
    v[:, 1] = v[:, 0]
    v[np.arange(T), 1, ax] = _even(rng, E, T)
    h = T // 2                                                       # second half: v0 -> v2 along a lattice diagonal
    dirs = np.array([[1, 1, 0], [1, 0, 1], [0, 1, 1], [1, -1, 0], [1, 1, 1], [1, -1, 1], [-1, 1, 1], [1, 1, -1]])
    d = dirs[_ri(rng, 0, len(dirs) - 1, T - h)]
    k = _ri(rng, 1, max(1, E // 2), T - h)
    base = np.where(d < 0, 2 * E, 0) + np.where(d == 0, _even(rng, E, (T - h, 3)), 0)
    v[h:, 0] = base
    v[h:, 2] = base + 2 * k[:, None] * d
    return v


def gen_corners_centres(rng, T, E):
    """all vertices on voxel corners, all on voxel centres, or one of each kind per vertex"""
    v = _even(rng, E - 1, (T, 3, 3))
    kind = _ri(rng, 0, 2, T)
    v[kind == 1] += 1
    mix = (kind == 2)
    v[mix] += _ri(rng, 0, 1, (int(mix.sum()), 3, 1))
    return v


def gen_touching(rng, T, E):
    """touch a box only at one corner, along one edge, or over (part of) one face: a vertex / an edge / an edge on a voxel corner, edge
    line or face plane, the rest going away to the positive side"""
    C = _even(rng, 1, (T, 3)) + 2                                    # a corner in [2, 4]
    far = _ri(rng, 1, 2 * E - 6, (T, 2, 3))
    v = np.empty((T, 3, 3), np.int64)
    v[:, 0] = C
    v[:, 1:] = C[:, None] + far
    kind = _ri(rng, 0, 2, T)
    ax = _ri(rng, 0, 2, T)
    e = kind == 1                                                    # edge along a voxel edge line (axis ax)
    v[e, 1] = C[e]
    v[e, 1, ax[e]] += 2 * _ri(rng, 1, E // 2, int(e.sum()))
    f = kind == 2                                                    # edge in the face plane ax = C.ax
    idx = np.nonzero(f)[0]
    v[idx, 1, ax[idx]] = C[idx, ax[idx]]
    return v


def gen_thin(rng, T, E):
    """long and thin with a non-zero normal: the third vertex one half voxel off the line of the first two"""
    v = np.empty((T, 3, 3), np.int64)
    v[:, 0] = _ri(rng, 0, 2, (T, 3))
    v[:, 1] = 2 * E - _ri(rng, 0, 2, (T, 3))
    mid = (v[:, 0] + v[:, 1]) // 2
    v[:, 2] = mid + _ri(rng, -1, 1, (T, 3))
    return v


def gen_zero_normal_components(rng, T, E):
    """normals with one zero component (an edge along an axis) or two (the plane of one constant coordinate, odd or even)"""
    v = gen_random(rng, T, E)
    ax = _ri(rng, 0, 2, T)
    two = _ri(rng, 0, 1, T) == 1
    r = np.arange(T)
    v[r, 1] = v[r, 0]                                               # v1 - v0 along axis ax only
    v[r, 1, ax] = _ri(rng, 0, 2 * E, T)
    c = _ri(rng, 0, 2 * E, T)
    v[two, :, ax[two]] = c[two][:, None]                            # constant coordinate on all three
    return v


FAMILIES = {
    "random": gen_random,
    "face_plane": gen_face_plane,
    "voxel_edges": gen_voxel_edges,
    "corners_centres": gen_corners_centres,
    "touching": gen_touching,
    "thin": gen_thin,
    "zero_normal_components": gen_zero_normal_components,
}


def _orient(rng, v, E):
    """random axis permutation, mirror images (H -> 2 E - H keeps the parity) and vertex order"""
    T = len(v)
    perm = np.argsort(rng.random((T, 3)), axis=1)
    v = np.take_along_axis(v, perm[:, None, :], axis=2)
    flip = rng.random((T, 1, 3)) < 0.5
    v = np.where(flip, 2 * E - v, v)
    order = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]])[_ri(rng, 0, 5, T)]
    return np.take_along_axis(v, order[:, :, None], axis=1)


def families(seed, per_family, E, names=None):
    """[T, 3, 3] local triangles in [0, 2 E]^3 with a non-zero normal, family labels [T]"""
    rng = np.random.default_rng(seed)
    out, lab = [], []
    for name in (names or FAMILIES):
        v = _orient(rng, FAMILIES[name](rng, per_family, E), E)
        v = np.clip(v, 0, 2 * E)
        v = v[nonzero_normal(v)]
        out.append(v)
        lab += [name] * len(v)
    return np.concatenate(out).astype(np.int64), np.array(lab)


def pack(local, n, E, seed=0, border=True):
    """One local triangle ([0, 2 E]^3) per lattice cell of pitch E + 4 voxels: candidate boxes (E + 2 voxels) stay >= 2 empty voxels
    apart.  With border=True, triangles of cells on the grid's outer faces are pushed to touch the outer plane from outside
    (a face / edge / corner on H = 0 or H = 2 n) or to cross it.  Returns the placed triangles (as many as there are cells)."""
    rng = np.random.default_rng(seed)
    P = E + 4
    k = max(1, (n - E - 1) // P + 1)                                 # cells per axis, cell c spans voxels [c P, c P + E]
    cells = np.stack(np.meshgrid(np.arange(k), np.arange(k), np.arange(k), indexing="ij"), axis=-1).reshape(-1, 3)
    cells = cells[rng.permutation(len(cells))][:len(local)]
    out = local[:len(cells)] + 2 * P * cells[:, None, :]
    if border:
        for ax in range(3):
            for side in (0, 1):
                at = np.nonzero(cells[:, ax] == (0 if side == 0 else k - 1))[0]
                mode = _ri(rng, 0, 2, len(at))                         # 0: stay, 1: touch the outer plane from outside, 2: cross it
                for i, m in zip(at, mode):
                    if m == 0:
                        continue
                    c = out[i, :, ax]
                    if side == 0:
                        shift = -c.max() if m == 1 else -(c.min() + c.max()) // 2
                    else:
                        shift = 2 * n - c.min() if m == 1 else 2 * n - (c.min() + c.max()) // 2
                    out[i, :, ax] = c + shift
    return out


def cells_per_call(n, E):
    P = E + 4
    return max(1, (n - E - 1) // P + 1) ** 3


def describe(H, exp, got, n, z0=0):
    """the first triangles whose candidate box holds a differing voxel, with the voxels (x, y, z) that differ"""
    diff = np.argwhere(exp != got)                                   # [z, y, x]
    if not len(diff):
        return "no difference"
    lo, hi = _cand(np.asarray(H, np.int64), 2)
    lines = ["%d voxels differ" % len(diff)]
    for z, y, x in diff[:8]:
        p = np.array([x, y, z + z0])
        t = np.nonzero(((lo <= p) & (hi >= p)).all(axis=1))[0]
        lines.append("voxel %s expected %d: triangles %s %s" % (p.tolist(), int(exp[z, y, x]), t[:3].tolist(),
                                                                  [H[i].tolist() for i in t[:2]]))
    return "\n".join(lines)
