"""The contract of vp_reconstruct and vp_extrema (include/vphip.h) restated in numpy, and the cases of tests/test_reconstruct_cpu.py /
test_reconstruct_gpu.py (helpers, no tests).  Fields are (z, y, x) uint32 arrays, the domain a (z, y, x) bool array or None (every voxel);
outside the grid counts as not in the domain.

  reconstruct(F, G, domain, mode, conn)        (R, stats): the definition word for word -- whole-array min(grey_dilation(R), G) with scipy on
                                               the work values until nothing changes
  reconstruct_queue(F, G, domain, mode, conn)  the same by a queue: the voxels that rose in one step are the only ones that push in the next
                                               (index arrays of a grid padded by one layer); pinned to the first form at n = 32, and what the
                                               larger cases use
  extrema(values, domain, kind, scale, h, conn)          (V, H, E bool, stats) through two reconstructions
  extrema_plateaus(values, domain, kind, scale, h, conn) E by the plateau definition: scipy.ndimage.label per value of H
  isqrt16(v)                                   floor(sqrt(256 v)) in exact integers
and the solids: the three balls of DESIGN.md section 25, markers on block seams, gates between blocks, the comb maze as a wall field."""
import functools
import math

import numpy as np
import scipy.ndimage as ndi

from fill_ref import bool_to_words, words_to_bool  # noqa: F401

DILATION, EROSION = 0, 1
MAXIMA, MINIMA = 0, 1
LINEAR, SQRT16 = 0, 1
TOP = 0xFFFFFFFF
CONNS = (6, 26)
MODES = (DILATION, EROSION)


def offsets(conn):
    return [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dx or dy or dz) and (conn == 26 or abs(dx) + abs(dy) + abs(dz) == 1)]


def footprint(conn):
    """the neighbours and the voxel itself"""
    return ndi.generate_binary_structure(3, 1 if conn == 6 else 3)


def work(v, mode, domain):
    """the work values as int64: v or ~v, 0 off the domain"""
    v = np.asarray(v, np.uint32).astype(np.int64)
    w = TOP - v if mode == EROSION else v
    return w if domain is None else np.where(domain, w, 0)


def _finish(r, r0, domain, mode):
    """(R, stats) from the work values"""
    inside = np.ones(r.shape, bool) if domain is None else np.asarray(domain, bool)
    real = (TOP - r if mode == EROSION else r).astype(np.uint32)
    count = int(inside.sum())
    if count == 0:
        return real, (0, 0, 0, 0)
    top = int(r[inside].max())
    return real, (count, int((r != r0)[inside].sum()), int(real[inside].astype(np.uint64).sum()), TOP - top if mode == EROSION else top)


def reconstruct(F, G, domain=None, mode=DILATION, conn=6):
    g = work(G, mode, domain)
    r0 = np.minimum(work(F, mode, domain), g)
    r, fp = r0, footprint(conn)
    while True:
        nxt = np.minimum(ndi.grey_dilation(r, footprint=fp, mode="constant", cval=0), g)
        if np.array_equal(nxt, r):
            return _finish(r, r0, domain, mode)
        r = nxt


def reconstruct_queue(F, G, domain=None, mode=DILATION, conn=6):
    n = np.asarray(G).shape[0]
    p = n + 2
    g3 = work(G, mode, domain)
    r03 = np.minimum(work(F, mode, domain), g3)
    g, r = np.pad(g3, 1).reshape(-1), np.pad(r03, 1).reshape(-1)
    off = np.array([dx + p * (dy + p * dz) for dx, dy, dz in offsets(conn)], np.int64)
    front = np.flatnonzero(r > 0)
    while len(front):
        to = (front[:, None] + off[None, :]).reshape(-1)
        cand = np.minimum(np.repeat(r[front], len(off)), g[to])
        ok = cand > r[to]
        to, cand = to[ok], cand[ok]
        if not len(to):
            break
        o = np.lexsort((-cand, to))                                # by voxel, then the largest candidate first
        to, cand = to[o], cand[o]
        first = np.r_[True, to[1:] != to[:-1]]
        front = to[first]
        r[front] = cand[first]
    return _finish(r.reshape(p, p, p)[1:-1, 1:-1, 1:-1], r03, domain, mode)


def isqrt16(v):
    x = np.asarray(v, np.uint32).astype(np.int64) << 8
    r = np.floor(np.sqrt(x.astype(np.float64))).astype(np.int64)
    for _ in range(2):
        r = np.where(r * r > x, r - 1, r)
        r = np.where((r + 1) * (r + 1) <= x, r + 1, r)
    assert (r * r <= x).all() and ((r + 1) * (r + 1) > x).all()
    return r.astype(np.uint32)


def scaled(values, scale):
    return isqrt16(values) if scale == SQRT16 else np.asarray(values, np.uint32).copy()


def shifted(v, h, kind):
    """v - h (maxima) or v + h (minima), saturating"""
    v = np.asarray(v, np.uint32).astype(np.int64)
    return (np.minimum(v + h, TOP) if kind == MINIMA else np.maximum(v - h, 0)).astype(np.uint32)


def extrema(values, domain=None, kind=MAXIMA, scale=LINEAR, h=0, conn=6, rec=None):
    rec = rec or reconstruct_queue
    mode = EROSION if kind == MINIMA else DILATION
    V = scaled(values, scale)
    H, hs = rec(shifted(V, h, kind), V, domain, mode, conn)
    S, _ = rec(shifted(H, 1, kind), H, domain, mode, conn)
    E = H < S if kind == MINIMA else H > S
    inside = np.ones(V.shape, bool) if domain is None else np.asarray(domain, bool)
    assert not (E & ~inside).any()
    return V, H, E, (hs[0], int(E.sum()), hs[3], int((H != V)[inside].sum()))


def extrema_plateaus(values, domain=None, kind=MAXIMA, scale=LINEAR, h=0, conn=6):
    """E by the definition: p is in E iff its work value is not 0 and its plateau (the connected set in M of equal H) has no neighbour in M
    with a larger work value"""
    mode = EROSION if kind == MINIMA else DILATION
    V = scaled(values, scale)
    H, _ = reconstruct_queue(shifted(V, h, kind), V, domain, mode, conn)
    w = work(H, mode, domain)
    around = ndi.grey_dilation(w, footprint=footprint(conn), mode="constant", cval=0)      # the largest work value among a voxel and its neighbours
    E = np.zeros(w.shape, bool)
    for value in np.unique(w[w > 0]):
        labels, k = ndi.label(w == value, structure=footprint(conn))
        if k:
            higher = ndi.maximum(around, labels, np.arange(1, k + 1)) > value
            E |= (labels > 0) & ~np.r_[True, higher][labels]
    return E


# ---- solids and fields -------------------------------------------------------------------------------------------------------------------
def ball(n, c, r):
    """voxel (x, y, z) is set iff dx^2 + dy^2 + dz^2 <= r^2, in integers"""
    z, y, x = np.ogrid[:n, :n, :n]
    return (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= r * r


THREE_BALLS = (((18, 32, 32), 14), ((37, 32, 32), 8), ((48, 32, 32), 4))
THREE_BALLS_VOXELS, THREE_BALLS_MAX_D2 = 13741, 197
# what DESIGN.md section 25 records for the three balls: the components of inset:R, R = 1 .. 8 (6-connected), and per h in sixteenths of a voxel
# (markers, |E|) of the extended maxima of V = isqrt16(D^2), the same at connectivity 6 and 26
THREE_BALLS_INSETS = (1, 1, 2, 2, 1, 2, 2, 2)
THREE_BALLS_MAXIMA = {0: (3, 3), 1: (3, 3), 4: (3, 3), 8: (3, 3), 16: (3, 21), 24: (2, None), 32: (2, None), 48: (1, None), 64: (1, None)}


@functools.lru_cache(maxsize=None)
def three_balls():
    """(mask, D^2) at n = 64, read-only"""
    import edt_ref
    m = np.zeros((64, 64, 64), bool)
    for c, r in THREE_BALLS:
        m |= ball(64, c, r)
    d2 = edt_ref.edt_numpy(m, edt_ref.UNSET)
    d2 = np.where(m, d2, 0).astype(np.uint32)
    m.setflags(write=False)
    d2.setflags(write=False)
    return m, d2


def field(n, seed, top, density=1.0):
    """a random field with values 0 .. top, a share 1 - density of them 0"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, int(top) + 1, (n, n, n), dtype=np.uint64).astype(np.uint32)
    return v if density >= 1.0 else np.where(rng.random((n, n, n)) < density, v, 0).astype(np.uint32)


def smooth_field(n, seed, top):
    """a field with broad hills: plateaus and ridges that cross every block seam"""
    rng = np.random.default_rng(seed)
    v = ndi.uniform_filter(rng.random((n, n, n)), 7, mode="wrap")
    v = (v - v.min()) / (v.max() - v.min())
    return np.floor(v * top).astype(np.uint32)


def point(n, at, value=TOP):
    f = np.zeros((n, n, n), np.uint32)
    f[at[2], at[1], at[0]] = value
    return f


def block_box(b):
    """the voxels of block (bx, by, bz) of 32 x 16 x 16 as slices (z, y, x)"""
    return (slice(16 * b[2], 16 * b[2] + 16), slice(16 * b[1], 16 * b[1] + 16), slice(32 * b[0], 32 * b[0] + 32))


# Block A = (0, 1, 1) at n = 64 holds the marker.  Block B is reached only through one voxel pair across a face, an edge or a corner: G is 0
# everywhere but on a line in A and in B, and only the last voxel of the line has a neighbour in B.  B holds nothing to pull at the start --
# its marker is 0 and so is the halo voxel it sees, whose value arrives only after A has run: B has to run again on A's flag alone.
GATE_A = (0, 1, 1)
GATES = {"+x": (1, 1, 1), "-y": (0, 0, 1), "+z": (0, 1, 2), "+x+y": (1, 2, 1), "-y+z": (0, 0, 2), "+x-z": (1, 1, 0), "+x+y+z": (1, 2, 2), "+x-y-z": (1, 0, 0)}


def gate(name):
    """(F, G): G = 9 on a line inside A from the marker to A's voxel nearest B, G = 7 on all of B; F = TOP at the marker"""
    n = 64
    b = GATES[name]
    G = np.zeros((n, n, n), np.uint32)
    G[block_box(b)] = 7
    d = [b[k] - GATE_A[k] for k in range(3)]
    lo = (32 * GATE_A[0], 16 * GATE_A[1], 16 * GATE_A[2])
    size = (32, 16, 16)
    end = [lo[k] + (size[k] - 1 if d[k] > 0 else 0 if d[k] < 0 else size[k] // 2) for k in range(3)]
    start = [lo[k] + size[k] // 2 for k in range(3)]
    at = list(start)
    G[at[2], at[1], at[0]] = 9
    for k in range(3):                                              # a staircase of face steps inside A
        while at[k] != end[k]:
            at[k] += 1 if end[k] > at[k] else -1
            G[at[2], at[1], at[0]] = 9
    return point(n, start), G


def steps_of(name):
    return sum(1 for c in name if c in "+-")


SEAM_POINTS = [(31, 5, 5), (32, 40, 21), (5, 15, 40), (40, 16, 9), (9, 9, 31), (50, 50, 32), (31, 15, 15), (32, 16, 16), (31, 16, 47), (0, 0, 0),
               (63, 63, 63), (30, 14, 14), (33, 17, 17)]


def comb_field():
    """(F, G, steps) at n = 32: geodesic_ref.comb()'s maze as G (walls 0, corridors 5) with one marker at its end"""
    import geodesic_ref
    maze, _, steps = geodesic_ref.comb()
    G = np.where(maze, 5, 0).astype(np.uint32)
    F = np.zeros_like(G)
    assert maze[5, 0, 30] and not maze[5, 0, 29]                    # the last corridor is entered at y = 15 and ends at y = 0
    F[5, 0, 30] = TOP
    return F, G, steps


def serpentine_field(n):
    """(F, G): geodesic_ref.serpentine's solid as G = 3 (walls 0), one marker of 2 at its start"""
    import geodesic_ref
    solid, seed = geodesic_ref.serpentine(n)
    return np.where(seed, 2, 0).astype(np.uint32), np.where(solid, 3, 0).astype(np.uint32)


def _case(name):
    """(F, G, domain or None)"""
    if name.startswith("gate "):
        return gate(name[5:]) + (None,)
    if name == "comb":
        return comb_field()[:2] + (None,)
    if name.startswith("serpentine "):
        return serpentine_field(int(name[11:])) + (None,)
    if name == "seams":
        G = smooth_field(64, 5, 40) + 1
        F = np.zeros_like(G)
        for k, (x, y, z) in enumerate(SEAM_POINTS):
            F[z, y, x] = 8 + 3 * k
        return F, G, None
    if name in ("plateaus", "plateaus from above"):                 # seven levels: wide plateaus; the marker touches G on a few voxels
        G = smooth_field(64, 6, 6)
        away = TOP if name == "plateaus from above" else 0         # (for reconstruction by erosion)
        return np.where(field(64, 7, 400) == 0, G, away).astype(np.uint32), G, field(64, 8, 1, 1.0) + field(64, 9, 1) > 0
    if name == "random 32":
        return field(32, 1, 255, 0.05), field(32, 2, 255), field(32, 3, 9) > 0
    if name == "random 96":
        return field(96, 4, 1000, 0.01), smooth_field(96, 5, 900), None
    if name == "ends":
        ends = np.array([0, 1, TOP - 1, TOP], np.uint32)
        rng = np.random.default_rng(21)
        return ends[rng.integers(0, 4, (32, 32, 32))], ends[rng.integers(0, 4, (32, 32, 32))], rng.random((32, 32, 32)) < 0.9
    if name == "empty domain":
        return field(32, 30, 9), field(32, 31, 9), np.zeros((32, 32, 32), bool)
    if name == "zero marker":
        return np.zeros((32, 32, 32), np.uint32), field(32, 32, 9), None
    if name == "marker above":
        G = field(32, 33, 9)
        return G + field(32, 34, 5), G, None
    raise KeyError(name)


CASES = (["gate " + k for k in GATES] + ["comb", "serpentine 64", "serpentine 96", "seams", "plateaus", "plateaus from above", "random 32", "random 96", "ends", "empty domain",
         "zero marker", "marker above"])


@functools.lru_cache(maxsize=None)
def case(name):
    out = []
    for a in _case(name):
        if a is not None:
            a = np.ascontiguousarray(a)
            a.setflags(write=False)
        out.append(a)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(name, mode, conn):
    """(R, stats) of a named case by the queue form, computed once and shared, read-only"""
    r, st = reconstruct_queue(*case(name), mode, conn)
    r.setflags(write=False)
    return r, st


EXTREMA_CASES = {
    # name: (values, domain, scale)
    "hills": lambda: (smooth_field(64, 11, 30), None, LINEAR),
    "hills domain": lambda: (smooth_field(64, 12, 12), field(64, 13, 7) > 0, LINEAR),
    "ends": lambda: (np.array([0, 1, TOP - 1, TOP], np.uint32)[np.random.default_rng(14).integers(0, 4, (32, 32, 32))], None, LINEAR),
    "sqrt": lambda: (field(32, 15, TOP), None, SQRT16),
    "balls": lambda: (three_balls()[1], three_balls()[0], SQRT16),
}


@functools.lru_cache(maxsize=None)
def extrema_case(name):
    v, d, s = EXTREMA_CASES[name]()
    return np.ascontiguousarray(v), d, s


@functools.lru_cache(maxsize=None)
def extrema_expected(name, kind, h, conn):
    v, d, s = extrema_case(name)
    return extrema(v, d, kind, s, h, conn)


def isqrt16_python(v):
    return math.isqrt(int(v) << 8)
