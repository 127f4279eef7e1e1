"""The contract of vp_watershed (include/vphip.h) restated in numpy, and the cases of tests/test_watershed_cpu.py / test_watershed_gpu.py
(helpers, no tests).  Grids are (z, y, x) arrays, outside counts as not in the mask.

  watershed_literal(...)   the definition word for word: per present level whole-array breadth-first layers, the minimum of the keys
                           (source level << 32 | label) over the neighbours of every voxel by shifted copies.  Slow; n = 32.
  watershed(...)           the same layers on index lists of a grid padded by one layer.  It starts a level from the labelled neighbours of
                           the voxels whose level IS h: level h - 1 ended with every voxel of its set A that a labelled voxel touches
                           labelled, so every path of level h passes a voxel of level h first.  test_watershed_cpu.py pins it to the
                           literal form.
  cut_of(W, conn)          the cut grid;  stats_of(...)  the four statistics
and the solids: balls, seams, the snake, the diagonal chain, random masks; the limits of the key (LIMITS): priorities up to 2^32 - 1 with
every rank up to 16383 and the extreme labels at once, quanta of 2^31 and more, blocks that are flooded only through a seam, and the comb
maze that outlasts the sweep cap of the TILED kernel."""
import functools

import numpy as np

from fill_ref import bool_to_words, words_to_bool  # noqa: F401

ASCENDING, DESCENDING = 0, 1
LABEL_MAX = (1 << 20) - 1
MAX_SPAN = 16384
_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def offsets(conn):
    """[(dx, dy, dz)] of the neighbours"""
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                k = abs(dx) + abs(dy) + abs(dz)
                if k == 1 or (k > 1 and conn == 26):
                    out.append((dx, dy, dz))
    assert len(out) == conn
    return out


def ranks(mask, priority, order, q):
    """(rank int64 (z, y, x): the level of every voxel counted in flood order from the first level present in M, 0 everywhere in zones mode;
    the number of distinct levels present in M)"""
    mask = np.asarray(mask, bool)
    if priority is None or not mask.any():
        return np.zeros(mask.shape, np.int64), int(mask.any())
    assert q >= 1 and order in (ASCENDING, DESCENDING)
    level = np.asarray(priority).astype(np.int64) // q
    lo, hi = int(level[mask].min()), int(level[mask].max())
    assert hi - lo < MAX_SPAN, "the span is refused: smallest quantum %d" % fitting_quantum(priority, mask, q)
    rank = hi - level if order == DESCENDING else level - lo
    return rank, int(np.unique(level[mask]).size)


def fitting_quantum(priority, mask, q):
    """the smallest quantum >= q whose levels over M span less than MAX_SPAN"""
    p = np.asarray(priority).astype(np.int64)[np.asarray(mask, bool)]
    lo, hi = int(p.min()), int(p.max())
    while hi // q - lo // q >= MAX_SPAN:
        q += 1
    return q


def cut_of(W, conn):
    """bit v: W(v) != 0 and no neighbour has a larger label"""
    n = W.shape[0]
    p = np.pad(W, 1)
    top = np.zeros_like(W)
    for dx, dy, dz in offsets(conn):
        top = np.maximum(top, p[1 + dz:1 + dz + n, 1 + dy:1 + dy + n, 1 + dx:1 + dx + n])
    return (W != 0) & (top <= W)


def stats_of(mask, markers, W, cut, levels):
    used = int(((np.asarray(markers) != 0) & np.asarray(mask, bool)).sum())
    labelled = int((W != 0).sum())
    return (used, labelled, int(levels), labelled - int(cut.sum()))


def _finish(mask, markers, W, conn, levels):
    W = W.astype(np.uint32)
    cut = cut_of(W, conn)
    return W, cut, stats_of(mask, markers, W, cut, levels)


def watershed_literal(mask, markers, priority=None, order=DESCENDING, q=1, conn=6):
    mask = np.asarray(mask, bool)
    n = mask.shape[0]
    rank, levels = ranks(mask, priority, order, q)
    used = mask & (np.asarray(markers) != 0)
    assert int(np.asarray(markers)[used].max(initial=0)) <= LABEL_MAX
    W = np.where(used, markers, 0).astype(np.uint64)
    for h in (np.unique(rank[mask]) if used.any() else ()):
        A = mask & (W == 0) & (rank <= h)
        front = np.where(W != 0, (rank.astype(np.uint64) << np.uint64(32)) | W, _NONE)
        while True:
            p = np.pad(front, 1, constant_values=_NONE)
            best = np.full(W.shape, _NONE, np.uint64)
            for dx, dy, dz in offsets(conn):
                best = np.minimum(best, p[1 + dz:1 + dz + n, 1 + dy:1 + dy + n, 1 + dx:1 + dx + n])
            new = A & (best != _NONE)
            if not new.any():
                break
            W[new] = best[new] & np.uint64(0xFFFFFFFF)
            A &= ~new
            front = np.where(new, best, _NONE)
    return _finish(mask, markers, W, conn, levels)


def watershed(mask, markers, priority=None, order=DESCENDING, q=1, conn=6):
    """(W uint32 (z, y, x), cut bool, stats)"""
    mask = np.asarray(mask, bool)
    n = mask.shape[0]
    p = n + 2
    rank3, levels = ranks(mask, priority, order, q)
    m = np.pad(mask, 1).reshape(-1)
    rank = np.pad(rank3, 1).reshape(-1)
    used = mask & (np.asarray(markers) != 0)
    assert int(np.asarray(markers)[used].max(initial=0)) <= LABEL_MAX
    W = np.pad(np.where(used, markers, 0).astype(np.int64), 1).reshape(-1)
    off = np.array([dx + p * (dy + p * dz) for dx, dy, dz in offsets(conn)], np.int64)
    inside = np.flatnonzero(m)
    inside = inside[np.argsort(rank[inside], kind="stable")]       # the voxels of M level by level
    bounds = np.flatnonzero(np.r_[True, rank[inside][1:] != rank[inside][:-1], True]) if len(inside) else [0]
    for a, b in zip(bounds[:-1], bounds[1:]) if used.any() else ():
        h = int(rank[inside[a]])
        fresh = inside[a:b]
        fresh = fresh[W[fresh] == 0]
        if not len(fresh):
            continue
        front = np.unique((fresh[:, None] + off[None, :]).reshape(-1))
        front = front[W[front] != 0]
        key = (rank[front] << 32) | W[front]
        while len(front):
            to = (front[:, None] + off[None, :]).reshape(-1)
            k = np.repeat(key, len(off))
            ok = m[to] & (W[to] == 0) & (rank[to] <= h)
            to, k = to[ok], k[ok]
            if not len(to):
                break
            o = np.lexsort((k, to))                                # by voxel, then by key: the first of every voxel is its minimum
            to, k = to[o], k[o]
            first = np.r_[True, to[1:] != to[:-1]]
            front, key = to[first], k[first]
            W[front] = key & 0xFFFFFFFF
    return _finish(mask, markers, W.reshape(p, p, p)[1:-1, 1:-1, 1:-1], conn, levels)


# ---- solids --------------------------------------------------------------------------------------------------------------------------
def ball(n, c, r):
    z, y, x = np.ogrid[:n, :n, :n]
    return (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= r * r


def power(n, c, r):
    """the power of every voxel with respect to the sphere: the radical plane of two spheres is where their powers are equal"""
    z, y, x = np.ogrid[:n, :n, :n]
    return (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 - r * r + np.zeros((n, n, n), np.int64)


def marker_volume(n, voxels):
    """voxels: [((x, y, z), label)]"""
    L = np.zeros((n, n, n), np.uint32)
    for (x, y, z), label in voxels:
        L[z, y, x] = label
    return L


def inside_d2(mask):
    """the exact squared distance to the nearest voxel outside the mask (tests/edt_ref.py: vp_edt's UNSET seeds)"""
    import edt_ref
    return edt_ref.edt_numpy(np.asarray(mask, bool), edt_ref.UNSET)


EQUAL_BALLS = (((22, 32, 32), 14), ((42, 32, 32), 14))
UNEQUAL_BALLS = (((20, 32, 32), 15), ((42, 30, 33), 10))


def two_balls(balls, swapped=False):
    """(mask, markers, D^2, side): two balls at n = 64 with one-voxel markers 1 and 2 at their centres (2 and 1 when swapped); side = the label
    of the ball on whose side of the radical plane a voxel lies, the plane itself going to label 1"""
    (c1, r1), (c2, r2) = balls
    mask = ball(64, c1, r1) | ball(64, c2, r2)
    a, b = (2, 1) if swapped else (1, 2)
    one, two = (power(64, c2, r2), power(64, c1, r1)) if swapped else (power(64, c1, r1), power(64, c2, r2))
    side = np.where(one <= two, 1, 2).astype(np.uint32)
    return mask, marker_volume(64, [(c1, a), (c2, b)]), inside_d2(mask), side


def snake(n=32):
    """(mask, the voxels of the path in order): a one-voxel-wide face-connected path -- a comb of pitch 2 over the whole plane z = 8, then a
    column up to z = 24: through every block of the plane and across the z seam"""
    path = []
    for k, x in enumerate(range(0, n, 2)):
        ys = range(n) if k % 2 == 0 else range(n - 1, -1, -1)
        path += [(x, y, 8) for y in ys]
        if x + 2 < n:
            path.append((x + 1, path[-1][1], 8))
    x, y, _ = path[-1]
    path += [(x, y, z) for z in range(9, 25)]
    mask = np.zeros((n, n, n), bool)
    for x, y, z in path:
        mask[z, y, x] = True
    assert int(mask.sum()) == len(path)
    return mask, path


def _random(n, density, pmax, seed):
    rng = np.random.default_rng([n, int(density * 10), pmax, seed])
    mask = rng.random((n, n, n)) < density
    P = rng.integers(0, pmax + 1, (n, n, n)).astype(np.uint32)
    L = np.zeros((n, n, n), np.uint32)
    at = rng.choice(n ** 3, 12, replace=False)
    L.reshape(-1)[at] = rng.integers(1, 6, 12)
    return mask, L, P


RANDOM = [(n, d, pmax, seed) for n in (32, 64) for d in (0.3, 0.7) for pmax in (3, 255) for seed in (1, 2, 3)]


def random_name(n, d, pmax, seed, q, order):
    return "random %d %.1f %d %d q%d %s" % (n, d, pmax, seed, q, "asc" if order == ASCENDING else "desc")


# markers on the seams of the 32 x 16 x 16 block lattice at n = 64: face, edge and corner voxels on both sides, one label each
SEAM_MARKERS = [((31, 5, 5), 1), ((32, 40, 21), 2), ((5, 15, 40), 3), ((40, 16, 9), 4), ((9, 9, 31), 5), ((50, 50, 32), 6),      # faces
                ((9, 15, 15), 7), ((32, 20, 16), 8), ((31, 16, 40), 9),                                                              # edges
                ((31, 15, 47), 10), ((32, 48, 48), 11)]                                                                              # corners


# ---- the limits of the key: priorities near 2^32, every rank up to 16383, the extreme labels at once -----------------------------------
TOP = 0xFFFFFFFF
EXTREME_LABELS = (1, 2, LABEL_MAX - 1, LABEL_MAX)


def _limit_mask_and_markers(n, rng):
    """a random mask of density 0.7 and 12 marker voxels inside it, three of each of EXTREME_LABELS"""
    mask = rng.random((n, n, n)) < 0.7
    L = np.zeros(n ** 3, np.uint32)
    L[rng.choice(np.flatnonzero(mask), 12, replace=False)] = rng.permutation(np.repeat(EXTREME_LABELS, 3))
    return mask, L.reshape(n, n, n)


def wide(n, seed, q, top, present, span=MAX_SPAN - 1):
    """(mask, markers, P): the levels of M are `present` distinct values (fewer where the mask has too few voxels) of first .. first + span
    with both ends among them, first = top // q - span; P = level * q + a random remainder, clipped to top: the largest level of M is
    exactly top // q, and with the default span the rank field takes both 0 and 16383"""
    rng = np.random.default_rng([n, seed, q % (1 << 32), top, present, span])
    mask, L = _limit_mask_and_markers(n, rng)
    assert 2 <= present <= span + 1 and top // q >= span
    inner = 1 + rng.choice(span - 1, present - 2, replace=False)
    level = np.r_[0, span, inner][rng.integers(0, present, n ** 3)].astype(np.int64)
    at = rng.choice(np.flatnonzero(mask), 2, replace=False)
    level[at] = 0, span                                             # both ends are in M whatever the draw
    first = top // q - span
    P = np.minimum((first + level) * q + rng.integers(0, q, n ** 3), top)
    assert int(P.min()) >= 0 and int(P.max()) <= TOP
    return mask, L, P.astype(np.uint32).reshape(n, n, n)


def huge_quantum(n, seed, q):
    """(mask, markers, P): a quantum of 2^31 or more -- two levels -- with P from the values around 0, q and 2^32"""
    rng = np.random.default_rng([n, seed, q % (1 << 32), q >> 32])
    mask, L = _limit_mask_and_markers(n, rng)
    values = np.array(sorted({0, 1, q - 1, q, min(q + 1, TOP), TOP - 1, TOP}), np.int64)
    P = values[rng.integers(0, len(values), n ** 3)]
    at = rng.choice(np.flatnonzero(mask), 2, replace=False)
    P[at] = 0, TOP
    return mask, L, P.astype(np.uint32).reshape(n, n, n)


SECOND_WRAP = 5 * MAX_SPAN + 9000                                   # a first level whose bit lies in the middle of the presence bitmap
# (q, top, present): P up to 2^32 - 1 at q = 1 (few levels: the literal form runs it; every level the mask can hold), at q = 3 (the first
# level is 0x55555555 - 16383: the index into the presence bitmap wraps) and at q = 2^18 (P covers nearly all of uint32), and a wrap
# far from the top
WIDE = [(1, TOP, 256), (1, TOP, MAX_SPAN), (3, TOP, 256), (3, TOP, 4096), (1 << 18, TOP, 4096), (1, SECOND_WRAP + MAX_SPAN - 1, 4096)]
HUGE_QUANTA = [1 << 31, (1 << 31) + 1, TOP]
LITERAL_LEVELS = 256                                                # watershed_literal takes minutes on thousands of levels


def wide_name(q, top, present, order):
    return "wide q%d top%d p%d %s" % (q, top, present, "asc" if order == ASCENDING else "desc")


# ---- gates: a full block that the flood enters through a seam at a level none of its own voxels has --------------------------------------
GATE_A = (0, 1, 1)                                                  # the block (bx, by, bz) with the marker, of 32 x 16 x 16 voxels at n = 64
GATES = {"+x": (1, 1, 1), "-y": (0, 0, 1), "+y": (0, 2, 1), "-z": (0, 1, 0), "+z": (0, 1, 2),                 # five faces
         "edge xy": (1, 2, 1), "edge xz": (1, 1, 0), "edge yz": (0, 0, 2), "corner ++": (1, 2, 2), "corner --": (1, 0, 0)}
TWO_FRONTS = {"y": ((0, 0, 1), (0, 1, 1), (0, 2, 1)), "z": ((0, 1, 0), (0, 1, 1), (0, 1, 2))}   # A, B between them, C


def block_box(b):
    """the (z, y, x) slices of block (bx, by, bz)"""
    return slice(16 * b[2], 16 * b[2] + 16), slice(16 * b[1], 16 * b[1] + 16), slice(32 * b[0], 32 * b[0] + 32)


def gate(blocks, markers, order):
    """(mask, markers, P) at n = 64: blocks = [A, B] or [A, B, C], all full; A and C hold P = 5 (ascending) or 0xFFFFFFF0 (descending) and a
    marker each, B holds 0 or 0xFFFFFFFF: B's own level runs first and floods nothing, and at the level of A no voxel of B has that level"""
    m = np.zeros((64,) * 3, bool)
    P = np.zeros((64,) * 3, np.uint32)
    for k, b in enumerate(blocks):
        m[block_box(b)] = True
        P[block_box(b)] = (0 if order == ASCENDING else TOP) if k == 1 else (5 if order == ASCENDING else 0xFFFFFFF0)
    voxels = []
    for b, ((dx, dy, dz), label) in zip((blocks[0],) + tuple(blocks[2:]), markers):
        voxels.append(((32 * b[0] + dx, 16 * b[1] + dy, 16 * b[2] + dz), label))
    return m, marker_volume(64, voxels), P


def comb_case(flood):
    """the comb maze of geodesic_ref inside one block, 271 voxels and 270 face steps, with one marker at its start; the flood has three
    levels that come back along the path"""
    import geodesic_ref
    m, start, _ = geodesic_ref.comb()
    L = np.where(start, 7, 0).astype(np.uint32)
    if not flood:
        return m, L, None
    d = geodesic_ref.geodesic(m, start, geodesic_ref.GEO_6)[0].astype(np.int64)
    return m, L, np.where(m, (d // 100) % 3, 0).astype(np.uint32)


def _case(name):
    """(mask, markers, priority or None, order, q) -- the connectivity is the caller's"""
    w = name.split()
    order = ASCENDING if w[-1] == "asc" else DESCENDING
    if w[0] == "wide":
        q, top, present = int(w[1][1:]), int(w[2][3:]), int(w[3][1:])
        return wide(32, 1, q, top, present) + (order, q)
    if w[0] == "quantum":
        return huge_quantum(32, 2, int(w[1])) + (order, int(w[1]))
    if w[0] == "gate":
        return gate([GATE_A, GATES[" ".join(w[1:-1])]], [((5, 3, 9), 9)], order) + (order, 1)
    if name.startswith("two fronts"):
        return gate(TWO_FRONTS[w[2]], [((5, 3, 9), 9), ((20, 11, 2), 4)], order) + (order, 1)
    if w[0] == "comb":
        return comb_case(w[1] == "flood") + (ASCENDING, 1)
    if name.startswith("equal balls"):
        m, L, P, _ = two_balls(EQUAL_BALLS)
        return m, L, P, DESCENDING, 1
    if name.startswith("unequal balls"):
        m, L, P, _ = two_balls(UNEQUAL_BALLS, swapped=name.endswith("swapped"))
        return m, L, P, DESCENDING, 1
    if name.startswith("seams"):
        full = np.ones((64,) * 3, bool)
        L = marker_volume(64, SEAM_MARKERS)
        if w[1] == "zones":
            return full, L, None, DESCENDING, 1
        z, y, x = np.ogrid[:64, :64, :64]
        return full, L, ((x * 7 + y * 5 + z * 3) % 11 + np.zeros((64,) * 3, np.int64)).astype(np.uint32), ASCENDING, 1
    if name == "interface along a seam":                            # equidistant from z = 15 | 16, the seam plane of n = 32
        return np.ones((32,) * 3, bool), marker_volume(32, [((16, 8, 10), 1), ((16, 8, 21), 2)]), None, DESCENDING, 1
    if name == "interface across a corner":                         # the bisector passes through the block corner (32, 16, 16)
        return np.ones((64,) * 3, bool), marker_volume(64, [((20, 10, 10), 2), ((44, 22, 22), 1)]), None, DESCENDING, 1
    if name.startswith("snake"):
        m, path = snake()
        L = marker_volume(32, [(path[0], 2), (path[-1], 1)])
        if w[1] == "zones":
            return m, L, None, DESCENDING, 1
        P = np.zeros((32,) * 3, np.uint32)
        for k, (x, y, z) in enumerate(path):
            P[z, y, x] = (k // 40) % 5                               # plateaus of 40 voxels: long hops inside a level, levels that come back
        return m, L, P, ASCENDING, 1
    if name == "diagonal chain":
        m = np.zeros((32,) * 3, bool)
        for k in range(32):
            m[k, k, k] = True
        return m, marker_volume(32, [((0, 0, 0), 3), ((31, 31, 31), 1)]), None, DESCENDING, 1
    if name.startswith("random"):
        n, d, pmax, seed, q = int(w[1]), float(w[2]), int(w[3]), int(w[4]), int(w[5][1:])
        m, L, P = _random(n, d, pmax, seed)
        return m, L, P, ASCENDING if w[6] == "asc" else DESCENDING, q
    if name == "labels 1 and max":
        m, L, P = _random(32, 0.7, 3, 9)
        L = marker_volume(32, [(tuple(int(v) for v in np.argwhere(m)[5][::-1]), 1), (tuple(int(v) for v in np.argwhere(m)[-5][::-1]), LABEL_MAX)])
        return m, L, P, DESCENDING, 1
    if name == "empty mask":
        _, L, P = _random(32, 0.5, 3, 10)
        return np.zeros((32,) * 3, bool), L, P, ASCENDING, 1
    if name == "no markers":
        m, _, P = _random(32, 0.5, 3, 11)
        return m, np.zeros((32,) * 3, np.uint32), P, ASCENDING, 1
    if name == "markers outside":
        m, _, P = _random(32, 0.5, 3, 12)
        return m, np.where(m, 0, 7).astype(np.uint32), P, ASCENDING, 1
    if name == "markers cover the mask":
        m, _, P = _random(32, 0.5, 255, 13)
        return m, (np.arange(32 ** 3, dtype=np.uint32).reshape((32,) * 3) % 9 + 1), P, DESCENDING, 7
    if name == "not a power of two":
        m = ball(96, (40, 48, 48), 30) | ball(96, (70, 50, 46), 20)
        z, y, x = np.ogrid[:96, :96, :96]
        P = ((x + 2 * y + 3 * z) % 6 + np.zeros((96,) * 3, np.int64)).astype(np.uint32)
        return m, marker_volume(96, [((40, 48, 48), 2), ((70, 50, 46), 1), ((95, 95, 95), 3)]), P, DESCENDING, 1
    raise KeyError(name)


HAND = ["equal balls", "unequal balls", "unequal balls swapped", "seams zones", "seams flood", "interface along a seam", "interface across a corner",
        "snake zones", "snake flood", "diagonal chain", "labels 1 and max", "empty mask", "no markers", "markers outside", "markers cover the mask",
        "not a power of two"]
# every random mask with both quanta and both orders, spread so that each mask runs two of the four combinations and each combination
# meets every side, density and range of P
RANDOMS = [random_name(n, d, pmax, seed, q, order) for k, (n, d, pmax, seed) in enumerate(RANDOM)
           for q, order in (((1, ASCENDING), (7, DESCENDING)) if (k + k // 3) % 2 == 0 else ((7, ASCENDING), (1, DESCENDING)))]
ORDERS = (ASCENDING, DESCENDING)
WIDES = [wide_name(q, top, present, order) for q, top, present in WIDE for order in ORDERS]
QUANTA = ["quantum %d %s" % (q, o) for q in HUGE_QUANTA for o in ("asc", "desc")]
GATE_CASES = ["gate %s %s" % (k, o) for k in GATES for o in ("asc", "desc")] + ["two fronts %s %s" % (k, o) for k in TWO_FRONTS for o in ("asc", "desc")]
COMBS = ["comb zones", "comb flood"]
LIMITS = WIDES + QUANTA + GATE_CASES + COMBS
CASES = HAND + RANDOMS + LIMITS
CONNS = (6, 26)


def has_literal(name):
    """whether watershed_literal is run on the case: side 32 and few levels, and the gates at side 64 (two levels, short paths)"""
    if name.startswith("wide"):
        return int(name.split()[3][1:]) <= LITERAL_LEVELS
    return case(name)[0].shape[0] == 32 or name in GATE_CASES


@functools.lru_cache(maxsize=None)
def case(name):
    m, L, P, order, q = _case(name)
    out = [np.ascontiguousarray(m, bool), np.ascontiguousarray(L, np.uint32), None if P is None else np.ascontiguousarray(P, np.uint32)]
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out[0], out[1], out[2], order, q


@functools.lru_cache(maxsize=None)
def expected(name, conn):
    """(W, cut, stats) of a named case by the reference, computed once and shared, read-only"""
    m, L, P, order, q = case(name)
    W, cut, stats = watershed(m, L, P, order, q, conn)
    W.setflags(write=False)
    cut.setflags(write=False)
    return W, cut, stats
