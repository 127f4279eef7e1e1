"""The contract of vp_watershed (include/vphip.h) restated in numpy, and the cases of tests/test_watershed_cpu.py / test_watershed_gpu.py
(helpers, no tests).  Grids are (z, y, x) arrays, outside counts as not in the mask.

  watershed_literal(...)   the definition word for word: per present level whole-array breadth-first layers, the minimum of the keys
                           (source level << 32 | label) over the neighbours of every voxel by shifted copies.  Slow; n = 32.
  watershed(...)           the same layers on index lists of a grid padded by one layer.  It starts a level from the labelled neighbours of
                           the voxels whose level IS h: level h - 1 ended with every voxel of its set A that a labelled voxel touches
                           labelled, so every path of level h passes a voxel of level h first.  test_watershed_cpu.py pins it to the
                           literal form.
  cut_of(W, conn)          the cut grid;  stats_of(...)  the four statistics
and the solids: balls, seams, the snake, the diagonal chain, random masks."""
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


def _case(name):
    """(mask, markers, priority or None, order, q) -- the connectivity is the caller's"""
    w = name.split()
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
CASES = HAND + RANDOMS
CONNS = (6, 26)


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
