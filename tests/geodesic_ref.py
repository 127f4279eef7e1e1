"""The contract of vp_geodesic (include/vphip.h) restated in numpy, and the cases of tests/test_geodesic_cpu.py / test_geodesic_gpu.py
(helpers, no tests).  Grids are (z, y, x) bool arrays, outside counts as not in the mask.

  geodesic(mask, seeds, metric)   (D uint32 (z, y, x), reach bool, stats): distance levels settled in ascending order -- the voxels with
                                  D = d are final, their allowed neighbours with D > d + w are lowered to d + w -- on index arrays of a
                                  grid padded by one layer, one level per step (Dial's buckets; the weights are at most 5)
  closed_form(n, metric, corner)  D of the full grid from a seed in a corner
and the solids: two boxes in corner / edge contact, the serpentine across blocks, the comb maze inside one block, balls, the torus."""
import functools
import os

import numpy as np

from fill_ref import bool_to_words, words_to_bool  # noqa: F401

GEO_6, GEO_26, GEO_CHAMFER = 0, 1, 2
METRICS = (GEO_6, GEO_26, GEO_CHAMFER)
NONE = 0xFFFFFFFF
MAX = 0xFFFFFFFE
WEIGHTS = {GEO_6: (1, None, None), GEO_26: (1, 1, 1), GEO_CHAMFER: (3, 4, 5)}


def steps(metric):
    """[((dx, dy, dz), w)] of the allowed steps"""
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                k = abs(dx) + abs(dy) + abs(dz)
                if k and WEIGHTS[metric][k - 1] is not None:
                    out.append(((dx, dy, dz), WEIGHTS[metric][k - 1]))
    return out


def stats_of(dist, used):
    """the four statistics of a distance map: seeds used, voxels reached, largest finite D, lowest linear index that attains it"""
    flat = dist.reshape(-1)
    finite = flat != NONE
    reached = int(finite.sum())
    if reached == 0:
        return (0, 0, 0, 0)
    top = int(flat[finite].max())
    return (int(used), reached, top, int(np.flatnonzero(flat == top)[0]))


def geodesic(mask, seeds, metric):
    n = mask.shape[0]
    p = n + 2
    m = np.pad(np.asarray(mask, bool), 1).reshape(-1)
    used = np.pad(np.asarray(seeds, bool) & np.asarray(mask, bool), 1).reshape(-1)
    d = np.full(p ** 3, NONE, np.int64)
    off = [(dx + p * (dy + p * dz), w) for (dx, dy, dz), w in steps(metric)]
    front = np.flatnonzero(used)
    d[front] = 0
    buckets = {0: [front]} if len(front) else {}
    level = 0
    while buckets:
        if level not in buckets:
            level = min(buckets)
        idx = np.unique(np.concatenate(buckets.pop(level)))
        idx = idx[d[idx] == level]                                 # the others were lowered after they were listed
        for o, w in off:
            t = min(level + w, MAX)
            q = idx + o
            q = q[m[q] & (d[q] > t)]
            if len(q):
                d[q] = t
                buckets.setdefault(t, []).append(q)
        level += 1
    dist = d.reshape(p, p, p)[1:-1, 1:-1, 1:-1].astype(np.uint32)
    return dist, dist != NONE, stats_of(dist, used.sum())


def closed_form(n, metric, corner=0):
    """D of the full grid of side n from the seed (0, 0, 0) (corner = 0) or (n - 1, n - 1, n - 1)"""
    z, y, x = np.meshgrid(*(np.arange(n),) * 3, indexing="ij")
    c = np.sort(np.stack([x, y, z] if corner == 0 else [n - 1 - x, n - 1 - y, n - 1 - z]), axis=0)
    lo, mid, hi = c[0], c[1], c[2]
    if metric == GEO_6:
        return (lo + mid + hi).astype(np.uint32)
    if metric == GEO_26:
        return hi.astype(np.uint32)
    return (3 * (hi - mid) + 4 * (mid - lo) + 5 * lo).astype(np.uint32)


# ---- solids --------------------------------------------------------------------------------------------------------------------------
def box(n, lo, hi):
    """voxels lo <= (x, y, z) < hi"""
    v = np.zeros((n, n, n), bool)
    v[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = True
    return v


def voxel(n, x, y, z):
    return box(n, (x, y, z), (x + 1, y + 1, z + 1))


def ball(n, c, r2):
    z, y, x = np.ogrid[:n, :n, :n]
    return (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= r2


def torus(n, c, major, minor):
    z, y, x = np.ogrid[:n, :n, :n]
    q = np.sqrt((x - c[0]) ** 2.0 + (y - c[1]) ** 2.0) - major
    return q * q + (z - c[2]) ** 2.0 <= minor * minor


def random_grid(n, density, seed):
    return np.random.default_rng(seed).random((n, n, n)) < density


def contact(kind):
    """(mask, seeds, second box) at n = 64: two boxes of side 16 that touch only at a corner or along an edge, on a word boundary in x that is
    a block seam in y and z ("corner", "edge") or inside the first block column ("corner in", "edge in"); the seed is in the first box"""
    n = 64
    a = {"corner": (16, 16, 16), "edge": (16, 16, 16), "corner in": (16, 0, 0), "edge in": (16, 0, 0)}[kind]
    first = box(n, a, (a[0] + 16, a[1] + 16, a[2] + 16))
    b = (a[0] + 16, a[1] + 16, a[2] + (16 if kind.startswith("corner") else 0))
    second = box(n, b, (b[0] + 16, b[1] + 16, b[2] + 16))
    return first | second, voxel(n, a[0] + 3, a[1] + 5, a[2] + 2), second


def serpentine(n):
    """(mask, seeds): the full grid with every fourth z plane (z = 3, 7, ...) cleared except one x row, at y = n - 1 and y = 0 alternately"""
    v = np.ones((n, n, n), bool)
    for k, z in enumerate(range(3, n, 4)):
        v[z] = False
        v[z, 0 if k % 2 else n - 1, :] = True
    return v, voxel(n, 0, 0, 0)


SERPENTINE_MAX = {32: {GEO_6: 310, GEO_26: 248, GEO_CHAMFER: 806}, 64: {GEO_6: 1134, GEO_26: 1008, GEO_CHAMFER: 3150}}
SERPENTINE_VOXELS = {32: 24832, 64: 197632}


def comb(z=5):
    """(mask, seeds, steps) at n = 32: a pitch-2 comb confined to the block x < 32, y < 16, z < 16, in the plane z -- corridors along y at even
    x, joined at y = 15 and y = 0 alternately; the seed is at its start and `steps` the face steps to its end"""
    n = 32
    v = np.zeros((n, n, n), bool)
    for k, x in enumerate(range(0, 32, 2)):
        v[z, 0:16, x] = True
        if x + 2 < 32:
            v[z, 15 if k % 2 == 0 else 0, x + 1] = True
    return v, voxel(n, 0, 0, z), 16 * 15 + 15 * 2


def lowest_plane(mask):
    """the set voxels of the lowest occupied z plane"""
    z = int(np.flatnonzero(mask.any(axis=(1, 2)))[0])
    s = np.zeros_like(mask)
    s[z] = mask[z]
    return s


def highest_plane(mask):
    z = int(np.flatnonzero(mask.any(axis=(1, 2)))[-1])
    s = np.zeros_like(mask)
    s[z] = mask[z]
    return s


# ---- the cases of the GPU tests, which the C++ host form runs as well ----------------------------------------------------------------------
def bunny64():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bunny_decimated_n64.grid.u32")
    return words_to_bool(np.fromfile(path, np.uint32), 64)


RANDOM_SPARSE = (32, 0.25, 7)                                      # random_grid arguments: a mask with voxels that no seed reaches


def two_balls():
    """two balls at n = 32 that no face step joins"""
    return ball(32, (10, 10, 10), 30), ball(32, (17, 17, 17), 30)


def _case(name):
    if name.startswith("contact "):
        return contact(name[8:])[:2]
    if name.startswith("serpentine "):
        return serpentine(int(name[11:]))
    if name == "comb":
        return comb()[:2]
    if name.startswith("torus"):
        t = torus(64, (32, 32, 32), 20, 6)
        return t, voxel(64, 52, 32, 32) | (voxel(64, 12, 32, 32) if name == "torus two seeds" else False)
    if name == "bunny":
        return bunny64(), lowest_plane(bunny64())
    if name == "seeds outside":
        m = random_grid(32, 0.5, 11)
        return m, ~m & random_grid(32, 0.1, 12)
    if name == "seeds equal mask":
        m = random_grid(32, 0.5, 13)
        return m, m
    if name == "seeds partly inside":
        return random_grid(32, 0.6, 14), random_grid(32, 0.01, 15)
    if name == "two balls":
        a, b = two_balls()
        return a | b, voxel(32, 10, 10, 10)
    if name == "random sparse":
        return random_grid(*RANDOM_SPARSE), random_grid(32, 0.002, 16)
    if name.startswith("full "):
        n, corner = int(name.split()[1]), int(name.split()[2])
        return np.ones((n,) * 3, bool), voxel(n, *((0, 0, 0) if corner == 0 else (n - 1,) * 3))
    if name in SEAMS:
        n, seed, rest = SEAMS[name]
        s = seam_set(n, seed)
        return s | seam_set(n, rest), s
    raise KeyError(name)


def seam_set(n, what):
    """a z plane ("z", k) or a list of voxels"""
    v = np.zeros((n, n, n), bool)
    if what[0] == "z":
        v[what[1]] = True
    else:
        for x, y, z in what:
            v[z, y, x] = True
    return v


# Seeds ON a block seam whose block (32 x 16 x 16 voxels) holds no other voxel of the mask: the seeds read 0 from the start, nothing in their
# block is ever lowered, and the only continuation lies in the block across the face, edge or corner.  name: (n, the seeds, the rest of M)
SEAMS = {
    "seam plane z15": (32, ("z", 15), ("z", 16)), "seam plane z16": (32, ("z", 16), ("z", 15)),
    "seam x31": (64, [(31, 5, 5)], [(32, 5, 5)]), "seam x32": (64, [(32, 5, 5)], [(31, 5, 5)]),
    "seam y15": (64, [(5, 15, 5)], [(5, 16, 5)]), "seam y16": (64, [(40, 16, 20)], [(40, 15, 20)]),
    "seam z31": (64, [(7, 3, 31)], [(7, 3, 32)]),
    "seam edge yz": (64, [(9, 15, 15)], [(9, 16, 16)]), "seam edge xz": (64, [(32, 20, 16)], [(31, 20, 15)]),
    "seam edge xy": (64, [(31, 16, 40)], [(32, 15, 40)]),
    "seam corner 31": (64, [(31, 15, 15)], [(32, 16, 16)]), "seam corner 32": (64, [(32, 16, 16)], [(31, 15, 15)]),
    "seam corner mixed": (64, [(31, 16, 47)], [(32, 15, 48)]),
}

CASES = (["contact " + k for k in ("corner", "edge", "corner in", "edge in")] + ["serpentine 32", "serpentine 64", "comb", "torus one seed",
         "torus two seeds", "bunny", "seeds outside", "seeds equal mask", "seeds partly inside", "two balls", "random sparse",
         "full 32 0", "full 32 1", "full 96 0", "full 96 1"] + list(SEAMS))


@functools.lru_cache(maxsize=None)
def case(name):
    """(mask, seeds) of a named case, read-only"""
    m, s = _case(name)
    m, s = np.ascontiguousarray(m, bool), np.ascontiguousarray(s, bool)
    m.setflags(write=False)
    s.setflags(write=False)
    return m, s


@functools.lru_cache(maxsize=None)
def expected(name, metric):
    """(D, reach, stats) of a named case by the reference, computed once and shared, read-only"""
    d, r, st = geodesic(*case(name), metric)
    d.setflags(write=False)
    r.setflags(write=False)
    return d, r, st
