"""The contract of vp_skeleton (include/vphip.h) restated in numpy: grids are (z, y, x) bool arrays, outside counts as empty.

  simple_shift(m)   the shift form over arrays of 27-bit masks (bit i = (dx+1) + 3 (dy+1) + 9 (dz+1))
  simple_plain(m)   the definition by a flood fill over coordinates, one mask at a time: the slow second opinion
  thin(vox, ...)    the iteration: border once, eight subfields in ascending order, masks for all candidates of a subfield at once
  thin_words(...)   the same on grid words, cropped to the bounding box at an EVEN offset (subfields are absolute parities), so that
                    sparse 1024^3 grids stay cheap
and the helpers of the tests: Euler characteristic of the closed-cube complex, hand-made solids, random grids."""
import itertools

import numpy as np

from fill_ref import bool_to_words, words_to_bool  # noqa: F401

KERNEL, CURVE = 0, 1
ALL = np.uint32(0x07FFFFFF)
CENTRE = np.uint32(1 << 13)
N26 = ALL & ~CENTRE
OFFSETS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]          # bit i <-> OFFSETS[i]
N6 = np.uint32(sum(1 << i for i, d in enumerate(OFFSETS) if sum(abs(c) for c in d) == 1))
N18 = np.uint32(sum(1 << i for i, d in enumerate(OFFSETS) if 1 <= sum(abs(c) for c in d) <= 2))
SIMPLE_COUNT = 25985144                                                                  # of the 2^26 neighbourhoods
_XLO = np.uint32(sum(1 << i for i, d in enumerate(OFFSETS) if d[0] == -1))
_XHI = np.uint32(sum(1 << i for i, d in enumerate(OFFSETS) if d[0] == 1))
_YLO = np.uint32(sum(1 << i for i, d in enumerate(OFFSETS) if d[1] == -1))
_YHI = np.uint32(sum(1 << i for i, d in enumerate(OFFSETS) if d[1] == 1))
STEPS_A, STEPS_B = 9, 11


def mask_of_index(c):
    """the 27-bit mask of table index c: the 26 non-centre bits packed"""
    c = np.asarray(c, np.uint32)
    return (c & np.uint32(0x1FFF)) | ((c >> np.uint32(13)) << np.uint32(14))


def index_of_mask(m):
    m = np.asarray(m, np.uint32)
    return (m & np.uint32(0x1FFF)) | ((m >> np.uint32(14)) << np.uint32(13))


def _dilate26(r):
    r = r | ((r & ~_XHI) << np.uint32(1)) | ((r & ~_XLO) >> np.uint32(1))
    r = r | ((r & ~_YHI) << np.uint32(3)) | ((r & ~_YLO) >> np.uint32(3))
    return (r | (r << np.uint32(9)) | (r >> np.uint32(9))) & ALL


def _dilate6(r):
    return (r | ((r & ~_XHI) << np.uint32(1)) | ((r & ~_XLO) >> np.uint32(1)) | ((r & ~_YHI) << np.uint32(3)) | ((r & ~_YLO) >> np.uint32(3))
            | (r << np.uint32(9)) | (r >> np.uint32(9))) & ALL


def _lowest(v):
    return v & (~v + np.uint32(1))


def simple_shift(m):
    """bool per mask: the shift form with its fixed step counts"""
    m = np.asarray(m, np.uint32)
    obj, bg = m & N26, ~m & N18
    faces = bg & N6
    a, b = _lowest(obj), _lowest(faces)
    for _ in range(STEPS_A):
        a = _dilate26(a) & obj
    for _ in range(STEPS_B):
        b = _dilate6(b) & bg
    return (obj != 0) & (faces != 0) & (a == obj) & ((faces & ~b) == 0)


def _components(cells, adjacent):
    cells, parts = set(cells), []
    while cells:
        stack, part = [cells.pop()], set()
        while stack:
            c = stack.pop()
            part.add(c)
            for d in cells.copy():
                if adjacent(c, d):
                    cells.discard(d)
                    stack.append(d)
        parts.append(part)
    return parts


def simple_plain(m):
    """one mask: the definition, by flood fills over coordinates"""
    m = int(m)
    obj = [d for i, d in enumerate(OFFSETS) if i != 13 and (m >> i) & 1]
    bg = [d for i, d in enumerate(OFFSETS) if not (m >> i) & 1 and 1 <= sum(abs(c) for c in d) <= 2]
    if not obj or len(_components(obj, lambda p, q: max(abs(a - b) for a, b in zip(p, q)) == 1)) != 1:
        return False
    parts = _components(bg, lambda p, q: sum(abs(a - b) for a, b in zip(p, q)) == 1)
    with_face = [p for p in parts if any(sum(abs(c) for c in d) == 1 for d in p)]
    return len(with_face) == 1


def masks_at(vox, idx):
    """the 27-bit masks of the voxels idx (k x 3: z, y, x) of a grid"""
    p = np.pad(vox, 1)
    m = np.zeros(len(idx), np.uint32)
    for i, (dx, dy, dz) in enumerate(OFFSETS):
        m |= p[idx[:, 0] + 1 + dz, idx[:, 1] + 1 + dy, idx[:, 2] + 1 + dx].astype(np.uint32) << np.uint32(i)
    return m


def popcount(m):
    m = np.ascontiguousarray(m, np.uint32)
    return np.unpackbits(m.reshape(-1, 1).view(np.uint8), axis=1).sum(1).reshape(m.shape)


def deletable(m, mode, plain=False):
    s = np.array([simple_plain(v) for v in m], bool) if plain else simple_shift(m)
    if mode == CURVE:
        s &= popcount(m & N26) != 1
    return s


def border(vox, anchor=None):
    p = np.pad(vox, 1)
    inner = p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1]
    b = vox & ~inner
    return b if anchor is None else b & ~anchor


def thin(vox, mode, max_iters=0, anchor=None, origin=(0, 0, 0), plain=False):
    """(result, (voxels left, iterations, voxels deleted)); origin = the absolute (z, y, x) of vox[0, 0, 0], for the parities"""
    s = vox.copy()
    z, y, x = np.ogrid[:s.shape[0], :s.shape[1], :s.shape[2]]
    sub = ((x + origin[2]) & 1) | (((y + origin[1]) & 1) << 1) | (((z + origin[0]) & 1) << 2)
    iterations = deleted = 0
    while True:
        b = border(s, anchor)
        lost = 0
        for k in range(8):
            idx = np.argwhere(b & s & (sub == k))
            if len(idx):
                d = deletable(masks_at(s, idx), mode, plain)
                idx = idx[d]
                s[idx[:, 0], idx[:, 1], idx[:, 2]] = False
                lost += len(idx)
        iterations += 1
        deleted += lost
        if lost == 0 or iterations == max_iters:
            return s, (int(s.sum()), iterations, deleted)


def thin_words(words, n, mode, max_iters=0, anchor_words=None):
    """the same on the words of a grid of side n: (words, stats); works on the bounding box of the set words, at an even offset"""
    w3 = np.asarray(words, np.uint32).reshape(n, n, n // 32)
    nz = np.nonzero(w3)
    if len(nz[0]) == 0:
        return w3.reshape(-1).copy(), (0, 1, 0)
    lo = [int(c.min()) for c in nz]
    hi = [int(c.max()) + 1 for c in nz]
    lo[0] &= ~1
    lo[1] &= ~1                                                    # x is cropped by whole words: a multiple of 32

    def unpack(a):
        c = np.ascontiguousarray(a[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]])
        return np.unpackbits(c.view(np.uint8), bitorder="little").reshape(c.shape[0], c.shape[1], c.shape[2] * 32).astype(bool)

    anchor = None if anchor_words is None else unpack(np.asarray(anchor_words, np.uint32).reshape(n, n, n // 32))
    res, stats = thin(unpack(w3), mode, max_iters, anchor, origin=(lo[0], lo[1], lo[2] * 32))
    out = np.zeros_like(w3)
    out[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = np.packbits(res, axis=2, bitorder="little").view(np.uint32).reshape(res.shape[0], res.shape[1], -1)
    return out.reshape(-1), stats


# ---- facts ---------------------------------------------------------------------------------------------------------------------------
def euler(vox):
    """Euler characteristic of the union of the closed unit cubes: vertices - edges + faces - cubes"""
    p = np.pad(vox, 1)

    def cells(axes):                                               # cells that extend along the complement of `axes`: OR over the cubes around
        acc = None
        for shift in itertools.product((0, 1), repeat=len(axes)):
            sl = [slice(None)] * 3
            for a, s in zip(axes, shift):
                sl[a] = slice(1, None) if s else slice(None, -1)
            acc = p[tuple(sl)] if acc is None else acc | p[tuple(sl)]
        return int(acc.sum())

    faces = sum(cells((a,)) for a in range(3))
    edges = sum(cells(pair) for pair in ((0, 1), (0, 2), (1, 2)))
    return cells((0, 1, 2)) - edges + faces - int(vox.sum())


def neighbours26(vox):
    """per voxel: its number of set 26-neighbours"""
    p = np.pad(vox, 1).astype(np.uint8)
    n = vox.shape
    acc = np.zeros(n, np.uint8)
    for dx, dy, dz in OFFSETS:
        if (dx, dy, dz) != (0, 0, 0):
            acc += p[1 + dz:1 + dz + n[0], 1 + dy:1 + dy + n[1], 1 + dx:1 + dx + n[2]]
    return acc


def remaining_deletable(vox, mode, anchor=None):
    """the voxels a further examination could delete: simple, no anchor, (curve) no line end -- empty after a run to the end"""
    idx = np.argwhere(vox if anchor is None else vox & ~anchor)
    return idx[deletable(masks_at(vox, idx), mode)] if len(idx) else idx


# ---- solids --------------------------------------------------------------------------------------------------------------------------
def ball(n, c, r2):
    z, y, x = np.ogrid[:n, :n, :n]
    return (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= r2


def box(n, lo, hi):
    """voxels lo <= (x, y, z) < hi"""
    v = np.zeros((n, n, n), bool)
    v[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = True
    return v


def torus(n, c, major, minor):
    z, y, x = np.ogrid[:n, :n, :n]
    q = np.sqrt((x - c[0]) ** 2.0 + (y - c[1]) ** 2.0) - major
    return q * q + (z - c[2]) ** 2.0 <= minor * minor


def random_grid(n, density, seed):
    return np.random.default_rng(seed).random((n, n, n)) < density
