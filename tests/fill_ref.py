"""Interior fill reference and case generators for tests/test_fill_cpu.py and tests/test_fill_gpu.py (helpers, no tests).

fill_numpy(words, n) restates the contract of vp_fill_interior (include/vphip.h) in its plainest form: the exterior E starts as the
empty voxels of the six faces and grows by a masked 6-neighbour dilation, E |= NOT W & (E shifted by one voxel along +-x, +-y, +-z),
until nothing changes; the result is NOT E.  It works on the bit-packed words (voxel (x, y, z) = bit x + n y + n^2 z, LSB first), so
one dilation step is a few array operations, but it takes one step per voxel of the longest flood path: no run fills, no sweeps."""
import numpy as np


def words_to_bool(words, n):
    """(z, y, x) bool array of a whole grid"""
    b = np.unpackbits(np.ascontiguousarray(words, np.uint32).view(np.uint8), bitorder="little")
    return b.reshape(n, n, n).astype(bool)


def bool_to_words(vox):
    n = vox.shape[0]
    return np.packbits(np.ascontiguousarray(vox, bool).reshape(-1), bitorder="little").view(np.uint32).copy().reshape(-1)[: n ** 3 // 32]


def fill_numpy(words, n, return_steps=False):
    w = n // 32
    W = np.asarray(words, np.uint32).reshape(n, n, w)
    P = ~W
    face = np.zeros((n, n, w), np.uint32)
    face[0] = face[-1] = 0xFFFFFFFF
    face[:, 0] = face[:, -1] = 0xFFFFFFFF
    face[:, :, 0] |= np.uint32(1)
    face[:, :, -1] |= np.uint32(0x80000000)
    E = P & face
    steps = 0
    while True:
        nb = (E << np.uint32(1)) | (E >> np.uint32(1))                   # x +- 1 inside a word
        nb[:, :, 1:] |= E[:, :, :-1] >> np.uint32(31)                   # x - 1 neighbour across the word edge (bit 31 -> bit 0)
        nb[:, :, :-1] |= E[:, :, 1:] << np.uint32(31)                   # x + 1 neighbour across the word edge (bit 0 -> bit 31)
        nb[:, 1:] |= E[:, :-1]
        nb[:, :-1] |= E[:, 1:]
        nb[1:] |= E[:-1]
        nb[:-1] |= E[1:]
        new = E | (P & nb)
        steps += 1
        if np.array_equal(new, E):
            break
        E = new
    out = (~E).reshape(-1)
    return (out, steps) if return_steps else out


# ---- generators (seeded) ---------------------------------------------------------------------------------------------------------

def random_grid(n, density, seed):
    rng = np.random.default_rng(seed)
    return bool_to_words(rng.random((n, n, n)) < density)


def box_shell(n, lo, hi, vox=None):
    """set the faces of the box [lo, hi]^3 (inclusive, per axis (x, y, z)); returns the (z, y, x) array"""
    vox = np.zeros((n, n, n), bool) if vox is None else vox
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    vox[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = True
    vox[z0 + 1:z1, y0 + 1:y1, x0 + 1:x1] = False
    return vox


def box_cavity(lo, hi):
    """the voxels strictly inside box_shell(lo, hi), as a (z, y, x) slice tuple"""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    return (slice(z0 + 1, z1), slice(y0 + 1, y1), slice(x0 + 1, x1))


def maze(n, seed, segments=400):
    """A solid grid with one serpentine corridor carved from the x = 0 face: a self-avoiding walk on the lattice of odd coordinates
    that turns after 1-3 lattice steps onto another axis, so a flood along it needs many axis turns.  Walls between corridor cells are
    one voxel thick, and corridors only meet through carved faces.  A few single-voxel cavities away from the corridor are left empty
    (they must be filled).  Returns (words, corridor length in voxels)."""
    rng = np.random.default_rng(seed)
    vox = np.ones((n, n, n), bool)
    m = (n - 1) // 2                                       # lattice cells at 2 i + 1, i in [0, m)
    seen = np.zeros((m, m, m), bool)
    cur = np.array([0, m // 2, m // 2])
    seen[tuple(cur[::-1])] = True
    x, y, z = 2 * cur + 1
    vox[z, y, 0:x + 1] = False                             # the entrance from the x = 0 face
    carved = x + 1
    axis = 0
    for _ in range(segments):
        options = []
        for a in range(3):
            if a == axis:
                continue
            for sgn in (-1, 1):
                for length in (3, 2, 1):
                    ok = True
                    for s in range(1, length + 1):
                        c = cur.copy()
                        c[a] += sgn * s
                        if c[a] < 0 or c[a] >= m or seen[tuple(c[::-1])]:
                            ok = False
                            break
                    if ok:
                        options.append((a, sgn, length))
                        break
        if not options:
            break
        a, sgn, length = options[rng.integers(len(options))]
        for s in range(1, length + 1):
            prev = cur.copy()
            cur[a] += sgn
            seen[tuple(cur[::-1])] = True
            p0, p1 = 2 * prev + 1, 2 * cur + 1
            lo, hi = np.minimum(p0, p1), np.maximum(p0, p1)
            vox[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = False
            carved += 2
        axis = a
    for _ in range(8):                                     # isolated cavities: even coordinates in all three axes touch no corridor
        c = 2 * rng.integers(1, max(2, m - 1), 3)
        if (vox[c[2] - 1:c[2] + 2, c[1], c[0]].all() and vox[c[2], c[1] - 1:c[1] + 2, c[0]].all()
                and vox[c[2], c[1], c[0] - 1:c[0] + 2].all()):
            vox[c[2], c[1], c[0]] = False
    return bool_to_words(vox), carved


def _full_box(n, lo, hi, vox=None):
    vox = np.zeros((n, n, n), bool) if vox is None else vox
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    vox[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = True
    return vox


def hand_cases(n):
    """[(name, input (z, y, x) bool, expected (z, y, x) bool)] -- every expectation written from the construction, not computed"""
    cases = []
    zero = np.zeros((n, n, n), bool)
    cases.append(("empty", zero.copy(), zero.copy()))
    cases.append(("full", ~zero, ~zero))
    lo, hi = (3, 4, 5), (n - 6, n - 5, n - 4)
    shell = box_shell(n, lo, hi)
    cases.append(("shell", shell, _full_box(n, lo, hi)))
    leak = shell.copy()
    leak[n // 2, n // 2, hi[0]] = False                    # one voxel of the +x face
    cases.append(("shell with a hole", leak, leak.copy()))
    # +x face replaced by two layers whose empty voxels meet only along edges (parity of y + z) or only at corners
    for kind in ("edge", "corner"):
        v = box_shell(n, lo, hi)
        ex = _full_box(n, lo, hi)
        x1 = hi[0]
        for z in range(lo[2] + 1, hi[2]):
            for y in range(lo[1] + 1, hi[1]):
                if kind == "edge":
                    inner, outer = (y + z) % 2 == 0, (y + z) % 2 == 1
                else:
                    inner, outer = not (y % 2 == 1 and z % 2 == 1), not (y % 2 == 0 and z % 2 == 0)
                v[z, y, x1] = inner
                v[z, y, x1 + 1] = outer
                ex[z, y, x1 + 1] = outer
        cases.append(("diagonal gaps (%s)" % kind, v, ex))
    # nested shells: a cavity inside the inner shell, a gap between the shells -- both enclosed
    inner_lo, inner_hi = (lo[0] + 4, lo[1] + 4, lo[2] + 4), (hi[0] - 4, hi[1] - 4, hi[2] - 4)
    nested = box_shell(n, inner_lo, inner_hi, box_shell(n, lo, hi))
    cases.append(("nested shells", nested, _full_box(n, lo, hi)))
    # walls on word edges and on the grid faces
    for (x0, x1) in [(0, n - 1), (31, 63), (32, 64), (0, 31), (31, n - 1), (32, n - 1), (1, 32), (30, 33)]:
        if x1 > n - 1 or x1 - x0 < 2:
            continue
        for (y0, y1, z0, z1) in [(0, n - 1, 0, n - 1), (2, n - 3, 0, n - 1), (0, n - 1, 3, n - 2)]:
            b_lo, b_hi = (x0, y0, z0), (x1, y1, z1)
            cases.append(("walls x %d..%d y %d..%d z %d..%d" % (x0, x1, y0, y1, z0, z1), box_shell(n, b_lo, b_hi), _full_box(n, b_lo, b_hi)))
    # a pocket on the boundary: a box against the x = 0 face (y = 0, z = n - 1 faces) with one empty voxel of that face: not filled
    for face in ("x0", "y0", "zn"):
        b_lo, b_hi = {"x0": ((0, 4, 4), (9, 12, 12)), "y0": ((4, 0, 4), (12, 9, 12)), "zn": ((4, 4, n - 10), (12, 12, n - 1))}[face]
        v = box_shell(n, b_lo, b_hi)
        c = tuple((a + b) // 2 for a, b in zip(b_lo, b_hi))
        pos = {"x0": (c[2], c[1], 0), "y0": (c[2], 0, c[0]), "zn": (n - 1, c[1], c[0])}[face]
        v[pos] = False
        cases.append(("pocket open to the %s face" % face, v, v.copy()))
    return cases
