"""Connected-component references and case generators for tests/test_components_cpu.py and tests/test_components_gpu.py (helpers, no
tests).

label_numpy(words, n, conn) restates the contract of vp_components_label (include/vphip.h) in its plainest form: every set voxel starts
with its own linear index x + n y + n^2 z, repeatedly takes the minimum over itself and its C neighbours until nothing changes, and the
distinct minima are ranked.  It takes one step per voxel of the longest path inside a component; jump=True also lets every voxel take
the value of the voxel its value names (a voxel of the same component with a value no larger) until that changes nothing either --
the same fixed point in far fewer steps, which the long-chain cases of the GPU tests need.  Neither is a union-find, an x-run
decomposition or a flood, so both are independent of the kernels and of the host restatement in vplib/src/components.cpp."""
import itertools

import numpy as np

from fill_ref import bool_to_words, box_shell, words_to_bool

KEEP_LARGEST, MIN_VOXELS = 0, 1
_BIG = np.uint32(0xFFFFFFFF)


def structure(conn):
    """the 3 x 3 x 3 neighbourhood of scipy.ndimage.generate_binary_structure(3, 1) (conn 6) / (3, 3) (conn 26)"""
    s = np.zeros((3, 3, 3), bool)
    for d in itertools.product((-1, 0, 1), repeat=3):
        s[d[0] + 1, d[1] + 1, d[2] + 1] = sum(c != 0 for c in d) <= (1 if conn == 6 else 3)
    return s


def _axis_min(a, axis):
    """min over the voxel and its two neighbours along one axis (outside the grid: nothing)"""
    out = a.copy()
    lo = [slice(None)] * 3
    hi = [slice(None)] * 3
    lo[axis], hi[axis] = slice(0, -1), slice(1, None)
    lo, hi = tuple(lo), tuple(hi)
    np.minimum(out[hi], a[lo], out=out[hi])
    np.minimum(out[lo], a[hi], out=out[lo])
    return out


def min_index_bool(vox, conn, jump=False):
    """(z, y, x) uint32 array: the lowest linear index of each set voxel's component, 0xFFFFFFFF for empty voxels"""
    assert conn in (6, 26)
    n = vox.shape[0]
    L = np.where(vox, np.arange(n ** 3, dtype=np.uint32).reshape(n, n, n), _BIG)
    flat_set = np.flatnonzero(vox.reshape(-1))
    while True:
        if conn == 6:
            new = np.minimum(np.minimum(_axis_min(L, 0), _axis_min(L, 1)), _axis_min(L, 2))
        else:
            new = _axis_min(_axis_min(_axis_min(L, 2), 1), 0)      # the 3 x 3 x 3 box: every voxel in it is a 26-neighbour
        new[~vox] = _BIG
        if jump:
            f = new.reshape(-1)
            while True:
                g = f[f[flat_set]]
                if np.array_equal(g, f[flat_set]):
                    break
                f[flat_set] = g
        if np.array_equal(new, L):
            return L
        L = new


def label_bool(vox, conn, jump=False):
    """(labels (z, y, x) uint32, K): components numbered 1 .. K in increasing order of their lowest linear voxel index"""
    L = min_index_bool(vox, conn, jump)
    roots = np.unique(L[vox])                                      # ascending: rank = label - 1
    labels = np.zeros(L.shape, np.uint32)
    labels[vox] = (np.searchsorted(roots, L[vox]) + 1).astype(np.uint32)
    return labels, int(roots.size)


def label_numpy(words, n, conn, jump=False):
    """(labels as a flat uint32 array of n^3, x fastest; K)"""
    labels, k = label_bool(words_to_bool(words, n), conn, jump)
    return labels.reshape(-1), k


def label_reference(vox, conn):
    """(labels (z, y, x) uint32, K) for the large grids of the GPU tests: scipy.ndimage.label where scipy is installed --
    tests/test_components_cpu.py pins label_numpy to it element for element -- and label_numpy with jump=True where it is not"""
    try:
        from scipy import ndimage
    except ImportError:
        return label_bool(vox, conn, jump=True)
    labels, k = ndimage.label(vox, structure(conn))
    return labels.astype(np.uint32), int(k)


def sizes_of(labels, k):
    return np.bincount(np.asarray(labels).reshape(-1), minlength=k + 1)[1:].astype(np.uint32)


def keep_flags(sizes, mode, param):
    """bool per component: the contract of vp_components_filter"""
    k = sizes.size
    if mode == MIN_VOXELS:
        return sizes >= param
    assert mode == KEEP_LARGEST and 1 <= param <= 16
    order = sorted(range(k), key=lambda i: (-int(sizes[i]), i))    # ties: the lower label first
    keep = np.zeros(k, bool)
    keep[order[:param]] = True
    return keep


def filter_labels(labels, k, mode, param):
    """(words, kept voxels) from a flat label volume"""
    keep = np.concatenate([[False], keep_flags(sizes_of(labels, k), mode, param)])
    out = keep[np.asarray(labels).reshape(-1)]
    n = round(out.size ** (1 / 3))
    return bool_to_words(out.reshape(n, n, n)), int(out.sum())


def filter_numpy(words, n, conn, mode, param, jump=False):
    """(words, K, kept voxels)"""
    labels, k = label_numpy(words, n, conn, jump)
    out, kept = filter_labels(labels, k, mode, param)
    return out, k, kept


# ---- hand-written cases ----------------------------------------------------------------------------------------------------------

def _assemble(n, parts):
    """parts: coordinate lists [(x, y, z), ...], each one component BY CONSTRUCTION and no two of them adjacent.  Returns the grid, K and
    the sizes in label order -- the order of each part's lowest linear index."""
    vox = np.zeros((n, n, n), bool)
    keyed = []
    for p in parts:
        p = sorted(set(p), key=lambda c: (c[2], c[1], c[0]))
        for (x, y, z) in p:
            assert 0 <= x < n and 0 <= y < n and 0 <= z < n and not vox[z, y, x]
            vox[z, y, x] = True
        keyed.append((p[0][0] + n * (p[0][1] + n * p[0][2]), len(p)))
    keyed.sort()
    return vox, len(parts), np.array([s for _, s in keyed], np.uint32)


def _box(lo, hi):
    return [(x, y, z) for z in range(lo[2], hi[2] + 1) for y in range(lo[1], hi[1] + 1) for x in range(lo[0], hi[0] + 1)]


def _perm(c, axis):
    """the comb cases are written along x; axis 1 / 2 swaps x with y / z"""
    c = list(c)
    c[0], c[axis] = c[axis], c[0]
    return tuple(c)


def hand_cases(n, conn):
    """[(name, (z, y, x) bool grid, K, sizes in label order)] -- every expectation written from the construction, not computed"""
    assert conn in (6, 26) and n >= 32
    cases = []

    def add(name, parts):
        cases.append((name,) + _assemble(n, parts))

    zero = np.zeros((n, n, n), bool)
    cases.append(("empty", zero.copy(), 0, np.zeros(0, np.uint32)))
    cases.append(("full", ~zero, 1, np.array([n ** 3], np.uint32)))
    m = n - 1
    add("eight corners", [[(x, y, z)] for z in (0, m) for y in (0, m) for x in (0, m)])
    # two voxels one step apart in each of the 26 directions: faces join under both connectivities, edges and corners under 26 only
    offsets = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]
    for tag, bx in (("", 10), (" across the word edge", 31)):
        if bx + 2 >= n:
            continue
        parts = []
        for i, d in enumerate(offsets):
            a = (bx + (1 if d[0] < 0 else 0), 5 + 4 * (i % 5), 5 + 4 * (i // 5))      # bx = 31: the pair is x = 31 | 32 whenever dx != 0
            b = (a[0] + d[0], a[1] + d[1], a[2] + d[2])
            touching = sum(c != 0 for c in d) == 1 or conn == 26
            parts += [[a, b]] if touching else [[a], [b]]
        add("pairs by face, edge and corner" + tag, parts)
    x1 = min(n - 4, 75)
    add("one run across the word edges", [[(x, 7, 9) for x in range(20 if n > 32 else 3, x1 + 1)]])
    # "1 0 1" beside "1 1 1" in each of the four backward rows (and mirrored): the three-run touches two runs of the other row
    for tag, a in (("", 10), (" across the word edge", 31)):
        if a + 3 >= n:
            continue
        parts = []
        for i, (dy, dz) in enumerate([(-1, 0), (-1, -1), (0, -1), (1, -1)]):
            for k, mirrored in enumerate((False, True)):
                y, z = 6 + 5 * i, 6 + 6 * k
                three = [(a, y, z), (a + 1, y, z), (a + 2, y, z)]
                two = [(a, y + dy, z + dz), (a + 2, y + dy, z + dz)]
                if mirrored:                                   # the "1 0 1" row is the later one
                    three, two = [(x, yy + dy, zz + dz) for (x, yy, zz) in three], [(x, y, z) for (x, _, _) in two]
                if conn == 26 or (dy != 0) + (dz != 0) == 1:
                    parts.append(three + two)
                else:
                    parts += [three, [two[0]], [two[1]]]
        add("1 0 1 beside 1 1 1" + tag, parts)
    # the 3D checkerboard: no two set voxels share a face; every set voxel has set edge neighbours
    zz, yy, xx = np.indices((n, n, n))
    board = (xx + yy + zz) % 2 == 0
    if conn == 6:
        cases.append(("checkerboard", board, n ** 3 // 2, np.ones(n ** 3 // 2, np.uint32)))
    else:
        cases.append(("checkerboard", board, 1, np.array([n ** 3 // 2], np.uint32)))
    # nested box shells, four voxels apart
    lo, hi = (3, 4, 5), (n - 6, n - 5, n - 4)
    ilo, ihi = tuple(c + 4 for c in lo), tuple(c - 4 for c in hi)
    nested = box_shell(n, ilo, ihi, box_shell(n, lo, hi))

    def shell_size(a, b):
        d = [q - p + 1 for p, q in zip(a, b)]
        return d[0] * d[1] * d[2] - (d[0] - 2) * (d[1] - 2) * (d[2] - 2)
    cases.append(("nested shells", nested, 2, np.array([shell_size(lo, hi), shell_size(ilo, ihi)], np.uint32)))
    # a comb whose teeth join only at their far end, along each axis
    for axis in range(3):
        teeth = range(2, n - 2, 2)
        comb = [_perm((x, t, 5), axis) for t in teeth for x in range(2, n - 2)]
        comb += [_perm((n - 3, t, 5), axis) for t in range(teeth[0], teeth[-1] + 1)]
        add("comb along %s" % "xyz"[axis], [comb])
    # two combs with interleaved teeth, three voxels apart wherever they come close
    ta, tb = range(2, n - 2, 4), range(4, n - 2, 4)
    comb_a = [(x, t, 8) for t in ta for x in range(2, n - 5)] + [(2, t, 8) for t in range(ta[0], ta[-1] + 1)]
    comb_b = [(x, t, 8) for t in tb for x in range(5, n - 2)] + [(n - 3, t, 8) for t in range(tb[0], tb[-1] + 1)]
    add("two interleaved combs", [comb_a, comb_b])
    add("two equal boxes", [_box((3, 3, 3), (7, 7, 7)), _box((12, 14, 16), (16, 18, 20))])
    c = n // 2
    add("six faces", [_box((0, c - 1, c - 1), (0, c + 1, c + 1)), _box((m, c - 1, c - 1), (m, c + 1, c + 1)),
                      _box((c - 1, 0, c - 1), (c + 1, 0, c + 1)), _box((c - 1, m, c - 1), (c + 1, m, c + 1)),
                      _box((c - 1, c - 1, 0), (c + 1, c + 1, 0)), _box((c - 1, c - 1, m), (c + 1, c + 1, m))])
    return cases


def serpentine_plane(n, z=3):
    """one serpentine that covers a whole plane: every other row of plane z is full, and the rows between them hold one voxel, at
    x = n - 1 and x = 0 in turn -- a single path of about n^2 / 2 voxels, one component under both connectivities"""
    vox = np.zeros((n, n, n), bool)
    for y in range(0, n, 2):
        vox[z, y, :] = True
        if y + 1 < n:
            vox[z, y + 1, n - 1 if (y // 2) % 2 == 0 else 0] = True
    return vox
