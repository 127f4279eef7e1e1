"""Local thickness references for tests/test_thickness_cpu.py and tests/test_thickness_gpu.py (helpers, no tests).

The contract of vp_thickness (include/vphip.h), restated from its text.  S = the set voxels of an n^3 grid, arrays are (z, y, x).
  capped_radius     D(c) = min(E(c), W(c), rmax^2) on S, 0 elsewhere: E = the exact squared distance to the nearest unset voxel (NONE if
                    there is none), W(c) = (1 + min(x, n-1-x, y, n-1-y, z, n-1-z))^2 -- outside the grid counts as empty
  thickness_numpy   T2(p) = max { D(c) : c in S, |p - c|^2 < D(c) }: one shifted maximum per offset d with |d|^2 < max D, over the bounding
                    box of the centres whose ball is that large
  thin_numpy        p in S and T2(p) < thin2
  ball_volume_sum   the sum over c of the number of p with |p - c|^2 < D(c): what the scatter form of the library costs
Everything is integer arithmetic."""
import numpy as np

from edt_ref import NONE, SET, UNSET, edt_numpy, edt_seeds  # noqa: F401
from fill_ref import bool_to_words, random_grid, words_to_bool  # noqa: F401

NAIVE_LIMIT = 2 * 10 ** 8              # a NAIVE launch is only made below this many (centre, voxel) pairs


def wall_radius(n):
    a = np.arange(n, dtype=np.int64)
    f = np.minimum(a, n - 1 - a)
    return (1 + np.minimum(np.minimum(f[:, None, None], f[None, :, None]), f[None, None, :])) ** 2


def capped_radius(vox, rmax, edt=None):
    """(z, y, x) int64; `edt` = the UNSET transform of vox if the caller has it"""
    n = vox.shape[0]
    e = (edt_numpy(vox, UNSET) if edt is None else edt).astype(np.int64)
    return np.where(vox, np.minimum(np.minimum(e, wall_radius(n)), rmax * rmax), 0)


def thickness_numpy(vox, rmax, D=None):
    """(z, y, x) uint32 T2"""
    n = vox.shape[0]
    D = capped_radius(vox, rmax) if D is None else D
    D16 = D.astype(np.int32)
    T = np.zeros((n, n, n), np.int32)
    m = int(D.max())
    if m == 0:
        return T.astype(np.uint32)
    r = int(np.ceil(np.sqrt(m))) - 1                         # the largest r with r^2 < m
    prof = [D.max(axis=tuple(a for a in range(3) if a != ax)) for ax in range(3)]
    boxes = {}

    def box(q):                                              # per axis [lo, hi) of the centres with D > q
        if q not in boxes:
            b = []
            for ax in range(3):
                idx = np.nonzero(prof[ax] > q)[0]
                b.append((int(idx[0]), int(idx[-1]) + 1))
            boxes[q] = b
        return boxes[q]

    for dz in range(-r, r + 1):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                q = dz * dz + dy * dy + dx * dx
                if q >= m:
                    continue
                src, dst = [], []
                for (lo, hi), d in zip(box(q), (dz, dy, dx)):
                    lo, hi = max(lo, -d, 0), min(hi, n - d, n)   # the target p = c + d stays in the grid (it does for every c with D(c) > q)
                    src.append(slice(lo, hi))
                    dst.append(slice(lo + d, hi + d))
                src, dst = tuple(src), tuple(dst)
                c = D16[src]
                np.maximum(T[dst], np.where(c > q, c, 0), out=T[dst])
    return T.astype(np.uint32)


def thin_numpy(vox, t2, thin2):
    return vox & (t2.astype(np.int64) < thin2)


def thin2_of_width(w):
    """a thickness of w whole voxels is thin iff 4 T2 < w^2"""
    return (w * w + 3) // 4


def ball_volume_sum(D):
    """sum over the voxels c of |{p : |p - c|^2 < D(c)}|"""
    m = int(D.max())
    if m == 0:
        return 0
    r = int(np.ceil(np.sqrt(m))) - 1
    a = np.arange(-r, r + 1, dtype=np.int64)
    q = (a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2).reshape(-1)
    vol = np.cumsum(np.bincount(q, minlength=m + 1))         # vol[t - 1] = the number of offsets with q < t
    return int(vol[D[D > 0] - 1].sum())


def saturated_by_transform(vox, rmax):
    """{T2 = rmax^2} by the identity of the header: voxels closer than rmax to a centre with min(E, W) >= rmax^2"""
    n = vox.shape[0]
    e = edt_numpy(vox, UNSET).astype(np.int64)
    seeds = vox & (np.minimum(e, wall_radius(n)) >= rmax * rmax)
    return edt_seeds(seeds).astype(np.int64) < rmax * rmax


def slab(n, lo, w, axis=2):
    v = np.zeros((n, n, n), bool)
    s = [slice(None)] * 3
    s[axis] = slice(lo, lo + w)
    v[tuple(s)] = True
    return v


def ball(n, centre, r2):
    """voxels with |p - centre|^2 <= r2, centre = (x, y, z)"""
    a = np.arange(n, dtype=np.int64)
    Z, Y, X = a[:, None, None], a[None, :, None], a[None, None, :]
    return (X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2 <= r2


def dumbbell(n=64):
    """two balls of radius 10 (|p - c|^2 <= 100) around (16, 32, 32) and (48, 32, 32) joined by a 3 x 3 rod along x: the balls end at x = 26
    and x = 38, so 11 cross-sections of the rod, 99 voxels, are reached by no ball larger than the rod's own (T2 = 4)"""
    v = ball(n, (16, 32, 32), 100) | ball(n, (48, 32, 32), 100)
    v[31:34, 31:34, 16:49] = True
    return v


def boxes_1024_words(n=1024):
    """three bars along x, y in 100 .. 899, x in 100 .. 899, of z widths 3, 20 and 200 -- as words, without the bool volume.
    Returns (words, [(z0, width)])"""
    w = n // 32
    words = np.zeros((n, n, w), np.uint32)
    bars = [(100, 3), (300, 20), (500, 200)]
    row = np.zeros(n, bool)
    row[100:900] = True
    roww = np.packbits(row, bitorder="little").view(np.uint32)
    for z0, wd in bars:
        words[z0:z0 + wd, 100:900, :] = roww
    return words.reshape(-1), bars


def hand_cases(n):
    """[(name, rmax, input (z, y, x) bool, expected (z, y, x) uint32 T2)] -- every expectation written from the construction"""
    cases = []
    zero = np.zeros((n, n, n), bool)
    u32 = lambda v: np.broadcast_to(v, (n, n, n)).astype(np.uint32)     # noqa: E731
    cases.append(("empty", 4, zero.copy(), u32(0)))
    for p in ((n // 2, n // 2 + 1, n // 2 - 1), (0, n - 1, 0)):         # a lone voxel, in the middle and in a corner: a ball of radius 1
        v = zero.copy()
        v[p[2], p[1], p[0]] = True
        cases.append(("single voxel %s" % (p,), 5, v, u32(v.astype(np.uint32))))
    # the full grid at rmax 1 and 2: every voxel is its own ball of radius 1; at rmax 2 the voxels at least one voxel off every wall
    # carry D = 4, and their open balls of squared radius 4 hold the whole 3 x 3 x 3 cube around them (its corners have q = 3): every
    # voxel of the grid is within 1 of such a centre along every axis
    cases.append(("full, rmax 1", 1, ~zero, u32(1)))
    cases.append(("full, rmax 2", 2, ~zero, u32(4)))
    # slabs of width w far from the walls: the centre plane(s) carry D = ceil(w/2)^2 and their balls reach the slab's faces
    for w in range(1, 8):
        for axis in (0, 1, 2):
            v = slab(n, 12, w, axis)
            inner = np.zeros((n, n, n), bool)
            inner[8:n - 8, 8:n - 8, 8:n - 8] = True
            exp = np.where(v, ((w + 1) // 2) ** 2, 0)
            cases.append(("slab w=%d axis=%d" % (w, axis), 8, v, (u32(exp), inner)))
    return cases
