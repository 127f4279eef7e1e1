"""The contract of vp_regions (include/vphip.h) restated in numpy, and the cases of tests/test_regions_cpu.py / test_regions_gpu.py (helpers,
no tests).  Label volumes are (z, y, x) uint32 arrays; outside the grid the label is 0.

  regions(W, K, values)   (table uint64 (K, 26), the four statistics): the volume padded by one layer, one bincount per summed word,
                          ufunc.at for the minima and maxima; n0 / n1 as the DISTINCT non-zero labels among the 8 / 4 voxels incident on
                          every lattice point / edge -- the per-element definition, not the ownership rule of the kernels.
  euler(table)            chi = n0 - n1 + (6 V + F) / 2 - V per label
and the solids and label volumes of the tests."""
import functools

import numpy as np

WORDS = 26
REGIONS_MAX = (1 << 20) - 1
_MIN_WORDS = (1, 2, 3, 23, 25)


def _isum(lab, w, size):
    """exact per-label integer sums of w (< 2^64 in total): bincount adds in float64, so w goes in as 16-bit digits"""
    w = np.asarray(w).astype(np.uint64).ravel()
    out = np.zeros(size, np.uint64)
    for shift in (0, 16, 32, 48):
        digit = ((w >> np.uint64(shift)) & np.uint64(0xFFFF)).astype(np.float64)
        if digit.any():
            out += np.bincount(lab, weights=digit, minlength=size).astype(np.uint64) << np.uint64(shift)
    return out


def _distinct(stack, size):
    """per label: the elements (columns of `stack`) among whose entries the label occurs"""
    s = np.sort(stack, axis=0)
    new = np.ones(s.shape, bool)
    new[1:] = s[1:] != s[:-1]
    return np.bincount(s[new & (s != 0)], minlength=size).astype(np.uint64)


def regions(W, K, values=None):
    W = np.asarray(W)
    n = W.shape[0]
    assert W.shape == (n, n, n) and 0 <= K <= REGIONS_MAX
    L = np.where((W >= 1) & (W <= K), W, 0).astype(np.int64)
    size = K + 1                                                    # row 0 collects the background and is dropped
    lab = L.ravel()
    z, y, x = (a.ravel().astype(np.uint64) for a in np.indices(L.shape))
    T = np.zeros((size, WORDS), np.uint64)
    T[:, 0] = np.bincount(lab, minlength=size)
    for j, c in enumerate((x, y, z)):
        lo = np.full(size, np.iinfo(np.uint64).max, np.uint64)
        np.minimum.at(lo, lab, c)
        np.maximum.at(T[:, 4 + j], lab, c)
        T[:, 1 + j] = lo
        T[:, 7 + j] = _isum(lab, c, size)
        T[:, 10 + j] = _isum(lab, c * c, size)
    T[:, 13] = _isum(lab, x * y, size)
    T[:, 14] = _isum(lab, x * z, size)
    T[:, 15] = _isum(lab, y * z, size)
    P = np.pad(L, 1)
    inner = (slice(1, n + 1),) * 3
    contact = np.zeros(L.shape, np.int64)
    for j, axis in enumerate((2, 1, 0)):                            # x, y, z
        faces = np.zeros(L.shape, np.int64)
        for step in (-1, 1):
            nb = np.roll(P, -step, axis)[inner]
            exposed = (L != 0) & (nb != L)
            faces += exposed
            contact += exposed & (nb != 0)
        T[:, 16 + j] = _isum(lab, faces, size)
    T[:, 19] = _isum(lab, contact, size)
    m = n + 1
    T[:, 20] = _distinct(np.stack([P[a:a + m, b:b + m, c:c + m].ravel() for a in (0, 1) for b in (0, 1) for c in (0, 1)]), size)
    along_x = np.stack([P[a:a + m, b:b + m, 1:m].ravel() for a in (0, 1) for b in (0, 1)])
    along_y = np.stack([P[a:a + m, 1:m, c:c + m].ravel() for a in (0, 1) for c in (0, 1)])
    along_z = np.stack([P[1:m, b:b + m, c:c + m].ravel() for b in (0, 1) for c in (0, 1)])
    T[:, 21] = _distinct(along_x, size) + _distinct(along_y, size) + _distinct(along_z, size)
    if values is not None:
        v = np.asarray(values).astype(np.uint64).ravel()
        lo = np.full(size, np.iinfo(np.uint64).max, np.uint64)
        np.minimum.at(lo, lab, v)
        np.maximum.at(T[:, 24], lab, v)
        T[:, 22] = _isum(lab, v, size)
        T[:, 23] = lo
    first = np.full(size, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(first, lab, np.arange(lab.size, dtype=np.uint64))
    T[:, 25] = first
    T[T[:, 0] == 0] = 0                                             # an empty label: an all-zero record
    T = np.ascontiguousarray(T[1:])
    stats = (int(T[:, 0].sum()), int((T[:, 0] != 0).sum()), int((W > K).sum()), int(T[:, 19].sum()) // 2)
    return T, stats


def euler(table):
    """chi per label (int64)"""
    t = np.asarray(table).astype(np.int64)
    faces = t[:, 16] + t[:, 17] + t[:, 18]
    return t[:, 20] - t[:, 21] + (6 * t[:, 0] + faces) // 2 - t[:, 0]


# ---- solids ((z, y, x) bool) ------------------------------------------------------------------------------------------------------------

def _grid(n):
    z, y, x = np.indices((n, n, n)).astype(np.int64)
    return x, y, z


def ball(n, centre, r2):
    x, y, z = _grid(n)
    return (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= r2


def shell(n, centre, r2_out, r2_in):
    return ball(n, centre, r2_out) & ~ball(n, centre, r2_in)


def torus(n, centre, R, r):
    x, y, z = _grid(n)
    ring = np.sqrt((x - centre[0]) ** 2.0 + (y - centre[1]) ** 2.0) - R
    return ring ** 2 + (z - centre[2]) ** 2.0 <= r * r


# ---- label volumes: name -> (W uint32 (z, y, x), K) ------------------------------------------------------------------------------------

def _single(n, at):
    W = np.zeros((n, n, n), np.uint32)
    W[at[2], at[1], at[0]] = 1
    return W


def _halves(n):
    """a ball cut by the plane x = 15 | 16: two labels of equal size that touch"""
    b = ball(n, (15.5, 15.5, 15.5), 100)
    x, _, _ = _grid(n)
    return np.where(b, np.where(x < 16, 1, 2), 0).astype(np.uint32)


def _seams(n):
    """label 1: a bar along x over the seam 31 | 32, a bar along y over 15 | 16, a bar along z over 15 | 16 and a 2 x 2 x 2 cube on the block
    corner (32, 16, 16); label 2 wraps the corner cube's far side, so contact faces cross the seams too"""
    W = np.zeros((n, n, n), np.uint32)
    W[5, 5, 28:37] = 1
    W[7, 12:20, 40] = 1
    W[12:20, 3, 3] = 1
    W[15:17, 15:17, 31:33] = 1
    W[17, 15:17, 31:33] = 2
    W[15:18, 17, 31:33] = 2
    W[15:18, 15:18, 33] = 2
    return W


def _faces(n):
    """voxels on all six grid faces, the twelve edges and the eight corners among them: a shell of the grid two labels thick"""
    W = np.zeros((n, n, n), np.uint32)
    W[:] = 1
    W[1:-1, 1:-1, 1:-1] = 2
    W[2:-2, 2:-2, 2:-2] = 0
    W[0, 0, 0] = 3
    W[n - 1, n - 1, n - 1] = 3
    return W


def _random(n, top, seed, density=1.0):
    rng = np.random.default_rng(seed)
    W = rng.integers(0, top + 1, (n, n, n), dtype=np.uint32)
    if density < 1.0:
        W[rng.random((n, n, n)) >= density] = 0
    return W


def _blobs(n, seed):
    """a few labels in large connected pieces (what a watershed writes): nearest of 7 random centres inside a ball"""
    rng = np.random.default_rng(seed)
    x, y, z = _grid(n)
    c = rng.integers(4, n - 4, (7, 3))
    d = np.stack([(x - a) ** 2 + (y - b) ** 2 + (z - e) ** 2 for a, b, e in c])
    W = (np.argmin(d, 0) + 1).astype(np.uint32)
    W[~ball(n, (n / 2, n / 2, n / 2), (n * 0.45) ** 2)] = 0
    return W


@functools.lru_cache(maxsize=None)
def case(name):
    """(W, K) of a named case; the arrays are shared between the tests and must not be written"""
    W, K = {
        "voxel": lambda: (_single(32, (7, 9, 11)), 1),
        "corner_voxel": lambda: (_single(32, (0, 0, 0)), 1),
        "far_corner_voxel": lambda: (_single(32, (31, 31, 31)), 1),
        "ball": lambda: (ball(32, (16, 15, 14), 81).astype(np.uint32), 1),
        "shell": lambda: (shell(32, (16, 16, 16), 144, 36).astype(np.uint32), 1),
        "torus": lambda: (torus(32, (15.5, 15.5, 15.5), 9.0, 3.2).astype(np.uint32), 1),
        "halves": lambda: (_halves(32), 2),
        "seams": lambda: (_seams(64), 2),
        "faces": lambda: (_faces(32), 3),
        "faces64": lambda: (_faces(64), 3),
        "random5": lambda: (_random(32, 8, 1), 5),                # labels 0 .. 8 in the volume, K = 5: 6, 7, 8 are ignored
        "random4000": lambda: (_random(32, 4000, 2), 4000),       # every voxel its own draw: nearly every run finds the slots taken
        "sparse300": lambda: (_random(64, 300, 3, 0.3), 300),
        "blobs": lambda: (_blobs(64, 4), 7),
        "blobs96": lambda: (_blobs(96, 5), 7),
        "whole96": lambda: (np.ones((96, 96, 96), np.uint32), 1),
        "whole128": lambda: (np.ones((128, 128, 128), np.uint32), 1),   # the smallest side whose sum x^2 and sum xy pass 2^32
        "above": lambda: (_random(32, 8, 6) + np.uint32(10), 9),  # every label above K
        "empty": lambda: (np.zeros((32, 32, 32), np.uint32), 4),
        "count0": lambda: (_random(32, 3, 7), 0),
    }[name]()
    W = np.ascontiguousarray(W, np.uint32)
    W.setflags(write=False)
    return W, K


CASES = ("voxel", "corner_voxel", "far_corner_voxel", "ball", "shell", "torus", "halves", "seams", "faces", "faces64", "random5", "random4000",
         "sparse300", "blobs", "blobs96", "whole96", "whole128", "above", "empty", "count0")


@functools.lru_cache(maxsize=None)
def values_of(name):
    """the value field of a case: whole96 and whole128 -- every value 0xFFFFFFFF (the sum needs 64 bits); the others -- random over the full
    uint32 range with 0 and 0xFFFFFFFF forced in"""
    W, _ = case(name)
    if name in ("whole96", "whole128"):
        v = np.full(W.shape, 0xFFFFFFFF, np.uint32)
    else:
        rng = np.random.default_rng(len(name) * 31 + W.shape[0])
        v = rng.integers(0, 1 << 32, W.shape, dtype=np.uint64).astype(np.uint32)
        pick = rng.random(W.shape)
        v[pick < 0.05] = 0
        v[pick > 0.95] = 0xFFFFFFFF
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def expected(name, with_values):
    """the reference of a case, computed once"""
    W, K = case(name)
    T, stats = regions(W, K, values_of(name) if with_values else None)
    T.setflags(write=False)
    return T, stats
