"""Sparse voxel octree references for tests/test_octree_cpu.py and tests/test_octree_gpu.py (helpers, no tests).

The contract of vp_octree (include/vphip.h), restated from its text.  Arrays are (z, y, x) bool.
  build_numpy     the pyramid of any / all bits over the cube of side P = NextPow2(n), the mixed cells of every level sorted by Morton code,
                  and their records: (nodes uint32[M, 2], level_offset uint32[11], full_leaves uint32[11])
  expand_numpy    the tree back into a grid of side n, level by level from the root
  validate_numpy  the structural check of vp_octree_validate_host: None, or the reason for the refusal
  query_numpy     the point query: descend from the root
Grid generators: random by density (fill_ref), ball, box, single voxel.  Everything is integer logic."""
import numpy as np

from fill_ref import bool_to_words, random_grid, words_to_bool  # noqa: F401

SLOTS = 11


def geometry(n):
    P = 32
    while P < n:
        P *= 2
    return P, P.bit_length() - 1


def morton(x, y, z):
    """interleave: bit i of x -> bit 3 i, of y -> 3 i + 1, of z -> 3 i + 2"""
    x, y, z = (np.asarray(a, np.uint64) for a in (x, y, z))
    m = np.zeros(x.shape, np.uint64)
    for i in range(10):
        s = np.uint64(i)
        one = np.uint64(1)
        m |= (((x >> s) & one) << np.uint64(3 * i)) | (((y >> s) & one) << np.uint64(3 * i + 1)) | (((z >> s) & one) << np.uint64(3 * i + 2))
    return m


def pyramid(vox):
    """any[l], all[l] for l = 0 .. L, each (side, side, side) bool in (z, y, x); level L is the padded voxel cube"""
    n = vox.shape[0]
    P, L = geometry(n)
    pad = np.zeros((P, P, P), bool)
    pad[:n, :n, :n] = vox
    anys, alls = [None] * (L + 1), [None] * (L + 1)
    anys[L] = alls[L] = pad
    for l in range(L - 1, -1, -1):
        s = 1 << l
        a = anys[l + 1].reshape(s, 2, s, 2, s, 2)
        b = alls[l + 1].reshape(s, 2, s, 2, s, 2)
        anys[l], alls[l] = a.any(axis=(1, 3, 5)), b.all(axis=(1, 3, 5))
    return anys, alls


def build_numpy(vox):
    n = vox.shape[0]
    P, L = geometry(n)
    anys, alls = pyramid(vox)
    cells = []                                                # per level: the (z, y, x) of the stored cells, in Morton order
    for l in range(L):
        stored = anys[l] & ~alls[l]
        if l == 0:
            stored = np.ones((1, 1, 1), bool)
        z, y, x = np.nonzero(stored)
        order = np.argsort(morton(x, y, z), kind="stable")
        cells.append((z[order], y[order], x[order]))
    counts = [len(c[0]) for c in cells]
    level_offset = np.zeros(SLOTS, np.uint32)
    level_offset[1:L + 1] = np.cumsum(counts)
    level_offset[L + 1:] = level_offset[L]
    full_leaves = np.zeros(SLOTS, np.uint32)
    nodes = np.zeros((int(level_offset[L]), 2), np.uint32)
    for l in range(L):
        z, y, x = cells[l]
        valid = np.zeros(len(x), np.uint32)
        full = np.zeros(len(x), np.uint32)
        for c in range(8):
            cz, cy, cx = 2 * z + (c >> 2), 2 * y + ((c >> 1) & 1), 2 * x + (c & 1)
            valid |= anys[l + 1][cz, cy, cx].astype(np.uint32) << np.uint32(c)
            full |= alls[l + 1][cz, cy, cx].astype(np.uint32) << np.uint32(c)
        mixed = valid & ~full
        kids = np.array([bin(int(m)).count("1") for m in mixed], np.int64)
        first = int(level_offset[l + 1]) + np.cumsum(kids) - kids
        lo, hi = int(level_offset[l]), int(level_offset[l + 1])
        nodes[lo:hi, 0] = valid | (full << np.uint32(8))
        nodes[lo:hi, 1] = np.where(kids > 0, first, 0)
        full_leaves[l] = sum(bin(int(f)).count("1") for f in full)
    return nodes, level_offset, full_leaves


def counts_of(level_offset, n):
    _, L = geometry(n)
    return [int(v) for v in np.diff(level_offset[:L + 1].astype(np.int64))]


def popcount_from_full_leaves(full_leaves, n):
    P, L = geometry(n)
    return sum(int(full_leaves[l]) * (P >> (l + 1)) ** 3 for l in range(L))


def expand_numpy(nodes, n):
    """the grid of side n of a VALID tree (validate_numpy first)"""
    P, L = geometry(n)
    out = np.zeros((P, P, P), bool)
    level = [(0, 0, 0, 0)]                                     # (node, z, y, x) of the cells of the level
    for l in range(L):
        side = P >> (l + 1)
        nxt = []
        for node, z, y, x in level:
            masks, child = int(nodes[node, 0]), int(nodes[node, 1])
            valid, full = masks & 0xFF, (masks >> 8) & 0xFF
            rank = 0
            for c in range(8):
                cz, cy, cx = 2 * z + (c >> 2), 2 * y + ((c >> 1) & 1), 2 * x + (c & 1)
                if (full >> c) & 1:
                    out[cz * side:(cz + 1) * side, cy * side:(cy + 1) * side, cx * side:(cx + 1) * side] = True
                elif (valid >> c) & 1:
                    nxt.append((child + rank, cz, cy, cx))
                    rank += 1
        level = nxt
    assert not out[n:].any() and not out[:, n:].any() and not out[:, :, n:].any()
    return out[:n, :n, :n].copy()


def query_numpy(nodes, n, x, y, z):
    P, L = geometry(n)
    node = 0
    for l in range(L):
        sh = L - 1 - l
        c = ((x >> sh) & 1) | (((y >> sh) & 1) << 1) | (((z >> sh) & 1) << 2)
        masks, child = int(nodes[node, 0]), int(nodes[node, 1])
        valid, full = masks & 0xFF, (masks >> 8) & 0xFF
        if not (valid >> c) & 1:
            return False
        if (full >> c) & 1:
            return True
        node = child + bin(valid & ~full & ((1 << c) - 1)).count("1")
    return False



def validate_numpy(nodes, n):
    """None for a well-formed tree, else one line saying what is wrong (the rules of vp_octree_validate_host)"""
    if n < 32 or n > 1024 or n % 32:
        return "side"
    P, L = geometry(n)
    M = len(nodes)
    if M < 1 or M >= 1 << 28:
        return "node count"
    level = [(0, 0, 0)]
    begin, running = 0, 1
    for l in range(L):
        side = P >> (l + 1)
        nxt = []
        for k, (z, y, x) in enumerate(level):
            masks, child = int(nodes[begin + k, 0]), int(nodes[begin + k, 1])
            valid, full = masks & 0xFF, (masks >> 8) & 0xFF
            if masks >> 16:
                return "upper bits"
            if full & ~valid:
                return "full not in valid"
            if l > 0 and (valid == 0 or full == 0xFF):
                return "a stored cell that is not mixed"
            mixed = valid & ~full
            if l == L - 1 and mixed:
                return "a voxel that is neither set nor unset"
            if child != (running if mixed else 0):
                return "child is not the running sum"
            for c in range(8):
                cz, cy, cx = 2 * z + (c >> 2), 2 * y + ((c >> 1) & 1), 2 * x + (c & 1)
                if (full >> c) & 1 and max(cz, cy, cx) * side + side > n:
                    return "a full child outside the grid"
                if (valid >> c) & 1 and max(cz, cy, cx) * side >= n:
                    return "a child outside the grid"
                if (mixed >> c) & 1:
                    nxt.append((cz, cy, cx))
            running += bin(mixed).count("1")
            if running > M:
                return "child out of range"
        begin += len(level)
        level = nxt
        if not level:
            break
    if running != M:
        return "the levels do not end at M"
    return None


# ---- grids -------------------------------------------------------------------------------------------------------------------------
def ball(n, centre, r2):
    a = np.arange(n, dtype=np.int64)
    cx, cy, cz = centre
    return ((a[:, None, None] - cz) ** 2 + (a[None, :, None] - cy) ** 2 + (a[None, None, :] - cx) ** 2) <= r2


def box(n, lo, hi):
    v = np.zeros((n, n, n), bool)
    v[lo:hi, lo:hi, lo:hi] = True
    return v


def single(n, x, y, z):
    v = np.zeros((n, n, n), bool)
    v[z, y, x] = True
    return v


def random_bool(n, density, seed):
    return words_to_bool(random_grid(n, density, seed), n)


def embed(vox, n):
    out = np.zeros((n, n, n), bool)
    m = vox.shape[0]
    out[:m, :m, :m] = vox
    return out


def boxes_words(n, boxes):
    """the words (z, y, x / 32) of a grid of boxes (x0, x1, y0, y1, z0, z1), half-open, without a voxel array: for sides where n^3 bools are
    too many"""
    words = np.zeros((n, n, n // 32), np.uint32)
    for x0, x1, y0, y1, z0, z1 in boxes:
        row = np.zeros(n, bool)
        row[x0:x1] = True
        words[z0:z1, y0:y1] |= np.packbits(row, bitorder="little").view(np.uint32)
    return words.reshape(-1)
