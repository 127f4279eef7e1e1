"""Exact distance transform references for tests/test_edt_cpu.py and tests/test_edt_gpu.py (helpers, no tests).

The contract of vp_edt (include/vphip.h): D(p) = min over the seed voxels q of |p - q|^2, integer voxel coordinates; NONE where the grid
has no seed.  Seeds: the set voxels, the unset voxels, or the JFA's border voxels (set, with an unset 26-neighbour or one outside the
grid).  All arrays are (z, y, x).
  edt_numpy    three separable integer min-plus passes, out[..., i] = min_j g[..., j] + (i - j)^2, int64, NONE handled apart
  edt_brute    the minimum over the seed list, in chunks
Everything is integer arithmetic, so they agree bit for bit with each other, with scipy.ndimage and with the library."""
import numpy as np

from fill_ref import bool_to_words, random_grid, words_to_bool  # noqa: F401

SET, UNSET, BORDER = 0, 1, 2
NONE = 0xFFFFFFFF
_BIG = np.int64(1) << 40              # "no seed" inside the passes: above any sum of three squares, far from overflow in int64


def border_mask(vox):
    """set voxels with an unset 26-neighbour or a 26-neighbour outside the grid: the padded 3 x 3 x 3 AND is false there"""
    n = vox.shape[0]
    pad = np.zeros((n + 2,) * 3, bool)
    pad[1:-1, 1:-1, 1:-1] = vox
    interior = np.ones_like(vox)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                interior &= pad[dz:dz + n, dy:dy + n, dx:dx + n]
    return vox & ~interior


def seeds_of(vox, mode):
    if mode == SET:
        return vox
    if mode == UNSET:
        return ~vox
    if mode == BORDER:
        return border_mask(vox)
    raise ValueError(mode)


def _pass(g, axis):
    """out[..., i] = min_j g[..., j] + (i - j)^2 along `axis`"""
    n = g.shape[axis]
    g = np.moveaxis(g, axis, -1)
    a = np.arange(n, dtype=np.int64)
    sq = (a[:, None] - a[None, :]) ** 2                     # [i, j]
    out = np.empty_like(g)
    for k in range(g.shape[0]):                              # one slab at a time: n^3 int64 temporaries
        out[k] = (g[k][:, None, :] + sq[None, :, :]).min(-1)
    return np.moveaxis(out, -1, axis)


def edt_seeds(seeds):
    """(z, y, x) bool seeds -> (z, y, x) uint32 squared distances, NONE if there is no seed"""
    if not seeds.any():
        return np.full(seeds.shape, NONE, np.uint32)
    g = np.where(seeds, np.int64(0), _BIG)
    for axis in (2, 1, 0):
        g = np.minimum(_pass(g, axis), _BIG)
    assert g.max() < _BIG
    return g.astype(np.uint32)


def edt_numpy(vox, mode):
    return edt_seeds(seeds_of(vox, mode))


def edt_brute(seeds, chunk=2048):
    """|p - q|^2 = |p|^2 + |q|^2 - 2 p.q over all pairs; the products run in float32, exact for these integers (n <= 64: below 2^24)"""
    n = seeds.shape[0]
    assert n <= 64
    q = np.argwhere(seeds).astype(np.float32)                # (z, y, x)
    if len(q) == 0:
        return np.full(seeds.shape, NONE, np.uint32)
    p = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    p2 = (p * p).sum(1)
    best = np.full(len(p), np.inf, np.float32)
    for s in range(0, len(q), chunk):
        c = q[s:s + chunk]
        np.minimum(best, ((c * c).sum(1)[None, :] - np.float32(2) * (p @ c.T)).min(1), out=best)
    return (best + p2).astype(np.int64).reshape(n, n, n).astype(np.uint32)


def sdf_numpy(vox, vs, fill=-np.inf):
    """vp_edt_sdf in np.float32 arithmetic: the product vs * vs once, one conversion, one multiply; the sign from the voxel"""
    d = edt_numpy(vox, BORDER)
    if (d == NONE).all():
        return np.full(vox.shape, fill, np.float32)
    vs2 = np.float32(vs) * np.float32(vs)
    mag = d.astype(np.float32) * vs2
    return np.where(vox, mag, np.copysign(mag, np.float32(fill))).astype(np.float32)


def morph_edt(vox, op, r):
    """vp_edt_morph: dilate = D_SET <= r^2, erode = D_UNSET > r^2 (NONE passes it), open = dilate(erode), close = erode(dilate)"""
    if r == 0:
        return vox.copy()
    dil = lambda v: edt_numpy(v, SET).astype(np.int64) <= r * r        # noqa: E731
    ero = lambda v: edt_numpy(v, UNSET).astype(np.int64) > r * r       # noqa: E731
    return {0: lambda: dil(vox), 1: lambda: ero(vox), 2: lambda: dil(ero(vox)), 3: lambda: ero(dil(vox))}[op]()


def hand_cases(n):
    """[(name, mode, input (z, y, x) bool, expected (z, y, x) uint32)] -- every expectation written from the construction"""
    cases = []
    zero = np.zeros((n, n, n), bool)
    a = np.arange(n, dtype=np.int64)
    Z, Y, X = a[:, None, None], a[None, :, None], a[None, None, :]
    none = np.full((n, n, n), NONE, np.uint32)
    u32 = lambda v: np.broadcast_to(v, (n, n, n)).astype(np.uint32)     # noqa: E731
    # an empty grid has no set and no border voxel; every voxel of it is an unset one, so the UNSET transform is 0 (were it NONE, the
    # erosion D_UNSET > r^2 of the empty grid would be the full grid)
    for mode in (SET, BORDER):
        cases.append(("empty, mode %d" % mode, mode, zero.copy(), none))
    cases.append(("empty, mode 1", UNSET, zero.copy(), u32(0)))
    cases.append(("full, SET", SET, ~zero, u32(0)))
    cases.append(("full, UNSET", UNSET, ~zero, none))
    face = np.minimum(np.minimum(np.minimum(X, n - 1 - X), np.minimum(Y, n - 1 - Y)), np.minimum(Z, n - 1 - Z))
    cases.append(("full, BORDER", BORDER, ~zero, u32(face ** 2)))
    points = {"middle": (n // 2, n // 2 + 1, n // 2 - 1), "corner": (0, n - 1, 0), "x=31": (31, 5, 7), "x=n-1": (n - 1, n // 2, 3)}
    if n > 32:
        points["x=32"] = (32, n - 3, n // 2)
    for name, (px, py, pz) in points.items():
        v = zero.copy()
        v[pz, py, px] = True
        d = (X - px) ** 2 + (Y - py) ** 2 + (Z - pz) ** 2
        cases.append(("single voxel " + name, SET, v, u32(d)))
        cases.append(("single voxel " + name + ", BORDER", BORDER, v, u32(d)))          # a lone voxel is its own border
        cases.append(("all but one voxel " + name, UNSET, ~v, u32(d)))
    v = zero.copy()
    v[0, 0, 0] = v[n - 1, n - 1, n - 1] = True
    cases.append(("two opposite corners", SET, v, u32(np.minimum(X ** 2 + Y ** 2 + Z ** 2, (X - n + 1) ** 2 + (Y - n + 1) ** 2 + (Z - n + 1) ** 2))))
    for c in (31, 32) if n > 32 else (15, 31):
        v = zero.copy()
        v[:, :, c] = True
        cases.append(("wall x=%d" % c, SET, v, u32((X - c) ** 2)))
    # UNSET on a box that touches the faces x = 0, y = n - 1 and z = 0: inside, the nearest unset voxel lies just past one of the three
    # free sides x1, y0, z1 (outside the grid is never a seed); outside the box the distance is 0
    x1, y0, z1 = n - 9, 6, n // 2
    v = zero.copy()
    v[0:z1 + 1, y0:n, 0:x1 + 1] = True
    inside = np.minimum(np.minimum(x1 + 1 - X, Y - (y0 - 1)), z1 + 1 - Z)
    cases.append(("UNSET on a box on three faces", UNSET, v, u32(np.where(v, inside ** 2, 0))))
    return cases
