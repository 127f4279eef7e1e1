"""Translation of the cases of regions_ref / geodesic_ref / watershed_ref into a larger grid (helpers, no tests).  vp_regions, vp_geodesic
and vp_watershed are exactly translation-equivariant: outside the grid counts as label 0, as outside the mask, as unset.  So the result
of a small case placed at an offset inside a grid of side 1024 -- where no numpy reference can run -- is the small reference moved, by the
rules below; tests/test_embed_cpu.py proves every rule against the plain references at small sides.

  embed(small, n, offset, device=None, fill=0)   a (z, y, x) array in a grid of side n that holds `fill` elsewhere.  device = None: numpy,
                                   the same dtype, (n, n, n).  With a device: a flat int32 torch tensor made ON that device, torch.full plus
                                   one slice assignment -- n^3 values of a volume (read as uint32), or the n^3 / 32 words of the
                                   library's bit layout for a bool array (the rows of the box are packed on the host, whole words wide).
                                   Nothing of size n^3 is made on the host.
  box(t, n, m, offset)             the sub-box of a flat device volume, on the host: uint32 (m, m, m)
  box_bits(t, n, m, offset)        the same of a flat device bit grid: bool (m, m, m)
  nonzero_words(small, offset)     how many words of the embedded bit grid are not 0 (what torch.count_nonzero must find in the whole grid)
  shift_regions(T, offset, n_small, n_big)          a reference table moved, in Python ints
  shift_geodesic_stats(stats, offset, n_small, n_big)   the statistics moved: only the linear index of the farthest voxel changes.  The
                                   order of the linear indices inside the box is kept, so the LOWEST index that attains the maximum stays
                                   the same voxel.  Watershed statistics do not change at all.
  full_block_table(x0, y0, z0, n, value)   the record of one label over one whole block of 32 x 16 x 16 voxels, by closed form
  PHASE_OFFSETS, phase_crossings   the eight placements of tests/test_phases_gpu.py and what each one crosses"""
import numpy as np

WORDS = 26


def embed(small, n, offset, device=None, fill=0):
    small = np.asarray(small)
    ox, oy, oz = (int(v) for v in offset)
    mz, my, mx = small.shape
    assert 0 <= ox and ox + mx <= n and 0 <= oy and oy + my <= n and 0 <= oz and oz + mz <= n and n % 32 == 0
    if device is None:
        big = np.full((n, n, n), fill, small.dtype)
        big[oz:oz + mz, oy:oy + my, ox:ox + mx] = small
        return big
    import torch
    if small.dtype == np.bool_:
        assert not fill
        rows, w0 = _packed_rows(small, ox)
        big = torch.zeros((n, n, n // 32), dtype=torch.int32, device=device)
        big[oz:oz + mz, oy:oy + my, w0:w0 + rows.shape[2]] = torch.from_numpy(rows.view(np.int32)).to(device)
        return big.view(-1)
    assert small.dtype.itemsize == 4
    big = torch.full((n, n, n), int(np.array(fill, np.uint32).view(np.int32)), dtype=torch.int32, device=device)
    big[oz:oz + mz, oy:oy + my, ox:ox + mx] = torch.from_numpy(np.array(small).view(np.int32)).to(device)
    return big.view(-1)


def _packed_rows(small, ox):
    """(the rows of a bool box whose x starts at ox as whole words, uint32 (mz, my, words); the index of their first word in a row)"""
    mz, my, mx = small.shape
    w0, w1 = ox // 32, (ox + mx + 31) // 32
    wide = np.zeros((mz, my, (w1 - w0) * 32), bool)
    wide[:, :, ox - 32 * w0:ox - 32 * w0 + mx] = small
    return np.packbits(wide.reshape(-1), bitorder="little").view(np.uint32).reshape(mz, my, w1 - w0), w0


def nonzero_words(small, offset):
    return int(np.count_nonzero(_packed_rows(np.asarray(small, bool), int(offset[0]))[0]))


def box(t, n, m, offset):
    ox, oy, oz = (int(v) for v in offset)
    return t.view(n, n, n)[oz:oz + m, oy:oy + m, ox:ox + m].cpu().numpy().view(np.uint32)


def box_bits(t, n, m, offset):
    ox, oy, oz = (int(v) for v in offset)
    w0, w1 = ox // 32, (ox + m + 31) // 32
    words = np.ascontiguousarray(t.view(n, n, n // 32)[oz:oz + m, oy:oy + m, w0:w1].cpu().numpy()).view(np.uint32)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little").reshape(m, m, (w1 - w0) * 32).astype(bool)
    return bits[:, :, ox - 32 * w0:ox - 32 * w0 + m]


def relinearise(index, offset, n_small, n_big):
    ox, oy, oz = (int(v) for v in offset)
    i = int(index)
    x, y, z = i % n_small, (i // n_small) % n_small, i // (n_small * n_small)
    return x + ox + n_big * (y + oy + n_big * (z + oz))


def shift_regions(T, offset, n_small, n_big):
    """words 1 - 6 add the offset, 7 - 9 add V o, 10 - 12 add 2 o S + V o^2, 13 - 15 add oa Sb + ob Sa + V oa ob, word 25 is linearised with
    n_big; words 0 and 16 - 24 stay, and so do the four totals; a record with V = 0 stays all zero"""
    o = [int(v) for v in offset]
    out = np.zeros(np.asarray(T).shape, np.uint64)
    for k, rec in enumerate(np.asarray(T)):
        r = [int(v) for v in rec]
        V, S = r[0], r[7:10]
        if V == 0:
            continue
        for a in range(3):
            r[1 + a] += o[a]
            r[4 + a] += o[a]
            r[7 + a] += V * o[a]
            r[10 + a] += 2 * o[a] * S[a] + V * o[a] * o[a]
        for word, (a, b) in ((13, (0, 1)), (14, (0, 2)), (15, (1, 2))):
            r[word] += o[a] * S[b] + o[b] * S[a] + V * o[a] * o[b]
        r[25] = relinearise(r[25], o, n_small, n_big)
        assert max(r) < 1 << 64
        out[k] = np.array(r, np.uint64)
    return out


def shift_geodesic_stats(stats, offset, n_small, n_big):
    if stats[1] == 0:
        return tuple(stats)
    return (stats[0], stats[1], stats[2], relinearise(stats[3], offset, n_small, n_big))


def full_block_table(x0, y0, z0, n, value=None):
    """label 1 on the voxels x0 <= x < x0 + 32, y0 <= y < y0 + 16, z0 <= z < z0 + 16 of a grid of side n, every value `value`: the table
    (1, 26) and the totals, in Python ints"""
    ex, ey, ez = 32, 16, 16
    V = ex * ey * ez
    s1 = [sum(range(c, c + e)) for c, e in ((x0, ex), (y0, ey), (z0, ez))]             # sum of a coordinate over its own axis
    s2 = [sum(v * v for v in range(c, c + e)) for c, e in ((x0, ex), (y0, ey), (z0, ez))]
    ext = (ex, ey, ez)
    r = [0] * WORDS
    r[0] = V
    r[1:4] = [x0, y0, z0]
    r[4:7] = [x0 + ex - 1, y0 + ey - 1, z0 + ez - 1]
    for a in range(3):
        r[7 + a] = s1[a] * V // ext[a]
        r[10 + a] = s2[a] * V // ext[a]
        r[16 + a] = 2 * V // ext[a]                                                     # the two faces across axis a
    for word, (a, b) in ((13, (0, 1)), (14, (0, 2)), (15, (1, 2))):
        r[word] = s1[a] * s1[b] * V // (ext[a] * ext[b])
    r[20] = (ex + 1) * (ey + 1) * (ez + 1)
    r[21] = ex * (ey + 1) * (ez + 1) + (ex + 1) * ey * (ez + 1) + (ex + 1) * (ey + 1) * ez
    if value is not None:
        r[22:25] = [V * int(value), int(value), int(value)]
    r[25] = x0 + n * (y0 + n * z0)
    return np.array([r], np.uint64), (V, 1, 0, 0)


# ---- the placements of tests/test_phases_gpu.py ------------------------------------------------------------------------------------------
# A piece of side PHASE_SIDE whose voxels fill the bounding box PHASE_LO .. PHASE_HI on every axis (12 voxels: it fits one block of 16
# and reaches the end of the piece) in a grid of side 64.  name: (ox, oy, oz)
PHASE_SIDE, PHASE_LO, PHASE_HI, PHASE_GRID = 24, 12, 23, 64
PHASE_OFFSETS = {
    "x word seam": (12, 5, 22),
    "y seam 15|16": (4, 2, 6),
    "z seam 31|32": (38, 6, 14),
    "z seam 47|48": (22, 21, 30),
    "edge xy": (14, 27, 5),
    "edge yz": (6, 10, 1),
    "block corner": (14, 14, 30),
    "last voxels": (40, 40, 40),
}
PHASE_CROSSINGS = {
    "x word seam": ((31,), (), ()), "y seam 15|16": ((), (15,), ()), "z seam 31|32": ((), (), (31,)), "z seam 47|48": ((), (), (47,)),
    "edge xy": ((31,), (47,), ()), "edge yz": ((), (31,), (15,)), "block corner": ((31,), (31,), (47,)), "last voxels": ((), (), ()),
}


def phase_crossings(offset):
    """per axis the seams s | s + 1 of the block lattice (x: words of 32, y and z: 16) that the piece's bounding box crosses at this offset"""
    out = []
    for axis, o in enumerate(offset):
        lo, hi = o + PHASE_LO, o + PHASE_HI
        out.append(tuple(s for s in range((32 if axis == 0 else 16) - 1, PHASE_GRID - 1, 32 if axis == 0 else 16) if lo <= s < hi))
    return tuple(out)


def phase_piece(feature):
    """the piece of a feature, read-only arrays of side PHASE_SIDE:
    regions    (W, K, values): a ball cut in two labels that touch (the kind of regions_ref's "halves")
    geodesic   (mask, seeds): two boxes of side 6 that touch only at a corner (the kind of geodesic_ref's "contact corner"), the seed in the
               first; at the placement "block corner" the shared corner is the block corner (32, 32, 48)
    watershed  (mask, markers, priority, order, q): two overlapping balls, a marker in each, flooded from the high end of the squared
               distance to the outside (the kind of watershed_ref's "equal balls")"""
    import regions_ref
    import watershed_ref
    m = PHASE_SIDE
    if feature == "regions":
        z, y, x = np.indices((m, m, m))
        W = np.where(regions_ref.ball(m, (17.5, 17.5, 17.5), 42), np.where(x < 18, 1, 2), 0).astype(np.uint32)
        values = np.random.default_rng(24).integers(0, 1 << 32, W.shape, dtype=np.uint64).astype(np.uint32)
        out = (W, 2, values)
    elif feature == "geodesic":
        mask = np.zeros((m, m, m), bool)
        mask[12:18, 12:18, 12:18] = True
        mask[18:24, 18:24, 18:24] = True
        seeds = np.zeros((m, m, m), bool)
        seeds[14, 15, 13] = True
        out = (mask, seeds)
    else:
        mask = watershed_ref.ball(m, (15.5, 15.5, 15.5), 3.9) | watershed_ref.ball(m, (19.5, 19.5, 19.5), 3.9)
        markers = watershed_ref.marker_volume(m, [((15, 15, 15), 2), ((20, 20, 20), 1)])
        out = (mask, markers, watershed_ref.inside_d2(mask).astype(np.uint32), watershed_ref.DESCENDING, 1)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
