"""Every tile shape of the dense JFA pass (csrc/jfa_dense.hip) against the one-pass reference of jfa_pass_ref.py, inside guarded buffers.

launch_dense / launch_dense_cyclic pick one of some sixty instantiations of jfa_pass_dense from the id format, the chain lengths, the
grid side and the step.  TABLE names, per line, the smallest frame found that reaches an instantiation and the shape record
(vp_jfa_last_shapes) the call must leave; every line runs ONE pass call on a synthetic state carved out between canaries and checks

  * the record read back from the library (instantiation, tiles, split count),
  * the planes of f in `out` against pass_ref -- every voxel of a frame of at most 2^21 voxels (and of the FULL lines); on larger frames
    the rows y in [0, 16) u [n - 16, n) and 32 seeded rows, every plane, all x, plus every voxel against the one-thread-per-voxel kernel
    (VP_ALGO_NAIVE), which the small frames hold to pass_ref on every voxel themselves,
  * for the fused last pass the sdf region against final_ref, bit for bit, for both fills,
  * that nothing else was written: `out` outside the planes of f (word planes and byte planes), every canary, `in`, the bitmask.

Equality is bit equality.  launch_mirror() restates the launcher's conditions in Python; a CPU test holds TABLE to it and to a sweep over
(n, planes, k, stride, last), so a leaf added to the launcher without a line here fails without a GPU.

What no line covers, and why:
  KNOWN_EXCEPTIONS  the compact ids (n > 1024) under the cyclic plane distribution: their smallest shape is a whole grid at n = 1152 held
                    three times over; test_slab_gpu.py::test_cyclic_passes_equal_whole_grid_passes runs them.
  not selectable    instantiations the file compiles that no frame the entry points accept reaches (a frame holds a multiple of 8 planes,
                    so the chains of a pass with k = 1 are whole and a multiple of 8 long): the fused last pass on 4-plane tiles, the
                    fused last pass with run-time chain lengths, and the two-launch split of a fused last pass.  The sweep cannot
                    produce them either."""
import gc
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

from cuda_mesh_voxelization_amd.capi import ALGO_NAIVE, ALGO_TILED, Frame, Window

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float_frames as FF  # noqa: E402
import jfa_pass_ref as R  # noqa: E402

INF = float("inf")
Shape = namedtuple("Shape", "id_format rows planes threads final_pass pair_mode closed full cyclic")
MI355X_CUS = 256                                      # the split column of TABLE is that of a device with this many compute units


def S(idf, rows, planes, threads, fin=0, pm=0, cl=0, full=0, cyc=0):
    return Shape(idf, rows, planes, threads, fin, pm, cl, full, cyc)


# ---- the launcher, restated (csrc/jfa_dense.hip: tail_split, launch_tile, launch_shape, launch_dense, launch_dense_cyclic) ----------
def id_format(n):
    return 9 if n <= 512 else 10 if n <= 1024 else 11


def _tile(cus, idf, ry, ch, nt, fin, pm, cl, full, cyc, n, nresy, ylen, nres, zlen):
    t = nresy * -(-ylen // ry) * nres * -(-zlen // ch)
    if idf == 11:
        per_cu = 2
    elif idf == 9:
        per_cu = 4 if ry == 8 else 5 if fin else 6
    else:
        per_cu = (2 if ry == 8 else 3) if nt == 512 else 4
    slots = cus * per_cu
    sp = 0 if n <= nt or t >= 16 * slots else min(t // 2, slots * 4 // 3)
    return Shape(idf, ry, ch, nt, int(fin), pm, cl, int(full), int(cyc)), t, sp


def _shape(cus, idf, ch, nt, fin, always_full, cyc, pairs_ok, whole, n, k, nresy, ylen, nres, zlen):
    ktab = {9: 512, 10: 1024, 11: 2048}[idf]
    ry = 8 if (ktab == 512 and not fin and ch >= 8) else 4
    can_full = ch >= 8 and (ktab != 1024 or fin)
    pm = 0
    if ch >= 8 and pairs_ok and n % nt == 0:
        pm = 1 if fin else 2 if (ktab != 512 and k == 2) else 4 if k == 4 else 8 if (k >= 8 and k & (k - 1) == 0) else 0
    if always_full or (cyc and can_full):
        full = True
    elif can_full and whole and ylen % ry == 0:
        full, cyc = True, False
    else:
        full = False
    return _tile(cus, idf, ry, ch, nt, fin, pm, 0, full, cyc, n, nresy, ylen, nres, zlen)


def launch_mirror(n, z0, z1, k, stride, fin, cus=MI355X_CUS):
    """[(Shape, tiles, split), ...] of vp_jfa_window_pass / vp_jfa_window_last_pass, in launch order"""
    idf, nz = id_format(n), z1 - z0
    nres, zlen = min(k, nz), -(-nz // k)
    nresy, ylen = min(k, n), -(-n // k)
    if stride == k and nz % k == 0 and k < nz and zlen > 8 and zlen % 8 != 0:
        cut = z0 + (zlen // 8) * 8 * k
        return launch_mirror(n, z0, cut, k, stride, fin, cus) + launch_mirror(n, cut, z1, k, stride, fin, cus)
    assert not fin or k == 1
    pow2 = n & (n - 1) == 0
    whole = zlen % 8 == 0 and nz % k == 0 and n % k == 0
    ntd, nts = 256 if idf == 9 else 512, 512 if idf == 11 else 256
    g = (n, k, nresy, ylen, nres, zlen)
    if idf != 11 and not fin and pow2 and stride == k and z0 == 0 and z1 == n and n == 8 * k and n % ntd == 0:
        return [_tile(cus, idf, 8, 8, ntd, False, 8, 3, idf == 9, False, n, nresy, ylen, nres, zlen)]
    if idf == 11 and zlen % 16 == 0 and stride == k:
        return [_shape(cus, idf, 16, ntd, fin, False, False, pow2 and (fin or k >= 2), whole, *g)]
    if idf == 9 and n == 512 and zlen % 16 == 0 and stride == k and whole:
        return [_shape(cus, idf, 16, 512, fin, True, False, pow2 and (fin or k >= 2), True, *g)]
    if zlen % 8 == 0 or 4 < zlen < 8:
        return [_shape(cus, idf, 8, ntd, fin, False, False, pow2 and (fin or k >= 2), whole, *g)]
    return [_shape(cus, idf, 4 if fin or zlen > 2 else 2, nts, fin, False, False, False, False, *g)]


def cyclic_steps(n, ranks):
    """the steps vp_jfa_window_pass_cyclic accepts (capi.hip): the leading steps of n/2, n/4, ... that are multiples of `ranks`, less the first two"""
    if n < 96 or ranks < 2 or ranks & (ranks - 1) or n % ranks or (n // ranks) % 8:
        return []
    ks, k = [], n // 2
    while k >= 1 and k % ranks == 0:
        ks.append(k)
        k //= 2
    return ks[2:] if len(ks) >= 2 else []


def launch_mirror_cyclic(n, k, ranks, cus=MI355X_CUS):
    idf, zsh = id_format(n), ranks.bit_length() - 1
    assert n % k == 0 and n // k >= 8 and (n // k) & (n // k - 1) == 0
    pow2 = n & (n - 1) == 0
    ntd = 256 if idf == 9 else 512
    g = (n, k, min(k, n), n // k, min(k >> zsh, n >> zsh), n // k)
    if idf != 11 and pow2 and n == 8 * k and n % ntd == 0:
        return [_tile(cus, idf, 8, 8, ntd, False, 8, 3, idf == 9, True, n, *g[2:])]
    return [_shape(cus, idf, 16 if idf == 11 and (n // k) % 16 == 0 else 8, ntd, False, False, True, pow2 and k >= 2, True, *g)]


def sweep():
    """every instantiation the entry points can select: {Shape: the cheapest (voxels, call, n, z0 | rank, z1 | ranks, k, stride, last) found}"""
    found = {}

    def note(launches, cost, case):
        for s, _, _ in launches:
            if s not in found or cost < found[s][0]:
                found[s] = (cost,) + case
    for n in range(96, 2049, 32):
        ks = sorted(set(list(range(1, 35)) + [48, 64, 96, 128, 256, 512, 1024] + [n >> j for j in range(1, 12)]))
        for nz in sorted(set(list(range(8, min(n, 256) + 1, 8)) + [n, n - 8, n // 2 // 8 * 8])):
            z0 = 0 if nz == n else 8 if 8 + nz <= n else n - nz
            for k in ks:
                if not 0 < k < n:
                    continue
                for stride in [k] + ([nz] if k >= nz and nz < n else []):
                    for fin in ((False, True) if k == 1 and stride == 1 else (False,)):
                        note(launch_mirror(n, z0, z0 + nz, k, stride, fin), n * n * nz, ("win", n, z0, z0 + nz, k, stride, fin))
        for ranks in (2, 4, 8, 16):
            for k in cyclic_steps(n, ranks):
                note(launch_mirror_cyclic(n, k, ranks), n * n * n // ranks, ("cyc", n, 0, ranks, k, k // ranks, False))
    return found


# ---- the table ---------------------------------------------------------------------------------------------------------------------
# call   "win": vp_jfa_window_pass / vp_jfa_window_last_pass; "plain": vp_jfa_pass(VP_ALGO_TILED) on plain ids that are one run of
#        consecutive planes (the same shapes); "cyc": vp_jfa_window_pass_cyclic, the z columns then hold (rank, ranks)
# kind   local / uniform / empty (local with 97 % none); frame: "dyadic" or the rounding frame "far" of float_frames.py
# expect one (shape record, split > 0 on a device of MI355X_CUS compute units) per launch; a trailing FULL asks for the reference on every voxel
Case = namedtuple("Case", "call n z0 z1 k stride last kind frame expect full")
FULL = "full"


def C(call, n, z0, z1, k, stride, last, kind, frame, *expect):
    full = bool(expect) and expect[-1] == FULL
    return Case(call, n, z0, z1, k, stride, last, kind, frame, list(expect[:-1] if full else expect), full)


TABLE = [
    # ---- IdU<9>, n <= 512
    C("win", 96, 8, 16, 4, 4, 0, "local", "dyadic", (S(9, 4, 2, 256), 0)),
    C("win", 288, 8, 16, 4, 4, 0, "local", "dyadic", (S(9, 4, 2, 256), 1)),
    C("win", 96, 24, 32, 16, 8, 0, "local", "dyadic", (S(9, 4, 2, 256), 0)),                      # stride != k, slabs on both sides
    C("win", 288, 0, 8, 16, 8, 0, "uniform", "dyadic", (S(9, 4, 2, 256), 1)),                     # stride != k at the lower wall
    C("win", 96, 8, 16, 2, 2, 0, "local", "dyadic", (S(9, 4, 4, 256), 0)),
    C("win", 288, 8, 16, 2, 2, 0, "empty", "dyadic", (S(9, 4, 4, 256), 1)),
    C("win", 96, 8, 24, 3, 3, 0, "local", "dyadic", (S(9, 8, 8, 256), 0)),                        # chains of six
    C("win", 288, 8, 24, 3, 3, 0, "local", "far", (S(9, 8, 8, 256), 1)),
    C("win", 96, 8, 16, 1, 1, 0, "local", "dyadic", (S(9, 8, 8, 256, full=1), 0)),                # k = 1 that is not the last pass
    C("win", 288, 8, 16, 1, 1, 0, "local", "dyadic", (S(9, 8, 8, 256, full=1), 1)),
    C("plain", 96, 8, 16, 1, 1, 0, "local", "dyadic", (S(9, 8, 8, 256, full=1), 0)),
    C("win", 96, 8, 48, 4, 4, 0, "local", "dyadic", (S(9, 8, 8, 256, full=1), 0), (S(9, 4, 2, 256), 0)),      # chains of ten: 8 + 2
    C("win", 96, 0, 96, 8, 8, 0, "local", "dyadic", (S(9, 8, 8, 256), 0), (S(9, 4, 4, 256), 0)),             # whole grid, chains of twelve: 8 + 4
    C("win", 256, 8, 32, 4, 4, 0, "local", "dyadic", (S(9, 8, 8, 256, pm=4), 0)),
    C("win", 256, 8, 40, 4, 4, 0, "local", "dyadic", (S(9, 8, 8, 256, pm=4, full=1), 0)),
    C("plain", 256, 8, 40, 4, 4, 0, "local", "dyadic", (S(9, 8, 8, 256, pm=4, full=1), 0)),
    C("win", 256, 8, 48, 8, 8, 0, "local", "dyadic", (S(9, 8, 8, 256, pm=8), 0)),
    C("win", 256, 8, 72, 8, 8, 0, "local", "dyadic", (S(9, 8, 8, 256, pm=8, full=1), 0)),
    C("win", 256, 0, 256, 32, 32, 0, "local", "dyadic", (S(9, 8, 8, 256, pm=8, cl=3, full=1), 0)),
    # A step that is no power of two on a power-of-two grid (the ABI accepts any 0 < k < n; no pipeline of the library asks for one): these
    # three lines ran in pair mode 8, whose lane -> x map masks with k - 1, and left ids of the planes of f unwritten.  They run the plain form.
    C("win", 256, 8, 80, 12, 12, 0, "local", "dyadic", (S(9, 8, 8, 256), 0)),
    C("win", 512, 8, 24, 1, 1, 0, "local", "dyadic", (S(9, 8, 16, 512, full=1), 0)),
    C("win", 512, 8, 72, 4, 4, 0, "local", "dyadic", (S(9, 8, 16, 512, pm=4, full=1), 0)),
    C("win", 512, 8, 136, 8, 8, 0, "local", "dyadic", (S(9, 8, 16, 512, pm=8, full=1), 0)),
    C("win", 96, 8, 16, 1, 1, 1, "local", "dyadic", (S(9, 4, 8, 256, fin=1, full=1), 0)),
    C("win", 288, 8, 16, 1, 1, 1, "local", "far", (S(9, 4, 8, 256, fin=1, full=1), 1)),
    C("win", 256, 8, 16, 1, 1, 1, "local", "dyadic", (S(9, 4, 8, 256, fin=1, pm=1, full=1), 0)),
    C("win", 512, 8, 16, 1, 1, 1, "local", "dyadic", (S(9, 4, 8, 256, fin=1, pm=1, full=1), 1)),
    C("win", 512, 496, 512, 1, 1, 1, "local", "dyadic", (S(9, 4, 16, 512, fin=1, pm=1, full=1), 0)),         # at the upper wall
    C("cyc", 128, 5, 16, 16, 1, 0, "local", "dyadic", (S(9, 8, 8, 256, full=1, cyc=1), 0)),
    C("cyc", 256, 1, 4, 4, 1, 0, "local", "dyadic", (S(9, 8, 8, 256, pm=4, full=1, cyc=1), 0)),
    C("cyc", 256, 15, 16, 16, 1, 0, "local", "dyadic", (S(9, 8, 8, 256, pm=8, full=1, cyc=1), 0)),
    C("cyc", 256, 0, 16, 32, 2, 0, "local", "dyadic", (S(9, 8, 8, 256, pm=8, cl=3, full=1, cyc=1), 0)),
    # ---- IdU<10>, 512 < n <= 1024
    C("win", 544, 8, 16, 4, 4, 0, "local", "dyadic", (S(10, 4, 2, 256), 1)),
    C("win", 544, 24, 32, 16, 8, 0, "local", "dyadic", (S(10, 4, 2, 256), 1)),                    # stride != k
    C("win", 544, 8, 16, 2, 2, 0, "local", "dyadic", (S(10, 4, 4, 256), 1)),
    C("win", 544, 8, 16, 1, 1, 0, "local", "dyadic", (S(10, 4, 8, 512), 1), FULL),
    C("plain", 544, 8, 16, 1, 1, 0, "uniform", "dyadic", (S(10, 4, 8, 512), 1)),
    C("win", 544, 8, 24, 3, 3, 0, "empty", "far", (S(10, 4, 8, 512), 1)),                         # chains of six
    C("win", 544, 8, 48, 4, 4, 0, "local", "dyadic", (S(10, 4, 8, 512), 1), (S(10, 4, 2, 256), 1)),          # chains of ten: 8 + 2
    C("win", 1024, 8, 24, 2, 2, 0, "local", "dyadic", (S(10, 4, 8, 512, pm=2), 1)),
    C("win", 1024, 8, 32, 4, 4, 0, "local", "dyadic", (S(10, 4, 8, 512, pm=4), 1)),
    C("win", 1024, 8, 48, 8, 8, 0, "local", "dyadic", (S(10, 4, 8, 512, pm=8), 1)),
    C("win", 1024, 8, 80, 12, 12, 0, "local", "dyadic", (S(10, 4, 8, 512), 1)),                   # no power of two: the plain form
    C("win", 1024, 0, 1024, 128, 128, 0, "local", "dyadic", (S(10, 8, 8, 512, pm=8, cl=3), 0)),   # the one unavoidable large case
    C("win", 544, 8, 16, 1, 1, 1, "local", "dyadic", (S(10, 4, 8, 512, fin=1, full=1), 1)),
    C("win", 1024, 8, 16, 1, 1, 1, "local", "dyadic", (S(10, 4, 8, 512, fin=1, pm=1, full=1), 1)),
    C("cyc", 640, 3, 16, 80, 5, 0, "local", "dyadic", (S(10, 4, 8, 512, cyc=1), 1)),
    C("cyc", 1024, 1, 2, 2, 1, 0, "local", "dyadic", (S(10, 4, 8, 512, pm=2, cyc=1), 0)),
    C("cyc", 1024, 2, 4, 4, 1, 0, "local", "dyadic", (S(10, 4, 8, 512, pm=4, cyc=1), 1)),
    C("cyc", 1024, 7, 16, 64, 4, 0, "local", "dyadic", (S(10, 4, 8, 512, pm=8, cyc=1), 1)),
    C("cyc", 1024, 0, 16, 128, 8, 0, "local", "dyadic", (S(10, 8, 8, 512, pm=8, cl=3, cyc=1), 1)),
    # ---- IdC, n > 1024
    C("win", 1056, 8, 16, 4, 4, 0, "local", "dyadic", (S(11, 4, 2, 512), 1)),
    C("win", 1056, 8, 16, 1024, 8, 0, "local", "dyadic", (S(11, 4, 2, 512), 0)),                  # stride != k, no slab below
    C("win", 1056, 8, 16, 2, 2, 0, "uniform", "dyadic", (S(11, 4, 4, 512), 1)),
    C("win", 1056, 8, 24, 3, 3, 0, "empty", "dyadic", (S(11, 4, 8, 512), 1)),                     # chains of six
    C("win", 1056, 8, 16, 1, 1, 0, "local", "dyadic", (S(11, 4, 8, 512, full=1), 1), FULL),
    C("win", 1056, 8, 24, 1, 1, 0, "local", "far", (S(11, 4, 16, 512, full=1), 1)),
    C("win", 1056, 8, 48, 4, 4, 0, "local", "dyadic", (S(11, 4, 8, 512, full=1), 1), (S(11, 4, 2, 512), 1)),  # chains of ten: 8 + 2
    C("win", 1088, 8, 56, 3, 3, 0, "local", "dyadic", (S(11, 4, 16, 512), 1)),
    C("win", 2048, 8, 24, 2, 2, 0, "local", "dyadic", (S(11, 4, 8, 512, pm=2, full=1), 1)),
    C("win", 2048, 8, 40, 2, 2, 0, "local", "dyadic", (S(11, 4, 16, 512, pm=2, full=1), 1)),
    C("win", 2048, 8, 32, 4, 4, 0, "local", "dyadic", (S(11, 4, 8, 512, pm=4), 1)),
    C("win", 2048, 8, 40, 4, 4, 0, "local", "dyadic", (S(11, 4, 8, 512, pm=4, full=1), 1)),
    C("win", 2048, 8, 72, 4, 4, 0, "local", "dyadic", (S(11, 4, 16, 512, pm=4, full=1), 1)),
    C("win", 2048, 8, 48, 8, 8, 0, "local", "dyadic", (S(11, 4, 8, 512, pm=8), 1)),
    C("win", 2048, 8, 72, 8, 8, 0, "local", "dyadic", (S(11, 4, 8, 512, pm=8, full=1), 1)),
    C("win", 2048, 8, 136, 8, 8, 0, "local", "dyadic", (S(11, 4, 16, 512, pm=8, full=1), 1)),
    C("win", 2048, 8, 256, 16, 16, 0, "local", "dyadic", (S(11, 4, 16, 512, pm=8), 0)),
    C("win", 2048, 8, 144, 9, 9, 0, "local", "dyadic", (S(11, 4, 16, 512), 1)),                    # a step that is no power of two, see below
    C("win", 1056, 8, 16, 1, 1, 1, "local", "dyadic", (S(11, 4, 8, 512, fin=1, full=1), 1)),
    C("win", 1056, 8, 24, 1, 1, 1, "local", "far", (S(11, 4, 16, 512, fin=1, full=1), 1)),
    C("win", 2048, 8, 16, 1, 1, 1, "local", "dyadic", (S(11, 4, 8, 512, fin=1, pm=1, full=1), 1)),
    C("win", 2048, 8, 24, 1, 1, 1, "local", "dyadic", (S(11, 4, 16, 512, fin=1, pm=1, full=1), 1)),
]

# the compact ids under the cyclic plane distribution (see the head of the file)
KNOWN_EXCEPTIONS = {S(11, 4, 8, 512, full=1, cyc=1), S(11, 4, 8, 512, pm=8, full=1, cyc=1), S(11, 4, 16, 512, full=1, cyc=1),
                    S(11, 4, 16, 512, pm=2, full=1, cyc=1), S(11, 4, 16, 512, pm=4, full=1, cyc=1), S(11, 4, 16, 512, pm=8, full=1, cyc=1)}


def _id(c):
    return "%s-n%d-z%d-%d-k%d-s%d%s-%s-%s" % (c.call, c.n, c.z0, c.z1, c.k, c.stride, "-last" if c.last else "", c.kind, c.frame)


def _mirror(c, cus=MI355X_CUS):
    return launch_mirror_cyclic(c.n, c.k, c.z1, cus) if c.call == "cyc" else launch_mirror(c.n, c.z0, c.z1, c.k, c.stride, bool(c.last), cus)


# ---- without a GPU -----------------------------------------------------------------------------------------------------------------
def test_table_is_what_the_launcher_mirror_selects():
    for c in TABLE:
        assert [(s, int(sp > 0)) for s, _, sp in _mirror(c)] == c.expect, _id(c)
        assert c.n % 32 == 0 and 96 <= c.n <= 2048 and 0 < c.k < c.n
        if c.call == "cyc":
            assert c.k in cyclic_steps(c.n, c.z1) and c.z0 < c.z1 and c.stride == c.k // c.z1 and not c.last
        else:
            nz = c.z1 - c.z0
            assert c.z0 % 8 == 0 and c.z1 % 8 == 0 and 0 <= c.z0 < c.z1 <= c.n and (not c.last or c.k == c.stride == 1)
            assert c.stride == c.k or (c.k >= nz and c.stride >= nz)
            assert c.call == "win" or (c.n <= 1024 and c.stride == c.k)


def test_table_covers_every_instantiation_the_sweep_can_produce():
    can = sweep()
    covered = {s for c in TABLE for s, _ in c.expect}
    assert KNOWN_EXCEPTIONS <= set(can) and not (KNOWN_EXCEPTIONS & covered)
    missing, stale = set(can) - KNOWN_EXCEPTIONS - covered, covered - set(can)
    assert not missing, "instantiations without a line in TABLE, and the cheapest case found for each: %s" % {s: can[s] for s in missing}
    assert not stale, "lines of TABLE for shapes the sweep cannot produce: %s" % stale
    # the two-launch split of a pass, a step that spans whole slabs and both split columns, per id format; slabs away from both walls and at each
    for idf in (9, 10, 11):
        mine = [c for c in TABLE if id_format(c.n) == idf]
        assert any(len(c.expect) == 2 for c in mine) and any(c.call == "win" and c.stride != c.k for c in mine)
        assert {sp for c in mine for _, sp in c.expect} == {0, 1}
        assert sum(c.full or (c.call != "cyc" and c.n * c.n * (c.z1 - c.z0) <= 1 << 21) for c in mine if c.kind == "local") >= 1
        assert {"uniform", "empty", "local"} <= {c.kind for c in mine} and "far" in {c.frame for c in mine}
    assert any(c.call == "win" and c.z0 == 0 and c.z1 < c.n for c in TABLE) and any(c.call == "win" and c.z0 > 0 and c.z1 == c.n for c in TABLE)
    # a fused last pass is never split and never runs on 4-plane tiles or with run-time chain lengths: nothing of that kind can be selected
    assert all(s.full and s.planes >= 8 for s in can if s.final_pass)
    assert all(len(launch_mirror(n, 8, 8 + nz, 1, 1, True)) == 1 for n in (96, 544, 1056, 2048) for nz in range(8, 89, 8))


# ---- on the GPU --------------------------------------------------------------------------------------------------------------------
GUARD = 4096
CANARY = 0xA5                                         # 0xA5A5A5A5 is no valid id at any n, and no "none" either (test_first_two_rows_gpu.py)


class Guarded:
    """`nbytes` between two canaries of GUARD bytes, all of it one allocation filled with CANARY"""

    def __init__(self, nbytes, device):
        assert nbytes % 16 == 0
        self.buf = torch.full((GUARD + nbytes + GUARD,), CANARY, dtype=torch.uint8, device=device)
        self.nbytes, self.ptr, self.body = nbytes, self.buf.data_ptr() + GUARD, self.buf[GUARD:GUARD + nbytes]
        assert self.ptr % 16 == 0

    def canaries_intact(self):
        return bool((self.buf[:GUARD] == CANARY).all()) and bool((self.buf[GUARD + self.nbytes:] == CANARY).all())

    def all_canary(self, a, b):
        return bool((self.body[a:b] == CANARY).all())


class Win(Guarded):
    """an id window of `planes` planes in the library's layout (4-byte ids up to n = 1024; above, the word planes and then the byte planes)"""

    def __init__(self, n, planes, device):
        self.n, self.planes, self.idf = n, planes, id_format(n)
        super().__init__(n * n * planes * (5 if n > 1024 else 4), device)
        self.w = self.body[:planes * n * n * 4].view(torch.int32).view(planes, n, n)
        self.b = self.body[planes * n * n * 4:].view(planes, n, n) if n > 1024 else None

    def window(self, at):
        return Window.make(self.ptr, self.nbytes, self.planes, at)

    def store(self, p0, s):
        if self.idf == 11:
            word, byte = R.encode_c(s)
            self.w[p0:p0 + word.shape[0]] = R.words(word)
            self.b[p0:p0 + word.shape[0]] = byte.to(torch.uint8)
        else:
            v = R.encode_u(s, self.idf)
            self.w[p0:p0 + v.shape[0]] = R.words(v)

    def load(self, p0, p1, rows=None):
        """the planes [p0, p1) (the rows `rows` of them) as a state on the device"""
        pick = (lambda t: t[p0:p1]) if rows is None else (lambda t: t[p0:p1][:, rows, :])
        if self.idf == 11:
            return R.decode_c(R.from_words(pick(self.w)), pick(self.b).long())
        return R.decode_u(R.from_words(pick(self.w)), self.idf)

    def untouched_outside(self, a, b):
        """every byte but those of the planes [a, b) still holds the canary"""
        pw, pb, wp = self.n * self.n * 4, self.n * self.n, self.planes * self.n * self.n * 4
        ok = self.canaries_intact() and self.all_canary(0, a * pw) and self.all_canary(b * pw, wp)
        return ok and (self.b is None or (self.all_canary(wp, wp + a * pb) and self.all_canary(wp + b * pb, self.nbytes)))


def _host(s):
    """a device state on the host, 32-bit"""
    g = lambda t: t.to(torch.int32).cpu().numpy()
    return R.State(g(s.x), g(s.y), g(s.z), s.none.cpu().numpy())


def _rows(n, seed):
    """y in [0, 16) u [n - 16, n) and 32 seeded rows"""
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([np.arange(16), np.arange(n - 16, n), rng.choice(np.arange(16, n - 16), 32, replace=False)]))


def _layout(c):
    """(planes of the window, at, the global z of every window plane) of a line: what the pass reads around the planes of f plus two spare
    planes on each side; planes outside the grid and the spare ones hold valid ids that nothing may read or write"""
    if c.call == "cyc":
        return c.n // c.z1, 0, c.z0 + c.z1 * np.arange(c.n // c.z1)
    nz = c.z1 - c.z0
    if c.stride == c.k:
        below, above = min(c.k, c.z0), min(c.k, c.n - c.z1)
        at = 2 + below
        planes = at + nz + above + 2
        return planes, at, c.z0 + np.arange(planes) - at
    below, above = (c.stride if c.z1 > c.k else 0), (c.stride if c.z0 + c.k < c.n else 0)     # capi.hip: pass_reach
    at = 2 + below
    planes = at + nz + above + 2
    zg = c.z0 + np.arange(planes) - at
    zg[:at] += c.stride - c.k                                         # [slab holding z - k | own slab | slab holding z + k]
    zg[at + nz:] += c.k - c.stride
    return planes, at, zg


def _fill_state(win, c, zg, device, seed):
    share = 0.97 if c.kind == "empty" else 0.3
    step = max(1, (1 << 25) // (c.n * c.n))
    for p in range(0, win.planes, step):
        z = zg[p:p + step]
        s = R.uniform_state(z, c.n, seed + p, share, device) if c.kind == "uniform" else R.local_state(z, c.n, c.k, seed + p, share, device)
        win.store(p, s)
        del s


def _record(ctx):
    return [(Shape(*(d[f] for f in ("id_format", "rows", "planes", "threads", "final_pass", "pair_mode", "closed", "full", "cyclic"))), d["tiles"], d["split"])
            for d in ctx.jfa_last_shapes()]


@pytest.mark.gpu
@pytest.mark.parametrize("c", TABLE, ids=_id)
def test_tile_shape_against_the_one_pass_reference(engine, c):
    ctx, dev, n, k = engine.ctx, engine.device, c.n, c.k
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    seed = 1000 * TABLE.index(c)
    if c.frame == "dyadic":
        vs, origin = R.DYADIC
    else:
        vs, origin, _ = FF.check_band("far", n)
    frame = (float(vs), tuple(float(o) for o in origin))
    planes, at, zg = _layout(c)
    cyc = c.call == "cyc"
    fr = Frame.make(n, frame[0], frame[1]) if cyc else Frame.make(n, frame[0], frame[1], c.z0, c.z1)
    nz = planes if cyc else c.z1 - c.z0
    voxels = n * n * nz
    plane_bytes = n * n * 4

    # 1. the state, in the window layout between canaries; `out` holds nothing but canary
    win_in, win_out = Win(n, planes, dev), Win(n, planes, dev)
    _fill_state(win_in, c, zg, dev, seed)
    before = win_in.buf.clone()
    fills = (-INF, INF) if c.last else (None,)
    if c.last:
        gw, gs = Guarded(voxels // 8, dev), Guarded(voxels * 4, dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed + 7)
        gw.body.view(torch.int32).copy_(torch.randint(-2 ** 31, 2 ** 31, (voxels // 32,), generator=gen, device=dev, dtype=torch.int64).to(torch.int32))
        words_before = gw.buf.clone()

    # the slab as the plain-id calls address it (vphip.h, vp_jfa_pass): d_in = plane z0, d_minus = the unclipped start of the planes z - k
    def plain_ptrs(base, id_bytes):
        pb = n * n * id_bytes
        d_in = base + at * pb
        d_minus = (d_in - c.stride * pb if at >= c.stride or c.stride == k else d_in) if c.z0 > 0 else None
        d_plus = d_in + (max(c.z1, c.z0 + k) - c.z0 if c.stride == k else c.stride) * pb if c.z1 < n else None
        return d_in, d_minus, d_plus

    for fill in fills:
        # 2. one call, and what it says it launched
        if cyc:
            ctx.jfa_window_pass_cyclic(fr, k, win_in.window(0), win_out.window(0), c.z1, c.z0)
        elif c.last:
            ctx.jfa_window_last_pass(fr, win_in.window(at), win_out.window(at), gw.ptr, fill, gs.ptr, stride=1)
        elif c.call == "plain":
            d_in, d_minus, d_plus = plain_ptrs(win_in.ptr, 4)
            ctx.jfa_pass(fr, k, d_in, d_minus, d_plus, win_out.ptr + at * plane_bytes, ALGO_TILED)
        else:
            ctx.jfa_window_pass(fr, k, win_in.window(at), win_out.window(at), stride=c.stride)
        got = _record(ctx)
        engine.sync()
        assert [(s, int(sp > 0)) for s, _, sp in got] == c.expect or cus != MI355X_CUS, (got, c.expect)
        assert got == _mirror(c, cus), (got, _mirror(c, cus))

        # 3. what it may write
        assert torch.equal(win_in.buf, before), "the pass wrote to its input window"
        assert win_out.untouched_outside(at, at + nz), "the pass wrote outside the planes of f (or into a canary)"
        if c.last:
            assert torch.equal(gw.buf, words_before) and gs.canaries_intact(), "the last pass wrote to the bitmask or outside the sdf region"

        # 4. the reference: every voxel of a small frame, the rows of a large one
        small = voxels <= (1 << 21) or c.full
        rows = None if small else _rows(n, seed)
        held = None if small else np.unique(np.clip(np.concatenate([rows + d * k for d in (-1, 0, 1)]), 0, n - 1))
        pick = None if small else torch.as_tensor(held, device=dev)
        state = _host(win_in.load(0, planes, pick))
        if cyc:
            ref = R.pass_ref(state, n, k, c.stride, frame, c.z0, n, 0, rows=rows, zstep=c.z1, state_rows=held)
        else:
            ref = R.pass_ref(state, n, k, c.stride, frame, c.z0, c.z1, at, rows=rows, state_rows=held)
        rpick = None if small else torch.as_tensor(rows, device=dev)
        if not c.last:
            # every id of the planes of f was written: no canary is left, and a byte of the compact ids is one of 0, 2, 4 (jfa_common.h)
            if n > 1024:
                assert bool(((win_out.b[at:at + nz] & 0xF9) == 0).all()), "byte plane of the planes of f"
            assert bool((win_out.w[at:at + nz] != R.words(torch.tensor(0xA5A5A5A5))).all()), "an id of the planes of f was not written"
            mine = _host(win_out.load(at, at + nz, rpick))
            assert mine.same(ref), ("tile kernel against pass_ref", mine.mismatches(ref), "of", ref.none.size)
        else:
            occ = FF.unpack(gw.body.view(torch.int32).cpu().numpy().view(np.uint32), n, nz)
            want = R.final_ref(ref, occ if small else occ[:, rows, :], fill)
            sdf = gs.body.view(torch.int32).view(nz, n, n)
            mine = (sdf if small else sdf[:, rpick, :]).cpu().numpy().view(np.uint32)
            assert np.array_equal(mine, want.view(np.uint32)), ("fused last pass against final_ref", fill, int((mine != want.view(np.uint32)).sum()))

        # 5. the one-thread-per-voxel kernel on the same state: held to the reference on the small frames, the stand-in for it on the large ones
        if not cyc:
            if n <= 1024:
                base, idb = win_in.ptr, 4
            else:                                                     # the same state as plain 8-byte ids
                plain = torch.empty((planes, n, n), dtype=torch.int64, device=dev)
                step = max(1, (1 << 25) // (n * n))
                for p in range(0, planes, step):
                    plain[p:p + step] = R.encode_64(win_in.load(p, min(planes, p + step)))
                base, idb = plain.data_ptr(), 8
            d_in, d_minus, d_plus = plain_ptrs(base, idb)
            nout = Guarded(voxels * idb, dev)
            if c.last:
                nsdf = Guarded(voxels * 4, dev)
                ctx.jfa_last_pass(fr, d_in, d_minus, d_plus, nout.ptr, gw.ptr, fill, nsdf.ptr, ALGO_NAIVE)
            else:
                ctx.jfa_pass(fr, k, d_in, d_minus, d_plus, nout.ptr, ALGO_NAIVE)
            assert _record(ctx) == []                                 # no tile kernel in that call
            engine.sync()
            assert nout.canaries_intact()
            if c.last:
                assert nsdf.canaries_intact() and torch.equal(nsdf.body, gs.body), "fused last pass against the direct kernel + finalize"
            elif n <= 1024:
                assert torch.equal(nout.body.view(torch.int32).view(nz, n, n), win_out.w[at:at + nz]), "tile kernel against the direct kernel"
            else:
                ids = nout.body.view(torch.int64).view(nz, n, n)
                step = max(1, (1 << 25) // (n * n))
                for p in range(0, nz, step):
                    assert R.decode_64(ids[p:p + step]).same(win_out.load(at + p, at + min(nz, p + step))), "tile kernel against the direct kernel"
            if small and not c.last:
                ids = nout.body.view(torch.int32 if idb == 4 else torch.int64).view(nz, n, n)
                naive = _host(R.decode_u(R.from_words(ids), id_format(n)) if idb == 4 else R.decode_64(ids))
                assert naive.same(ref), ("direct kernel against pass_ref", naive.mismatches(ref))
            del nout
        if c.last and fill == -INF:                                   # the second fill starts from clean outputs
            win_out.buf.fill_(CANARY)
            gs.buf.fill_(CANARY)
    del win_in, win_out, before
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_the_record_is_that_of_the_last_pass_call_only(engine):
    """vp_jfa_last_shapes: cleared by every pass call -- one that is refused and one served by another kernel leave it empty"""
    from cuda_mesh_voxelization_amd import capi
    ctx, dev, n = engine.ctx, engine.device, 96
    fr = Frame.make(n, *R.DYADIC, 8, 16)
    a, b = Win(n, 16, dev), Win(n, 16, dev)
    _fill_state(a, TABLE[0], np.arange(16), dev, 5)
    ctx.jfa_window_pass(fr, 4, a.window(4), b.window(4))
    assert [s for s, _, _ in _record(ctx)] == [S(9, 4, 2, 256)]
    with pytest.raises(capi.VPError):
        ctx.jfa_window_pass(fr, 4, a.window(4), b.window(14))       # the windows differ in `at`: refused
    assert _record(ctx) == []
    ctx.jfa_window_pass(fr, 4, a.window(4), b.window(4))
    assert len(_record(ctx)) == 1
    ctx.jfa_pass(fr, 4, a.ptr + 4 * n * n * 4, a.ptr, a.ptr + 12 * n * n * 4, b.ptr, ALGO_NAIVE)
    assert _record(ctx) == []
    engine.sync()
