"""tests/jfa_pass_ref.py against the CPU oracle and against itself (no GPU): the one-pass reference that test_jfa_dense_shapes_gpu.py
holds the tile kernels to has to BE the reference's pass.

Iterated from the oracle's own zero set over k = n/2 .. 1 and converted by final_ref it must give the oracle's sdf bit for bit, for both
fills, on a dyadic frame and on one whose positions round; a slab and a window of three slabs must give the planes of the whole-grid
evaluation; every id layout must survive encode -> decode, the far corner (the pattern closest to "none") and "none" itself included."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import float_frames as FF  # noqa: E402
import jfa_pass_ref as R  # noqa: E402

INF = float("inf")


@functools.lru_cache(maxsize=None)
def _words(kind, n):
    rng = np.random.default_rng([n, len(kind)])
    occ = rng.random((n, n, n)) < (0.5 if kind == "noise" else 0.01)
    w = FF.pack(occ)
    w.setflags(write=False)
    return w


def _seed_state(zero):
    """every voxel of the zero set its own seed, nothing else has one (jfa/sequential.cpp:55-60)"""
    n = zero.shape[0]
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    return R.State(np.where(zero, x, 0), np.where(zero, y, 0), np.where(zero, z, 0), ~zero)


@pytest.mark.parametrize("frame", [R.DYADIC, R.ROUNDING], ids=["dyadic", "rounding"])
@pytest.mark.parametrize("kind,n", [("noise", 32), ("sparse", 32), ("sparse", 64)])
def test_iterated_passes_give_the_oracle_sdf(kind, n, frame):
    words = _words(kind, n)
    vs, origin = frame
    occ = FF.unpack(words, n)
    oracle = {fill: O.jfa(words, n, vs, origin, fill=fill).reshape(n, n, n) for fill in (-INF, INF)}
    # the seeds are the oracle's own: its border rule is not restated here
    zero = oracle[-INF] == 0
    assert zero.any() and np.array_equal(zero, oracle[INF] == 0)
    s = _seed_state(zero)
    k = n // 2
    while k >= 1:
        s = R.pass_ref(s, n, k, k, frame, 0, n, 0)
        k //= 2
    for fill in (-INF, INF):
        got = R.final_ref(s, occ, fill)
        assert got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), oracle[fill].view(np.uint32)), (kind, n, fill, int((got.view(np.uint32) != oracle[fill].view(np.uint32)).sum()))


def _np_state(kind, n, k, seed, share=0.3):
    zg = np.arange(n)
    s = R.local_state(zg, n, k, seed, share) if kind == "local" else R.uniform_state(zg, n, seed, share)
    return s.numpy()


@pytest.mark.parametrize("kind", ["local", "uniform"])
@pytest.mark.parametrize("k", [1, 4, 8, 24])
def test_slab_and_rows_equal_the_whole_grid_evaluation(kind, k):
    n = 48
    s = _np_state(kind, n, k, 7 + k)
    whole = R.pass_ref(s, n, k, k, R.ROUNDING, 0, n, 0)
    assert not whole.none.all()
    z0, z1 = 16, 32
    # a window of consecutive planes that holds exactly what the pass reads, the slab somewhere inside it
    lo, hi = max(0, z0 - k), min(n, z1 + k)
    slab = R.pass_ref(s.planes(lo, hi), n, k, k, R.ROUNDING, z0, z1, z0 - lo)
    assert slab.same(whole.planes(z0, z1)) and np.array_equal(slab.d, whole.d[z0:z1])
    # both walls
    for a, b in ((0, 8), (n - 8, n)):
        lo, hi = max(0, a - k), min(n, b + k)
        part = R.pass_ref(s.planes(lo, hi), n, k, k, R.ROUNDING, a, b, a - lo)
        assert part.same(whole.planes(a, b))
    rows = [0, 1, 17, n - 1]
    some = R.pass_ref(s, n, k, k, R.ROUNDING, z0, z1, z0, rows=rows)
    assert some.same(R.State(whole.x[z0:z1, rows], whole.y[z0:z1, rows], whole.z[z0:z1, rows], whole.none[z0:z1, rows]))
    # ... and from a state that holds nothing but the rows the evaluation reads
    held = np.unique(np.clip(np.concatenate([np.array(rows) + d * k for d in (-1, 0, 1)]), 0, n - 1))
    few = R.pass_ref(R.State(s.x[:, held], s.y[:, held], s.z[:, held], s.none[:, held]), n, k, k, R.ROUNDING, z0, z1, z0, rows=rows, state_rows=held)
    assert few.same(some) and np.array_equal(few.d, some.d)


@pytest.mark.parametrize("z0,k", [(16, 16), (0, 16), (32, 16), (16, 24)])
def test_window_of_three_slabs_equals_the_whole_grid_evaluation(z0, k):
    """stride != k: [slab holding z - k | own slab | slab holding z + k], each `nz` planes, where they exist (planes nobody reads are none)"""
    n, nz = 48, 16 if k == 16 else 8
    z1 = z0 + nz
    s = _np_state("local", n, k, 3 * z0 + k)
    whole = R.pass_ref(s, n, k, k, R.DYADIC, 0, n, 0)
    parts = []
    for base in (z0 - k, z0, z0 + k):
        if 0 <= base and base + nz <= n:
            parts.append(s.planes(base, base + nz))
        else:
            e = np.zeros((nz, n, n), np.int64)
            parts.append(R.State(e, e, e, np.ones((nz, n, n), bool)))
    win = R.State(*(np.concatenate([getattr(p, f) for p in parts]) for f in ("x", "y", "z", "none")))
    got = R.pass_ref(win, n, k, nz, R.DYADIC, z0, z1, nz)
    assert got.same(whole.planes(z0, z1)) and np.array_equal(got.d, whole.d[z0:z1])


def test_cyclic_planes_equal_the_whole_grid_evaluation():
    n, k, ranks = 64, 8, 4
    s = _np_state("local", n, k, 11)
    whole = R.pass_ref(s, n, k, k, R.DYADIC, 0, n, 0)
    for rank in range(ranks):
        mine = R.State(s.x[rank::ranks], s.y[rank::ranks], s.z[rank::ranks], s.none[rank::ranks])
        got = R.pass_ref(mine, n, k, k // ranks, R.DYADIC, rank, n, 0, zstep=ranks)
        assert got.same(R.State(whole.x[rank::ranks], whole.y[rank::ranks], whole.z[rank::ranks], whole.none[rank::ranks]))


def test_ties_keep_the_first_candidate_and_the_own_state():
    """two seeds at the same distance: the voxel's own state wins over any candidate, and an earlier candidate over a later one"""
    n, k = 32, 4
    e = np.zeros((n, n, n), np.int64)
    s = R.State(e.copy(), e.copy(), e.copy(), np.ones((n, n, n), bool))

    def put(at, seed):
        s.x[at[2], at[1], at[0]], s.y[at[2], at[1], at[0]], s.z[at[2], at[1], at[0]] = seed
        s.none[at[2], at[1], at[0]] = False
    v = (12, 12, 12)
    put((v[0] - k, v[1], v[2]), (10, 12, 12))          # dx = -1: 2 away along x -- comes before ...
    put((v[0] + k, v[1], v[2]), (14, 12, 12))          # ... dx = +1: 2 away as well
    r = R.pass_ref(s, n, k, k, R.DYADIC, 0, n, 0)
    assert (r.x[12, 12, 12], r.y[12, 12, 12], r.z[12, 12, 12], r.none[12, 12, 12]) == (10, 12, 12, False)
    put(v, (12, 14, 12))                               # its own state at the same distance stays
    r = R.pass_ref(s, n, k, k, R.DYADIC, 0, n, 0)
    assert (r.x[12, 12, 12], r.y[12, 12, 12], r.z[12, 12, 12]) == (12, 14, 12)
    put((v[0], v[1], v[2] - k), (12, 12, 10))          # dz = -1 comes before every dy / dx of the own plane
    s.none[12, 12, 12] = True
    r = R.pass_ref(s, n, k, k, R.DYADIC, 0, n, 0)
    assert (r.x[12, 12, 12], r.y[12, 12, 12], r.z[12, 12, 12]) == (12, 12, 10)
    assert r.d[12, 12, 12] == np.float32(4 * 0.03125 * 0.03125)


def _corner_cases(n, rng):
    """the far corner, the origin, single-axis extremes and random voxels; the last entry is none"""
    c = np.concatenate([np.array([[n - 1] * 3, [0, 0, 0], [n - 1, 0, 0], [0, n - 1, 0], [0, 0, n - 1], [31, 32, 33]]), rng.integers(0, n, (500, 3)), [[0, 0, 0]]])
    none = np.zeros(len(c), bool)
    none[-1] = True
    return R.State(c[:, 0].copy(), c[:, 1].copy(), c[:, 2].copy(), none)


@pytest.mark.parametrize("n", [96, 512, 1024, 2048])
@pytest.mark.parametrize("lib", ["numpy", "torch"])
def test_layouts_round_trip(n, lib):
    s = _corner_cases(n, np.random.default_rng(n))
    if lib == "torch":
        s = R.State(*(torch.from_numpy(a) for a in (s.x, s.y, s.z, s.none)))
    every = lambda a: bool(a.all())
    if n <= 512:
        w = R.encode_u(s, 9)
        assert int(w[-1]) == R.NONE9 == 0xFF9FF200 and int(w[0]) != R.NONE9 and every(w[:-1] != R.NONE9)
        assert R.decode_u(R.from_words(R.words(w)), 9).same(s)
    if n <= 1024:
        w = R.encode_u(s, 10)
        assert int(w[-1]) == R.NONE10 == 0xFFDFFC00 and every(w[:-1] != R.NONE10)
        assert R.decode_u(R.from_words(R.words(w)), 10).same(s)
    t = R.encode_64(s)
    assert int(t[-1]) == -1 and every(t[:-1] >= 0)
    assert R.decode_64(t).same(s)
    word, byte = R.encode_c(s)
    assert (int(word[-1]), int(byte[-1])) == (0xFFFFF800, 4) and every((byte[:-1] == 0) | (byte[:-1] == 2))
    assert every((word >= 0) & (word < 2 ** 32))
    assert R.decode_c(R.from_words(R.words(word)), byte).same(s)
    # the formats agree on what a state is
    assert R.decode_c(word, byte).same(R.decode_64(t))


def test_words_storage_keeps_the_bits():
    v = np.array([0, 1, 2 ** 31 - 1, 2 ** 31, R.NONE9, 2 ** 32 - 1], np.int64)
    assert np.array_equal(R.words(v), v.astype(np.uint32))
    t = R.words(torch.from_numpy(v))
    assert t.dtype == torch.int32 and np.array_equal(t.numpy().view(np.uint32), v.astype(np.uint32))
    assert np.array_equal(R.from_words(t).numpy(), v)


@pytest.mark.parametrize("kind", ["local", "uniform"])
def test_generators_give_valid_seeded_states(kind):
    n, k = 96, 8
    zg = np.arange(8, 24)
    make = (lambda seed, share=0.3: R.local_state(zg, n, k, seed, share)) if kind == "local" else (lambda seed, share=0.3: R.uniform_state(zg, n, seed, share))
    a, b, c = make(1).numpy(), make(1).numpy(), make(2).numpy()
    assert a.same(b) and not a.same(c)
    for s in (a, make(3, 0.97).numpy()):
        for v in (s.x, s.y, s.z):
            assert v.min() >= 0 and v.max() < n
    assert 0.25 < a.none.mean() < 0.35 and 0.95 < make(3, 0.97).numpy().none.mean() < 0.99
    if kind == "local":
        z, y, x = np.meshgrid(zg, np.arange(n), np.arange(n), indexing="ij")
        for v, own in ((a.x, x), (a.y, y), (a.z, z)):
            assert np.abs(np.where(a.none, 0, v - own)).max() <= 2 * k
