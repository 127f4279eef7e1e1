"""One JFA pass, restated: shared by test_jfa_pass_ref_cpu.py, test_jfa_dense_shapes_gpu.py and test_gpu_parity.py.

The COORDINATE FORM of a state is what an id means, free of any layout: integer arrays x, y, z (the voxel coordinates of the best seed so
far) and a boolean `none` (no seed yet), one entry per voxel of a run of window planes, shaped [planes, n, n] (z, y, x).  Where `none` is
set the coordinates mean nothing (the decoders give 0 there).

pass_ref     one pass with step k in numpy: the voxel's own state first (distance +inf if it is none), then the 26 candidates with dz, dy,
             dx over -1, 0, 1 in that nesting order, a candidate being the state of the voxel at +-k along x and y and of the plane
             `stride` WINDOW planes away along z; skipped when the global coordinate leaves [0, n) or when it is none; accepted on
             d < best only (the reference's jfa/sequential.cpp:84-112).  Distances are float32 and written as csrc/jfa_common.h writes
             them (axis_pos / seed_distance): o + float(i) * vs per axis, ((sx - px)^2 + (sy - py)^2) + (sz - pz)^2, nothing contracted.
final_ref    ids -> sdf by the rule of csrc/jfa_seed.hip: jfa_final.
encode_* / decode_*   between the coordinate form and the four id layouts of csrc/jfa_common.h (IdU<9>, IdU<10>, Id64, IdC), on numpy
             arrays and on torch tensors alike; they return / take the VALUES of the words (int64 in [0, 2^32)) and bytes, words() /
             from_words() turn them into the int32 / uint32 storage.
local_state / uniform_state   seeded states of valid ids (torch, any device)."""
import numpy as np

F = np.float32
NONE9, NONE10 = 0xFF9FF200, 0xFFDFFC00                # IdU<9> / IdU<10>: x = 2^BITS, y and z fields all ones
NONE_C_WORD, NONE_C_BYTE = 0xFFFFF800, 4              # IdC
DYADIC = (0.03125, (0.25, -1.0, 3.5))                 # every position, difference, square and sum is exact: equidistant seeds tie exactly
ROUNDING = (0.37, (-1.5, 2.25, 0.125))                # the positions round


class State:
    """x, y, z, none [planes, n, n]; d: the float32 distance of a pass_ref result (+inf where none)"""

    def __init__(self, x, y, z, none, d=None):
        self.x, self.y, self.z, self.none, self.d = x, y, z, none, d

    def planes(self, a, b):
        return State(self.x[a:b], self.y[a:b], self.z[a:b], self.none[a:b], None if self.d is None else self.d[a:b])

    def numpy(self):
        g = lambda t: t if isinstance(t, np.ndarray) else t.cpu().numpy()
        return State(g(self.x), g(self.y), g(self.z), g(self.none), None if self.d is None else g(self.d))

    def same(self, other):
        """equal as states: the same `none`, and the same coordinates wherever a seed is held"""
        if isinstance(self.none, np.ndarray):
            return bool(np.array_equal(self.none, other.none)) and all(bool(np.array_equal(np.where(self.none, 0, a), np.where(other.none, 0, b)))
                                                                       for a, b in ((self.x, other.x), (self.y, other.y), (self.z, other.z)))
        import torch
        return bool(torch.equal(self.none, other.none)) and all(bool(torch.equal(torch.where(self.none, 0, a), torch.where(other.none, 0, b)))
                                                                for a, b in ((self.x, other.x), (self.y, other.y), (self.z, other.z)))

    def mismatches(self, other):
        bad = self.none != other.none
        for a, b in ((self.x, other.x), (self.y, other.y), (self.z, other.z)):
            bad = bad | (~self.none & (a != b))
        return int(bad.sum())


def _where(c, a, b):
    if isinstance(c, np.ndarray):
        return np.where(c, a, b)
    import torch
    return torch.where(c, a, b)


def _i64(a):
    return a.astype(np.int64) if isinstance(a, np.ndarray) else a.long()


def scr(i):
    """the scramble of the y and z fields (jfa_common.h): the low five bits XORed with the next five; an involution"""
    return i ^ ((i >> 5) & 31)


# ---- the four layouts ------------------------------------------------------------------------------------------------------------
def encode_u(s, bits):
    """IdU<bits>, bits = 9 | 10: x | scr(y) << kYS | scr(z) << kZS; "none" = NONE9 / NONE10"""
    ys, zs, none = (12, 23, NONE9) if bits == 9 else (11, 22, NONE10)
    v = _i64(s.x) | (scr(_i64(s.y)) << ys) | (scr(_i64(s.z)) << zs)
    return _where(s.none, none, v)


def decode_u(word, bits):
    ys, zs, none = (12, 23, NONE9) if bits == 9 else (11, 22, NONE10)
    m = (1 << bits) - 1
    isn = word == none
    z = lambda a: _where(isn, 0, a)
    return State(z(word & (2 * m + 1)), z(scr((word >> ys) & m)), z(scr((word >> zs) & m)), isn)


def encode_64(s):
    """Id64 as ONE int64 per id (little endian: .x the low word = scr(z) << 2 | x << 13, .y the high word = scr(y) << 2); "none" = all ones"""
    lo = (scr(_i64(s.z)) << 2) | (_i64(s.x) << 13)
    return _where(s.none, -1, lo | ((scr(_i64(s.y)) << 2) << 32))


def decode_64(t):
    x, sy, sz, isn = coords_plain64(t)
    z = lambda a: _where(isn, 0, a)
    return State(z(x), z(scr(sy)), z(scr(sz)), isn)


def encode_c(s):
    """IdC: (word, byte) -- word = x | scr(y) << 11 | (scr(z) & 1023) << 22, byte = top bit of scr(z) << 1; "none" = (0xFFFFF800, 4)"""
    sz = scr(_i64(s.z))
    word = _i64(s.x) | (scr(_i64(s.y)) << 11) | ((sz & 1023) << 22)
    return _where(s.none, NONE_C_WORD, word), _where(s.none, NONE_C_BYTE, (sz >> 10) << 1)


def decode_c(word, byte):
    isn = (byte & 4) != 0
    z = lambda a: _where(isn, 0, a)
    return State(z(word & 2047), z(scr((word >> 11) & 2047)), z(scr(((word >> 22) & 1023) | ((byte & 2) << 9))), isn)


def words(v):
    """word VALUES (int64 in [0, 2^32)) -> storage: uint32 in numpy, int32 of the same bits in torch"""
    if isinstance(v, np.ndarray):
        return v.astype(np.uint32)
    import torch
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)


def from_words(t):
    """storage -> word VALUES"""
    return t.astype(np.int64) & 0xFFFFFFFF if isinstance(t, np.ndarray) else t.long() & 0xFFFFFFFF


# the decoders test_gpu_parity.py compares its two pass sequences with above n = 1024 (torch; y and z stay scrambled)
def coords_plain64(t):
    """(x, scr(y), scr(z), none) of plain 8-byte ids (jfa_common.h: Id64 -- .x = scr(z) << 2 | x << 13, .y = scr(y) << 2, "none" = all ones)"""
    lo, hi = (t & 0xFFFFFFFF), ((t >> 32) & 0xFFFFFFFF)
    none = lo == 0xFFFFFFFF
    return (lo >> 13) & 2047, (hi >> 2) & 2047, (lo >> 2) & 2047, none


def coords_window(w, planes, n):
    """the same of a window above n = 1024 (IdC: word plane x | scr(y) << 11 | (scr(z) & 1023) << 22, byte plane = top z bit << 1 | none << 2)"""
    import torch
    vox = planes * n * n
    word = w[:vox * 4].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    byte = w[vox * 4:vox * 5].to(torch.int64)
    return word & 2047, (word >> 11) & 2047, ((word >> 22) & 1023) | ((byte & 2) << 9), (byte & 4) != 0


# ---- one pass --------------------------------------------------------------------------------------------------------------------
def positions(n, frame):
    """float32 voxel positions per axis: o + (float(i) * vs) (jfa_common.h: axis_pos)"""
    vs, o = F(frame[0]), np.asarray(frame[1], F)
    return [o[a] + (np.arange(n, dtype=np.int64).astype(F) * vs) for a in range(3)]


def pass_ref(state, n, k, stride, frame, z0, z1, at, rows=None, zstep=1, state_rows=None):
    """The planes [z0, z1) after one pass with step k.  `state` holds window planes (numpy); the plane of global z0 is state plane `at`,
    the planes z - k / z + k of a plane are found `stride` state planes below / above it.  rows: evaluate these y rows only (every plane,
    all x; the result is then [planes, len(rows), n]).  state_rows: the state holds only these y rows, in ascending order (they must
    include `rows` and their neighbours at -+k inside the grid).  zstep > 1: a cyclic plane distribution -- the state planes hold the
    global planes z0, z0 + zstep, ... below z1.  Returns a State with .d, the float32 distance of the winner."""
    pos = positions(n, frame)
    ys = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    zg = np.arange(z0, z1, zstep, dtype=np.int64)
    nzp, planes = zg.size, state.x.shape[0]
    px, py, pz = pos[0][None, None, :], pos[1][ys][None, :, None], pos[2][zg][:, None, None]
    held = None if state_rows is None else np.asarray(state_rows, np.int64)

    def rows_at(dy):              # every state plane at the rows ys + dy k (vy: which exist): the seeds held there and their positions
        yy = ys + dy * k
        vy = (yy >= 0) & (yy < n)
        yc = np.clip(yy, 0, n - 1)
        if held is not None:
            at_ = np.clip(np.searchsorted(held, yc), 0, held.size - 1)
            assert (held[at_] == yc)[vy].all(), "the state does not hold the rows this pass reads"
            yc = at_
        x, y, z, none = (a[:, yc, :] for a in (state.x, state.y, state.z, state.none))
        return vy, (pos[0][x], pos[1][y], pos[2][z], none), (x, y, z)

    def dist(c, lo, hi, x0, x1, bx, by, bz):                          # of the seeds c[lo:hi, :, x0:x1] from the voxels at (bx, by, bz)
        dx, dy, dz = c[0][lo:hi, :, x0:x1] - bx, c[1][lo:hi, :, x0:x1] - by, c[2][lo:hi, :, x0:x1] - bz
        return ((dx * dx) + (dy * dy)) + (dz * dz)

    at_rows = {dy: rows_at(dy) for dy in (-1, 0, 1)}
    own = at_rows[0][1]
    bn = own[3][at:at + nzp].copy()
    best = np.where(bn, F(np.inf), dist(own, at, at + nzp, 0, n, px, py, pz)).astype(F)
    won = np.full(best.shape, 13, np.int8)                           # which of the 27 won (13: the own state); coordinates are fetched at the end
    out = [a[at:at + nzp].astype(np.int64) for a in at_rows[0][2]]

    def boxes(p0, p1):                                                # (candidate, output box, source box) in the order of the scan
        for dz in (-1, 0, 1):
            ok_z = np.flatnonzero((zg[p0:p1] + dz * k >= 0) & (zg[p0:p1] + dz * k < n))
            if ok_z.size == 0:
                continue
            a, b = p0 + int(ok_z[0]), p0 + int(ok_z[-1]) + 1            # zg is monotonic: the planes that have this neighbour are one run
            sa, sb = at + a + dz * stride, at + b + dz * stride
            assert 0 <= sa and sb <= planes, "the state does not hold the planes this pass reads"
            for dy in (-1, 0, 1):
                if not at_rows[dy][0].any():
                    continue
                for dx in (-1, 0, 1):
                    xlo, xhi = max(0, -dx * k), min(n, n - dx * k)
                    if (dz, dy, dx) != (0, 0, 0) and xlo < xhi:
                        yield (dz + 1) * 9 + (dy + 1) * 3 + dx + 1, dy, (slice(a, b), slice(None), slice(xlo, xhi)), (slice(sa, sb), slice(None), slice(xlo + dx * k, xhi + dx * k))

    def run(p0, p1):                                                  # the output planes [p0, p1)
        for c, dy, o, s_ in boxes(p0, p1):
            vy, src, _ = at_rows[dy]
            d = dist(src, s_[0].start, s_[0].stop, s_[2].start, s_[2].stop, px[:, :, o[2]], py, pz[o[0]])
            take = (d < best[o]) & ~src[3][s_] & vy[None, :, None]
            np.copyto(best[o], d, where=take)
            np.copyto(won[o], c, where=take)
            bn[o] &= ~take
        for c, dy, o, s_ in boxes(p0, p1):
            take = won[o] == c
            for dst, src in zip(out, at_rows[dy][2]):
                np.copyto(dst[o], src[s_], where=take)

    step = max(1, -(-nzp // 16))
    chunks = [(p, min(nzp, p + step)) for p in range(0, nzp, step)]
    if best.size < (1 << 18) or len(chunks) == 1:
        run(0, nzp)
    else:                                                             # disjoint plane ranges side by side (numpy releases the lock)
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=len(chunks)) as ex:
            list(ex.map(lambda c: run(*c), chunks))
    return State(*(np.where(bn, 0, v) for v in out), bn, best)


def final_ref(state, occ, fill):
    """The sdf of a pass_ref result (jfa_seed.hip: jfa_final): init = +inf for a set voxel, `fill` otherwise; a none id gives init,
    anything else copysign(d, init).  occ: bool, shaped like the state."""
    init = np.where(occ, F(np.inf), F(fill)).astype(F)
    return np.where(state.none, init, np.copysign(state.d, init)).astype(F)


# ---- states ----------------------------------------------------------------------------------------------------------------------
def _gen(seed, device):
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    return g


def _finish(x, y, z, n, none_share, g):
    import torch
    none = torch.rand(x.shape, generator=g, device=x.device) < none_share
    zero = lambda a: torch.where(none, 0, a.clamp(0, n - 1))
    return State(zero(x), zero(y), zero(z), none)


def local_state(zglobal, n, k, seed, none_share=0.3, device="cpu"):
    """Valid ids near their voxel: the seed of voxel (x, y, z) is the voxel plus, per axis, an offset a * c with a drawn from -2 .. 2 and
    c from {1, k} (so up to 2 k away), clipped to the grid -- full of candidates at exactly the same distance.  zglobal: the global z of
    each plane of the state.  none_share of the voxels hold no seed (0.97: the nearly empty variant)."""
    import torch
    g = _gen(seed, device)
    zg = torch.as_tensor(np.asarray(zglobal, np.int64), device=device)
    shape = (zg.numel(), n, n)
    ar = torch.arange(n, device=device)

    def off():
        a = torch.randint(-2, 3, shape, generator=g, device=device)
        c = torch.where(torch.rand(shape, generator=g, device=device) < 0.5, 1, int(k))
        return a * c
    return _finish(ar[None, None, :] + off(), ar[None, :, None] + off(), zg[:, None, None] + off(), n, none_share, g)


def uniform_state(zglobal, n, seed, none_share=0.3, device="cpu"):
    """Valid ids anywhere: every voxel holds any voxel of the grid"""
    import torch
    g = _gen(seed, device)
    shape = (len(zglobal), n, n)
    r = lambda: torch.randint(0, n, shape, generator=g, device=device)
    return _finish(r(), r(), r(), n, none_share, g)
