"""numpy restatements of the generalized winding number (include/vphip.h, vp_winding).

winding_f32    the contract: float32 arrays, one IEEE operation per numpy call in the header's association, the library's own atan2
               polynomial, every term quantised to int64 before it is added, the pyramid of bricks and the per-(brick, node) far test.
               Returns (w float32[n^3], inside words uint32[n^3 / 32]).
winding_f64    an independent float64 brute force over all voxels x all valid triangles with np.arctan2.  Returns w float64[n^3].
parity_f64     float64 crossing parity along +x from the voxel centres (closed meshes): bool[n^3].
Results are cached per argument bytes, computed once and handed out read-only."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import meshdist_ref as MR

F = np.float32
D = np.float64
_CHUNK = 1 << 19            # (voxel, term) pairs per numpy pass
_cache = {}

ATAN_C = [F(float.fromhex(h)) for h in ("0x1.000000p+0", "-0x1.5554eep-2", "0x1.9986eap-3", "-0x1.23c878p-3", "0x1.bd901cp-4",
                                        "-0x1.506f4ap-4", "0x1.c2c986p-5", "-0x1.d2c990p-6", "0x1.397f42p-7", "-0x1.8ba540p-10")]
HALF_PI, PI = F(float.fromhex("0x1.921fb6p+0")), F(float.fromhex("0x1.921fb6p+1"))
FOUR_PI = float.fromhex("0x1.921fb54442d18p+3")
Q36 = 2.0 ** 36

centres = MR.centres
valid_triangles = MR.valid_triangles


def _dot(a, b):
    return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2])


def atan2w(y, x):
    """the library's atan2 on float32 arrays (x, y finite, not both zero where the value is used)"""
    with np.errstate(all="ignore"):
        ax, ay = np.abs(x), np.abs(y)
        t = np.minimum(ax, ay) / np.maximum(ax, ay)
        s = t * t
        q = np.full_like(s, ATAN_C[9])
        for c in ATAN_C[8::-1]:
            q = (q * s) + c
        r = q * t
        r = np.where(ay > ax, HALF_PI - r, r)
        r = np.where(x < 0, PI - r, r)
        return np.where(y < 0, -r, r)


def _quantise(om):
    return np.rint(om.astype(D) * Q36).astype(np.int64)


def exact_terms(P, A, B, C):
    """quantised solid angles, int64 (V, T): points P (V, 3) against triangles A, B, C (T, 3), float32"""
    with np.errstate(all="ignore"):
        a = [A[None, :, i] - P[:, i, None] for i in range(3)]
        b = [B[None, :, i] - P[:, i, None] for i in range(3)]
        c = [C[None, :, i] - P[:, i, None] for i in range(3)]
        la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
        x = [(b[1] * c[2]) - (b[2] * c[1]), (b[2] * c[0]) - (b[0] * c[2]), (b[0] * c[1]) - (b[1] * c[0])]
        det = _dot(a, x)
        den = ((((la * lb) * lc) + (_dot(a, b) * lc)) + (_dot(b, c) * la)) + (_dot(c, a) * lb)
        ok = (det != 0) & np.isfinite(det) & np.isfinite(den)
        om = F(2.0) * atan2w(det, den)
        return _quantise(np.where(ok, om, F(0.0)))


def _ord(v):
    b = np.ascontiguousarray(v, F).view(np.uint32)
    return b ^ np.where(b >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def _unord(k):
    return (k ^ np.where(k >> 31 != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(F)


def level_dims(n):
    nb, dims = n // 8, []
    while True:
        dims.append((nb + (1 << len(dims)) - 1) >> len(dims))
        if dims[-1] == 1:
            return dims


def pyramid(xyz, tri, n, vs, origin):
    """the hierarchy of the contract: (records (T', 3, 3) sorted by leaf, leaf offsets, levels) with levels[k] = dict(count, c, r, N)"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    tri = np.asarray(tri, np.uint32).reshape(-1, 3)
    vs, origin = F(vs), np.asarray(origin, F)
    nb, dims = n // 8, level_dims(n)
    ok = valid_triangles(xyz, tri)
    v = xyz[tri[ok].astype(np.int64)] if ok.size else np.zeros((0, 3, 3), F)       # (T', vertex, axis)
    with np.errstate(all="ignore"):
        g = ((v[:, 0] + v[:, 1]) + v[:, 2]) / F(3.0)
        q = np.floor(((g - origin[None, :]) / vs) / F(8.0))
        b = np.where(q >= F(nb - 1), nb - 1, np.where(q > 0, q, 0).astype(np.int64)).astype(np.int64)
        e0, e1 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 1]
        nrm = np.stack([(e0[:, 1] * e1[:, 2]) - (e0[:, 2] * e1[:, 1]), (e0[:, 2] * e1[:, 0]) - (e0[:, 0] * e1[:, 2]),
                        (e0[:, 0] * e1[:, 1]) - (e0[:, 1] * e1[:, 0])], 1)
        u = D(vs) * D(vs)
        s = (nrm.astype(D) * 2.0 ** 23) / u
        s = np.where(s > 2.0 ** 62, 2.0 ** 62, s)
        s = np.where(s < -2.0 ** 62, -2.0 ** 62, s)
        s = np.where(s != s, 0.0, s)
        area = np.rint(s).astype(np.int64)
    leaf = b[:, 0] + nb * (b[:, 1] + nb * b[:, 2])
    order = np.argsort(leaf, kind="stable")
    rec = v[order]
    count = np.bincount(leaf, minlength=nb ** 3).astype(np.int64)
    leaf_off = np.concatenate([[0], np.cumsum(count)])
    keys = _ord(v)                                                 # (T', 3, 3) uint32
    lo = np.full((nb ** 3, 3), 0xFFFFFFFF, np.uint32)
    hi = np.zeros((nb ** 3, 3), np.uint32)
    A = np.zeros((nb ** 3, 3), np.int64)
    for k in range(3):
        np.minimum.at(lo, leaf, keys[:, k])
        np.maximum.at(hi, leaf, keys[:, k])
    np.add.at(A, leaf, area)                                       # wraps modulo 2^64
    levels = []
    for k, d in enumerate(dims):
        if k:
            dl = dims[k - 1]
            z, y, x = np.meshgrid(np.arange(dl), np.arange(dl), np.arange(dl), indexing="ij")
            parent = ((x >> 1) + d * ((y >> 1) + d * (z >> 1))).reshape(-1)
            c2, l2, h2, A2 = np.zeros(d ** 3, np.int64), np.full((d ** 3, 3), 0xFFFFFFFF, np.uint32), np.zeros((d ** 3, 3), np.uint32), np.zeros((d ** 3, 3), np.int64)
            some = count > 0
            np.add.at(c2, parent, count)
            np.minimum.at(l2, parent[some], lo[some])
            np.maximum.at(h2, parent[some], hi[some])
            np.add.at(A2, parent, A)
            count, lo, hi, A = c2, l2, h2, A2
        with np.errstate(all="ignore"):
            flo, fhi = _unord(lo), _unord(hi)
            h = (fhi - flo) / F(2.0)
            c = flo + h
            r = np.sqrt(_dot([h[:, 0], h[:, 1], h[:, 2]], [h[:, 0], h[:, 1], h[:, 2]]))
            N = (A.astype(D) * (u * 2.0 ** -24)).astype(F)
        levels.append(dict(count=count, c=c, r=r, N=N, dim=d))
    return rec, leaf_off, levels


def _brick_centres(n, vs, origin, first):
    nb = n // 8
    i = (np.arange(nb, dtype=np.int64) * 8 + (0 if first else 7)).astype(F)
    ax = [F(origin[a]) + ((i * F(vs)) + (F(vs) / F(2.0))) for a in range(3)]
    z, y, x = np.meshgrid(np.arange(nb), np.arange(nb), np.arange(nb), indexing="ij")
    return np.stack([ax[0][x.reshape(-1)], ax[1][y.reshape(-1)], ax[2][z.reshape(-1)]], 1)           # brick index x + nb (y + nb z)


def walk(n, vs, origin, levels, beta):
    """the per-(brick, node) evaluation of the contract for every brick at once: (far pairs [(brick, level, node)], near pairs (brick, leaf))"""
    nb = n // 8
    blo, bhi = _brick_centres(n, vs, origin, True), _brick_centres(n, vs, origin, False)
    beta = F(beta)
    top = len(levels) - 1
    bricks, nodes = np.arange(nb ** 3, dtype=np.int64), np.zeros(nb ** 3, np.int64)
    far, near = [], (np.zeros(0, np.int64), np.zeros(0, np.int64))
    for k in range(top, -1, -1):
        L = levels[k]
        live = L["count"][nodes] > 0
        bricks, nodes = bricks[live], nodes[live]
        with np.errstate(all="ignore"):
            c = L["c"][nodes]
            g = []
            for a in range(3):
                m = np.where(blo[bricks, a] - c[:, a] > c[:, a] - bhi[bricks, a], blo[bricks, a] - c[:, a], c[:, a] - bhi[bricks, a])
                g.append(np.where(F(0.0) > m, F(0.0), m))
            br = beta * L["r"][nodes]
            isfar = (_dot(g, g) > br * br) & (beta > 0)
        far.append((bricks[isfar], k, nodes[isfar]))
        bricks, nodes = bricks[~isfar], nodes[~isfar]
        if k == 0:
            near = (bricks, nodes)
            break
        d, dl = L["dim"], levels[k - 1]["dim"]
        x, y, z = nodes % d, (nodes // d) % d, nodes // (d * d)
        nb_, nn_ = [], []
        for j in range(8):
            cx, cy, cz = 2 * x + (j & 1), 2 * y + ((j >> 1) & 1), 2 * z + (j >> 2)
            inside = (cx < dl) & (cy < dl) & (cz < dl)
            nb_.append(bricks[inside])
            nn_.append((cx + dl * (cy + dl * cz))[inside])
        bricks, nodes = np.concatenate(nb_), np.concatenate(nn_)
    return far, near


def _key(*arrays):
    return tuple(np.ascontiguousarray(a).tobytes() if isinstance(a, np.ndarray) else a for a in arrays)


def winding_sums(xyz, tri, n, vs, origin, beta):
    """S: the int64 sum of the quantised terms per voxel, x fastest"""
    xyz, tri, origin = np.asarray(xyz, F).reshape(-1, 3), np.asarray(tri, np.uint32).reshape(-1, 3), np.asarray(origin, F)
    key = ("S", _key(xyz, tri, origin), n, float(F(vs)), float(F(beta)))
    if key in _cache:
        return _cache[key]
    nb = n // 8
    rec, leaf_off, levels = pyramid(xyz, tri, n, vs, origin)
    far, (nbrick, nleaf) = walk(n, vs, origin, levels, beta)
    P = centres(n, vs, origin).reshape(nb, 8, nb, 8, nb, 8, 3).transpose(0, 2, 4, 1, 3, 5, 6).reshape(nb ** 3, 512, 3)   # [brick][voxel in brick]
    S = np.zeros((nb ** 3, 512), np.int64)
    # far terms: one per (brick, node) pair and voxel of the brick
    for bricks, k, nodes in far:
        c, N = levels[k]["c"], levels[k]["N"]
        for s in range(0, bricks.size, _CHUNK // 512):
            b_, n_ = bricks[s:s + _CHUNK // 512], nodes[s:s + _CHUNK // 512]
            with np.errstate(all="ignore"):
                d = [c[n_, i][:, None] - P[b_, :, i] for i in range(3)]
                r2 = _dot(d, d)
                om = _dot(d, [N[n_, i][:, None] for i in range(3)]) / (r2 * np.sqrt(r2))
                q = _quantise(np.where(np.isfinite(om), om, F(0.0)))
            np.add.at(S, b_, q)
    # exact terms: the triangles of the near leaves, brick by brick
    order = np.argsort(nbrick, kind="stable")
    nbrick, nleaf = nbrick[order], nleaf[order]
    starts = np.searchsorted(nbrick, np.arange(nb ** 3 + 1))
    for b in range(nb ** 3):
        leaves = nleaf[starts[b]:starts[b + 1]]
        if not leaves.size:
            continue
        idx = np.concatenate([np.arange(leaf_off[l], leaf_off[l + 1]) for l in leaves])
        for s in range(0, idx.size, _CHUNK // 512):
            r = rec[idx[s:s + _CHUNK // 512]]
            S[b] += exact_terms(P[b], r[:, 0], r[:, 1], r[:, 2]).sum(1)
    out = S.reshape(nb, nb, nb, 8, 8, 8).transpose(0, 3, 1, 4, 2, 5).reshape(-1)
    out.setflags(write=False)
    _cache[key] = out
    return out


def finish(S, level):
    """(w float32, inside words uint32) from the integer sums"""
    w = ((S.astype(D) * 2.0 ** -36) / FOUR_PI).astype(F)
    bits = (w >= F(level))
    words = np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1)
    return w, words


def winding_f32(xyz, tri, n, vs, origin, beta=0.0, level=0.5):
    return finish(winding_sums(xyz, tri, n, vs, origin, beta), level)


def winding_f64(xyz, tri, n, vs, origin):
    """independent float64 brute force (np.arctan2) at the float32 voxel centres over the valid triangles"""
    xyz, tri, origin = np.asarray(xyz, F).reshape(-1, 3), np.asarray(tri, np.uint32).reshape(-1, 3), np.asarray(origin, F)
    key = ("w64", _key(xyz, tri, origin), n, float(F(vs)))
    if key in _cache:
        return _cache[key]
    ok = valid_triangles(xyz, tri)
    v = xyz[tri[ok].astype(np.int64)].astype(D) if ok.size else np.zeros((0, 3, 3))
    P = centres(n, vs, origin).astype(D)
    w = np.zeros(P.shape[0])
    step = max(1, (_CHUNK // 4) // max(1, v.shape[0]))

    def part(s):
        p = P[s:s + step, None, :]
        a, b, c = v[None, :, 0] - p, v[None, :, 1] - p, v[None, :, 2] - p
        la, lb, lc = np.linalg.norm(a, axis=2), np.linalg.norm(b, axis=2), np.linalg.norm(c, axis=2)
        det = np.einsum("vti,vti->vt", a, np.cross(b, c))
        den = la * lb * lc + np.einsum("vti,vti->vt", a, b) * lc + np.einsum("vti,vti->vt", b, c) * la + np.einsum("vti,vti->vt", c, a) * lb
        w[s:s + step] = (2.0 * np.arctan2(det, den)).sum(1)

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:      # numpy releases the GIL
        list(ex.map(part, range(0, P.shape[0], step)))
    w /= 4.0 * np.pi
    w.setflags(write=False)
    _cache[key] = w
    return w


def parity_f64(xyz, tri, n, vs, origin):
    """float64 crossing parity of the ray from each voxel centre along +x (closed meshes in general position): bool[n^3]"""
    xyz, tri, origin = np.asarray(xyz, F).reshape(-1, 3), np.asarray(tri, np.uint32).reshape(-1, 3), np.asarray(origin, F)
    ok = valid_triangles(xyz, tri)
    v = xyz[tri[ok].astype(np.int64)].astype(D)
    P = centres(n, vs, origin).astype(D).reshape(n, n, n, 3)
    ys, zs, xs = P[0, :, 0, 1], P[:, 0, 0, 2], P[0, 0, :, 0]
    cnt = np.zeros((n, n, n), np.int64)                            # (z, y, x)
    for t in v:
        a, b, c = t
        ylo, yhi, zlo, zhi = t[:, 1].min(), t[:, 1].max(), t[:, 2].min(), t[:, 2].max()
        jy = np.nonzero((ys >= ylo) & (ys <= yhi))[0]
        jz = np.nonzero((zs >= zlo) & (zs <= zhi))[0]
        if not jy.size or not jz.size:
            continue
        Y, Z = np.meshgrid(ys[jy], zs[jz], indexing="xy")         # (len jz, len jy)
        # barycentric coordinates of (Y, Z) in the projection of the triangle onto the yz plane
        d = (b[1] - a[1]) * (c[2] - a[2]) - (c[1] - a[1]) * (b[2] - a[2])
        if d == 0:
            continue
        u = ((Y - a[1]) * (c[2] - a[2]) - (c[1] - a[1]) * (Z - a[2])) / d
        w_ = ((b[1] - a[1]) * (Z - a[2]) - (Y - a[1]) * (b[2] - a[2])) / d
        hit = (u >= 0) & (w_ >= 0) & (u + w_ <= 1)
        X = a[0] + u * (b[0] - a[0]) + w_ * (c[0] - a[0])
        zi, yi = np.nonzero(hit)
        for k in range(zi.size):
            cnt[jz[zi[k]], jy[yi[k]], :] += xs < X[zi[k], yi[k]]
    return (cnt & 1).astype(bool).reshape(-1)
