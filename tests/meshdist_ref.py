"""numpy restatements of the mesh distance field (include/vphip.h, vp_mesh_distance).

mesh_distance_f32   the contract: brute force over all voxels x all triangles, every intermediate an np.float32 array, one IEEE operation per
                    numpy call in the header's association, the region walk's branches by np.where.  Returns (dist2, nearest).
mesh_distance_f64   an independent float64 distance in another formulation: the minimum of the in-triangle plane projection and the three
                    segment distances.  Returns (dist2 unsigned float64, nearest, second-best dist2) without any band.
Results are cached per argument bytes, computed once and handed out read-only."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
_CHUNK = 1 << 18            # (voxel, triangle) pairs per numpy pass
_cache = {}


def centres(n, vs, origin):
    """(n^3, 3) float32 voxel centres, x fastest: o.a + (((float)i * vs) + (vs / 2.0f))"""
    vs = F(vs)
    i = np.arange(n, dtype=np.int64).astype(F)
    ax = [F(origin[a]) + ((i * vs) + (vs / F(2.0))) for a in range(3)]
    out = np.empty((n, n, n, 3), F)
    out[..., 0] = ax[0][None, None, :]
    out[..., 1] = ax[1][None, :, None]
    out[..., 2] = ax[2][:, None, None]
    return out.reshape(-1, 3)


def valid_triangles(xyz, tri):
    """indices of the triangles that contribute: every index < nverts, every coordinate finite, Cross(e0, e1) != 0 in float32"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    tri = np.asarray(tri, np.uint32).reshape(-1, 3)
    ok = (tri < xyz.shape[0]).all(1)
    safe = np.where(ok[:, None], tri, 0).astype(np.int64)
    if xyz.shape[0] == 0:
        return np.zeros(0, np.int64)
    v = xyz[safe]                                                 # (T, 3 vertices, 3 axes)
    ok &= np.isfinite(v).all((1, 2))
    with np.errstate(all="ignore"):
        e0, e1 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 1]
        nx = (e0[:, 1] * e1[:, 2]) - (e0[:, 2] * e1[:, 1])
        ny = (e0[:, 2] * e1[:, 0]) - (e0[:, 0] * e1[:, 2])
        nz = (e0[:, 0] * e1[:, 1]) - (e0[:, 1] * e1[:, 0])
    ok &= ~((nx == 0) & (ny == 0) & (nz == 0))
    return np.nonzero(ok)[0]


def _dot(a, b):
    return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2])


def pair_d2_f32(P, A, B, C, clamp=True):
    """D2 of the contract for points P (V, 3) against triangles A, B, C (T, 3): a (V, T) float32 array (NaN / inf where the contract gives them).
    clamp=False leaves the two clamps of the face region out: NOT the contract, only there so that a test can show a case needs them"""
    p = [P[:, i, None] for i in range(3)]
    a = [A[None, :, i] for i in range(3)]
    b = [B[None, :, i] for i in range(3)]
    c = [C[None, :, i] for i in range(3)]
    with np.errstate(all="ignore"):
        ab = [b[i] - a[i] for i in range(3)]
        ac = [c[i] - a[i] for i in range(3)]
        bc = [c[i] - b[i] for i in range(3)]
        ap = [p[i] - a[i] for i in range(3)]
        bp = [p[i] - b[i] for i in range(3)]
        cp = [p[i] - c[i] for i in range(3)]
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc = (d1 * d4) - (d3 * d2)
        vb = (d5 * d2) - (d1 * d6)
        va = (d3 * d6) - (d5 * d4)
        e43, e56 = d4 - d3, d5 - d6
        c1 = (d1 <= 0) & (d2 <= 0)
        c2 = (d3 >= 0) & (d4 <= d3)
        c3 = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        c4 = (d6 >= 0) & (d5 <= d6)
        c5 = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        c6 = (va <= 0) & (e43 >= 0) & (e56 >= 0)
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = e43 / (e43 + e56)
        den = (va + vb) + vc
        v0, w0 = vb / den, vc / den
        zero, one = F(0.0), F(1.0)
        v = np.where(v0 > 0, v0, zero)
        v = np.where(v < 1, v, one)
        wl = one - v
        w = np.where(w0 > 0, w0, zero)
        w = np.where(w < wl, w, wl)
        if not clamp:
            v, w = v0, w0
        d = []
        for i in range(3):
            q = np.where(c1, a[i], np.where(c2, b[i], np.where(c3, a[i] + (ab[i] * v_ab), np.where(c4, c[i], np.where(
                c5, a[i] + (ac[i] * w_ac), np.where(c6, b[i] + (bc[i] * w_bc), (a[i] + (ab[i] * v)) + (ac[i] * w)))))))
            assert q.dtype == F
            d.append(p[i] - q)
        out = ((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])
    assert out.dtype == F
    return out


def _key(*parts):
    return tuple(np.ascontiguousarray(x).tobytes() if isinstance(x, np.ndarray) else x for x in parts)


def _nearest_f32(xyz, tri, n, vs, origin):
    """(best float32[n^3], idx uint32[n^3]) over ALL valid triangles, no band: the smallest finite D2 of each voxel (inf without one) and
    the lowest index that attains it.  A band only ever removes pairs with D2 >= B2, so the banded minimum and its first index follow from
    these two; they are what every band and sign of one (mesh, frame) share, and are computed once.  Chunks of triangles run on a few
    threads (numpy releases the GIL) and are merged in index order with a strict '<'."""
    k = _key("nearest", xyz, tri, n, F(vs), origin)
    if k in _cache:
        return _cache[k]
    P = centres(n, vs, origin)
    V = P.shape[0]
    best = np.full(V, np.inf, F)
    idx = np.full(V, NONE, np.uint32)
    keep = valid_triangles(xyz, tri)
    step = max(1, _CHUNK // V)

    def chunk(s):
        t = keep[s:s + step]
        vtx = xyz[tri[t].astype(np.int64)]
        D = pair_d2_f32(P, vtx[:, 0], vtx[:, 1], vtx[:, 2])
        with np.errstate(all="ignore"):
            D = np.where(np.isfinite(D), D, F(np.inf))
        return D.min(1), t[D.argmin(1)]                            # the first minimum of the chunk = its lowest index

    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as pool:
        for m, am in pool.map(chunk, range(0, keep.size, step)):
            up = m < best                                          # strict: an earlier (lower) index keeps a tie
            best[up] = m[up]
            idx[up] = am[up].astype(np.uint32)
    best.setflags(write=False)
    idx.setflags(write=False)
    _cache[k] = (best, idx)
    return _cache[k]


def mesh_distance_f32(xyz, tri, n, vs, origin, band, sign_words=None):
    """(dist2 float32[n^3], nearest uint32[n^3]) of the contract; sign_words: + on set voxels, - on unset ones"""
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    tri = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    origin = np.asarray(origin, F)
    k = _key("f32", xyz, tri, n, F(vs), origin, band, sign_words)
    if k in _cache:
        return _cache[k]
    best, idx = _nearest_f32(xyz, tri, n, vs, origin)
    V = best.shape[0]
    Bf = F(band) * F(vs)
    B2 = Bf * Bf
    dist = np.where(best < B2, best, B2).astype(F)
    idx = np.where(best < B2, idx, np.uint32(NONE)).astype(np.uint32)
    if sign_words is not None:
        bits = np.unpackbits(np.ascontiguousarray(sign_words, np.uint32).view(np.uint8), bitorder="little")[:V].astype(bool)
        dist = np.where(bits, dist, -dist).astype(F)
    dist.setflags(write=False)
    idx.setflags(write=False)
    _cache[k] = (dist, idx)
    return _cache[k]


def _seg_d2(P, A, B):
    """float64 squared distance of points (V, 1, 3) to segments A B (1, T, 3)"""
    ab = B - A
    t = ((P - A) * ab).sum(-1) / (ab * ab).sum(-1)
    t = np.clip(t, 0.0, 1.0)
    d = P - (A + t[..., None] * ab)
    return (d * d).sum(-1)


def mesh_distance_f64(xyz, tri, n, vs, origin):
    """(dist2 float64[n^3], nearest int64[n^3], second float64[n^3]): the unsigned squared distance to the nearest valid triangle in
    float64 -- min(plane projection where it falls inside the triangle, the three segment distances) -- the lowest index that attains it
    and the smallest distance among the OTHER triangles (inf with one triangle); no band"""
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    tri = np.ascontiguousarray(tri, np.uint32).reshape(-1, 3)
    origin = np.asarray(origin, F)
    k = _key("f64", xyz, tri, n, F(vs), origin)
    if k in _cache:
        return _cache[k]
    P = centres(n, vs, origin).astype(np.float64)[:, None, :]
    V = P.shape[0]
    best = np.full(V, np.inf)
    second = np.full(V, np.inf)
    idx = np.full(V, -1, np.int64)
    keep = valid_triangles(xyz, tri)
    step = max(1, _CHUNK // (4 * V))
    for s in range(0, keep.size, step):
        t = keep[s:s + step]
        vtx = xyz[tri[t].astype(np.int64)].astype(np.float64)
        A, B, C = vtx[None, :, 0], vtx[None, :, 1], vtx[None, :, 2]
        with np.errstate(all="ignore"):
            nrm = np.cross(B - A, C - A)
            nn = (nrm * nrm).sum(-1)
            h = ((P - A) * nrm).sum(-1) / nn                       # signed height in units of |nrm|
            Q = P - h[..., None] * nrm
            inside = ((np.cross(B - A, Q - A) * nrm).sum(-1) >= 0) & ((np.cross(C - B, Q - B) * nrm).sum(-1) >= 0) & \
                     ((np.cross(A - C, Q - C) * nrm).sum(-1) >= 0)
            D = np.minimum(np.minimum(_seg_d2(P, A, B), _seg_d2(P, B, C)), _seg_d2(P, C, A))
            D = np.where(inside, np.minimum(D, h * h * nn), D)
        for j in range(t.size):                                    # running best and runner-up, triangle by triangle
            dj = D[:, j]
            better = dj < best
            second = np.where(better, best, np.minimum(second, dj))
            idx = np.where(better, t[j], idx)
            best = np.where(better, dj, best)
    for a in (best, idx, second):
        a.setflags(write=False)
    _cache[k] = (best, idx, second)
    return _cache[k]
