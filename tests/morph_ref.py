"""Ball morphology references for tests/test_morph_cpu.py and tests/test_morph_gpu.py (helpers, no tests).

The contract of vp_morph (include/vphip.h): B_r = {d in Z^3 : |d|^2 <= r^2}; dilate reads voxels outside the grid as empty, erode =
NOT dilate(NOT W) reads them as set; open = dilate(erode), close = erode(dilate).  Two restatements, both on (z, y, x) bool arrays:
  morph_numpy       the brute form: OR of the zero-padded array shifted by every offset of B_r
  morph_numpy_sep   the exact squared distance to the nearest set voxel, capped, in three separable integer passes, then <= r^2
Everything is integer arithmetic, so they agree bit for bit with each other, with scipy.ndimage and with the library."""
import numpy as np

from fill_ref import bool_to_words, random_grid, words_to_bool  # noqa: F401

DILATE, ERODE, OPEN, CLOSE = 0, 1, 2, 3


def ball(r):
    """(2 r + 1)^3 bool array, [dz + r, dy + r, dx + r]"""
    a = np.arange(-r, r + 1)
    return (a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2) <= r * r


def _dilate_brute(vox, r):
    n = vox.shape[0]
    pad = np.zeros((n + 2 * r,) * 3, bool)
    pad[r:r + n, r:r + n, r:r + n] = vox
    out = np.zeros_like(vox)
    for dz, dy, dx in np.argwhere(ball(r)) - r:
        out |= pad[r - dz:r - dz + n, r - dy:r - dy + n, r - dx:r - dx + n]
    return out


def _dilate_sep(vox, r):
    n = vox.shape[0]
    inf = np.int32(1 << 20)
    g = np.where(vox, np.int32(0), inf)
    for axis in (2, 1, 0):
        best = g.copy()
        for d in range(1, r + 1):
            for sgn in (-1, 1):
                src = [slice(None)] * 3
                dst = [slice(None)] * 3
                if sgn > 0:                     # the value at index i + d reaches index i
                    src[axis], dst[axis] = slice(d, n), slice(0, n - d)
                else:
                    src[axis], dst[axis] = slice(0, n - d), slice(d, n)
                cand = g[tuple(src)] + np.int32(d * d)
                np.minimum(best[tuple(dst)], cand, out=best[tuple(dst)])
        g = best
    return g <= r * r


def _morph(dilate, vox, op, r):
    if r == 0:
        return vox.copy()
    erode = lambda v: ~dilate(~v, r)            # noqa: E731
    if op == DILATE:
        return dilate(vox, r)
    if op == ERODE:
        return erode(vox)
    if op == OPEN:
        return dilate(erode(vox), r)
    if op == CLOSE:
        return erode(dilate(vox, r))
    raise ValueError(op)


def morph_bool(vox, op, r):
    return _morph(_dilate_brute, vox, op, r)


def morph_bool_sep(vox, op, r):
    return _morph(_dilate_sep, vox, op, r)


def morph_numpy(words, n, op, r):
    return bool_to_words(morph_bool(words_to_bool(words, n), op, r))


def morph_numpy_sep(words, n, op, r):
    return bool_to_words(morph_bool_sep(words_to_bool(words, n), op, r))


def shell_with_hole(n, k):
    """one-voxel-thick box shell with a k x k hole in the middle of its +x face; returns (shell, full box), (z, y, x) bool"""
    from fill_ref import box_shell
    lo, hi = (12, 12, 12), (n - 13, n - 13, n - 13)
    shell = box_shell(n, lo, hi)
    c = n // 2 - k // 2
    shell[c:c + k, c:c + k, hi[0]] = False
    full = np.zeros((n, n, n), bool)
    full[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    return shell, full


def hand_cases(n, r):
    """[(name, op, input (z, y, x) bool, expected (z, y, x) bool)] -- every expectation written from the construction"""
    cases = []
    zero = np.zeros((n, n, n), bool)
    a = np.arange(n)
    Z, Y, X = a[:, None, None], a[None, :, None], a[None, None, :]
    points = {"middle": (n // 2, n // 2 + 1, n // 2 - 1), "corner": (0, n - 1, 0), "x=31": (31, 5, 7), "x=n-1": (n - 1, n // 2, 3)}
    if n > 32:
        points["x=32"] = (32, n - 3, n // 2)
    for name, (px, py, pz) in points.items():
        v = zero.copy()
        v[pz, py, px] = True
        cases.append(("single voxel " + name, DILATE, v, (X - px) ** 2 + (Y - py) ** 2 + (Z - pz) ** 2 <= r * r))
    cases.append(("erode full", ERODE, ~zero, ~zero))
    cases.append(("dilate empty", DILATE, zero.copy(), zero.copy()))
    for c in (31, 32) if n > 32 else (15, 31):
        v = zero.copy()
        v[:, :, c] = True
        cases.append(("wall x=%d" % c, DILATE, v, np.broadcast_to(np.abs(X - c) <= r, (n, n, n)).copy()))
    # erode of a box: shrunk by r per side, except against a grid face; a box thinner than 2 r + 1 vanishes
    def box(x0, x1, y0, y1, z0, z1):
        v = zero.copy()
        if x0 <= x1 and y0 <= y1 and z0 <= z1:
            v[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = True
        return v
    if n >= 64:
        x0, x1, y0, y1, z0, z1 = 3, n - 6, 4, n - 4, 5, n - 7
        cases.append(("erode box", ERODE, box(x0, x1, y0, y1, z0, z1), box(x0 + r, x1 - r, y0 + r, y1 - r, z0 + r, z1 - r)))
        cases.append(("erode box on faces", ERODE, box(0, x1, y0, n - 1, 0, z1), box(0, x1 - r, y0 + r, n - 1, 0, z1 - r)))
    cases.append(("erode thin box", ERODE, box(2, n - 3, 4, 4 + 2 * r - 1, 2, n - 3), zero.copy()))
    return cases
