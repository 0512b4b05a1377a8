"""Second source of LR_WARP_BORDER: the border index and the bordered bilinear and bicubic
warp for u8, u8x3 and f32 in int64 / float32 NumPy, sharing nothing with kernels_warp.hip.  The coordinates are
numpy_warp_ref.fixed_coords', the bicubic weights numpy_warp_cubic_ref.TABLE.

A border is (mode, value): mode 0 constant, 1 replicate, 2 reflect, 4 reflect-101 (OpenCV's numbers); value, used by mode 0
only, is a number (u8, f32) or three (u8x3).  Taps, weights, rounding and the order of the f32 sums are those of the
unbordered rules; only a tap outside the source differs: mode 0 gives it `value`, the others the value of source pixel
(index(cx, w), index(cy, h)).
"""
import numpy as np

from numpy_warp_cubic_ref import TABLE
from numpy_warp_ref import fixed_coords

CONSTANT, REPLICATE, REFLECT, REFLECT_101 = 0, 1, 2, 4


def index(p, n, mode):
    """OpenCV's borderInterpolate for int64 coordinates p on an axis of n pixels, as floor-modulo arithmetic"""
    p = np.asarray(p, np.int64)
    if mode == REPLICATE:
        return np.clip(p, 0, n - 1)
    if mode == REFLECT:
        q = np.mod(p, 2 * n)
        return np.where(q < n, q, 2 * n - 1 - q)
    if mode == REFLECT_101:
        if n == 1:
            return np.zeros_like(p)
        q = np.mod(p, 2 * n - 2)
        return np.where(q < n, q, 2 * n - 2 - q)
    raise ValueError("no index rule for mode %r" % (mode,))


def word(mode, value, src):
    """the border word mode + 8 * value for a source array's format"""
    if mode != CONSTANT:
        return mode
    if src.dtype == np.float32:
        bits = int(np.float32(value).view(np.uint32))
    elif src.ndim == 3:
        bits = int(value[0]) | int(value[1]) << 8 | int(value[2]) << 16
    else:
        bits = int(value)
    return 8 * bits


def tap(src, cx, cy, mode, value):
    """the values of the taps at (cx, cy), in the source's dtype"""
    h, w = src.shape[:2]
    if mode == CONSTANT:
        ok = (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h)
        v = src[np.clip(cy, 0, h - 1), np.clip(cx, 0, w - 1)]
        fill = np.asarray(value, src.dtype)
        return np.where(ok[..., None] if src.ndim == 3 else ok, v, fill).astype(src.dtype)
    return src[index(cy, h, mode), index(cx, w, mode)]


def warp(src, M, out_w, out_h, mode=CONSTANT, value=0, cubic=False):
    """Warps src ((h, w) uint8 or float32, or (h, w, 3) uint8) by M into out_h x out_w with the border (mode, value), by the
    bilinear or (cubic) the bicubic rule."""
    src = np.asarray(src)
    X, Y = fixed_coords(M, out_w, out_h)
    ix, iy, ax, ay = X >> 5, Y >> 5, X & 31, Y & 31
    ex = (lambda a: a[..., None]) if src.ndim == 3 else (lambda a: a)
    f32 = src.dtype == np.float32
    assert f32 or src.dtype == np.uint8
    if not cubic:
        wts = [(32 - ax) * (32 - ay), ax * (32 - ay), (32 - ax) * ay, ax * ay]
        vals = [tap(src, ix + dx, iy + dy, mode, value) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1))]
        if f32:
            f = [(w.astype(np.float64) / 1024.0).astype(np.float32) for w in wts]
            with np.errstate(all="ignore"):
                acc = vals[0] * f[0] + vals[1] * f[1]
                acc = acc + vals[2] * f[2]
                return acc + vals[3] * f[3]
        acc = np.full(X.shape + src.shape[2:], 512, np.int64)
        for v, w in zip(vals, wts):
            acc += v.astype(np.int64) * ex(w)
        return (acc >> 10).astype(np.uint8)
    cx, cy = TABLE[ax], TABLE[ay]
    rows = [[tap(src, ix - 1 + i, iy - 1 + j, mode, value) for i in range(4)] for j in range(4)]
    if f32:
        fx = (cx.astype(np.float32) / np.float32(2048)).astype(np.float32)
        fy = (cy.astype(np.float32) / np.float32(2048)).astype(np.float32)
        with np.errstate(all="ignore"):
            h = []
            for j in range(4):
                v = rows[j]
                acc = v[0] * fx[..., 0] + v[1] * fx[..., 1]
                acc = acc + v[2] * fx[..., 2]
                h.append(acc + v[3] * fx[..., 3])
            out = h[0] * fy[..., 0] + h[1] * fy[..., 1]
            out = out + h[2] * fy[..., 2]
            out = out + h[3] * fy[..., 3]
        assert out.dtype == np.float32
        return out
    s = np.zeros(X.shape + src.shape[2:], np.int64)
    for j in range(4):
        hj = np.zeros_like(s)
        for i in range(4):
            hj += ex(cx[..., i]) * rows[j][i].astype(np.int64)
        s += ex(cy[..., j]) * hj
    return np.clip((s + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def crop(H, M, width, height, out_w, out_h, margin=0, aspect=None):
    """The constrained crop's rule, restated with arrays: (M_out, (x0, y0, crop_width, crop_height), (bounds, s, c, a, Q)), bounds
    being the eight values whose minimum is the half-height s.  Assumes a valid input (positive denominators or negative, a convex
    quadrilateral)."""
    H = np.asarray(H, np.float64).reshape(3, 3)
    M = np.asarray(M, np.float64).reshape(3, 3)
    a = float(aspect) if aspect is not None and aspect > 0 else width / height
    m = margin
    P = np.array([[m, m, 1], [width - 1 - m, m, 1], [width - 1 - m, height - 1 - m, 1], [m, height - 1 - m, 1],
                  [(width - 1) / 2, (height - 1) / 2, 1]], np.float64)
    q = P @ H.T
    q = q[:, :2] / q[:, 2:]
    Q, c = q[:4], q[4]
    bounds = [c[0] / a, (out_w - 1 - c[0]) / a, c[1], out_h - 1 - c[1]]
    R = np.roll(Q, -1, axis=0)
    area2 = float(np.sum(Q[:, 0] * R[:, 1] - R[:, 0] * Q[:, 1]))
    for Pk, Rk in zip(Q, R):
        e = Rk - Pk
        n = np.array([-e[1], e[0]]) * (1.0 if area2 > 0 else -1.0)
        bounds.append(float(n @ (c - Pk)) / (abs(n[0]) * a + abs(n[1])))
    s = min(bounds)
    x0, x1 = int(np.ceil(c[0] - s * a)), int(np.floor(c[0] + s * a))
    y0, y1 = int(np.ceil(c[1] - s)), int(np.floor(c[1] + s))
    M_out = M.copy()  # M T(x0, y0): the third column alone changes
    M_out[:, 2] = (M[:, 0] * x0 + M[:, 1] * y0) + M[:, 2]
    return M_out, (x0, y0, x1 - x0 + 1, y1 - y0 + 1), (bounds, s, c, a, Q)
