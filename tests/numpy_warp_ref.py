"""Second source of the perspective warp ("rectified images"): the canonical arithmetic restated in
float64 / int64 NumPy, sharing nothing with kernels_warp.hip.

For destination pixel (x, y), M the destination-to-source map (row-major 3x3):
  W0 = (M6 x + M7 y) + M8;  Wq = 32 / W0, or 0 where W0 == 0
  X = rint(clamp(((M0 x + M1 y) + M2) * Wq)), Y likewise; clamp to [INT_MIN, INT_MAX], NaN -> INT_MIN; half to even
  ix, ax = X >> 5, X & 31 (iy, ay likewise); taps (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1) with weights
  (32-ax)(32-ay), ax(32-ay), (32-ax)ay, ax ay; a tap outside the source is 0
  u8: (sum v w + 512) >> 10 per channel;  f32: ((v00 w00 + v01 w01) + v10 w10) + v11 w11 in float32, w / 1024
"""
import numpy as np

INT_MIN, INT_MAX = -2147483648.0, 2147483647.0


def fixed_coords(M, out_w, out_h, rows=None):
    """(X, Y) int64 arrays of shape (len(rows), out_w): the 5-bit fixed-point source coordinates."""
    M = np.asarray(M, np.float64).reshape(9)
    ys = np.arange(out_h, dtype=np.float64) if rows is None else np.asarray(rows, np.float64)
    y = ys[:, None]
    x = np.arange(out_w, dtype=np.float64)[None, :]
    with np.errstate(all="ignore"):
        W0 = (M[6] * x + M[7] * y) + M[8]
        Wq = np.where(W0 != 0.0, 32.0 / np.where(W0 != 0.0, W0, 1.0), 0.0)
        out = []
        for a, b, c in ((M[0], M[1], M[2]), (M[3], M[4], M[5])):
            v = ((a * x + b * y) + c) * Wq
            v = np.where(v >= INT_MAX, INT_MAX, np.where(v >= INT_MIN, v, INT_MIN))  # NaN fails both: INT_MIN
            out.append(np.rint(v).astype(np.int64))
    return out[0], out[1]


def _taps(src, X, Y):
    """Values (float64 for f32 sources, int64 otherwise) of the four taps and their integer weights."""
    h, w = src.shape[:2]
    ix, iy = X >> 5, Y >> 5
    ax, ay = X & 31, Y & 31
    weights = [(32 - ax) * (32 - ay), ax * (32 - ay), (32 - ax) * ay, ax * ay]
    vals = []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        cx, cy = ix + dx, iy + dy
        ok = (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h)
        v = src[np.clip(cy, 0, h - 1), np.clip(cx, 0, w - 1)]
        if src.ndim == 3:
            v = np.where(ok[..., None], v, 0)
        else:
            v = np.where(ok, v, 0)
        vals.append(v.astype(src.dtype))
    return vals, weights


def warp(src, M, out_w, out_h, rows=None):
    """Warps src ((h, w) uint8 or float32, or (h, w, 3) uint8) by M into out_h x out_w (or only the listed rows)."""
    src = np.asarray(src)
    X, Y = fixed_coords(M, out_w, out_h, rows)
    vals, wts = _taps(src, X, Y)
    if src.dtype == np.float32:
        f = [(w.astype(np.float64) / 1024.0).astype(np.float32) for w in wts]
        acc = vals[0] * f[0] + vals[1] * f[1]
        acc = acc + vals[2] * f[2]
        return acc + vals[3] * f[3]
    assert src.dtype == np.uint8
    acc = np.full(X.shape + src.shape[2:], 512, np.int64)
    for v, w in zip(vals, wts):
        acc += v.astype(np.int64) * (w[..., None] if src.ndim == 3 else w)
    return (acc >> 10).astype(np.uint8)
