"""Second source of the bicubic perspective warp, LR_WARP_CUBIC: the canonical arithmetic
restated in int64 / float32 NumPy, sharing nothing with kernels_warp.hip, and the table of weights computed from its formula
(csrc/tables.h holds it as literals).

X, Y are the bilinear warp's 5-bit fixed-point source coordinates (numpy_warp_ref.fixed_coords); ix, ax = X >> 5, X & 31 (iy,
ay likewise).  Taps: columns ix - 1 .. ix + 2 of rows iy - 1 .. iy + 2, 0 outside the source.  Weights: C[ax], C[ay], integers
at scale 2048 (the Keys kernel with A = -0.75).
  u8, per channel: h_j = sum_i C[ax][i] v(i, j);  s = sum_j C[ay][j] h_j;  clamp((s + 2^21) >> 22, 0, 255)
  f32: f = float32(C) / 2048;  h_j = ((v0 fx0 + v1 fx1) + v2 fx2) + v3 fx3;  out = ((h0 fy0 + h1 fy1) + h2 fy2) + h3 fy3,
       every product and sum rounded to float32; no clamp
"""
import numpy as np

from numpy_warp_ref import fixed_coords

A = -0.75


def kernel_f64(t):
    """The four unrounded weights (float64, shape t.shape + (4,)) of the taps -1, 0, 1, 2 for the fraction t in [0, 1)."""
    t = np.asarray(t, np.float64)
    c0 = ((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A
    c1 = ((A + 2) * t - (A + 3)) * t * t + 1
    u = 1 - t
    c2 = ((A + 2) * u - (A + 3)) * u * u + 1
    return np.stack([c0, c1, c2, 1 - c0 - c1 - c2], axis=-1)


def table():
    """C[32][4], int64: floor(c * 2048 + 0.5), the row's remainder to 2048 added to [1] (a <= 16) or [2] (a > 16)."""
    C = np.floor(kernel_f64(np.arange(32) / 32.0) * 2048 + 0.5).astype(np.int64)
    rest = 2048 - C.sum(axis=1)
    assert np.abs(rest).max() <= 1
    for a in range(32):
        C[a, 1 if a <= 16 else 2] += rest[a]
    return C


TABLE = table()


def _tap_rows(src, X, Y):
    """rows[j][i]: the values of tap (ix - 1 + i, iy - 1 + j), 0 outside the source, in the source's dtype"""
    h, w = src.shape[:2]
    ix, iy = X >> 5, Y >> 5
    rows = []
    for j in range(4):
        row = []
        for i in range(4):
            cx, cy = ix - 1 + i, iy - 1 + j
            ok = (cx >= 0) & (cx < w) & (cy >= 0) & (cy < h)
            v = src[np.clip(cy, 0, h - 1), np.clip(cx, 0, w - 1)]
            row.append(np.where(ok[..., None] if src.ndim == 3 else ok, v, 0).astype(src.dtype))
        rows.append(row)
    return rows


def warp(src, M, out_w, out_h, rows=None, stats=None):
    """Warps src ((h, w) uint8 or float32, or (h, w, 3) uint8) by M into out_h x out_w (or only the listed rows) by the
    bicubic rule.  stats (a dict, 8-bit sources): 'max_abs_s' becomes the largest |s| met."""
    src = np.asarray(src)
    X, Y = fixed_coords(M, out_w, out_h, rows)
    taps = _tap_rows(src, X, Y)
    cx, cy = TABLE[X & 31], TABLE[Y & 31]  # (..., 4)
    if src.dtype == np.float32:
        fx = (cx.astype(np.float32) / np.float32(2048)).astype(np.float32)
        fy = (cy.astype(np.float32) / np.float32(2048)).astype(np.float32)
        with np.errstate(all="ignore"):
            h = []
            for j in range(4):
                v = taps[j]
                acc = v[0] * fx[..., 0] + v[1] * fx[..., 1]
                acc = acc + v[2] * fx[..., 2]
                h.append(acc + v[3] * fx[..., 3])
            out = h[0] * fy[..., 0] + h[1] * fy[..., 1]
            out = out + h[2] * fy[..., 2]
            out = out + h[3] * fy[..., 3]
        assert out.dtype == np.float32
        return out
    assert src.dtype == np.uint8
    ex = (lambda a: a[..., None]) if src.ndim == 3 else (lambda a: a)
    s = np.zeros(X.shape + src.shape[2:], np.int64)
    for j in range(4):
        hj = np.zeros_like(s)
        for i in range(4):
            hj += ex(cx[..., i]) * taps[j][i].astype(np.int64)
        s += ex(cy[..., j]) * hj
    if stats is not None:
        stats["max_abs_s"] = max(stats.get("max_abs_s", 0), int(np.abs(s).max()))
    return np.clip((s + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def warp_f64(src, M, out_w, out_h):
    """The same kernel at the same quantised coordinates in float64: unrounded weights, no integer rounding, clipped to
    [0, 255].  What the integer rule is held against."""
    src = np.asarray(src)
    X, Y = fixed_coords(M, out_w, out_h)
    taps = _tap_rows(src, X, Y)
    kx, ky = kernel_f64((X & 31) / 32.0), kernel_f64((Y & 31) / 32.0)
    ex = (lambda a: a[..., None]) if src.ndim == 3 else (lambda a: a)
    out = np.zeros(X.shape + src.shape[2:], np.float64)
    for j in range(4):
        hj = np.zeros_like(out)
        for i in range(4):
            hj += ex(kx[..., i]) * taps[j][i].astype(np.float64)
        out += ex(ky[..., j]) * hj
    return np.clip(out, 0.0, 255.0)
