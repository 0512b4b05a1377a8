"""Second source of LR_WARP_LENS: the lens rule restated operation for operation in float64
NumPy, sharing nothing with warp_lane.h.  Only the coordinates are new: X, Y go to the sampling of the existing references
(numpy_warp_border_ref.warp, which with the constant zero border is numpy_warp_ref's and numpy_warp_cubic_ref's rule), whose
taps and blends are imported, not copied.

For destination pixel (x, y), M the map into the IDEAL picture and lens = (fx, fy, cx, cy, k1, k2, p1, p2, k3):
  W0 = (M6 x + M7 y) + M8;  Wq = 32 / W0, or 0 where W0 == 0;  U = ((M0 x + M1 y) + M2) * Wq;  V likewise
  a = (U * 0.03125 - cx) / fx;  b = (V * 0.03125 - cy) / fy
  r2 = a a + b b;  rad = r2 (k1 + r2 (k2 + r2 k3))
  ta = (2 p1) (a b) + p2 (r2 + 2 (a a));  tb = p1 (r2 + 2 (b b)) + (2 p2) (a b)
  du = fx (a rad + ta);  dv = fy (b rad + tb)
  X = fixed(U + 32 du);  Y = fixed(V + 32 dv);  fixed: clamp to [INT_MIN, INT_MAX], NaN -> INT_MIN, half to even
A lens whose five coefficients are all zero (of either sign) is the plain rule: X = fixed(U), Y = fixed(V).
"""
import contextlib

import numpy as np

import numpy_warp_border_ref as border_ref
from numpy_warp_ref import INT_MAX, INT_MIN


def _fixed(v):
    v = np.where(v >= INT_MAX, INT_MAX, np.where(v >= INT_MIN, v, INT_MIN))  # NaN fails both: INT_MIN
    return np.rint(v).astype(np.int64)


def has_lens(lens):
    return any(float(c) != 0.0 for c in lens[4:9])


def fixed_coords(M, out_w, out_h, lens=None):
    """(X, Y) int64 arrays (out_h, out_w): the 5-bit fixed-point coordinates in the stored frame."""
    M = np.asarray(M, np.float64).reshape(9)
    y = np.arange(out_h, dtype=np.float64)[:, None]
    x = np.arange(out_w, dtype=np.float64)[None, :]
    with np.errstate(all="ignore"):
        W0 = (M[6] * x + M[7] * y) + M[8]
        Wq = np.where(W0 != 0.0, 32.0 / np.where(W0 != 0.0, W0, 1.0), 0.0)
        U = ((M[0] * x + M[1] * y) + M[2]) * Wq
        V = ((M[3] * x + M[4] * y) + M[5]) * Wq
        if lens is not None and has_lens(lens):
            fx, fy, cx, cy, k1, k2, p1, p2, k3 = (np.float64(v) for v in lens)
            a = (U * 0.03125 - cx) / fx
            b = (V * 0.03125 - cy) / fy
            r2 = a * a + b * b
            rad = r2 * (k1 + r2 * (k2 + r2 * k3))
            ta = (2.0 * p1) * (a * b) + p2 * (r2 + 2.0 * (a * a))
            tb = p1 * (r2 + 2.0 * (b * b)) + (2.0 * p2) * (a * b)
            du = fx * (a * rad + ta)
            dv = fy * (b * rad + tb)
            U = U + 32.0 * du
            V = V + 32.0 * dv
        return _fixed(U), _fixed(V)


@contextlib.contextmanager
def _coords(X, Y):
    """numpy_warp_border_ref.warp takes its coordinates from its module's fixed_coords: for one call that name gives X, Y"""
    saved = border_ref.fixed_coords
    border_ref.fixed_coords = lambda M, out_w, out_h: (X, Y)
    try:
        yield
    finally:
        border_ref.fixed_coords = saved


def warp(src, M, out_w, out_h, lens=None, mode=border_ref.CONSTANT, value=0, cubic=False):
    """Warps src ((h, w) uint8 or float32, or (h, w, 3) uint8) by M and the lens into out_h x out_w with the border (mode,
    value), by the bilinear or (cubic) the bicubic rule: the bordered reference's sampling at this module's coordinates."""
    X, Y = fixed_coords(M, out_w, out_h, lens)
    with _coords(X, Y):
        return border_ref.warp(src, M, out_w, out_h, mode, value, cubic)
