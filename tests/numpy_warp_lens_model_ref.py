"""Second source of LR_WARP_LENS_MODEL: the rule of the seventeen-entry lens restated operation
for operation in float64 NumPy, sharing nothing with warp_lane.h, the header or the package.  Only the coordinates are new: X, Y
go to numpy_warp_border_ref.warp as numpy_warp_lens_ref's do, and with area= to numpy_warp_area_ref's fine map and box mean.

lens = (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4, model); U, V, a, b, r2 and fixed as in numpy_warp_lens_ref.
model 0:
  radn = r2 (k1 + r2 (k2 + r2 k3));  radd = r2 (k4 + r2 (k5 + r2 k6));  rad = (radn - radd) / (1 + radd)
  ta = ((2 p1) (a b) + p2 (r2 + 2 (a a))) + r2 (s1 + r2 s2);  tb = (p1 (r2 + 2 (b b)) + (2 p2) (a b)) + r2 (s3 + r2 s4)
  du = fx (a rad + ta);  dv = fy (b rad + tb);  X = fixed(U + 32 du);  Y = fixed(V + 32 dv)
  entries [4..15] all zero (of either sign): the plain rule, X = fixed(U), Y = fixed(V).
model 1 (the fisheye; entries [4..7] are its k1..k4):
  r = sqrt(r2);  th = ATAN(r);  t2 = th th;  thd = th (1 + t2 (k1 + t2 (k2 + t2 (k3 + t2 k4))));  sc = thd / r, or 1 where r == 0
  X = fixed(32 (fx (a sc) + cx));  Y = fixed(32 (fy (b sc) + cy))
ATAN(r): t = 1 / r where r > 1, else r;  i = rint(8 t) (0 where that is no number from 0 to 8);  c = i / 8;
  z = (t - c) / (1 + t c);  z2 = z z;  p = -1/3 + z2 (1/5 + z2 (-1/7 + z2 (1/9 + z2 (-1/11 + z2 (1/13 + z2 (-1/15))))))
  A[i] + (z + z (z2 p)), and PI_2 minus that where r > 1.
"""
import contextlib

import numpy as np

import numpy_warp_area_ref as area_ref
import numpy_warp_border_ref as border_ref
from numpy_warp_ref import INT_MAX, INT_MIN

A = np.array([float.fromhex(v) for v in (
    "0x0.0p+0", "0x1.fd5ba9aac2f6ep-4", "0x1.f5b75f92c80ddp-3", "0x1.6f61941e4def1p-2", "0x1.dac670561bb4fp-2", "0x1.1e00babdefeb4p-1",
    "0x1.4978fa3269ee1p-1", "0x1.700a7c5784634p-1", "0x1.921fb54442d18p-1")], np.float64)
PI_2 = float.fromhex("0x1.921fb54442d18p+0")


def atan(r):
    r = np.asarray(r, np.float64)
    with np.errstate(all="ignore"):
        big = r > 1.0
        t = np.where(big, 1.0 / np.where(big, r, 1.0), r)
        n = np.rint(8.0 * t)
        i = np.where((n >= 0.0) & (n <= 8.0), n, 0.0).astype(np.int64)
        c = i.astype(np.float64) / 8.0
        z = (t - c) / (1.0 + t * c)
        z2 = z * z
        p = -1.0 / 3.0 + z2 * (1.0 / 5.0 + z2 * (-1.0 / 7.0 + z2 * (1.0 / 9.0 + z2 * (-1.0 / 11.0 + z2 * (1.0 / 13.0 + z2 * (-1.0 / 15.0))))))
        at = A[i] + (z + z * (z2 * p))
        return np.where(big, PI_2 - at, at)


def _fixed(v):
    v = np.where(v >= INT_MAX, INT_MAX, np.where(v >= INT_MIN, v, INT_MIN))  # NaN fails both: INT_MIN
    return np.rint(v).astype(np.int64)


def has_lens(lens):
    return float(lens[16]) == 1.0 or any(float(c) != 0.0 for c in lens[4:16])


def unrounded_coords(M, out_w, out_h, lens=None):
    """(U', V') float64 arrays (out_h, out_w): the coordinates in the stored frame, in 1/32 pixels, before `fixed`."""
    M = np.asarray(M, np.float64).reshape(9)
    y = np.arange(out_h, dtype=np.float64)[:, None]
    x = np.arange(out_w, dtype=np.float64)[None, :]
    with np.errstate(all="ignore"):
        W0 = (M[6] * x + M[7] * y) + M[8]
        Wq = np.where(W0 != 0.0, 32.0 / np.where(W0 != 0.0, W0, 1.0), 0.0)
        U = ((M[0] * x + M[1] * y) + M[2]) * Wq
        V = ((M[3] * x + M[4] * y) + M[5]) * Wq
        if lens is None or not has_lens(lens):
            return U, V
        fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4, model = (np.float64(v) for v in lens)
        a = (U * 0.03125 - cx) / fx
        b = (V * 0.03125 - cy) / fy
        r2 = a * a + b * b
        if model == 1.0:
            r = np.sqrt(r2)
            th = atan(r)
            t2 = th * th
            thd = th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (p1 + t2 * p2))))  # (entries [4..7]: the fisheye's k1..k4)
            sc = np.where(r != 0.0, thd / np.where(r != 0.0, r, 1.0), 1.0)
            return 32.0 * (fx * (a * sc) + cx), 32.0 * (fy * (b * sc) + cy)
        radn = r2 * (k1 + r2 * (k2 + r2 * k3))
        radd = r2 * (k4 + r2 * (k5 + r2 * k6))
        rad = (radn - radd) / (1.0 + radd)
        ta = ((2.0 * p1) * (a * b) + p2 * (r2 + 2.0 * (a * a))) + r2 * (s1 + r2 * s2)
        tb = (p1 * (r2 + 2.0 * (b * b)) + (2.0 * p2) * (a * b)) + r2 * (s3 + r2 * s4)
        du = fx * (a * rad + ta)
        dv = fy * (b * rad + tb)
        return U + 32.0 * du, V + 32.0 * dv


def fixed_coords(M, out_w, out_h, lens=None):
    """(X, Y) int64 arrays (out_h, out_w): the 5-bit fixed-point coordinates in the stored frame."""
    U, V = unrounded_coords(M, out_w, out_h, lens)
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


def warp(src, M, out_w, out_h, lens=None, mode=border_ref.CONSTANT, value=0, cubic=False, area=None):
    """Warps src ((h, w) uint8 or float32, or (h, w, 3) uint8) by M and the seventeen-entry lens into out_h x out_w with the
    border (mode, value), by the bilinear or (cubic) the bicubic rule; area=S (2 .. 8): S x S samples per pixel under
    numpy_warp_area_ref's fine map, averaged by its box mean."""
    S = 1 if area is None else int(area)
    if S > 1:
        return area_ref.box_mean(warp(src, area_ref.fine_map(M, S), S * out_w, S * out_h, lens, mode, value, cubic), S)
    X, Y = fixed_coords(M, out_w, out_h, lens)
    with _coords(X, Y):
        return border_ref.warp(src, M, out_w, out_h, mode, value, cubic)
