"""Second source of LR_WARP_AREA: the area-sampled warp restated in NumPy, sharing nothing with
warp_lane.h or kernels_warp_area.hip.  It is the existing second source of the warp (numpy_warp_lens_ref.warp: the lens, the
5-bit coordinates, both sampling rules, every border mode) at the fine size, followed by the box mean.

For a frame with map M (destination to source) and sampling factor S (1 .. 8):
  F[k][0] = M[k][0] / S;  F[k][1] = M[k][1] / S;  F[k][2] = M[k][2] - ((M[k][0] + M[k][1]) * (S - 1)) / (2 S), in double,
  every operation rounded on its own;
  v(i, j) = pixel (S x + i, S y + j) of the warp without the bit under F into S ow x S oh, rounded as that warp rounds it;
  u8, u8x3 per channel: s = the sum of the S^2 bytes, out = (2 s + S^2) // (2 S^2);
  f32: acc = 0.0f; for j from 0, for i from 0: acc = acc + v(i, j), every sum rounded to float; out = acc / float32(S * S).
S = 1 is the plain rule itself.
"""
import numpy as np

import numpy_warp_border_ref as border_ref
import numpy_warp_lens_ref as lens_ref


def fine_map(M, S):
    M = np.asarray(M, np.float64).reshape(3, 3)
    F = np.zeros((3, 3), np.float64)
    s = np.float64(S)
    with np.errstate(all="ignore"):
        F[:, 0] = M[:, 0] / s
        F[:, 1] = M[:, 1] / s
        F[:, 2] = M[:, 2] - ((M[:, 0] + M[:, 1]) * np.float64(S - 1)) / np.float64(2 * S)
    return F


def box_mean(fine, S):
    """The S x S box mean of a picture (S oh, S ow[, 3]) by the rule above: uint8 in integers, round half up; float32 summed in
    the order j outer, i inner from 0.0f, every sum rounded to float, then divided by float32(S * S)."""
    S = int(S)
    oh, ow = fine.shape[0] // S, fine.shape[1] // S
    assert fine.shape[0] == oh * S and fine.shape[1] == ow * S
    if fine.dtype == np.uint8:
        s = np.zeros((oh, ow) + fine.shape[2:], np.int64)
        for j in range(S):
            for i in range(S):
                s += fine[j::S, i::S]
        return ((2 * s + S * S) // (2 * S * S)).astype(np.uint8)
    assert fine.dtype == np.float32
    with np.errstate(all="ignore"):
        acc = np.zeros((oh, ow), np.float32)
        for j in range(S):
            for i in range(S):
                acc = acc + fine[j::S, i::S]
        return acc / np.float32(S * S)


def warp_area(src, M, ow, oh, S, lens=None, mode=border_ref.CONSTANT, value=0, cubic=False):
    """Warps src ((h, w) uint8 or float32, or (h, w, 3) uint8) by M into oh x ow with S x S samples per pixel, through the
    lens and with the border (mode, value), by the bilinear or (cubic) the bicubic rule."""
    S = int(S)
    if S == 1:
        return lens_ref.warp(src, M, ow, oh, lens, mode, value, cubic)
    return box_mean(lens_ref.warp(src, fine_map(M, S), S * ow, S * oh, lens, mode, value, cubic), S)
