"""Second source of the prepare step (lr_warp_perspective_device with LR_WARP_PREPARE): the
canonical arithmetic restated in NumPy, sharing nothing with kernels_prepare.hip.

Luma: u8 the value; u8x3 (4899 c0 + 9617 c1 + 1868 c2 + 8192) >> 14; both then p = float32(luma) * float32(1 / 256).
f32: p = the value.
Per axis, s = n_src / n_dst in double: destination sample i covers [i s, min(n_src, (i + 1) s)); its taps are
a = floor(lo) .. b = min(n_src - 1, ceil(hi) - 1); tap j weighs float32(max(0, min(hi, j + 1) - max(lo, j)) / s).
Horizontal, per source row: h = 0; h = h + w_x * p over the taps in order.  Vertical: v = 0; v = v + w_y * h_row over
the rows in order.  NumPy never fuses a product with a sum, so float32 arrays round each on its own.

prepare(src, ow, oh) is that in float32; prepare(src, ow, oh, np.float64) runs the same sums in float64 with the same
float32 weights (what the float32 result is measured against).
"""
import math

import numpy as np


def spans(n_src, n_dst):
    """[(first tap, float32 weights)] for each of the n_dst destination samples of one axis"""
    out = []
    s = float(n_src) / float(n_dst)
    for i in range(n_dst):
        lo, hi = i * s, min(float(n_src), (i + 1) * s)
        a, b = int(math.floor(lo)), min(n_src - 1, int(math.ceil(hi)) - 1)
        w = [np.float32(max(0.0, min(hi, j + 1.0) - max(lo, float(j))) / s) for j in range(a, b + 1)]
        out.append((a, np.array(w, np.float32)))
    return out


def unit_values(src):
    """p of every source pixel, float32 (H x W)"""
    src = np.asarray(src)
    if src.dtype == np.float32 and src.ndim == 2:
        return src
    if src.dtype != np.uint8:
        raise ValueError("uint8 or float32 frames")
    if src.ndim == 3:
        c = src.astype(np.int64)
        luma = (4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14
    else:
        luma = src
    return luma.astype(np.float32) * np.float32(1.0 / 256.0)


def prepare(src, out_w, out_h, dtype=np.float32):
    p = unit_values(src).astype(dtype)
    h, w = p.shape
    rows = np.zeros((h, out_w), dtype)
    for x, (a, wgt) in enumerate(spans(w, out_w)):
        acc = np.zeros(h, dtype)
        for j, wj in enumerate(wgt):
            acc = acc + dtype(wj) * p[:, a + j]
        rows[:, x] = acc
    out = np.zeros((out_h, out_w), dtype)
    for y, (a, wgt) in enumerate(spans(h, out_h)):
        acc = np.zeros(out_w, dtype)
        for j, wj in enumerate(wgt):
            acc = acc + dtype(wj) * rows[a + j]
        out[y] = acc
    return out


def max_taps(n_src, n_dst):
    return max(len(w) for _, w in spans(n_src, n_dst))
