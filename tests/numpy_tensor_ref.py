"""lr_pack_tensor_device restated in NumPy, independent of the library's code.

An element of channel c whose level is v (0 .. 255; pad[c] outside the picture):
    p = v * scale[c]   in float64
    y = p + bias[c]    in float64
    f = float32(y)     round to nearest even
    f16: float16(f); bf16: the bits of f, + 0x7FFF + ((bits >> 16) & 1), >> 16   (round to nearest even, on uint32)
Placement, pad, swap, gray3 and the two layouts are plain slicing and transpose.
"""
import numpy as np


def convert(levels, scale, bias, dtype):
    """levels: integer array (..., C) with the channel LAST; scale, bias: C float64 each.  Returns float32, float16 or the
    uint16 bit patterns of bfloat16, same shape."""
    p = levels.astype(np.float64) * np.asarray(scale, np.float64)
    y = p + np.asarray(bias, np.float64)
    f = y.astype(np.float32)
    if dtype == "f32":
        return f
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return f.astype(np.float16)
    assert dtype == "bf16"
    bits = np.ascontiguousarray(f).view(np.uint32)
    return ((bits + np.uint32(0x7FFF) + ((bits >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def slot(picture, left, top, size, dtype="f32", layout="nchw", scale=(1, 1, 1), bias=(0, 0, 0), pad=(0, 0, 0), swap=False, gray3=False):
    """One slot: picture is uint8 H_b x W_b (gray) or H_b x W_b x 3, or None (nothing but pad; `channels` then comes from gray3
    alone: call slot_of_pad); size = (H, W).  Returns C x H x W ("nchw") or H x W x C ("nhwc")."""
    H, W = size
    pic = np.asarray(picture)
    assert pic.dtype == np.uint8
    if pic.ndim == 2:
        pic = np.repeat(pic[:, :, None], 3 if gray3 else 1, axis=2)
    else:
        assert pic.shape[2] == 3 and not gray3
    C = pic.shape[2]
    assert not (swap and C == 1)
    if swap and picture.ndim == 3:
        pic = pic[:, :, ::-1]  # channel c comes from source channel 2 - c
    h, w = pic.shape[:2]
    assert 0 <= left and left + w <= W and 0 <= top and top + h <= H
    levels = np.empty((H, W, C), np.int64)
    levels[:] = np.asarray(pad, np.int64)[:C]
    levels[top:top + h, left:left + w] = pic
    out = convert(levels, np.asarray(scale, np.float64)[:C], np.asarray(bias, np.float64)[:C], dtype)
    return np.ascontiguousarray(out.transpose(2, 0, 1)) if layout == "nchw" else out


def slot_of_pad(channels, size, dtype="f32", layout="nchw", scale=(1, 1, 1), bias=(0, 0, 0), pad=(0, 0, 0)):
    """A slot that holds no picture"""
    H, W = size
    levels = np.empty((H, W, channels), np.int64)
    levels[:] = np.asarray(pad, np.int64)[:channels]
    out = convert(levels, np.asarray(scale, np.float64)[:channels], np.asarray(bias, np.float64)[:channels], dtype)
    return np.ascontiguousarray(out.transpose(2, 0, 1)) if layout == "nchw" else out


def place(size, picture_size, how="center"):
    """(left, top) of a picture of (w, h) in a slot of (H, W)"""
    (H, W), (w, h) = size, picture_size
    return ((W - w) // 2, (H - h) // 2) if how == "center" else (0, 0)


def fit_box_brute(out_size, box):
    """The largest N <= max(ow, oh) whose bounded size fits the box, by trying them all"""
    (ow, oh), (W, H) = out_size, box
    longer = max(ow, oh)
    best = None
    for N in range(1, longer + 1):
        if max(1, ow * N // longer) <= W and max(1, oh * N // longer) <= H:
            best = N
    return best
