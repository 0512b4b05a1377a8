"""LR_WARP_CUBIC without a GPU: the table of weights (formula, the printed rows, the literals of csrc/tables.h), the int32
bound of the integer rule, its distance from a float64 evaluation, the identity map, what the rule buys on a magnified
picture, and the constant and the interp= argument of the Python package."""
import math
import os
import re

import numpy as np
import pytest

import numpy_warp_cubic_ref as RC
import numpy_warp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# rows 0 .. 16 as DESIGN.md section 3, item 15 prints them
ROWS_0_16 = [
    [0, 2048, 0, 0], [-45, 2043, 51, -1], [-84, 2031, 107, -6], [-118, 2009, 169, -12],
    [-147, 1981, 235, -21], [-171, 1946, 305, -32], [-190, 1903, 379, -44], [-205, 1854, 456, -57],
    [-216, 1800, 536, -72], [-223, 1740, 618, -87], [-227, 1676, 702, -103], [-227, 1607, 787, -119],
    [-225, 1535, 873, -135], [-220, 1460, 959, -151], [-213, 1380, 1046, -165], [-203, 1299, 1131, -179],
    [-192, 1216, 1216, -192],
]


def header_table():
    text = open(os.path.join(ROOT, "librectify_amd", "csrc", "tables.h")).read()
    m = re.search(r"kCubicWeights\[32\]\[4\]\s*=\s*\{(.*?)\};", text, re.S)
    assert m, "csrc/tables.h holds no kCubicWeights[32][4]"
    rows = re.findall(r"\{\s*(-?\d+)\s*,\s*(-?\d+)\s*,\s*(-?\d+)\s*,\s*(-?\d+)\s*\}", m.group(1))
    return np.array(rows, dtype=np.int64)


def test_table_from_the_formula_is_the_printed_one_and_the_headers():
    C = RC.table()
    assert C.shape == (32, 4)
    np.testing.assert_array_equal(C[:17], np.array(ROWS_0_16))
    H = header_table()
    assert H.shape == (32, 4)
    np.testing.assert_array_equal(H, C)
    assert (C.sum(axis=1) == 2048).all()
    for a in range(1, 32):
        np.testing.assert_array_equal(C[32 - a], C[a][::-1])
    assert int(np.abs(C).sum(axis=1).max()) == 2816
    assert int(np.abs(C).sum()) == 81896
    # the formula's operands are dyadic: float64 evaluates it exactly, and the unrounded weights sum to 1
    k = RC.kernel_f64(np.arange(32) / 32.0)
    assert (k.sum(axis=1) == 1.0).all() and (k * 2 ** 17 == np.rint(k * 2 ** 17)).all()


def maps(w, h, ow, oh):
    c, s = math.cos(0.3), math.sin(0.3)
    cx, cy = w / 2.0, h / 2.0
    return {
        "identity": np.eye(3),
        "half_pixel": np.array([[1.0, 0, 0.5], [0, 1, 0.5], [0, 0, 1]]),
        "third": np.array([[1.0, 0, 0.34375], [0, 1, 0.65625], [0, 0, 1]]),  # phases 11 and 21: the rows of sum |C| = 2816
        "scale_up": np.array([[0.37, 0, 0.2], [0, 0.41, -0.1], [0, 0, 1]]),
        "scale_down": np.array([[2.3, 0, 0], [0, 1.7, 0.5], [0, 0, 1]]),
        "rotation": np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy], [0, 0, 1.0]]),
        "perspective": np.array([[1.2, 0.3, -0.1 * w], [-0.05, 1.0, 0.05 * h], [0.6 / ow, 0.4 / oh, 1.0]]),
    }


def checkerboard(w, h, ch=None, cell=2):
    """0 / 255 squares of `cell` pixels: with 2, a row of taps can read 0, 255, 255, 0 -- the pattern of the weights' signs"""
    b = (((np.arange(h)[:, None] // cell + np.arange(w)[None, :] // cell) & 1) * 255).astype(np.uint8)
    return b if ch is None else np.ascontiguousarray(np.stack([b, 255 - b, b], axis=-1))


def test_the_integer_rule_fits_int32_on_a_checkerboard():
    assert 255 * 2816 ** 2 + 2 ** 21 == 2024210432 < 2 ** 31
    stats = {}
    for cell in (1, 2, 3):
        src = checkerboard(41, 37, cell=cell)
        for name, M in maps(41, 37, 90, 80).items():
            RC.warp(src, M, 90, 80, stats=stats)
    print("largest |s|: %d" % stats["max_abs_s"])
    assert stats["max_abs_s"] < 2 ** 31 - 2 ** 21, stats
    assert stats["max_abs_s"] > 255 * 2048 * 2048  # (the overshoot is met: without the clamp the result would leave 0 .. 255)


def test_the_integer_rule_stays_within_a_level_of_float64():
    """|integer result - float64 evaluation| < 1.  The bound: a rounded weight is within 0.5 / 2048 of its value (1 / 2048
    for the one entry that takes the row's remainder), so the two-pass sum of products of weights differs from the float64
    one by at most 255 * 0.00172 = 0.44 levels, and the final rounding adds 0.5: 0.94."""
    rng = np.random.default_rng(7)
    w, h = 61, 47
    worst = 0.0
    low = high = False
    for ch in (None, 3):
        src = rng.integers(0, 256, (h, w) if ch is None else (h, w, 3), dtype=np.uint8)
        src[10:30, 20:44] = checkerboard(24, 20, ch)
        for name, M in maps(w, h, 97, 71).items():
            got = RC.warp(src, M, 97, 71).astype(np.float64)
            f = RC.warp_f64(src, M, 97, 71)
            worst = max(worst, float(np.abs(got - f).max()))
            low, high = low or bool((f == 0.0).any() and (got == 0).any()), high or bool((f == 255.0).any())
    print("largest distance from float64: %.4f levels" % worst)
    assert worst < 1.0, worst
    assert low and high  # both clamps fired


def test_identity_reproduces_the_source_exactly():
    rng = np.random.default_rng(3)
    for shape, dtype in (((19, 23), np.uint8), ((19, 23, 3), np.uint8), ((19, 23), np.float32)):
        if dtype == np.uint8:
            src = rng.integers(0, 256, shape, dtype=np.uint8)
        else:
            src = ((rng.random(shape, dtype=np.float32) - np.float32(0.5)) * np.float32(1e6)).astype(np.float32)
            src[3, 4], src[5, 6] = np.float32(0.0), np.float32(3e38)
        out = RC.warp(src, np.eye(3), shape[1], shape[0])
        assert out.dtype == src.dtype
        assert out.tobytes() == src.tobytes()


def test_cubic_halves_the_error_of_a_magnified_picture():
    w, h, scale, inset = 128, 96, 2.7, 2.0
    f = lambda x, y: 127.5 + 60.0 * np.sin(x) + 55.0 * np.cos(y / 0.9 + x / 9.0)  # noqa: E731
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    src = np.rint(f(xs, ys)).astype(np.uint8)
    ow, oh = int((w - 2 * inset) * scale), int((h - 2 * inset) * scale)
    M = np.array([[1 / scale, 0, inset], [0, 1 / scale, inset], [0, 0, 1.0]])
    X, Y = R.fixed_coords(M, ow, oh)
    truth = f(X / 32.0, Y / 32.0)  # the function at the very coordinates both rules sample
    rms = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - truth) ** 2)))  # noqa: E731
    cubic, linear = rms(RC.warp(src, M, ow, oh)), rms(R.warp(src, M, ow, oh))
    print("rms error: cubic %.3f, bilinear %.3f" % (cubic, linear))
    assert cubic <= 0.5 * linear, (cubic, linear)


def test_the_constant_and_the_header():
    import librectify_amd as L

    assert L.WARP_CUBIC == 0x8000
    header = open(os.path.join(ROOT, "include", "librectify_amd.h")).read()
    assert re.search(r"enum\s+lr_warp_sampling\s*\{\s*LR_WARP_CUBIC\s*=\s*0x8000\s*\}", header)
    others = [L.WARP_PREPARE, L.WARP_PACKED, L.WARP_RAGGED, L.WARP_LINES, L.WARP_JPEG, L.WARP_JPEG_DECODE]
    for o in others:
        assert L.WARP_CUBIC & o == 0
    assert L.WARP_CUBIC & (0x400 | 0x10000 | 1 << 30 | 0xFF) == 0  # (the bits existing tests expect to be refused, and the format)


@pytest.mark.parametrize("method,args", [
    ("warp_perspective", (np.zeros((4, 4), np.uint8), np.eye(3), (4, 4))),
    ("rectify", (np.zeros((8, 8), np.uint8),)),
    ("rectify_batch", (np.zeros((1, 8, 8), np.uint8),)),
    ("rectify_batch_device", (0, 1, 8, 8, 0)),
    ("rectify_frames_device", (0, [(8, 8, 0, 8)], 0)),
])
def test_an_unknown_interp_is_a_value_error_without_a_context(method, args):
    import librectify_amd as L

    ctx = object.__new__(L.Context)  # no device, no library call: the argument is checked first
    ctx._h = None
    for bad in ("bogus", "CUBIC", None, 1):
        with pytest.raises(ValueError, match="interp"):
            getattr(ctx, method)(*args, interp=bad)
