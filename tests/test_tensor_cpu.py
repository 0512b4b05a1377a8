"""Network input tensors (lr_pack_tensor_device), what the CPU can show: the rounding rule of tests/numpy_tensor_ref.py against
exact rational arithmetic, fit_box against brute force, tensor_table's rows and refusals, TensorSpec's derivation, the
tensor map.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import librectify_amd as lr
import numpy_tensor_ref as ref

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TIE_SCALE = 13.0 / 1024.0  # v * 13 / 1024 is exact in float32; levels tie both ways in float16 and in bfloat16 (checked below)


def round_even(x, precision, emin):
    """The Fraction x rounded to nearest, ties to even, into a binary format of `precision` significand bits whose smallest
    normal number is 2^emin (below it the spacing stays 2^(emin - precision + 1)); also whether x was an exact tie, and if
    so whether it went up in magnitude.  By hand: the quotient by the spacing, its remainder against one half."""
    if x == 0:
        return Fraction(0), False, False
    sign, a = (-1 if x < 0 else 1), abs(x)
    e = 0  # 2^e <= a < 2^(e + 1)
    while Fraction(2) ** (e + 1) <= a:
        e += 1
    while Fraction(2) ** e > a:
        e -= 1
    ulp = Fraction(2) ** (max(e, emin) - precision + 1)
    q, rem = divmod(a, ulp)
    q = int(q)
    tie = rem * 2 == ulp
    up = rem * 2 > ulp or (tie and q % 2 == 1)
    return sign * (q + (1 if up else 0)) * ulp, tie, tie and up


def bf16_to_fraction(bits):
    f = (np.asarray(bits, np.uint32) << np.uint32(16)).view(np.float32)
    return [Fraction(float(v)) for v in f.reshape(-1)]


def spec_cases():
    mean, std = np.array(IMAGENET_MEAN), np.array(IMAGENET_STD)
    return {
        "imagenet": (np.float64(1.0) / (np.float64(255.0) * std), -mean / std),
        "unit": (np.full(3, np.float64(1.0) / np.float64(255.0)), np.zeros(3)),
        "tie": (np.full(3, TIE_SCALE), np.zeros(3)),
    }


@pytest.mark.parametrize("case", ["imagenet", "unit", "tie"])
def test_rounding_rule_against_fractions(case):
    scale, bias = spec_cases()[case]
    levels = np.repeat(np.arange(256)[:, None], 3, axis=1)
    f32 = ref.convert(levels, scale, bias, "f32")
    f16 = ref.convert(levels, scale, bias, "f16")
    b16 = ref.convert(levels, scale, bias, "bf16")
    assert f32.dtype == np.float32 and f16.dtype == np.float16 and b16.dtype == np.uint16
    ties = {"f16": [0, 0], "bf16": [0, 0]}  # [down, up]
    for c in range(3):
        b16_c = bf16_to_fraction(b16[:, c])
        for v in range(256):
            # the two double operations, each rounded to 53 bits by hand
            p, _, _ = round_even(Fraction(v) * Fraction(float(scale[c])), 53, -1022)
            y, _, _ = round_even(p + Fraction(float(bias[c])), 53, -1022)
            f, _, _ = round_even(y, 24, -126)
            assert Fraction(float(f32[v, c])) == f, (case, c, v)
            h, tie, up = round_even(f, 11, -14)
            assert Fraction(float(f16[v, c])) == h, (case, c, v)
            ties["f16"][up] += tie
            b, tie, up = round_even(f, 8, -126)
            assert b16_c[v] == b, (case, c, v)
            ties["bf16"][up] += tie
    if case == "tie":  # the tie rule is exercised, not assumed: both directions, both narrow types
        assert min(ties["f16"]) > 0 and min(ties["bf16"]) > 0, ties


def test_round_even_by_hand():
    # 1 + 2^-11 lies half way between the float16 neighbours 1 and 1 + 2^-10: to the even 1; 1 + 3 * 2^-11 goes up to 1 + 2^-9
    assert round_even(Fraction(2049, 2048), 11, -14) == (Fraction(1), True, False)
    assert round_even(Fraction(2051, 2048), 11, -14) == (Fraction(2052, 2048), True, True)
    assert round_even(Fraction(2050, 2048), 11, -14) == (Fraction(2050, 2048), False, False)
    # below 2^-14 float16 keeps the spacing 2^-24
    assert round_even(Fraction(3, 2 ** 25), 11, -14) == (Fraction(2, 2 ** 24), True, True)
    assert round_even(Fraction(-1, 2 ** 25), 11, -14) == (Fraction(0), True, False)
    # bfloat16: 8 bits
    assert round_even(Fraction(257, 256), 8, -126) == (Fraction(1), True, False)
    assert round_even(Fraction(259, 256), 8, -126) == (Fraction(260, 256), True, True)


BOXES = [(1, 1), (7, 5), (16, 16), (40, 3), (3, 40), (64, 64)]


@pytest.mark.parametrize("box", BOXES)
def test_fit_box_against_brute_force(box):
    for ow in range(1, 41):
        for oh in range(1, 41):
            assert lr.fit_box((ow, oh), box) == ref.fit_box_brute((ow, oh), box), (ow, oh, box)


def test_fit_box_properties():
    assert lr.fit_box((30, 20), (64, 64)) == 30  # fits already: never enlarged
    assert lr.fit_box((1, 40), (7, 5)) == 5  # a sliver: the short side stays 1
    assert lr.fit_box((40, 1), (7, 5)) == 7
    N = lr.fit_box((4000, 3000), (640, 640))
    _, _, size, _ = lr.shrink_homography(None, np.eye(3), (4000, 3000), N)
    assert size == (640, 480)
    with pytest.raises(ValueError):
        lr.fit_box((0, 5), (4, 4))
    with pytest.raises(ValueError):
        lr.fit_box((5, 5), (4, 0))


def test_tensor_spec_derivation():
    s = lr.TensorSpec((5, 7))
    assert s.size == (5, 7) and s.dtype == "f32" and s.layout == "nchw" and s.place == "center"
    assert np.array_equal(s.scale, np.full(3, np.float64(1.0) / np.float64(255.0))) and np.array_equal(s.bias, np.zeros(3))
    assert np.array_equal(s.pad, np.zeros(3))
    s = lr.TensorSpec((5, 7), "bf16", "nhwc", mean=IMAGENET_MEAN, std=IMAGENET_STD, pad=(1, 2, 255), bgr=True)
    want_scale, want_bias = spec_cases()["imagenet"]
    assert np.array_equal(s.scale, want_scale) and np.array_equal(s.bias, want_bias)  # two operations in float64, to the bit
    assert s.np_dtype == np.uint16 and s.shape(4, lr.PIX_U8X3) == (4, 5, 7, 3)
    assert lr.TensorSpec((5, 7), "f16").shape(2, lr.PIX_U8) == (2, 1, 5, 7)
    assert lr.TensorSpec((5, 7), gray3=True).shape(2, lr.PIX_U8) == (2, 3, 5, 7)
    s = lr.TensorSpec((5, 7), scale=(2, 3, 4), bias=0.5)
    assert np.array_equal(s.scale, [2, 3, 4]) and np.array_equal(s.bias, [0.5, 0.5, 0.5])
    a = s.args(np.zeros((1, 8)), 3)
    assert (a.n, a.height, a.width, a.dtype, a.layout, a.flags) == (3, 5, 7, lr.TENSOR_F32, lr.TENSOR_NCHW, 0)
    assert list(a.scale) == [2, 3, 4] and list(a.pad) == [0, 0, 0]
    assert lr.TensorSpec((1, 1), bgr=True, gray3=True).args(np.zeros((1, 8)), 1).flags == lr.TENSOR_SWAP | lr.TENSOR_GRAY3


@pytest.mark.parametrize("kwargs", [
    dict(size=(0, 4)), dict(size=(4,)), dict(size=(4, 2 ** 30 + 1)), dict(size=(4.5, 4)), dict(dtype="f64"), dict(layout="chw"),
    dict(place="bottom"), dict(std=(1, 0, 1)), dict(mean=(0, float("nan"), 0)), dict(mean=(1, 2)), dict(pad=256), dict(pad=-1),
    dict(pad=0.5), dict(pad=(0, 0, float("inf"))), dict(scale=float("inf")), dict(bias=(0, float("nan"), 0)),
])
def test_tensor_spec_refusals(kwargs):
    kw = dict(size=(4, 4))
    kw.update(kwargs)
    with pytest.raises(ValueError):
        lr.TensorSpec(**kw)


def test_tensor_spec_channel_refusals():
    with pytest.raises(ValueError):
        lr.TensorSpec((4, 4), gray3=True).channels(lr.PIX_U8X3)
    with pytest.raises(ValueError):
        lr.TensorSpec((4, 4), bgr=True).channels(lr.PIX_U8)
    with pytest.raises(ValueError):
        lr.TensorSpec((4, 4)).channels(lr.PIX_F32)
    assert lr.TensorSpec((4, 4), bgr=True, gray3=True).channels(lr.PIX_U8) == 3


def test_tensor_table_rows():
    spec = lr.TensorSpec((33, 130))
    sizes = np.array([[130, 33], [1, 1], [7, 5], [129, 32]])
    sources = np.array([[0, 130], [5000, 3], [6001, 40], [9000, 400]])
    t = lr.tensor_table(sizes, sources, np.array([3, 0, 6, 1]), spec)
    assert t.dtype == np.float64 and t.shape == (4, 8)
    assert t.tolist() == [[130, 33, 0, 130, 3, 0, 0, 0], [1, 1, 5000, 3, 0, 64, 16, 0], [7, 5, 6001, 40, 6, 61, 14, 0],
                          [129, 32, 9000, 400, 1, 0, 0, 0]]
    for row in t:  # the reference's placement rule
        assert (row[5], row[6]) == ref.place((33, 130), (int(row[0]), int(row[1])))
    t = lr.tensor_table(sizes, sources, np.array([3, 0, 6, 1]), lr.TensorSpec((33, 130), place="topleft"))
    assert not t[:, 5:].any()


@pytest.mark.parametrize("sizes, sources, slots", [
    ([[131, 33]], [[0, 131]], [0]),  # wider than the slot
    ([[130, 34]], [[0, 130]], [0]),  # taller
    ([[0, 3]], [[0, 4]], [0]),  # a size below 1
    ([[4, 3]], [[-1, 4]], [0]),  # a negative offset
    ([[4, 3]], [[0, 2 ** 53 + 2]], [0]),  # above 2^53
    ([[4, 3]], [[0, 4]], [-1]),  # a negative slot
    ([[4, 3], [4, 3]], [[0, 4], [12, 4]], [1, 1]),  # two frames in one slot
    ([[4, 3], [4, 3]], [[0, 4]], [0, 1]),  # shapes that do not agree
    ([[4, 3]], [[0, 4]], [[0]]),
    ([[4.0, 3.0]], [[0, 4]], [0]),  # not integers
    (np.zeros((0, 2), np.int64), np.zeros((0, 2), np.int64), np.zeros(0, np.int64)),  # no frames
])
def test_tensor_table_refusals(sizes, sources, slots):
    with pytest.raises(ValueError):
        lr.tensor_table(np.asarray(sizes), np.asarray(sources), np.asarray(slots), lr.TensorSpec((33, 130)))


def test_tensor_map_by_hand():
    M = np.array([[2.0, 0.5, 10.0], [0.25, 3.0, -4.0], [0.001, 0.002, 1.0]])
    T = lr.tensor_map(M, 7, 3)
    assert T.dtype == np.float64 and T.shape == (3, 3)
    # columns 0 and 1 stay; column 2 is M (-7, -3, 1), worked out by hand
    assert np.array_equal(T[:, :2], M[:, :2])
    assert np.allclose(T[:, 2], [10.0 - 14.0 - 1.5, -4.0 - 1.75 - 9.0, 1.0 - 0.007 - 0.006], rtol=0, atol=1e-15)
    # the tensor pixel (7 + x, 3 + y) reads what the picture's pixel (x, y) read
    for x, y in [(0, 0), (12, 0), (0, 9), (12, 9)]:
        a, b = T @ [7 + x, 3 + y, 1.0], M @ [x, y, 1.0]
        assert np.allclose(a[:2] / a[2], b[:2] / b[2], rtol=1e-14, atol=0)
    assert np.array_equal(lr.tensor_map(M, 0, 0), M)


def test_out_max_size_with_tensor_is_refused():
    # (refused before any GPU work: the tensor's box is the bound)
    ctx = lr.Context.__new__(lr.Context)
    ctx._h = None
    spec = lr.TensorSpec((64, 64))
    frame = np.zeros((48, 64), np.uint8)
    with pytest.raises(ValueError, match="out_max_size"):
        ctx.rectify(frame, tensor=spec, out_max_size=32)
    with pytest.raises(ValueError, match="out_max_size"):
        ctx.rectify_batch([frame, frame], tensor=spec, out_max_size=32)
