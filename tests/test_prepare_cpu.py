"""The prepare step without a GPU: its second source (tests/numpy_prepare_ref.py) in float32 against float64, the
cases whose result is known exactly, prepared_size against hand-computed cases, and the constant in the header."""
import os
import re

import numpy as np
import pytest

import numpy_prepare_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_u8(w, h, seed, channels=1):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3) if channels == 3 else (h, w), dtype=np.uint8)


@pytest.mark.parametrize("w,h,ow,oh", [(1999, 1201, 1200, 721), (3840, 2160, 1200, 675), (640, 480, 200, 150), (700, 300, 9, 4)])
def test_float32_sums_stay_within_their_rounding_bound_of_float64(w, h, ow, oh):
    """Each multiply-add rounds twice, at half an ulp of a partial sum that is at most 1 (the weights of an axis sum to
    1 and p < 1): 2^-24 per tap, so (Kx + Ky) 2^-24 with Kx, Ky the largest tap counts."""
    src = random_u8(w, h, 1)
    f32, f64 = P.prepare(src, ow, oh), P.prepare(src, ow, oh, np.float64)
    bound = (P.max_taps(w, ow) + P.max_taps(h, oh)) * 2.0 ** -24
    worst = float(np.abs(f32.astype(np.float64) - f64).max())
    print("%dx%d -> %dx%d: max |f32 - f64| = %.3f * 2^-24, bound %.0f * 2^-24" % (w, h, ow, oh, worst * 2.0 ** 24, bound * 2.0 ** 24))
    assert f32.dtype == np.float32 and worst <= bound


@pytest.mark.parametrize("channels", [1, 3])
def test_identity_size_is_the_conversion_alone(channels):
    src = random_u8(131, 77, 2, channels)
    c = src.astype(np.int64)
    luma = src if channels == 1 else (4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14
    exp = luma.astype(np.float32) / np.float32(256.0)
    np.testing.assert_array_equal(P.prepare(src, 131, 77).view(np.uint32), exp.view(np.uint32))
    for _, w in P.spans(131, 131):
        assert w.tolist() == [1.0]


def test_identity_size_leaves_a_float_frame_alone():
    src = np.random.default_rng(3).random((40, 50), dtype=np.float32)
    np.testing.assert_array_equal(P.prepare(src, 50, 40).view(np.uint32), src.view(np.uint32))


def test_pixels_repeated_2x2_come_back_at_half_size():
    src = random_u8(97, 61, 4)
    big = np.repeat(np.repeat(src, 2, axis=0), 2, axis=1)
    exp = src.astype(np.float32) / np.float32(256.0)
    np.testing.assert_array_equal(P.prepare(big, 97, 61).view(np.uint32), exp.view(np.uint32))


def test_weights_of_an_axis():
    # 10 -> 4: s = 2.5; sample 1 covers [2.5, 5): half of tap 2, taps 3 and 4
    sp = P.spans(10, 4)
    assert [a for a, _ in sp] == [0, 2, 5, 7]
    np.testing.assert_array_equal(sp[1][1], np.array([0.5 / 2.5, 1 / 2.5, 1 / 2.5], np.float32))
    np.testing.assert_array_equal(sp[3][1], np.array([0.5 / 2.5, 1 / 2.5, 1 / 2.5], np.float32))
    for n_src, n_dst in ((8192, 1), (1999, 1200), (563, 563), (7, 3)):
        sp = P.spans(n_src, n_dst)
        assert sp[0][0] == 0 and sp[-1][0] + len(sp[-1][1]) == n_src
        assert all(abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-5 for _, w in sp)


def test_prepared_size_against_hand_computed_cases():
    import librectify_amd as L

    f = np.float32
    cases = [
        # w, h, max_size -> out_w, out_h, scale
        (1000, 563, 1200, 1000, 563, f(1.0)),            # smaller than max_size: unchanged
        (3840, 2160, 1200, 1200, 675, f(0.3125)),        # 2160 * 0.3125 = 675 exactly
        (2000, 1125, 1000, 1000, 563, f(0.5)),           # 562.5 rounds away from zero
        (2000, 1126, 1000, 1000, 563, f(0.5)),
        (2000, 1126, 0.5, 1000, 563, f(0.5)),            # a fraction of the longer side
        (563, 1000, 500, 282, 500, f(0.5)),              # 281.5 rounds up; portrait
        (8192, 8192, 1200, 1200, 1200, f(1200) / f(8192)),
        (5000, 3, 100, 100, 1, f(0.02)),                 # 0.06 rounds to 0: at least 1
        (1200, 1200, 1200, 1200, 1200, f(1.0)),
    ]
    for w, h, m, ow, oh, scale in cases:
        got = L.prepared_size(w, h, m)
        assert got[:2] == (ow, oh) and got[2] == scale and type(got[2]) is np.float32, (w, h, m, got)


def test_header_and_python_agree_on_the_option():
    import librectify_amd as L

    header = open(os.path.join(ROOT, "include", "librectify_amd.h")).read()
    m = re.search(r"enum\s+lr_warp_option\s*\{\s*LR_WARP_PREPARE\s*=\s*(0x[0-9A-Fa-f]+|\d+)\s*\}", header)
    assert m and int(m.group(1), 0) == 0x100 == L.WARP_PREPARE
    assert L.WARP_PREPARE & 0xFF == 0 and (L.PIX_U8, L.PIX_U8X3, L.PIX_F32) == (0, 1, 2)
