"""8-bit frames in the detector, what can be checked without a GPU: the header's
lr_frames_option and the mirror's constants agree, the mirror's word helper round-trips and leaves the plain flag
alone, and the definition p = float(luma) * (1/256.f) stated here in NumPy equals tests/numpy_prepare_ref.py at
out == src."""
import os
import re

import numpy as np
import pytest

import numpy_prepare_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def L():
    import librectify_amd as L

    return L


def _header_enum(name):
    txt = open(os.path.join(ROOT, "include", "librectify_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"enum\s+%s\s*\{([^}]*)\}" % name, txt)
    assert m, "enum %s is not declared" % name
    out = {}
    for item in m.group(1).split(","):
        if item.strip():
            k, v = item.split("=")
            out[k.strip()] = int(v.strip(), 0)
    return out


def test_header_declares_the_frames_option_and_the_mirror_agrees(L):
    opt = _header_enum("lr_frames_option")
    assert opt == {"LR_FRAMES_U8": 0x100, "LR_FRAMES_U8X3": 0x200, "LR_FRAMES_F32": 0x300}
    assert (L.FRAMES_U8, L.FRAMES_U8X3, L.FRAMES_F32) == (opt["LR_FRAMES_U8"], opt["LR_FRAMES_U8X3"], opt["LR_FRAMES_F32"])
    pix = _header_enum("lr_pixel_format")
    assert (L.PIX_U8, L.PIX_U8X3, L.PIX_F32) == (pix["LR_PIX_U8"], pix["LR_PIX_U8X3"], pix["LR_PIX_F32"])
    for name, fmt in (("LR_FRAMES_U8", "LR_PIX_U8"), ("LR_FRAMES_U8X3", "LR_PIX_U8X3"), ("LR_FRAMES_F32", "LR_PIX_F32")):
        assert opt[name] == (pix[fmt] + 1) << 8


def test_word_helper_round_trips_and_leaves_the_plain_flag_alone(L):
    # fp32 frames: the word is the flag, 0 or 1, as every call before this feature passed it
    assert L.frames_word(L.PIX_F32, False) == 0 and L.frames_word(L.PIX_F32, True) == 1
    assert L.frames_word(L.PIX_F32, 0) == 0 and L.frames_word(L.PIX_F32, 7) == 1
    assert L.frames_word(L.PIX_U8, False) == L.FRAMES_U8 and L.frames_word(L.PIX_U8, True) == L.FRAMES_U8 | 1
    assert L.frames_word(L.PIX_U8X3, False) == L.FRAMES_U8X3 and L.frames_word(L.PIX_U8X3, True) == L.FRAMES_U8X3 | 1
    for fmt in (L.PIX_U8, L.PIX_U8X3, L.PIX_F32):
        for flag in (False, True):
            assert L.split_frames_word(L.frames_word(fmt, flag)) == (fmt, flag)
    # the explicit fp32 word reads as fp32 too
    assert L.split_frames_word(L.FRAMES_F32) == (L.PIX_F32, False) and L.split_frames_word(L.FRAMES_F32 | 1) == (L.PIX_F32, True)
    # every value outside 256 .. 1023 is the plain flag on fp32 frames
    for word, flag in ((0, False), (1, True), (-1, True), (2, True), (255, True), (1024, True), (0x10100, True), (-256, True),
                       (-(1 << 31), True), ((1 << 31) - 1, True)):
        assert L.split_frames_word(word) == (L.PIX_F32, flag), word
    for word in (256, 257, 511, 512, 767, 768, 1023):
        assert L.split_frames_word(word)[0] == (word >> 8) - 1
    with pytest.raises(ValueError):
        L.frames_word(3, False)


def _p(frame):
    """DESIGN.md section 3, item 11"""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8
    if frame.ndim == 3:
        c = frame.astype(np.uint32)
        luma = (4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14
    else:
        luma = frame
    assert luma.max() <= 255
    return luma.astype(np.float32) * np.float32(1.0 / 256.0)


def test_definition_equals_the_prepare_reference_at_the_frames_own_size():
    gray = np.load(os.path.join(G, "doc_image_gray.npy"))
    assert gray.dtype == np.uint8 and gray.shape == (563, 1000)
    crop = np.ascontiguousarray(gray[100:180, 300:420])
    rng = np.random.RandomState(5)
    rgb = np.stack([crop, np.roll(crop, 3, axis=1), rng.randint(0, 256, crop.shape).astype(np.uint8)], axis=2)
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    for frame in (crop, rgb, ramp, np.stack([ramp, ramp.T, ramp[::-1]], axis=2)):
        h, w = frame.shape[:2]
        p = _p(frame)
        assert p.dtype == np.float32
        assert p.tobytes() == np.ascontiguousarray(P.unit_values(frame), np.float32).tobytes()
        assert p.tobytes() == np.ascontiguousarray(P.prepare(frame, w, h)).tobytes()
        # exact: every value is k / 256 with k an integer below 256
        assert np.array_equal(p.astype(np.float64) * 256.0, np.round(p.astype(np.float64) * 256.0))
    # luma of equal channels is the channel (the weights sum to 2^14)
    assert _p(np.stack([ramp] * 3, axis=2)).tobytes() == _p(ramp).tobytes()
