"""LR_JPEG_ANY_SAMPLING without a GPU: the header parser through the C ABI in probe mode, the restatement
(tests/numpy_jpeg_sampling_ref.py) against numpy_jpeg_decode_ref on the files that need no option and against PIL's decodes
of the files that do (tests/golden/jpeg_sampling_kat.npz, tools/make_jpeg_sampling_fixtures.py), the option's encoding, and
the Python keyword.

Measured against PIL 12.2 / libjpeg-turbo, colour output, the largest difference per sampling over the fixtures
(DESIGN.md section 3, item 14): see MEASURED.  Where no component has a ratio of 4 on one axis and 2 on the other the
difference is today's 3 at most.  0x42 and 0x24 stand apart (25 and 52): for such a component libjpeg-turbo has no triangle
and replicates along both axes, while the rule here keeps the triangle along the ratio-2 axis."""
import ctypes as C
import os

import numpy as np
import pytest

import numpy_jpeg_decode_ref as D
import numpy_jpeg_sampling_ref as S

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
G = os.path.join(ROOT, "tests", "golden")
# the first word of a fixture's name: the largest difference of colour output from PIL's decode, over the fixtures of that word
MEASURED = {"s12": 3, "s41": 3, "s14": 2, "s42": 25, "s24": 52, "s21x3": 3, "s22": 3, "t440": 2, "big440": 3}
SAMPLING_BYTE = {"s12": 0x12, "s41": 0x41, "s14": 0x14, "s42": 0x42, "s24": 0x24, "s21x3": 0x21, "s22": 0x22, "t440": 0x12, "big440": 0x12}


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(G, "jpeg_sampling_kat.npz"))


@pytest.fixture(scope="module")
def old():
    return np.load(os.path.join(G, "jpeg_decode_kat.npz"))


@pytest.fixture(scope="module")
def L():
    import librectify_amd as L
    from librectify_amd import build

    build.build(verbose=False)
    L.lib()
    return L


def word(name):
    return name.split("_")[0]


def test_probe_through_the_c_abi(L, kat, old):
    names = [str(n) for n in kat["names"]]
    streams = [kat["stream_" + n].tobytes() for n in names]
    assert {word(n) for n in names} == set(MEASURED)
    without = L.jpeg_info(streams)
    assert without[:, 5].tolist() == [2] * len(names), "without the bit the files are refused as before"
    for n, s, row in zip(names, streams, without):
        assert row.tolist() == D.probe(s).row(), n
    L.jpeg_info(streams[:1])
    assert b"sampling other than 4:2:0, 4:4:4, 4:2:2" in L.lib().lr_last_error()
    info = L.jpeg_info(streams, any_sampling=True)
    assert info.dtype == np.int32 and info.shape == (len(names), 8)
    for n, s, row in zip(names, streams, info):
        pil = kat["pil_" + n]
        assert row.tolist() == [pil.shape[1], pil.shape[0], 3, SAMPLING_BYTE[word(n)], row[4], 0, 0, 0], n
        assert row.tolist() == S.info_row(s), n
    restarts = {n: int(row[4]) for n, row in zip(names, info)}
    assert restarts["s12_67x35_r1"] == 1 and restarts["s41_67x35_r3"] == 3 and restarts["s12_67x35_rows"] == 9 and restarts["s12_67x35"] == 0
    # what needs no option is told as without it
    accepted = [old["stream_" + str(n)].tobytes() for n in old["names"]]
    assert np.array_equal(L.jpeg_info(accepted, any_sampling=True), L.jpeg_info(accepted))
    # the old rejects: progressive and CMYK stay refused; the header-patched c440 is a 4:2:0 scan under a 1 x 2 header, whose
    # damage only the device can see, so that the headers alone now pass
    rejects = [str(n) for n in old["rejects"]]
    assert rejects == ["progressive", "c440", "cmyk"]
    got = L.jpeg_info([old["stream_" + n].tobytes() for n in rejects], any_sampling=True)
    assert got[:, 5].tolist() == [2, 0, 2] and got[1].tolist() == [40, 24, 3, 0x12, 0, 0, 0, 0]
    for n in rejects:
        assert S.probe(old["stream_" + n].tobytes()).status == got[rejects.index(n), 5]


def patched(stream, y, cb=0x11, cr=0x11):
    s = bytearray(stream)
    at = S.sof_sampling(bytes(s))
    s[at], s[at + 3], s[at + 6] = y, cb, cr
    return bytes(s)


def test_what_the_bit_does_not_admit(L, kat):
    base = kat["stream_s12_9x7"].tobytes()
    refused = {
        "luminance below chrominance, horizontally": (0x11, 0x21, 0x11),
        "luminance below chrominance, vertically": (0x21, 0x11, 0x12),
        "a factor of 3": (0x31, 0x11, 0x11),
        "a factor of 3 in the chrominance": (0x44, 0x13, 0x11),
        "a factor of 0": (0x20, 0x11, 0x11),
        "more than 10 blocks": (0x44, 0x11, 0x11),
        "12 blocks": (0x22, 0x22, 0x22),
        "11 blocks": (0x42, 0x21, 0x11),
    }
    for what, hv in refused.items():
        s = patched(base, *hv)
        assert L.jpeg_info([s], any_sampling=True)[0, 5] == 2 and S.probe(s).status == 2, what
    for what, hv in {"10 blocks": (0x42, 0x11, 0x11), "Cb and Cr differ": (0x22, 0x12, 0x21), "4:2:0": (0x22, 0x11, 0x11)}.items():
        s = patched(base, *hv)
        row = L.jpeg_info([s], any_sampling=True)[0]
        assert row[5] == 0 and row.tolist() == S.info_row(s), what
    assert L.jpeg_info([patched(base, 0x22)], any_sampling=True)[0, 3] == 0, "the three layouts keep 0, 1, 2"
    # a one-component file is one block to the MCU whatever its header says, with the bit and without
    gray = np.load(os.path.join(G, "jpeg_decode_kat.npz"))["stream_g_9x7"].tobytes()
    at = gray.index(b"\xFF\xC0") + 4 + 7
    odd = gray[:at] + b"\x32" + gray[at + 1:]
    assert L.jpeg_info([odd], any_sampling=True)[0].tolist() == L.jpeg_info([odd])[0].tolist() == [9, 7, 1, 0, 0, 0, 0, 0]


def test_restatement_on_the_files_that_need_no_option(old):
    for n in old["names"]:
        s = old["stream_" + str(n)].tobytes()
        assert S.info_row(s) == D.probe(s).row()
        for fmt in ("u8", "u8x3"):
            status, want = D.decode(s, fmt)
            got_status, got = S.decode(s, fmt)
            assert status == got_status == 0 and got.dtype == want.dtype and np.array_equal(got, want), (str(n), fmt)
    for n in ("progressive", "cmyk"):
        assert S.decode(old["stream_" + n].tobytes())[0] == 2
    assert S.decode(old["stream_c440"].tobytes())[0] == D.DAMAGED, "a 4:2:0 scan under a 1 x 2 header"


def test_restatement_against_pil(kat):
    """asserts the recorded maxima exactly: a change of the rule, of the fixtures or of PIL's decodes shows"""
    worst = {}
    for n in kat["names"]:
        n = str(n)
        s, pil = kat["stream_" + n].tobytes(), kat["pil_" + n]
        assert D.decode(s)[0] == 2 and S.decode(s, any_sampling=False)[0] == 2, n
        status, ours = S.decode(s)
        assert status == 0 and ours.shape == pil.shape and ours.dtype == np.uint8, n
        diff = int(np.abs(ours.astype(int) - pil.astype(int)).max())
        print("%-20s differs by at most %d" % (n, diff))
        worst[word(n)] = max(worst.get(word(n), 0), diff)
        status, y = S.decode(s, "u8")
        assert status == 0 and y.shape == pil.shape[:2]
    assert worst == MEASURED


def test_upsampling_rule_by_hand():
    """the rule on a plane small enough to write the result down"""
    p = np.array([[0, 16, 64], [32, 48, 128]])
    assert S.upsample(p, 3, 2, 1, 1).tolist() == p.tolist()
    assert S.upsample(p, 6, 2, 2, 1)[0].tolist() == [0, 4, 12, 28, 52, 64]
    assert S.upsample(p, 11, 2, 4, 1)[1].tolist() == [32] * 4 + [48] * 4 + [128] * 3
    assert S.upsample(p, 3, 4, 1, 2)[:, 1].tolist() == [16, 24, 40, 48]
    # ratio 4 across and 2 down: the triangle down, over the replicated samples
    assert S.upsample(p, 9, 4, 4, 2)[:, 4].tolist() == [16, 24, 40, 48] and S.upsample(p, 9, 4, 4, 2)[1].tolist() == [8] * 4 + [24] * 4 + [80]
    # both 2: today's (9, 3, 3, 1)
    assert S.upsample(p, 6, 4, 2, 2).tolist() == D.upsample(p, 6, 4, 2, 2).tolist()


def test_the_option_bit(L):
    others = L.WARP_PREPARE | L.WARP_PACKED | L.WARP_RAGGED | L.WARP_LINES | L.WARP_JPEG | L.WARP_JPEG_DECODE | L.WARP_CUBIC
    assert L.JPEG_ANY_SAMPLING == 0x20000 == S.ANY_SAMPLING
    assert L.JPEG_ANY_SAMPLING & (0x400 | 0x10000 | (1 << 30) | 0xFF | others) == 0
    with open(os.path.join(ROOT, "include", "librectify_amd.h")) as f:
        header = f.read()
    assert "LR_JPEG_ANY_SAMPLING = 0x20000" in header
    for name in ("LR_WARP_PREPARE", "LR_WARP_PACKED", "LR_WARP_RAGGED", "LR_WARP_LINES", "LR_WARP_JPEG", "LR_WARP_JPEG_DECODE", "LR_WARP_CUBIC"):
        value = int(header.split(name + " = ")[1].split(" ")[0], 16)
        assert value & 0x20000 == 0 and value & others == value, name
    assert not any("any_sampling" in e.lower() for e in L.EXPORTS), "the bit adds no exported symbol"


def test_the_bit_travels_with_the_decoder_call_alone(L, kat):
    """through the routed call in probe mode: with the bit and another unknown bit the call still fails, and a warp call
    that is no decoder call refuses the bit"""
    s = kat["stream_s41_9x7"].tobytes()
    region = np.frombuffer(s, np.uint8)
    table = np.array([[0, len(s), 0, 0, 0, 0, 0, 0]], np.float64)

    def call(word):
        info = np.full((1, 8), -7, np.int32)
        args = L.JpegDecodeArgs(L._ptr(region), L._ptr(table), L._ptr(info))
        rc = L.lib().lr_warp_perspective_device(None, None, region.nbytes, 1, 0, 0, 0, word, C.cast(C.byref(args), C.c_void_p), None, 0, 0, 0, 0)
        return rc, info[0].tolist()

    assert call(L.PIX_U8X3 | L.WARP_JPEG_DECODE) == (0, [9, 7, 3, 0, 0, 2, 0, 0])
    assert call(L.PIX_U8X3 | L.WARP_JPEG_DECODE | L.JPEG_ANY_SAMPLING) == (0, [9, 7, 3, 0x41, 0, 0, 0, 0])
    assert call(L.PIX_U8 | L.WARP_JPEG_DECODE | L.JPEG_ANY_SAMPLING) == (0, [9, 7, 3, 0x41, 0, 0, 0, 0])
    for extra in (0x400, 0x10000, 1 << 30, L.WARP_RAGGED):
        rc, info = call(L.PIX_U8X3 | L.WARP_JPEG_DECODE | L.JPEG_ANY_SAMPLING | extra)
        assert rc != 0 and info == [-7] * 8
    rc, info = call(L.PIX_U8X3 | L.JPEG_ANY_SAMPLING)
    assert rc != 0 and info == [-7] * 8, "without LR_WARP_JPEG_DECODE the bit is an unknown option of the warp"


def test_any_sampling_goes_with_files(L):
    arrays = [np.zeros((16, 16, 3), np.uint8)]
    assert L._all_streams([b"x"], "rectify_batch", any_sampling=True)
    with pytest.raises(ValueError, match="any_sampling"):
        L._all_streams(arrays, "rectify_batch", any_sampling=True)
    ctx = object.__new__(L.Context)  # (the keyword is refused before anything touches a device)
    for call in (lambda: ctx.rectify(arrays[0], any_sampling=True), lambda: ctx.rectify_batch(arrays, any_sampling=True),
                 lambda: ctx.rectify_batch(np.stack(arrays), any_sampling=True),
                 lambda: ctx.draw_lines_batch(arrays, [np.zeros(0, L.LINE_DTYPE)], any_sampling=True)):
        with pytest.raises(ValueError, match="any_sampling"):
            call()
