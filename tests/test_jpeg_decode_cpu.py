"""The JPEG decoder without a GPU: the restatement (tests/numpy_jpeg_decode_ref.py) against
float64 and against PIL's decodes kept in tests/golden/jpeg_decode_kat.npz (tools/make_jpeg_decode_fixtures.py), the round
trip through the encoder's restatement, and the header parser through the C ABI in probe mode (no context, no device).

Measured against PIL 12.2 / libjpeg-turbo (profiles/jpeg_decode.txt), colour output, per layout over the fixtures and
doc_image.jpg: 4:4:4 maximum difference 3, lowest PSNR 60.06 dB; 4:2:2 maximum 3, lowest 52.90 dB; 4:2:0 maximum 3, lowest
54.77 dB (the 9 x 7 pictures; 56.53 dB on doc_image.jpg).  One-component output differs by at most 1."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import numpy_jpeg_decode_ref as D
import numpy_jpeg_ref as R

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
G = os.path.join(ROOT, "tests", "golden")
# layout: (the measured maximum difference, the measured lowest PSNR) of colour output against PIL
MEASURED = {D.LAYOUT_444: (3, 60.06), D.LAYOUT_422: (3, 52.90), D.LAYOUT_420: (3, 54.77)}


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(G, "jpeg_decode_kat.npz"))


@pytest.fixture(scope="module")
def doc():
    with open(os.path.join(G, "doc_image.jpg"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def L():
    import librectify_amd as L
    from librectify_amd import build

    build.build(verbose=False)
    L.lib()
    return L


def float_idct(f):
    """(..., 8, 8) dequantised coefficients f[v][u] -> samples, float64"""
    x, u = np.arange(8), np.arange(8)
    c = np.where(u == 0, np.sqrt(0.5), 1.0)
    basis = 0.5 * c[:, None] * np.cos((2 * x[None, :] + 1) * u[:, None] * np.pi / 16)  # [u][x]
    return np.einsum("vy,...vu,ux->...yx", basis, f.astype(np.float64), basis) + 128.0


def test_idct_is_within_one_level_of_float64():
    rng = np.random.default_rng(1180)
    ones = np.ones(64, np.int64)
    worst = 0
    for amplitude in (5, 50, 256, 300):  # IEEE 1180-1990's ranges (5, 256, 300) and one between: uniform coefficients
        f = rng.integers(-amplitude, amplitude + 1, (20000, 64))
        ours = D.idct(f, ones)
        exact = np.clip(np.rint(float_idct(f.reshape(-1, 8, 8))), 0, 255)
        diff = np.abs(ours - exact)
        worst = max(worst, int(diff.max()))
        print("amplitude %4d: %.3f %% of the samples differ, at most by %d" % (amplitude, 100.0 * (diff != 0).mean(), diff.max()))
    assert worst <= 1


def test_idct_on_extreme_coefficients_is_the_rule_in_big_integers():
    rng = np.random.default_rng(7)
    blocks = [np.full(64, 32767), np.full(64, -32768), np.where(np.arange(64) % 2, 32767, -32768), rng.integers(-32768, 32768, 64),
              np.eye(1, 64, 0, dtype=np.int64)[0] * 2047, rng.integers(-2048, 2048, 64)]
    for q in (1, 16, 255):
        for c in blocks:
            got = D.idct(np.asarray(c, np.int64), np.full(64, q, np.int64))
            T = [[int(v) for v in row] for row in R.DCT]
            f = [[max(-D.COEF_LIMIT, min(D.COEF_LIMIT, int(c[v * 8 + u]) * q)) for u in range(8)] for v in range(8)]
            a = [[max(-D.MID_LIMIT, min(D.MID_LIMIT, (sum(T[u][x] * f[v][u] for u in range(8)) + 64) >> 7)) for x in range(8)] for v in range(8)]
            want = [[max(0, min(255, ((sum(T[v][y] * a[v][x] for v in range(8)) + (1 << 18)) >> 19) + 128)) for x in range(8)] for y in range(8)]
            assert max(abs(sum(T[v][y] * a[v][x] for v in range(8))) for x in range(8) for y in range(8)) < 2 ** 31 - 2 ** 18
            assert got.tolist() == want


def pil_decodes(kat, doc):
    """(name, stream, PIL's decode) of every accepted fixture and of doc_image.jpg"""
    out = [(str(n), kat["stream_" + str(n)].tobytes(), kat["pil_" + str(n)]) for n in kat["names"]]
    status, ours = D.decode(doc)
    assert status == 0
    pil = (ours.astype(np.int16) - kat["doc_diff"]).astype(np.uint8)
    assert hashlib.sha256(pil.tobytes()).digest() == kat["doc_sha"].tobytes(), "the stored difference no longer leads to PIL's decode"
    return out + [("doc_image", doc, pil)]


def test_restatement_against_pil(kat, doc):
    """One component: within 2 levels (each side is within 1 of the ideal inverse transform).  Colour: the measured
    maximum plus one level and the measured PSNR minus 0.5 dB, per layout (this file's docstring)."""
    seen = set()
    for name, stream, pil in pil_decodes(kat, doc):
        info = D.probe(stream)
        fmt = "u8x3" if pil.ndim == 3 else "u8"
        status, ours = D.decode(stream, fmt)
        assert status == 0 and ours.shape == pil.shape, name
        diff = int(np.abs(ours.astype(int) - pil.astype(int)).max())
        print("%-20s layout %d: differs by at most %d, %.2f dB" % (name, info.layout, diff, R.psnr(ours, pil)))
        if pil.ndim == 2:
            assert diff <= 2, name
            continue
        worst, psnr = MEASURED[info.layout]
        assert diff <= worst + 1, name
        assert R.psnr(ours, pil) >= psnr - 0.5, name
        seen.add(info.layout)
        # the luminance plane of a colour stream has the picture's size
        status, y = D.decode(stream, "u8")
        assert status == 0 and y.shape == pil.shape[:2]
    assert seen == set(MEASURED)


@pytest.mark.parametrize("q", (50, 90, 95))
def test_round_trip_matches_pil_decode_of_the_same_stream(q):
    """the encoder test's shape (257 x 131) and margin (0.1 dB); PIL's figures are those of tests/golden/jpeg_kat.npz"""
    enc = np.load(os.path.join(G, "jpeg_kat.npz"))
    img = R.synth_u8(257, 131, 12, False)
    stream = R.encode(img, q, 0)
    assert stream == enc["stream_g_%d" % q].tobytes()
    status, ours = D.decode(stream, "u8")
    assert status == 0
    assert abs(R.psnr(ours, img) - float(enc["ref_g_%d" % q][0])) <= 0.1
    col = R.synth_u8(203, 117, 21, True)
    for name, layout in (("c420", 0), ("c444", 1)):
        stream = enc["stream_%s_%d" % (name, q)].tobytes()
        status, ours = D.decode(stream, "u8x3")
        assert status == 0
        assert abs(R.psnr(ours, col) - float(enc["ref_%s_%d" % (name, q)][0])) <= 0.1, name


def test_probe_through_the_c_abi(L, kat, doc):
    names = [str(n) for n in kat["names"]]
    rejects = [str(n) for n in kat["rejects"]]
    dht = doc.index(b"\xFF\xC4")
    streams = [kat["stream_" + n].tobytes() for n in names + rejects] + [doc, b"", b"\xFF\xD8", doc[:dht + 40]]
    info = L.jpeg_info(streams)
    assert info.dtype == np.int32 and info.shape == (len(streams), 8)
    for n, row in zip(names, info):
        pil = kat["pil_" + n]
        assert row[:3].tolist() == [pil.shape[1], pil.shape[0], 3 if pil.ndim == 3 else 1] and row[5] == 0, n
        assert row.tolist() == D.probe(kat["stream_" + n].tobytes()).row(), n
    layouts = {n: int(row[3]) for n, row in zip(names, info)}
    assert layouts["c444_17x33"] == 1 and layouts["c422_9x7"] == 2 and layouts["c420_9x7"] == 0 and layouts["g_9x7"] == 0
    restarts = {n: int(row[4]) for n, row in zip(names, info)}
    assert restarts["c444_203x117_r1"] == 1 and restarts["g_17x33_r3"] == 3 and restarts["c420_203x117_rows"] == 13 and restarts["c420_203x117"] == 0
    k = len(names)
    assert info[k:k + 3, 5].tolist() == [2, 2, 2], "progressive, 4:4:0, CMYK"
    assert info[k, :3].tolist() == [40, 24, 3] and info[k + 2, 2] == 4
    assert info[k + 3].tolist() == [1000, 563, 3, 0, 0, 0, 0, 0]
    assert info[k + 4:, 5].tolist() == [1, 1, 1], "empty, SOI alone, cut inside its DHT"
    assert b"status 1" in L.lib().lr_last_error()
    L.jpeg_info([kat["stream_progressive"].tobytes()])
    assert b"progressive" in L.lib().lr_last_error()
    for s in streams:
        assert D.probe(s).status == L.jpeg_info([s])[0, 5]


def call(L, region, table, word=None, dst_bytes=0, info=None):
    """the routed call in probe mode, ctx == NULL; returns (rc, info)"""
    region = np.frombuffer(region, np.uint8)
    table = np.ascontiguousarray(table, np.float64)
    info = np.full((len(table), 8), -7, np.int32) if info is None else info
    args = L.JpegDecodeArgs(L._ptr(region), L._ptr(table), L._ptr(info))
    word = (L.PIX_U8X3 | L.WARP_JPEG_DECODE) if word is None else word
    rc = L.lib().lr_warp_perspective_device(None, None, region.nbytes, len(table), 0, 0, 0, word, C.cast(C.byref(args), C.c_void_p),
                                            None, dst_bytes, 0, 0, 0)
    return rc, info


def test_probe_table_errors_and_the_expected_size(L, kat):
    a, b = kat["stream_c420_9x7"].tobytes(), kat["stream_g_9x7"].tobytes()
    region = a + b
    good = np.array([[0, len(a), 0, 27, 9, 7, 0, 0], [len(a), len(b), 400, 32, 9, 7, 0, 0]], np.float64)
    rc, info = call(L, region, good, dst_bytes=1000)
    assert rc == 0 and info[:, 5].tolist() == [0, 0] and info[:, :3].tolist() == [[9, 7, 3], [9, 7, 1]]
    wrong = good.copy()
    wrong[1, 4:6] = (7, 9)
    rc, info = call(L, region, wrong, dst_bytes=1000)
    assert rc == 0 and info[:, 5].tolist() == [0, 3] and info[1, :2].tolist() == [9, 7]
    # stream extents are only read and may overlap
    shared = good.copy()
    shared[1, :2] = good[0, :2]
    rc, info = call(L, region, shared, dst_bytes=1000)
    assert rc == 0 and info[:, 2].tolist() == [3, 3]

    def bad(what, entry, **kw):
        t = good.copy()
        for (r, c), v in kw.pop("cells", {}).items():
            t[r, c] = v
        rc, info = call(L, region, t, dst_bytes=kw.pop("dst_bytes", 1000), **kw)
        assert rc != 0, what
        assert (info == -7).all(), what + ": info is untouched"
        err = L.lib().lr_last_error().decode()
        assert err.startswith("lr_"), what
        if entry is not None:
            assert "frame 1" in err and "[%d]" % entry in err, (what, err)

    bad("overlapping pictures", 2, cells={(1, 2): 100})
    bad("a picture out of its region", 2, dst_bytes=500)
    bad("a stream out of its region", 0, cells={(1, 1): len(b) + 1})
    bad("a non-integer offset", 0, cells={(1, 0): len(a) + 0.5})
    bad("a non-integer stride", 3, cells={(1, 3): 32.5})
    bad("a stride below a row", 3, cells={(1, 3): 26})
    bad("a NaN", 1, cells={(1, 1): float("nan")})
    bad("beyond 2^53", 2, cells={(1, 2): 2.0 ** 54})
    bad("a reserved entry", 6, cells={(1, 6): 1})
    bad("the other reserved entry", 7, cells={(1, 7): -1})
    for extra in (L.WARP_PREPARE, L.WARP_PACKED, L.WARP_RAGGED, L.WARP_LINES, L.WARP_JPEG, 0x400, 0x10000, 1 << 30):
        bad("another option bit", None, word=L.PIX_U8X3 | L.WARP_JPEG_DECODE | extra)
    bad("a format that is none", None, word=L.PIX_F32 | L.WARP_JPEG_DECODE)
    # a non-zero one of the routed call's own sizes
    args = L.JpegDecodeArgs(L._ptr(np.frombuffer(region, np.uint8)), L._ptr(good), L._ptr(np.zeros((2, 8), np.int32)))
    rc = L.lib().lr_warp_perspective_device(None, None, len(region), 2, 8, 0, 0, L.PIX_U8X3 | L.WARP_JPEG_DECODE,
                                            C.cast(C.byref(args), C.c_void_p), None, 1000, 0, 0, 0)
    assert rc != 0


def test_the_option_bit_and_the_python_table(L):
    others = L.WARP_PREPARE | L.WARP_PACKED | L.WARP_RAGGED | L.WARP_LINES | L.WARP_JPEG
    assert L.WARP_JPEG_DECODE == 0x4000 and "lr_decode_jpeg_device" not in L.EXPORTS
    assert L.WARP_JPEG_DECODE & (others | 0x400 | 0x10000 | (1 << 30) | 0xFF) == 0
    t = L.jpeg_decode_table([(0, 100), (100, 50)], [(0, 27), (400, 32)], [(9, 7), (9, 7)])
    assert t.dtype == np.float64 and t.tolist() == [[0, 100, 0, 27, 9, 7, 0, 0], [100, 50, 400, 32, 9, 7, 0, 0]]
    assert L.jpeg_decode_table([(5, 6)]).tolist() == [[5, 6, 0, 0, 0, 0, 0, 0]]
    for kw in (dict(streams=[]), dict(streams=[(0.5, 3)]), dict(streams=[(-1, 3)]), dict(streams=[(0, 2 ** 31)]),
               dict(streams=[(0, 3)], outputs=[(0, 3)]), dict(streams=[(0, 3)], outputs=[(0, 3)], sizes=[(0, 1)]),
               dict(streams=[(0, 3)], outputs=[(0, 3)], sizes=[(1, 65536)])):
        with pytest.raises(ValueError):
            L.jpeg_decode_table(**kw)
    with pytest.raises(ValueError):
        L._all_streams([b"x", np.zeros((2, 2), np.uint8)], "rectify_batch")


def test_damaged_scans_are_status_4_in_the_restatement(doc):
    assert D.decode(doc[:100000])[0] == D.DAMAGED
    rng = np.random.default_rng(3)
    half = D.probe(doc).scan + (len(doc) - D.probe(doc).scan) // 2
    assert D.decode(doc[:half] + rng.integers(0, 256, len(doc) - half, dtype=np.uint8).tobytes())[0] == D.DAMAGED
    s = R.encode(R.synth_u8(128, 96, 3, True), 80, 0)
    at = s.index(b"\xFF\xD1")
    assert D.decode(s)[0] == 0 and D.decode(s[:at + 1] + b"\xD2" + s[at + 2:])[0] == D.DAMAGED, "a misnumbered RSTm"
    assert D.decode(s[:at] + s[at + 2:])[0] == D.DAMAGED, "a missing RSTm"
