"""LR_JPEG_OPTIMIZE without a GPU: tests/numpy_jpeg_optimize_ref.py (the second source the GPU is compared with, byte for
byte) against PIL's decoder and PIL's own optimize=True, the validity of every code it makes, the K.3 limiter on crafted and
on real statistics, the streams' sizes, and jpeg_table / jpeg_bound with optimize=.

Sizes recorded when the test was written, the doc image as RGB, 1000 x 563, quality 95, 4:2:0: the reference's standard
stream 217 322 bytes, its optimised stream 183 523, PIL's optimize=True file 183 934: 411 bytes shorter than PIL's although
the stream carries 141 restart markers and their padding that PIL's has not.  The bound asserted is PIL's size + 3 bytes per
restart interval (the marker and up to a byte of padding, test_jpeg_cpu's allowance): the codes are IJG's, so nothing else
may cost a byte."""
import io
import os

import numpy as np
import pytest

import numpy_jpeg_optimize_ref as O
import numpy_jpeg_ref as R

Image = pytest.importorskip("PIL.Image")

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 1), (8, 8), (9, 7), (17, 33), (47, 33), (203, 117)]
KINDS = ["u8", "420", "444"]
QUALITIES = [1, 50, 95, 100]


def layout_of(kind):
    return 1 if kind == "444" else 0


@pytest.fixture(scope="module")
def doc():
    return np.asarray(Image.open(os.path.join(HERE, "golden", "doc_image.jpg")).convert("RGB"))


def picture(doc, w, h, kind):
    """a w x h piece of the doc image where it has text and an edge (gray: its green channel)"""
    crop = np.ascontiguousarray(doc[150:150 + h, 300:300 + w])
    assert crop.shape[:2] == (h, w)
    return crop if kind != "u8" else np.ascontiguousarray(crop[..., 1])


def decoded(stream):
    return np.asarray(Image.open(io.BytesIO(stream)))


_cache = {}


def both(img, quality, layout, key):
    """(standard stream, optimised stream, tables) of a frame, made once"""
    if key not in _cache:
        coefs, comp_of = R.coefficients(img, quality, layout)
        h, w = img.shape[:2]
        counts, tables = O.tables_of(coefs, comp_of, w, layout)
        _cache[key] = (R.encode_coefficients(coefs, comp_of, w, h, quality, layout),
                       O.encode_coefficients(coefs, comp_of, w, h, quality, layout), counts, tables)
    return _cache[key]


def check_table(counts, bits, vals):
    lengths = [length for length, n in enumerate(bits, 1) for _ in range(n)]
    assert len(bits) == 16 and all(1 <= l <= 16 for l in lengths)
    assert sum(bits) == len(vals) == len(lengths)
    assert sorted(vals) == [s for s in range(256) if counts[s]], "HUFFVAL is exactly the symbols that occur"
    kraft = sum(2 ** (16 - l) for l in lengths)
    assert kraft < 2 ** 16, "the all-ones code is unused"
    codes = R.huff_table(bits, vals)
    assert all(code != (1 << l) - 1 for code, l in codes.values()), "no code is all ones"


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_pil_decodes_both_streams_to_the_same_pixels(doc, shape, kind, quality):
    w, h = shape
    img = picture(doc, w, h, kind)
    plain, optimised, counts, tables = both(img, quality, layout_of(kind), (shape, kind, quality))
    a, b = decoded(plain), decoded(optimised)
    assert a.shape == img.shape and (a == b).all()
    assert len(optimised) <= len(plain)
    for t, (dc, ac) in enumerate(tables):
        check_table(counts[t][0], *dc)
        check_table(counts[t][1], *ac)
    # only the DHT payloads and the code bits differ
    cut = lambda s: (s[:s.index(b"\xFF\xC4")], s[s.index(b"\xFF\xDD"):s.index(b"\xFF\xDA") + 2])  # noqa: E731
    assert cut(plain) == cut(optimised)
    assert [s.count(b"\xFF\xC4") for s in (plain, optimised)] == [2 if kind == "u8" else 4] * 2


@pytest.mark.parametrize("kind", KINDS)
def test_flat_frames_and_noise(kind):
    shape = (24, 40) if kind == "u8" else (24, 40, 3)
    flat = np.full(shape, 128, np.uint8)  # every table a single symbol: DC category 0, EOB
    plain, optimised, counts, tables = both(flat, 75, layout_of(kind), ("flat", kind))
    assert (decoded(plain) == decoded(optimised)).all() and len(optimised) < len(plain)
    for t, (dc, ac) in enumerate(tables):
        assert dc == ([1] + [0] * 15, [0]) and ac == ([1] + [0] * 15, [0]), "one symbol: the code 0 of one bit"
        check_table(counts[t][0], *dc)
        check_table(counts[t][1], *ac)
    noise = np.random.default_rng(5).integers(0, 256, shape, dtype=np.uint8)
    plain, optimised, counts, tables = both(noise, 100, layout_of(kind), ("noise", kind))
    assert (decoded(plain) == decoded(optimised)).all() and len(optimised) <= len(plain)
    for t, (dc, ac) in enumerate(tables):
        check_table(counts[t][0], *dc)
        check_table(counts[t][1], *ac)
    comps = 1 if kind == "u8" else 3
    assert len(optimised) <= O.bound(40, 24, comps, layout_of(kind))


def test_statistics_count_what_the_standard_encoder_emits(doc):
    """the standard stream's scan has exactly sum(count * (code length + magnitude bits)) bits, interval padding apart: the
    counted symbols are the emitted ones (dummy blocks, ZRL, EOB and the DC reset at every interval included)"""
    img = picture(doc, 47, 33, "420")  # (dummy luminance blocks at the right and below; one interval)
    for im, layout in ((img, 0), (picture(doc, 203, 117, "420"), 0), (picture(doc, 203, 117, "444"), 1)):
        coefs, comp_of = R.coefficients(im, 95, layout)
        h, w = im.shape[:2]
        counts = O.statistics(coefs, comp_of, w, layout)
        std = [(R.huff_table(R.DC_LUMA_BITS, R.DC_VALS), R.huff_table(R.AC_LUMA_BITS, R.AC_LUMA_VALS)),
               (R.huff_table(R.DC_CHROMA_BITS, R.DC_VALS), R.huff_table(R.AC_CHROMA_BITS, R.AC_CHROMA_VALS))]
        bits = 0
        for t in range(2):
            bits += sum(n * (std[t][0][s][1] + s) for s, n in enumerate(counts[t][0]) if n)
            bits += sum(n * (std[t][1][s][1] + (s & 15)) for s, n in enumerate(counts[t][1]) if n)
        stream = R.encode_coefficients(coefs, comp_of, w, h, 95, layout)
        scan = stream[stream.index(b"\xFF\xDA") + 14:-2].replace(b"\xFF\x00", b"\xFF")
        n_int = R.intervals(w, h, layout, 3)
        assert 0 <= 8 * (len(scan) - 2 * (n_int - 1)) - bits < 8 * n_int
        blocks = coefs.shape[0] * coefs.shape[1]
        assert sum(counts[0][0]) + sum(counts[1][0]) == blocks, "every block a DC symbol"


def fibonacci(n):
    """1, 2, 3, 5, 8 ...: with the pseudo-symbol's 1 in front every merge takes the node of all earlier ones, a tree as deep as
    it has symbols (from 1, 1, 2, 3 ... the pseudo-symbol's 1 would start a second chain and halve the depth)"""
    f = [1, 2]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


@pytest.mark.parametrize("n", [20, 40])
def test_the_limiter_on_fibonacci_counts(n):
    counts = [0] * 256
    for i, c in enumerate(fibonacci(n)):
        counts[7 * i % 256] = c  # (scattered over the symbols)
    size = O.code_sizes(counts)
    assert max(size) >= n > 16 and size[256] == max(size), "as deep as it has symbols; the pseudo-symbol has a longest code"
    assert sum(2.0 ** -s for s in size if s) == 1.0, "a full tree before the limit"
    bits, vals = O.optimal_table(counts)
    check_table(counts, bits, vals)
    assert bits[15] > 0
    codes = R.huff_table(bits, vals)
    by_count = sorted(range(256), key=lambda s: -counts[s])[:n]
    assert all(codes[a][1] <= codes[b][1] for a, b in zip(by_count, by_count[1:]) if counts[a] > counts[b]), "rarer is never shorter"


def test_the_doc_decimation_reaches_17_bits_before_the_limit(doc):
    img = np.ascontiguousarray(doc[::2, ::2])
    assert img.shape == (282, 500, 3)
    plain, optimised, counts, tables = both(img, 95, 0, "doc_half")
    assert max(O.code_sizes(counts[0][1])) == 17, "luminance AC: the GPU test of this frame exercises the limiter"
    assert (len(plain), len(optimised)) == (81689, 78306)
    assert (decoded(plain) == decoded(optimised)).all()
    for t, (dc, ac) in enumerate(tables):
        check_table(counts[t][0], *dc)
        check_table(counts[t][1], *ac)


def test_the_doc_image_against_pil_optimize(doc):
    assert doc.shape == (563, 1000, 3)
    plain, optimised, _, _ = both(doc, 95, 0, "doc")
    buf = io.BytesIO()
    Image.fromarray(doc).save(buf, "JPEG", quality=95, subsampling=2, optimize=True)
    pil = len(buf.getvalue())
    n = R.intervals(1000, 563, 0, 3)
    print("standard %d, optimised %d (%.3f), PIL optimize=True %d, %d intervals" % (len(plain), len(optimised), len(optimised) / len(plain), pil, n))
    assert (len(plain), len(optimised)) == (217322, 183523)
    assert len(optimised) <= len(plain)
    assert len(optimised) <= pil + 3 * n
    assert (decoded(plain) == decoded(optimised)).all()


def test_jpeg_table_and_jpeg_bound():
    import librectify_amd as L

    assert L.JPEG_OPTIMIZE == 0x10
    args = ([(203, 117), (64, 16)], [(5, 610), (80000, 192)], [(9000, 500), (0, 9000)], [95, 10], [0, 1])
    plain = L.jpeg_table(*args)
    np.testing.assert_array_equal(plain, L.jpeg_table(*args, optimize=False))
    np.testing.assert_array_equal(plain[:, 7], [0, 1])
    np.testing.assert_array_equal(L.jpeg_table(*args, optimize=True)[:, 7], [16, 17])
    np.testing.assert_array_equal(L.jpeg_table(*args, optimize=[False, True])[:, 7], [0, 17])
    np.testing.assert_array_equal(L.jpeg_table(*args, optimize=np.array([True, False]))[:, 7], [16, 1])
    np.testing.assert_array_equal(L.jpeg_table(*args, optimize=True)[:, :7], plain[:, :7])
    for bad in (dict(optimize=[True]), dict(optimize=[True, False, True]), dict(optimize=1), dict(optimize=[0, 16]), dict(optimize=None)):
        with pytest.raises(ValueError):
            L.jpeg_table(*args, **bad)
    for layout in (2, 16, 17, [0, 16]):
        with pytest.raises(ValueError):
            L.jpeg_table(*args[:4], layout, optimize=True)
        with pytest.raises(ValueError):
            L.jpeg_table(*args[:4], layout)
    for w, h, fmt, layout in ((1, 1, L.PIX_U8, 0), (17, 9, L.PIX_U8X3, 0), (17, 9, L.PIX_U8X3, 1), (203, 117, L.PIX_U8X3, 0),
                              (65535, 65535, L.PIX_U8X3, 1)):
        comps = 1 if fmt == L.PIX_U8 else 3
        assert L.jpeg_bound(w, h, fmt, layout) == L.jpeg_bound(w, h, fmt, layout, optimize=False) == R.bound(w, h, comps, layout)
        assert L.jpeg_bound(w, h, fmt, layout, optimize=True) == O.bound(w, h, comps, layout) >= L.jpeg_bound(w, h, fmt, layout)
    assert L.jpeg_bound(1, 1, L.PIX_U8, 0, optimize=True) == 640 + 2 + 418 and L.jpeg_bound(17, 9, L.PIX_U8X3, 0, True) == 640 + 2 + 418 * 12
    for bad in ((0, 5, L.PIX_U8, 0), (5, 65536, L.PIX_U8, 0), (5, 5, L.PIX_F32, 0), (5, 5, L.PIX_U8, 1), (5, 5, L.PIX_U8X3, 2),
                (5, 5, L.PIX_U8X3, 16)):
        assert L.jpeg_bound(*bad, optimize=True) == 0 and L.jpeg_bound(*bad) == 0
    # the longest block: 16 + 11 bits of DC, 63 times 16 + 10 of AC; an interval of them, every byte stuffed
    assert 27 + 63 * 26 == 1665 and all(2 * -(-1665 * n // 8) <= 418 * n for n in range(1, 97))


def test_recipe_takes_optimize_with_jpeg_alone(tmp_path):
    import subprocess

    from librectify_amd import build

    build.build(verbose=False)
    root = os.path.dirname(HERE)
    exe, lib_dir = str(tmp_path / "rectify_recipe"), os.path.join(root, "librectify_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(root, "examples", "rectify_recipe.cpp"),
                           "-I", os.path.join(root, "include"), "-L", lib_dir, "-l:librectify_amd.so", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    usage = subprocess.run([exe], text=True, capture_output=True)
    assert usage.returncode == 2 and "--optimize" in usage.stderr
    for extra in ([], ["--warp"], ["--lines"]):  # (refused while the options are read: no file is opened, no device asked for)
        r = subprocess.run([exe, "none.pgm", str(tmp_path / "out"), "--optimize"] + extra, text=True, capture_output=True)
        assert r.returncode == 2 and "--optimize goes with --jpeg Q" in r.stderr
    r = subprocess.run([exe, "none.pgm", str(tmp_path / "out"), "--jpeg", "90", "--optimize"], text=True, capture_output=True)
    assert r.returncode == 1 and "cannot read none.pgm" in r.stderr, "the options are accepted together"
