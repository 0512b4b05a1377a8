"""The EXIF orientation of the JPEG decoder without a GPU: the restatement
(tests/numpy_jpeg_orient_ref.py) against PIL's ImageOps.exif_transpose as a second source, and the library's reading of
the tag through the C ABI in probe mode (lr_jpeg_info: no context, no device) -- entry [7] of the table, the upright
size and the orientation in info, the expected size, and tags that are malformed or oddly placed."""
import ctypes as C
import io

import numpy as np
import pytest

import numpy_jpeg_decode_ref as D
import numpy_jpeg_orient_ref as X
import numpy_jpeg_ref as R

W, H = 47, 70


@pytest.fixture(scope="module")
def L():
    import librectify_amd as L
    from librectify_amd import build

    build.build(verbose=False)
    L.lib()
    return L


def picture(w=W, h=H, colour=True):
    """asymmetric under every one of the eight orientations: a ramp that differs along x and y, a bright corner block and
    a mild texture"""
    rng = np.random.default_rng(112)
    y, x = np.mgrid[0:h, 0:w]
    g = 40 + 2 * x + y + rng.integers(-6, 7, (h, w))
    g[:h // 4, :w // 3] += 60
    g = np.clip(g, 0, 255)
    if not colour:
        return g.astype(np.uint8)
    return np.clip(np.stack([g, 255 - g // 2 - x, 30 + 3 * y - x // 2], axis=-1), 0, 255).astype(np.uint8)


def call(L, region, table, dst_bytes=0):
    """the routed call in probe mode, ctx == NULL; returns (rc, info), info filled with -7 beforehand"""
    region = np.frombuffer(region, np.uint8)
    table = np.ascontiguousarray(table, np.float64)
    info = np.full((len(table), 8), -7, np.int32)
    args = L.JpegDecodeArgs(L._ptr(region), L._ptr(table), L._ptr(info))
    rc = L.lib().lr_warp_perspective_device(None, None, region.nbytes, len(table), 0, 0, 0, L.PIX_U8X3 | L.WARP_JPEG_DECODE,
                                            C.cast(C.byref(args), C.c_void_p), None, dst_bytes, 0, 0, 0)
    return rc, info


def test_the_table_is_pil_s_exif_transpose():
    """The second source.  Files PIL saves with exif[0x0112] = o (it writes MM), and the same scans behind a hand-built II
    segment: the restatement reads o, and its decode, turned by the table, is PIL's exif_transpose of the file within
    what the restatement is held to against PIL's decode: 1 level for one component, 3 for colour.  A wrong row of the
    table misses by tens of levels on this picture, which the test shows first."""
    from PIL import Image, ImageOps

    for colour, fmt, bound in ((True, "u8x3", 3), (False, "u8", 1)):
        img = picture(colour=colour)
        turned = [X.orient(img, o) for o in range(1, 9)]
        for a in range(8):
            for b in range(a + 1, 8):
                if turned[a].shape == turned[b].shape:
                    assert np.abs(turned[a].astype(int) - turned[b].astype(int)).max() >= 30, "orientations %d and %d look alike" % (a + 1, b + 1)
        for o in range(1, 9):
            exif = Image.Exif()
            exif[0x0112] = o
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, "JPEG", quality=90, exif=exif)
            mm = buf.getvalue()
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, "JPEG", quality=90)
            ii = X.with_exif(buf.getvalue(), o, "II")
            assert b"Exif\0\0MM" in mm and b"Exif\0\0II" in ii
            for name, data in (("MM", mm), ("II", ii)):
                assert X.exif_orientation(data) == o, name
                pil = np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(data))))
                status, ours = X.decode(data, fmt)
                assert status == 0 and ours.shape == pil.shape == turned[o - 1].shape, (name, o)
                diff = int(np.abs(ours.astype(int) - pil.astype(int)).max())
                print("%s %s orientation %d: differs from PIL by at most %d" % (fmt, name, o, diff))
                assert diff <= bound, (name, o)
                assert np.array_equal(ours, X.orient(D.decode(data, fmt)[1], o))


@pytest.fixture(scope="module")
def plain():
    return R.encode(picture(), 85, 0)


def test_probe_with_entry_7(L, plain):
    files = [plain] + [X.with_exif(plain, o, "II" if o & 1 else "MM") for o in range(1, 9)]
    region, extents = L._stream_region(files)
    # [7] = 0: the rows are what they were, the last column 0
    rc, info = call(L, region, L.jpeg_decode_table(extents))
    assert rc == 0 and info.tolist() == [[W, H, 3, 0, D.probe(plain).restart, 0, 0, 0]] * 9
    assert info.tolist() == [X.info_row(f, False) for f in files]
    # [7] = 1: the upright size, the orientation; 1 for the file without Exif
    table = L.jpeg_decode_table(extents, orient=True)
    assert table[:, 7].tolist() == [1.0] * 9 and table[:, 6].tolist() == [0.0] * 9
    rc, info = call(L, region, table)
    assert rc == 0 and info.tolist() == [X.info_row(f, True) for f in files]
    assert info[:, 7].tolist() == [1, 1, 2, 3, 4, 5, 6, 7, 8] and (info[:, 5] == 0).all()
    assert info[:5, :2].tolist() == [[W, H]] * 5 and info[5:, :2].tolist() == [[H, W]] * 4
    assert L.jpeg_info(files, orient=True).tolist() == info.tolist() and L.jpeg_info(files)[:, 7].tolist() == [0] * 9
    # every frame has its own [7]
    mixed = L.jpeg_decode_table(extents, orient=np.arange(9) % 2 == 0)
    rc, info = call(L, region, mixed)
    assert rc == 0 and info.tolist() == [X.info_row(f, b % 2 == 0) for b, f in enumerate(files)]


def test_the_expected_size_is_the_upright_one(L, plain):
    six = X.with_exif(plain, 6)
    stored = np.array([[0, len(six), 0, 3 * W, W, H, 0, 1]], np.float64)
    rc, info = call(L, six, stored, dst_bytes=3 * W * H)
    assert rc == 0 and info[0].tolist() == [H, W, 3, 0, D.probe(plain).restart, 3, 0, 6]
    assert ("the stream is %d x %d" % (H, W)) in L.lib().lr_last_error().decode()
    upright = np.array([[0, len(six), 0, 3 * H, H, W, 0, 1]], np.float64)
    rc, info = call(L, six, upright, dst_bytes=3 * W * H)
    assert rc == 0 and info[0, 5] == 0 and info[0, :2].tolist() == [H, W] and info[0, 7] == 6
    # the stride is held against the upright row: 3 * W bytes are less than a row of H pixels
    short = upright.copy()
    short[0, 3] = 3 * W
    assert W < H and call(L, six, short, dst_bytes=3 * W * H)[0] != 0 and "[3]" in L.lib().lr_last_error().decode()
    # without [7] the same file is the stored one
    stored[0, 7] = 0
    rc, info = call(L, six, stored, dst_bytes=3 * W * H)
    assert rc == 0 and info[0].tolist() == [W, H, 3, 0, D.probe(plain).restart, 0, 0, 0]


@pytest.mark.parametrize("entry, value", [(7, 2), (7, 0.5), (7, -1), (7, float("nan")), (6, 1), (6, 2)])
def test_other_values_of_7_and_any_of_6_fail_the_call(L, plain, entry, value):
    table = np.array([[0, len(plain), 0, 0, 0, 0, 0, 0], [0, len(plain), 0, 0, 0, 0, 0, 1]], np.float64)
    table[1, entry] = value
    rc, info = call(L, plain, table)
    assert rc != 0 and (info == -7).all(), "info is untouched"
    err = L.lib().lr_last_error().decode()
    assert "frame 1" in err and "[%d]" % entry in err


def malformed(plain):
    """(name, file, the orientation it tells): a tag that does not count is no orientation, 1"""
    x = X.exif_payload
    return [
        ("a payload of 5 bytes", X.splice(plain, [X.app1(b"Exif\0")]), 1),
        ("a payload of the six bytes alone", X.splice(plain, [X.app1(X.EXIF)]), 1),
        ("a TIFF block cut inside its offset", X.splice(plain, [X.app1(x(6)[:6 + 7])]), 1),
        ("a bad byte-order mark", X.with_exif(plain, 6, mark=b"MM*\0"), 1),
        ("a mixed byte-order mark", X.with_exif(plain, 6, "II", mark=b"IM*\0"), 1),
        ("an IFD offset beyond the segment", X.with_exif(plain, 6, ifd=4000), 1),
        ("an IFD offset of 2^32 - 1", X.with_exif(plain, 6, "II", ifd=2 ** 32 - 1), 1),
        ("an IFD offset at the last byte", X.splice(plain, [X.app1(x(6, ifd=len(x(6)) - 6 - 1))]), 1),
        ("an entry count that runs past the segment", X.with_exif(plain, 6, count=5), 1),
        ("an entry count of 65535", X.with_exif(plain, 6, "II", count=65535), 1),
        ("a segment cut inside the orientation's entry", X.splice(plain, [X.app1(x(6)[:6 + 8 + 2 + 24 + 9])]), 1),
        ("type 4", X.with_exif(plain, 6, typ=4), 1),
        ("count 2", X.with_exif(plain, 6, "II", n=2), 1),
        ("the value 0", X.with_exif(plain, 0), 1),
        ("the value 9", X.with_exif(plain, 9, "II"), 1),
        ("the value 65535", X.with_exif(plain, 65535), 1),
        ("the value in the other byte order", X.with_exif(plain, 6 << 8, "II"), 1),
        ("no orientation among the entries", X.splice(plain, [X.app1(x(6).replace(b"\x01\x12", b"\x01\x13"))]), 1),
        ("an XMP APP1 in front of the Exif one", X.splice(plain, [X.app1(X.XMP), X.app1(x(7, "II"))]), 7),
        ("two Exif segments: the first wins", X.splice(plain, [X.app1(x(8)), X.app1(x(3))]), 8),
        ("two Exif segments, the first with a bad value: none", X.splice(plain, [X.app1(x(9)), X.app1(x(3))]), 1),
        # (everything before SOS is walked, so the segment counts wherever it lies there)
        ("an Exif APP1 behind SOF", X.splice(plain, [X.app1(x(5))], at=X.after_sof(plain)), 5),
        ("the orientation as the IFD's only entry", X.with_exif(plain, 4, "II", before=0, after=0), 4),
    ]


def test_malformed_and_oddly_placed_tags(L, plain):
    """none of them fails the frame or the call; the library reads what the restatement reads"""
    cases = malformed(plain)
    for name, data, o in cases:
        assert X.exif_orientation(data) == (0 if o == 1 else o), name
        assert D.probe(data).status == 0, name
    region, extents = L._stream_region([c[1] for c in cases])
    rc, info = call(L, region, L.jpeg_decode_table(extents, orient=True))
    assert rc == 0
    for row, (name, data, o) in zip(info.tolist(), cases):
        size = [H, W] if o >= 5 else [W, H]
        assert row == size + [3, 0, D.probe(plain).restart, 0, 0, o], name
    # and one by one, each segment the last bytes the parser may read before the next marker
    for name, data, o in cases:
        assert L.jpeg_info([data], orient=True)[0, 5:].tolist() == [0, 0, o], name


def test_the_python_table(L):
    t = L.jpeg_decode_table([(0, 100), (100, 50)], [(0, 27), (400, 32)], [(9, 7), (9, 7)], orient=True)
    assert t.dtype == np.float64 and t.tolist() == [[0, 100, 0, 27, 9, 7, 0, 1], [100, 50, 400, 32, 9, 7, 0, 1]]
    assert L.jpeg_decode_table([(5, 6), (11, 6)], orient=[False, True]).tolist() == [[5, 6, 0, 0, 0, 0, 0, 0], [11, 6, 0, 0, 0, 0, 0, 1]]
    assert L.jpeg_decode_table([(5, 6)], orient=False).tolist() == L.jpeg_decode_table([(5, 6)]).tolist() == [[5, 6, 0, 0, 0, 0, 0, 0]]
    for bad in (1, 2, [True], "yes", None):
        with pytest.raises(ValueError):
            L.jpeg_decode_table([(5, 6), (11, 6)], orient=bad)
    for what in ("rectify_batch", "draw_lines_batch"):
        with pytest.raises(ValueError, match="orient"):
            L._all_streams([np.zeros((2, 2), np.uint8)], what, True)
        assert L._all_streams([b"x"], what, True)
