"""LR_JPEG_SCALED without a GPU: the restatement (tests/numpy_jpeg_scale_ref.py) by hand, at N = 1 against
numpy_jpeg_sampling_ref, and at N = 2, 4, 8 against the N x N box average of PIL's full-size decodes; the option and entry [6]
through the C ABI in probe mode; the Python keywords.

Measured against PIL 12.2 / libjpeg-turbo over the output pixels whose cells lie wholly inside the picture (X < w // N,
Y < h // N), per first word of a fixture's name the largest (MEASURED, asserted exactly) and the mean difference in levels,
N = 2 / 4 / 8:

    word     largest        mean                      word     largest        mean
    g         1 /  1 / 1    0.02 / 0.02 / 0.05        s14     50 /  4 / 1    3.49 / 0.51 / 0.44
    c444     16 /  7 / 3    0.69 / 0.59 / 0.49        s42     59 /  6 / 2    5.13 / 0.61 / 0.54
    c422     32 / 12 / 4    2.80 / 1.38 / 0.80        s24     55 /  7 / 2    3.78 / 0.56 / 0.38
    c420     47 / 18 / 6    4.09 / 1.95 / 1.06        s21x3   11 /  5 / 2    0.63 / 0.53 / 0.48
    s12      26 /  8 / 3    1.80 / 0.87 / 0.64        s22     43 / 15 / 5    2.64 / 1.41 / 0.81
    s41      54 /  7 / 2    5.23 / 0.53 / 0.55        t440    30 / 10 / 3    2.61 / 1.26 / 0.79
    big440   49 / 17 / 5    7.82 / 2.30 / 0.92        doc     28 / 11 / 5    0.41 / 0.44 / 0.39

One component differs by a level at most: the rule is the box average but for the rounding.  The colour fixtures are small
synthetic pictures of saturated colours with chrominance that changes from sample to sample; there the order of averaging
and the clamped colour rule matters (c444, where nothing else differs: 16), and so does the chrominance that is taken as it is
where PIL's full decode first smooths it (triangle) or replicates it (ratio 4) and the box then averages that.  On the
photograph (doc, 1000 x 563, 4:2:0) the mean is 0.4 levels at every scale."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import numpy_jpeg_orient_ref as X
import numpy_jpeg_sampling_ref as S
import numpy_jpeg_scale_ref as Z

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
G = os.path.join(ROOT, "tests", "golden")
MEASURED = {"g": (1, 1, 1), "c444": (16, 7, 3), "c422": (32, 12, 4), "c420": (47, 18, 6), "s12": (26, 8, 3), "s41": (54, 7, 2),
            "s14": (50, 4, 1), "s42": (59, 6, 2), "s24": (55, 7, 2), "s21x3": (11, 5, 2), "s22": (43, 15, 5), "t440": (30, 10, 3),
            "big440": (49, 17, 5), "doc": (28, 11, 5)}


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(G, "jpeg_sampling_kat.npz"))


@pytest.fixture(scope="module")
def old():
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


def fixtures(old, kat):
    """(name, stream, PIL's recorded decode) of every status-0 fixture of the two files"""
    return [(str(n), k["stream_" + str(n)].tobytes(), k["pil_" + str(n)]) for k in (old, kat) for n in k["names"]]


def test_the_averaging_by_hand():
    block = np.arange(64).reshape(8, 8)
    assert Z.average(block, 1, 1).tolist() == block.tolist()
    # 2 x 1: (0 + 1 + 1) >> 1 = 1, the .5 goes up; 1 x 2: (0 + 8 + 1) >> 1 = 4
    assert Z.average(block, 2, 1)[0].tolist() == [1, 3, 5, 7] and Z.average(block, 2, 1).shape == (8, 4)
    assert Z.average(block, 1, 2)[:, 0].tolist() == [4, 20, 36, 52] and Z.average(block, 1, 2).shape == (4, 8)
    assert Z.average(block, 2, 2)[0].tolist() == [(0 + 1 + 8 + 9 + 2) >> 2, (2 + 3 + 10 + 11 + 2) >> 2, 9, 11]
    assert Z.average(block, 8, 8).tolist() == [[(63 * 64 // 2 + 32) >> 6]] == [[32]]  # 31.5 goes up
    assert Z.average(np.array([[1, 2], [2, 2]]), 2, 2).tolist() == [[2]] and Z.average(np.array([[1, 2], [1, 1]]), 2, 2).tolist() == [[1]]  # 1.75, 1.25
    assert Z.average(np.full((8, 16), 255), 8, 4).tolist() == [[255, 255], [255, 255]]
    # a cell never straddles two blocks: two blocks side by side reduce to their own means
    two = np.concatenate([np.zeros((8, 8), int), np.full((8, 8), 200)], axis=1)
    assert Z.average(two, 8, 8).tolist() == [[0, 200]]
    # how a scale splits between the blocks' reduction and the upsampling that is left
    assert [Z.split(2, r) for r in (1, 2, 4)] == [(2, 1), (1, 1), (1, 2)]
    assert [Z.split(4, r) for r in (1, 2, 4)] == [(4, 1), (2, 1), (1, 1)]
    assert [Z.split(8, r) for r in (1, 2, 4)] == [(8, 1), (4, 1), (2, 1)]
    assert [Z.split(1, r) for r in (1, 2, 4)] == [(1, 1), (1, 2), (1, 4)]


def test_scale_1_is_the_unscaled_decode(old, kat):
    for n, s, pil in fixtures(old, kat):
        for fmt in ("u8", "u8x3"):
            status, want = S.decode(s, fmt)
            got_status, got = Z.decode(s, 1, fmt)
            assert status == got_status == 0 and got.dtype == want.dtype and np.array_equal(got, want), (n, fmt)
        assert Z.probe_row(s, 1) == S.info_row(s)
    assert Z.decode(old["stream_progressive"].tobytes(), 2)[0] == 2


def box(picture, N):
    """the N x N box average of the cells that lie wholly inside the picture"""
    p = np.asarray(picture, np.int64)
    h, w = p.shape[:2]
    p = p[:h // N * N, :w // N * N]
    return (p.reshape((h // N, N, w // N, N) + p.shape[2:]).sum(axis=(1, 3)) + N * N // 2) // (N * N)


def test_restatement_against_pil(old, kat, doc):
    """asserts the recorded maxima exactly: a change of the rule, of the fixtures or of PIL's decodes shows"""
    Image = pytest.importorskip("PIL.Image")
    items = [f for f in fixtures(old, kat) if f[2].shape[0] * f[2].shape[1] >= 67 * 35]
    assert len(items) == 21
    items.append(("doc", doc, np.asarray(Image.open(io.BytesIO(doc)))))
    worst = {}
    for n, s, pil in items:
        h, w = pil.shape[:2]
        fmt = "u8" if pil.ndim == 2 else "u8x3"
        for k, N in enumerate((2, 4, 8)):
            status, ours = Z.decode(s, N, fmt)
            assert status == 0 and ours.dtype == np.uint8 and ours.shape == (-(-h // N), -(-w // N)) + pil.shape[2:], (n, N)
            assert ours.shape[0] - h // N <= 1 and ours.shape[1] - w // N <= 1, "at most one row and one column are left out"
            diff = np.abs(ours[:h // N, :w // N].astype(int) - box(pil, N))
            print("%-20s 1/%d: differs by at most %2d, mean %.2f" % (n, N, diff.max(), diff.mean()))
            word = n.split("_")[0]
            worst.setdefault(word, [0, 0, 0])[k] = max(worst.setdefault(word, [0, 0, 0])[k], int(diff.max()))
    assert {w: tuple(v) for w, v in worst.items()} == MEASURED


def call(L, region, table, word, dst_bytes=0):
    """the routed call in probe mode, ctx == NULL; returns (rc, info)"""
    region = np.frombuffer(region, np.uint8)
    table = np.ascontiguousarray(table, np.float64)
    info = np.full((len(table), 8), -7, np.int32)
    args = L.JpegDecodeArgs(L._ptr(region), L._ptr(table), L._ptr(info))
    rc = L.lib().lr_warp_perspective_device(None, None, region.nbytes, len(table), 0, 0, 0, word, C.cast(C.byref(args), C.c_void_p),
                                            None, dst_bytes, 0, 0, 0)
    return rc, info


def test_probe_sizes_through_the_c_abi(L, old, kat):
    names = ["c420_203x117", "c422_9x7", "g_17x33_r3"]
    streams = [old["stream_" + n].tobytes() for n in names] + [kat["stream_s41_67x35"].tobytes()]
    sizes = [(203, 117), (9, 7), (17, 33), (67, 35)]
    for N in (1, 2, 4, 8):
        info = L.jpeg_info(streams, any_sampling=True, scale=N)
        assert info[:, 5].tolist() == [0] * 4
        assert info[:, :2].tolist() == [[-(-w // N), -(-h // N)] for w, h in sizes]
        for s, row in zip(streams, info):
            assert row.tolist() == Z.probe_row(s, N)
    mixed = L.jpeg_info(streams, any_sampling=True, scale=[1, 2, 4, 8])
    assert mixed[:, :2].tolist() == [[203, 117], [5, 4], [5, 9], [9, 5]]
    assert L.jpeg_info(streams[:3], scale=2)[:, :2].tolist() == [[102, 59], [5, 4], [9, 17]], "the two bits are independent"
    assert L.jpeg_info(streams, scale=2)[3, 5] == 2
    assert np.array_equal(L.jpeg_info(streams, any_sampling=True, scale=1), L.jpeg_info(streams, any_sampling=True))
    # with [7] = 1 the reduced size is swapped, after the reduction
    turned = [X.with_exif(streams[0], o) for o in (1, 3, 6, 8)]
    for N in (2, 4, 8):
        info = L.jpeg_info(turned, orient=True, scale=N)
        rw, rh = -(-203 // N), -(-117 // N)
        assert info[:, :2].tolist() == [[rw, rh], [rw, rh], [rh, rw], [rh, rw]] and info[:, 7].tolist() == [1, 3, 6, 8]
        for s, row in zip(turned, info):
            assert row.tolist() == Z.probe_row(s, N, orient=True)
        assert L.jpeg_info(turned, scale=N)[:, [0, 1, 7]].tolist() == [[rw, rh, 0]] * 4
    # the header's helper
    with open(os.path.join(ROOT, "include", "librectify_amd.h")) as f:
        header = f.read()
    assert "static inline int lr_jpeg_scaled_size(int n, int N)" in header and "LR_JPEG_SCALED = 0x80000" in header


def test_status_3_and_the_table_errors(L, old):
    a, b = old["stream_c420_203x117"].tobytes(), old["stream_g_9x7"].tobytes()
    region = a + b
    word = L.PIX_U8X3 | L.WARP_JPEG_DECODE | L.JPEG_SCALED
    good = np.array([[0, len(a), 0, 102 * 3, 102, 59, 2, 0], [len(a), len(b), 100000, 3 * 3, 3, 2, 4, 0]], np.float64)
    rc, info = call(L, region, good, word, dst_bytes=300000)
    assert rc == 0 and info[:, 5].tolist() == [0, 0] and info[:, :2].tolist() == [[102, 59], [3, 2]]
    # the full size where the reduced one is due: status 3, and its message speaks of the reduced size
    wrong = good.copy()
    wrong[0, 3:6] = (203 * 3, 203, 117)
    rc, info = call(L, region, wrong, word, dst_bytes=300000)
    assert rc == 0 and info[:, 5].tolist() == [3, 0] and info[0, :2].tolist() == [102, 59]
    assert b"102 x 59" in L.lib().lr_last_error() and b"status 3" in L.lib().lr_last_error()
    full = good.copy()
    full[0, 3:7] = (203 * 3, 203, 117, 1)
    assert call(L, region, full, word, dst_bytes=300000)[1][:, 5].tolist() == [0, 0]
    full[0, 6] = 0  # (0 is 1)
    assert call(L, region, full, word, dst_bytes=300000)[1][:, :2].tolist() == [[203, 117], [3, 2]]
    # the stride is held against the reduced row
    narrow = good.copy()
    narrow[1, 3] = 3 * 3 - 1
    rc, info = call(L, region, narrow, word, dst_bytes=300000)
    assert rc != 0 and (info == -7).all() and b"[3]" in L.lib().lr_last_error()
    for value in (3, 16, -2, 2.5, float("nan")):
        t = good.copy()
        t[1, 6] = value
        rc, info = call(L, region, t, word, dst_bytes=300000)
        err = L.lib().lr_last_error().decode()
        assert rc != 0 and (info == -7).all(), value
        assert "frame 1" in err and "[6]" in err and "reserved" not in err, (value, err)
    # without the bit a non-zero [6] is the error it always was
    rc, info = call(L, region, good, L.PIX_U8X3 | L.WARP_JPEG_DECODE, dst_bytes=300000)
    err = L.lib().lr_last_error().decode()
    assert rc != 0 and (info == -7).all() and "frame 0" in err and "[6]" in err and "reserved" in err
    # the bit beside another option, and on calls that are no decoder call (no context is needed to be refused)
    for extra in (L.WARP_RAGGED, L.WARP_JPEG, L.WARP_LINES, L.WARP_CUBIC, L.WARP_BORDER, 0x400, 0x10000, 1 << 30):
        rc, info = call(L, region, good, word | extra, dst_bytes=300000)
        assert rc != 0 and (info == -7).all(), hex(extra)
    for other in (L.PIX_U8X3 | L.JPEG_SCALED, L.PIX_U8X3 | L.WARP_JPEG | L.JPEG_SCALED, L.PIX_U8X3 | L.WARP_RAGGED | L.JPEG_SCALED):
        rc, info = call(L, region, good, other, dst_bytes=300000)
        assert rc != 0 and (info == -7).all(), hex(other)


def test_the_option_bit(L):
    others = (L.WARP_PREPARE | L.WARP_PACKED | L.WARP_RAGGED | L.WARP_LINES | L.WARP_JPEG | L.WARP_JPEG_DECODE | L.WARP_CUBIC | L.WARP_BORDER |
              L.JPEG_ANY_SAMPLING | L.JPEG_OPTIMIZE)
    assert L.JPEG_SCALED == 0x80000 == Z.SCALED and L.WARP_BORDER == 0x40000
    assert L.JPEG_SCALED & (0x400 | 0x10000 | (1 << 30) | 0xFF | others) == 0
    with open(os.path.join(ROOT, "include", "librectify_amd.h")) as f:
        header = f.read()
    for name in ("LR_WARP_PREPARE", "LR_WARP_PACKED", "LR_WARP_RAGGED", "LR_WARP_LINES", "LR_WARP_JPEG", "LR_WARP_JPEG_DECODE", "LR_WARP_CUBIC",
                 "LR_WARP_BORDER", "LR_JPEG_ANY_SAMPLING"):
        value = int(header.split(name + " = ")[1].split(" ")[0].rstrip(",;"), 16)
        assert value & 0x80000 == 0, name
    assert not any("scale" in e.lower() for e in L.EXPORTS), "the bit adds no exported symbol (test_abi holds the library to the list)"


def test_the_python_table(L):
    streams, outputs, sizes = [(0, 10), (10, 20), (30, 5)], [(0, 32), (400, 32), (800, 32)], [(9, 7)] * 3
    plain = L.jpeg_decode_table(streams, outputs, sizes)
    assert L.jpeg_decode_table(streams, outputs, sizes, scale=None).tolist() == plain.tolist() and plain[:, 6].tolist() == [0, 0, 0]
    for scale, column in ((2, [2, 2, 2]), (1, [1, 1, 1]), ([1, 4, 8], [1, 4, 8]), (np.array([8, 8, 2]), [8, 8, 2])):
        t = L.jpeg_decode_table(streams, outputs, sizes, scale=scale)
        assert t.dtype == np.float64 and t[:, 6].tolist() == column
        assert np.delete(t, 6, axis=1).tolist() == np.delete(plain, 6, axis=1).tolist()
    assert L.jpeg_decode_table(streams, orient=[True, False, True], scale=4)[:, 6:].tolist() == [[4, 1], [4, 0], [4, 1]]
    for wrong in (0, 3, 16, -2, 2.5, [2, 2], [1, 2, 3], "2", True):
        with pytest.raises(ValueError, match="scale"):
            L.jpeg_decode_table(streams, outputs, sizes, scale=wrong)


def test_decode_max_size_picks_the_scale(L):
    assert L.jpeg_scale_for([(4000, 3000), (3000, 4000)], 2000) == [2, 2]
    assert L.jpeg_scale_for([(4000, 3000)], 2001) == [1]
    assert L.jpeg_scale_for([(4000, 3000)], 100) == [8]
    assert L.jpeg_scale_for([(4000, 3000), (4001, 10), (1999, 1999), (1998, 1998), (800, 600), (15, 16)], 1000) == [4, 4, 2, 1, 1, 1]
    assert L.jpeg_scale_for([(16, 16)], 2) == [8] and L.jpeg_scale_for([(15, 15)], 2) == [8] and L.jpeg_scale_for([(8, 7)], 2) == [4]
    with pytest.raises(ValueError, match="decode_max_size"):
        L.jpeg_scale_for([(4000, 3000)], 0)


def test_the_keywords_go_with_files(L):
    arrays = [np.zeros((16, 16, 3), np.uint8)]
    assert L._all_streams([b"x"], "rectify_batch", decode_scale=2) and L._all_streams([b"x"], "rectify_batch", decode_max_size=100)
    ctx = object.__new__(L.Context)  # (the keywords are refused before anything touches a device)
    for kw in ({"decode_scale": 2}, {"decode_max_size": 100}):
        for what in (lambda: ctx.rectify(arrays[0], **kw), lambda: ctx.rectify_batch(arrays, **kw), lambda: ctx.rectify_batch(np.stack(arrays), **kw),
                     lambda: ctx.draw_lines_batch(arrays, [np.zeros(0, L.LINE_DTYPE)], **kw)):
            with pytest.raises(ValueError, match="decode_scale"):
                what()
    both = {"decode_scale": 2, "decode_max_size": 100}
    for what in (lambda: ctx.rectify(b"x", **both), lambda: ctx.rectify_batch([b"x"], **both), lambda: ctx.draw_lines_batch([b"x"], [np.zeros(0, L.LINE_DTYPE)], **both)):
        with pytest.raises(ValueError, match="decode_scale and decode_max_size"):
            what()
