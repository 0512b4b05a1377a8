"""LR_JPEG_ANY_SAMPLING on the GPU: lr_decode_jpeg_device with the bit (kernels_jpeg_decode.hip, the kAny instantiations)
against tests/numpy_jpeg_sampling_ref.py, byte for byte.  Every file of tests/golden/jpeg_sampling_kat.npz into both output
formats; one mixed batch of new samplings, the three layouts that need no bit, a one-component file, a progressive file and a
4:1:1 file cut inside its scan, at places of its own with guard bytes, with the bit and without it; the files that need no
bit with it; EXIF orientations of both shapes of the output pass on 4:4:0 and 4:1:1; the pipeline on files."""
import os
import subprocess
import sys

import numpy as np
import pytest

import numpy_jpeg_orient_ref as X
import numpy_jpeg_sampling_ref as S

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
G = os.path.join(ROOT, "tests", "golden")
GUARD = 0xAB


@pytest.fixture(scope="module")
def L():
    import librectify_amd as L
    from librectify_amd import build

    build.build(verbose=False)
    L.lib()
    return L


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    c.set_seed(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(G, "jpeg_sampling_kat.npz"))


@pytest.fixture(scope="module")
def old():
    return np.load(os.path.join(G, "jpeg_decode_kat.npz"))


_wanted = {}


def wanted(stream, fmt):
    """the restatement's decode (as stored), computed once per (stream, format) and never changed"""
    key = (stream, fmt)
    if key not in _wanted:
        status, img = S.decode(stream, fmt)
        assert status == 0
        img.setflags(write=False)
        _wanted[key] = img
    return _wanted[key]


def same(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d values differ, the first at %s" % (what, len(bad), bad[0].tolist()))


def batch_call(L, ctx, streams, fmt, sizes, order, bit=True, orient=False, pad=7, gap=13):
    """tests/test_gpu_jpeg_orient.py's: the streams one behind the other (odd gaps), the pictures in `order`, each allocated
    for sizes[b], rows padded by `pad` bytes and `gap` guard bytes between them.  Returns (info, the destination region, per
    stream its (offset, row bytes, w, h))."""
    bpp = 3 if fmt == L.PIX_U8X3 else 1
    offs, end = [], 3
    for s in streams:
        offs.append(end)
        end += len(s) + 5
    region = np.full(end, 0x11, np.uint8)
    for s, o in zip(streams, offs):
        region[o:o + len(s)] = np.frombuffer(s, np.uint8)
    places, at = {}, gap
    for b in order:
        w, h = sizes[b]
        places[b] = (at, w * bpp + pad, w, h)
        at += h * (w * bpp + pad) + gap
    table = L.jpeg_decode_table([(o, len(s)) for s, o in zip(streams, offs)], [places[b][:2] for b in range(len(streams))],
                                [places[b][2:] for b in range(len(streams))], orient=orient)
    d_src, d_dst = ctx.device_upload(region), ctx.device_upload(np.full(at, GUARD, np.uint8))
    try:
        info = ctx.decode_jpeg_device(d_src, region, fmt | (L.JPEG_ANY_SAMPLING if bit else 0), table, d_dst, at)
        return info, ctx.device_download(d_dst, (at,), np.uint8), places
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)


def pictures_and_guards(dst, places, bpp):
    """(per stream its picture, a mask of the bytes that belong to no picture)"""
    free = np.ones(len(dst), bool)
    out = {}
    for b, (off, row, w, h) in places.items():
        rows = np.lib.stride_tricks.as_strided(dst[off:], (h, w * bpp), (row, 1))
        out[b] = np.ascontiguousarray(rows).reshape((h, w) + ((3,) if bpp == 3 else ()))
        for y in range(h):
            free[off + y * row: off + y * row + w * bpp] = False
    return out, free


def test_every_fixture(L, ctx, kat):
    """all files in one call per format, each at a place of its own"""
    names = [str(n) for n in kat["names"]]
    streams = [kat["stream_" + n].tobytes() for n in names]
    sizes = [kat["pil_" + n].shape[1::-1] for n in names]
    for fmt, name, bpp in ((L.PIX_U8X3, "u8x3", 3), (L.PIX_U8, "u8", 1)):
        info, dst, places = batch_call(L, ctx, streams, fmt, sizes, order=list(range(len(names)))[::-1])
        assert info[:, 5].tolist() == [0] * len(names)
        got, free = pictures_and_guards(dst, places, bpp)
        assert (dst[free] == GUARD).all(), "a byte outside the pictures was written"
        for b, n in enumerate(names):
            assert info[b, :5].tolist() == S.info_row(streams[b])[:5] and info[b, 7] == 0, n
            same(got[b], wanted(streams[b], name), "%s %s" % (name, n))
    assert info[names.index("big440"), 6] >= 1 and len(streams[names.index("big440")]) > 2 * 256 * 128


def mixed(kat, old):
    """(streams, sizes, expected statuses with the bit, the indices of the frames that need the bit)"""
    new = ["s12_67x35", "s41_67x35_r1", "s14_9x7", "s42_67x35", "s24_67x35", "s21x3_67x35", "s22_11_21_67x35", "t440_35x67", "s12_67x35_rows"]
    legacy = ["c420_17x33_r1_opt", "c444_17x33", "c422_9x7", "g_17x33_r3"]
    streams = [kat["stream_" + n].tobytes() for n in new] + [old["stream_" + n].tobytes() for n in legacy]
    sizes = [kat["pil_" + n].shape[1::-1] for n in new] + [old["pil_" + n].shape[1::-1] for n in legacy]
    status = [0] * len(streams)
    streams.append(old["stream_progressive"].tobytes())
    sizes.append((40, 24))
    status.append(2)
    whole = kat["stream_s41_67x35"].tobytes()
    scan = S.probe(whole).scan
    streams.append(whole[:scan + (len(whole) - scan) // 2])  # cut in the middle of its scan
    sizes.append((67, 35))
    status.append(4)
    return streams, sizes, status, list(range(len(new))) + [len(streams) - 1]


ORDER = [5, 14, 2, 9, 0, 13, 7, 11, 3, 12, 1, 10, 6, 4, 8]


@pytest.mark.parametrize("fmt", ["u8x3", "u8"])
def test_mixed_batch_with_the_bit(L, ctx, kat, old, fmt):
    streams, sizes, status, _ = mixed(kat, old)
    assert sorted(ORDER) == list(range(len(streams)))
    bpp = 3 if fmt == "u8x3" else 1
    info, dst, places = batch_call(L, ctx, streams, L.PIX_U8X3 if bpp == 3 else L.PIX_U8, sizes, ORDER)
    assert info[:, 5].tolist() == status == [S.probe(s).status or S.coefficients(S.probe(s), s)[0] for s in streams]
    got, free = pictures_and_guards(dst, places, bpp)
    assert (dst[free] == GUARD).all(), "a byte outside the pictures was written"
    for b, st in enumerate(status):
        if st == 0:
            assert info[b, :5].tolist() == S.info_row(streams[b])[:5]
            same(got[b], wanted(streams[b], fmt), "%s frame %d" % (fmt, b))
        elif st == 2:
            assert (got[b] == GUARD).all(), "the skipped frame's extent is untouched"


@pytest.mark.parametrize("fmt", ["u8x3", "u8"])
def test_mixed_batch_without_the_bit(L, ctx, kat, old, fmt):
    """the new samplings are refused as before and their extents untouched; every other frame is, byte for byte, what the
    call with the bit makes of it"""
    streams, sizes, status, need = mixed(kat, old)
    bpp = 3 if fmt == "u8x3" else 1
    word = L.PIX_U8X3 if bpp == 3 else L.PIX_U8
    info, dst, places = batch_call(L, ctx, streams, word, sizes, ORDER, bit=False)
    assert info[:, 5].tolist() == [2 if b in need else st for b, st in enumerate(status)]
    with_bit, dst_bit, _ = batch_call(L, ctx, streams, word, sizes, ORDER, bit=True)
    assert with_bit[:, 5].tolist() == status
    got, free = pictures_and_guards(dst, places, bpp)
    got_bit, _ = pictures_and_guards(dst_bit, places, bpp)
    assert (dst[free] == GUARD).all(), "a byte outside the pictures was written"
    for b, st in enumerate(status):
        if b in need or st != 0:
            assert (got[b] == GUARD).all(), "frame %d: the extent of a skipped frame is untouched" % b
        else:
            assert info[b].tolist() == with_bit[b].tolist()
            same(got[b], got_bit[b], "frame %d" % b)
            same(got[b], wanted(streams[b], fmt), "frame %d against the restatement" % b)


def test_files_that_need_no_bit_with_it(L, ctx, old):
    names = [str(n) for n in old["names"]]
    streams = [old["stream_" + n].tobytes() for n in names]
    sizes = [old["pil_" + n].shape[1::-1] for n in names]
    for fmt in (L.PIX_U8X3, L.PIX_U8):
        a, dst_a, _ = batch_call(L, ctx, streams, fmt, sizes, list(range(len(names))), bit=True)
        b, dst_b, _ = batch_call(L, ctx, streams, fmt, sizes, list(range(len(names))), bit=False)
        assert a[:, 5].tolist() == [0] * len(names) and np.array_equal(a, b) and np.array_equal(dst_a, dst_b)


@pytest.mark.parametrize("o", [3, 6])
@pytest.mark.parametrize("name", ["s12_67x35", "s41_67x35"])
def test_orientation(L, ctx, kat, name, o):
    """2..4 keep the thread-per-pixel shape of the output pass, 5..8 take the transposing squares"""
    plain = kat["stream_" + name].tobytes()
    stream = X.with_exif(plain, o)
    size = (67, 35) if o < 5 else (35, 67)
    for fmt, word, bpp in (("u8x3", L.PIX_U8X3, 3), ("u8", L.PIX_U8, 1)):
        info, dst, places = batch_call(L, ctx, [stream], word, [size], [0], orient=True)
        assert info[0, 5] == 0 and info[0, 7] == o and info[0, :4].tolist() == list(size) + [3, plain[S.sof_sampling(plain)]]
        got, free = pictures_and_guards(dst, places, bpp)
        assert (dst[free] == GUARD).all()
        status, want = S.decode(stream, fmt, orient=True)
        assert status == 0
        same(got[0], want, "%s orientation %d" % (fmt, o))
        same(want, X.orient(wanted(plain, fmt), o), "the restatement's own orientation")


def detector_frame(w, h, seed):
    from librectify_amd import synth

    g = np.clip(synth.frame(w, h, seed, bars=40) * 255.0, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([g, (g.astype(np.int32) * 3 // 4).astype(np.uint8), 255 - g], axis=-1))


_file_440 = []


def detector_file_440():
    """a 4:4:0 file of a picture with lines in it, from the fixtures' writer; written once"""
    if not _file_440:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import make_jpeg_sampling_fixtures as F

        _file_440.append(F.encode(detector_frame(320, 240, 5), F.SAMPLINGS["s12"], 92))
    return _file_440[0]


def test_rectify_batch_on_files_of_any_sampling(L, ctx):
    frame = detector_frame(320, 240, 5)
    file_440 = detector_file_440()
    file_420 = ctx.encode_jpeg(frame, 92, 0)
    assert L.jpeg_info([file_440, file_420], any_sampling=True)[:, 3].tolist() == [0x12, 0]
    decoded = ctx.decode_jpeg(file_440, any_sampling=True)
    same(decoded, wanted(file_440, "u8x3"), "decode_jpeg")
    got = ctx.rectify_batch([file_440, file_420], any_sampling=True)
    ref = [ctx.rectify(decoded), ctx.rectify(ctx.decode_jpeg(file_420, any_sampling=True))]
    assert len(got[0][0]) > 10 and got[0][2] is not None
    for b, (g, r) in enumerate(zip(got, ref)):
        assert g[0].tobytes() == r[0].tobytes() and bytes(g[1]) == bytes(r[1]) and np.array_equal(g[2], r[2]), "frame %d" % b
    one = ctx.rectify(file_440, any_sampling=True)
    assert one[0].tobytes() == ref[0][0].tobytes() and np.array_equal(one[2], ref[0][2])
    with pytest.raises(L.LibrectifyError, match="frame 0"):
        ctx.rectify_batch([file_440, file_420])
    with pytest.raises(L.LibrectifyError, match="frame 1"):
        ctx.decode_jpeg_batch([file_420, file_440])


def test_recipe_any_sampling(L, ctx, tmp_path):
    lib_dir = os.path.join(ROOT, "librectify_amd")
    exe = str(tmp_path / "rectify_recipe")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "rectify_recipe.cpp"),
                           "-I", os.path.join(ROOT, "include"), "-L", lib_dir, "-l:librectify_amd.so",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    path, prefix = str(tmp_path / "rotated.jpg"), str(tmp_path / "out")
    with open(path, "wb") as f:
        f.write(detector_file_440())
    r = subprocess.run([exe, path, prefix, "--jpeg-in", "--any-sampling"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines, _, _ = ctx.rectify(detector_file_440(), max_size=1200, any_sampling=True)
    rows = ["%g,%g,%g,%g,%g,%g,%d" % (l["x1"], l["y1"], l["x2"], l["y2"], l["weight"], l["err"], l["group_id"]) for l in lines]
    with open(prefix + "_lines.csv") as f:
        assert f.read().splitlines() == rows and len(rows) > 10
    r = subprocess.run([exe, path, prefix, "--jpeg-in"], capture_output=True, text=True)
    assert r.returncode != 0 and "sampling other than" in r.stderr
    r = subprocess.run([exe, path, prefix, "--any-sampling"], capture_output=True, text=True)
    assert r.returncode != 0 and "--any-sampling" in r.stderr
