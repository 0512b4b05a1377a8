"""lr_decode_jpeg_device (kernels_jpeg_decode.hip) on streams that no encoder library wrote: the cases of
tests/jpeg_stream_cases.py, built symbol by symbol by tests/jpeg_stream_writer.py.  The expected picture of a case comes from
the WRITER's coefficients through the second source's back half (component_planes, upsample, rgb); no entropy decoder of ours
stands between a case and its truth.  Pictures are compared byte for byte, with guard bytes around every one.

Every case of status 0 in u8 and u8x3; the refused ones; one call of eight mixed cases in
scrambled order at odd offsets; two cases at LR_JPEG_SCALED N = 2 and one under its EXIF orientation.

The scan that does not resynchronise (`no_resync`, 525 parts in 3 workgroups, no part's guess right): info entry [6], the
decodes of the most often decoded part, is printed by the test and was 257 on an MI355X, in u8 and in u8x3 (3 is what the
test asks: a guess, the predecessor's wrong exit state, the truth).  The round count is not told by the call; by the kernel's text the parts of a workgroup settle one per turn, so the last lane of a
workgroup decodes up to 256 times in one launch, workgroup k settles in launch k, and the host loop sees its first idle
launch in round 3 of the most_wg + 2 = 5 it allows.

Status 2: no byte of the destination is written, the frame's extent included.  Status 4: the issue that asked for these
tests wanted the destination untouched there too, and that wording is NOT followed.  held() asserts nothing about a damaged
frame's extent; only the guard bytes outside it are checked.  The library's contract (the decoder's section)
leaves a damaged frame's extent unspecified, because jd_output_kernel runs for every live frame in the same chain of
launches, before the host learns which scans were damaged; holding the output back for that answer would cost every call a
wait, which is timing work and not the business of a tests change."""
import numpy as np
import pytest

import jpeg_stream_cases as K
import numpy_jpeg_decode_ref as D
import numpy_jpeg_orient_ref as X
import numpy_jpeg_sampling_ref as S
import numpy_jpeg_scale_ref as Z

pytestmark = pytest.mark.gpu

GUARD = 0xAB
NAMES = K.names()


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


def batch_call(L, ctx, streams, fmt, sizes, order=None, bits=0, scale=None, orient=False, pad=7, gap=13):
    """The streams one behind the other (odd gaps), the pictures in `order`, each allocated for sizes[b], rows padded by
    `pad` bytes and `gap` guard bytes between and around them.  Returns (info, the destination region, per stream its
    (offset, row bytes, w, h))."""
    bpp = 3 if fmt == L.PIX_U8X3 else 1
    offs, end = [], 3
    for s in streams:
        offs.append(end)
        end += len(s) + 5
    region = np.full(end, 0x11, np.uint8)
    for s, o in zip(streams, offs):
        region[o:o + len(s)] = np.frombuffer(s, np.uint8)
    places, at = {}, gap
    for b in (order or range(len(streams))):
        w, h = sizes[b]
        places[b] = (at, w * bpp + pad, w, h)
        at += h * (w * bpp + pad) + gap
    table = L.jpeg_decode_table([(o, len(s)) for s, o in zip(streams, offs)], [places[b][:2] for b in range(len(streams))],
                                [places[b][2:] for b in range(len(streams))], orient=orient, scale=scale)
    d_src, d_dst = ctx.device_upload(region), ctx.device_upload(np.full(at, GUARD, np.uint8))
    try:
        info = ctx.decode_jpeg_device(d_src, region, fmt | bits, table, d_dst, at)
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


def same(got, want, what):
    assert got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d values differ, the first at %s" % (what, len(bad), bad[0].tolist()))


def size_of(case):
    return (case.spec["width"], case.spec["height"])


def held(case, fmt, status, picture):
    """what every frame of every call owes: the status, the picture or the untouched extent"""
    assert status == case.status, "%s: status %d" % (case.name, status)
    if case.status == 0:
        same(picture, K.expected(case, fmt), "%s %s" % (case.name, fmt))
    elif case.status == K.UNSUPPORTED:
        assert (picture == GUARD).all(), case.name + ": the refused file's extent is untouched"


@pytest.mark.parametrize("fmt", ["u8", "u8x3"])
@pytest.mark.parametrize("name", NAMES)
def test_case(L, ctx, name, fmt):
    case = K.get(name)
    pix, bpp = (L.PIX_U8X3, 3) if fmt == "u8x3" else (L.PIX_U8, 1)
    info, dst, places = batch_call(L, ctx, [case.stream], pix, [size_of(case)], bits=L.JPEG_ANY_SAMPLING if case.any_sampling else 0)
    got, free = pictures_and_guards(dst, places, bpp)
    assert (dst[free] == GUARD).all(), "a byte outside the picture was written"
    held(case, fmt, int(info[0, 5]), got[0])
    probe = S.probe(case.stream) if case.any_sampling else D.probe(case.stream)
    assert info[0, :5].tolist() == probe.row()[:5] and info[0, 7] == 0
    if name == "no_resync":
        print("no_resync: the most often decoded part was decoded %d times" % info[0, 6])
        assert info[0, 6] >= 3, "a guess, the predecessor's wrong exit state, the truth"
    if name == "scan_of_1_bytes":
        assert info[0, 6] == 1


MIXED = ["no_resync", "ri_1_constant", "colour_420_three_table_sets", "rgb_by_adobe_transform_0", "colour_444_three_table_sets",
         "edge_part_stuffed", "padding_rst_zeros_3", "fill_bytes_200"]


@pytest.mark.parametrize("fmt", ["u8x3", "u8"])
def test_eight_mixed_cases_in_one_call(L, ctx, fmt):
    """per-frame tables (three sets, one set, tables of one code) side by side in the workgroups of one launch"""
    cases = [K.get(n) for n in MIXED]
    pix, bpp = (L.PIX_U8X3, 3) if fmt == "u8x3" else (L.PIX_U8, 1)
    info, dst, places = batch_call(L, ctx, [c.stream for c in cases], pix, [size_of(c) for c in cases], order=[5, 2, 7, 0, 3, 6, 1, 4])
    assert info[:, 5].tolist() == [0, 0, 0, 2, 0, 0, 4, 0]
    got, free = pictures_and_guards(dst, places, bpp)
    assert (dst[free] == GUARD).all(), "a byte outside the pictures was written"
    for b, c in enumerate(cases):
        held(c, fmt, int(info[b, 5]), got[b])
    assert info[0, 6] >= 3


@pytest.mark.parametrize("name", ["colour_420_three_table_sets", "intervals_64"])
def test_at_half_size(L, ctx, name):
    case = K.get(name)
    assert np.array_equal(D.coefficients(D.probe(case.stream), case.stream)[1], case.coefs), "the restatement reads the writer's coefficients"
    status, want = Z.decode(case.stream, 2, "u8x3", any_sampling=False)
    assert status == 0
    info, dst, places = batch_call(L, ctx, [case.stream], L.PIX_U8X3, [want.shape[1::-1]], bits=L.JPEG_SCALED, scale=[2])
    got, free = pictures_and_guards(dst, places, 3)
    assert info[0, 5] == 0 and (dst[free] == GUARD).all()
    same(got[0], want, name + " at 1/2")


def test_the_binding_names_the_reason_of_a_refused_rgb_file(L, ctx):
    good = K.get("ycbcr_with_adobe_transform_1")
    same(ctx.decode_jpeg(good.stream), K.expected(good, "u8x3"), good.name)
    for name in ("rgb_by_adobe_transform_0", "rgb_by_component_ids"):
        with pytest.raises(L.LibrectifyError, match="frame 1: status 2: .*an RGB file"):
            ctx.decode_jpeg_batch([good.stream, K.get(name).stream])


def test_under_its_orientation(L, ctx):
    case = K.get("app1_that_is_not_exif_first")
    assert X.exif_orientation(case.stream) == 6
    want = X.orient(K.expected(case, "u8x3"), 6)
    info, dst, places = batch_call(L, ctx, [case.stream], L.PIX_U8X3, [want.shape[1::-1]], orient=True)
    got, free = pictures_and_guards(dst, places, 3)
    assert info[0, 5] == 0 and info[0, 7] == 6 and (dst[free] == GUARD).all()
    same(got[0], want, "orientation 6")
