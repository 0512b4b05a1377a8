"""The JPEG decoder's second source and header parser on streams that no encoder library wrote: every case of
tests/jpeg_stream_cases.py (built symbol by symbol by tests/jpeg_stream_writer.py from its coefficients, which are the
truth).  Per case: the status from the restatement's probe and from the C ABI's probe mode (no GPU); for status 0 the
restatement's sequential entropy decoder gives the writer's coefficients exactly; PIL reads the stream as the same picture
(luminance within 2 levels of the restatement's, each side being within 1 of the ideal inverse transform; Cb and Cr too
where nothing is upsampled); and what the case claims to reach holds on the writer's log.

The rules the cases forced (docs/jpeg_decode_bounds.md): padding in front of an RSTm is 1-bits, anything else is status 4,
while in front of EOI any padding is taken; a three-component file that libjpeg would read as RGB (Adobe transform 0, or the
ids 'R', 'G', 'B' without a JFIF segment) is status 2."""
import io

import numpy as np
import pytest

import jpeg_stream_cases as K
import numpy_jpeg_decode_ref as D
import numpy_jpeg_sampling_ref as S

NAMES = K.names()


@pytest.fixture(scope="module")
def L():
    import librectify_amd as L
    from librectify_amd import build

    build.build(verbose=False)
    L.lib()
    return L


def probe(case):
    return S.probe(case.stream) if case.any_sampling else D.probe(case.stream)


def coefficients(case, info):
    return S.coefficients(info, case.stream) if case.any_sampling else D.coefficients(info, case.stream)


@pytest.mark.parametrize("name", NAMES)
def test_status_and_coefficients(name):
    case = K.get(name)
    info = probe(case)
    if case.status == K.UNSUPPORTED:
        assert info.status == K.UNSUPPORTED and case.message in info.message
        return
    assert info.status == 0, info.message
    assert (info.width, info.height, info.restart, info.scan) == (case.spec["width"], case.spec["height"], case.log.ri, case.log.scan)
    assert all(np.array_equal(a, b) for a, b in zip(info.q, case.log.q)), "the divisors are the writer's, component by component"
    status, coefs = coefficients(case, info)
    assert status == case.status
    if status == 0:
        assert coefs.shape == case.coefs.shape and np.array_equal(coefs, case.coefs), "the sequential decoder against the writer's input"


@pytest.mark.parametrize("name", NAMES)
def test_the_case_reaches_what_it_claims(name):
    case = K.get(name)
    assert case._reach is not None, "every case says what it reaches"
    case.reach()
    if name == "no_resync":
        print("no_resync: %.1f %% of the parts' guesses miss the true state at the next boundary" % (100 * case.missed))


def test_the_writers_typical_tables_are_annex_k():
    """typed in twice, here and in the encoder's restatement: the two copies agree"""
    import jpeg_stream_writer as W
    import numpy_jpeg_ref as R

    assert W.STD_DC_LUM == (R.DC_LUMA_BITS, R.DC_VALS) and W.STD_DC_CHR == (R.DC_CHROMA_BITS, R.DC_VALS)
    assert W.STD_AC_LUM == (R.AC_LUMA_BITS, R.AC_LUMA_VALS) and W.STD_AC_CHR == (R.AC_CHROMA_BITS, R.AC_CHROMA_VALS)
    assert np.array_equal(W.ZIGZAG, R.ZIGZAG)
    for bad in ([(0, 1), (1, 1)], [(0, 1), (1, 2), (2, 2)], [(0, 2), (1, 2), (2, 2), (3, 2)]):  # too many codes; a code of all 1-bits
        with pytest.raises(AssertionError):
            W.codes(W.table_from_lengths(bad))


def test_the_sizes_cover_the_part_and_workgroup_counts():
    parts = {n: K.get("scan_of_%d_bytes" % n).n_parts for n in K.SIZES}
    assert parts == K.SIZES and set(parts.values()) == {1, 2, 256, 257, 512, 513}, parts  # (the parts count EOI's two bytes)
    assert K.get("edge_workgroup_end").n_parts > 256 and K.get("no_resync").n_parts > 512


def pil_planes(stream, rgb=False, truncated=False):
    """truncated: the file has no EOI, which PIL takes only when told to (libjpeg then supplies the EOI)"""
    from PIL import Image, ImageFile

    im = Image.open(io.BytesIO(stream))
    if im.mode != "L" and not rgb:
        im.draft("YCbCr", im.size)
        assert im.mode == "YCbCr"
    if rgb:
        assert im.mode == "RGB"  # (libjpeg converts nothing then: the planes are the components)
    before = ImageFile.LOAD_TRUNCATED_IMAGES
    ImageFile.LOAD_TRUNCATED_IMAGES = truncated
    try:
        a = np.asarray(im).astype(np.int64)
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = before
    return [a] if a.ndim == 2 else [a[..., i] for i in range(3)]


@pytest.mark.parametrize("name", NAMES)
def test_pil_reads_the_same_picture(name):
    case = K.get(name)
    pil = pil_planes(case.stream, rgb=case.status == K.UNSUPPORTED, truncated=name == "no_eoi")
    if case.status == K.UNSUPPORTED:  # PIL reads the file as RGB, and its planes are the writer's components
        info = D.probe(K.get("ycbcr_with_adobe_transform_1").stream)  # (the same size, sampling and divisors)
        assert info.status == 0 and (info.width, info.height) == (case.spec["width"], case.spec["height"])
        for c, plane in enumerate(D.component_planes(info, case.coefs)):
            assert int(np.abs(pil[c] - plane).max()) <= 2, (name, c)
        return
    if case.status == 0:
        status, y = D.decode(case.stream, "u8") if not case.any_sampling else S.decode(case.stream, "u8")
        assert status == 0
    else:  # a stream we refuse for its padding still means what the writer says
        y = K.expected_from_headers_of(case)
    diff = int(np.abs(pil[0] - y.astype(np.int64)).max())
    print("%s: luminance differs from PIL's by at most %d" % (name, diff))
    assert pil[0].shape == y.shape and diff <= 2
    info = probe(case)
    if info.components == 3 and info.layout == D.LAYOUT_444 and case.status == 0:
        planes = D.component_planes(info, case.coefs)
        for c in (1, 2):
            diff = int(np.abs(pil[c] - planes[c]).max())
            print("%s: component %d differs from PIL's by at most %d" % (name, c, diff))
            assert diff <= 2


def test_statuses_through_the_c_abi(L):
    for any_sampling in (False, True):
        cases = [K.get(n) for n in NAMES if K.get(n).any_sampling == any_sampling]
        info = L.jpeg_info([c.stream for c in cases], any_sampling=any_sampling)
        for c, row in zip(cases, info):
            want = c.status if c.status != K.DAMAGED else 0  # (the probe reads the headers alone)
            assert row[5] == want, c.name
            assert row.tolist()[:6] == probe(c).row()[:6], c.name
    for name in ("rgb_by_adobe_transform_0", "rgb_by_component_ids"):
        assert L.jpeg_info([K.get(name).stream])[0, 5] == 2
        assert b"RGB" in L.lib().lr_last_error(), name
