"""The EXIF orientation of a JPEG file and what it does to the decoded picture, restated in
numpy for the tests of lr_decode_jpeg_device's entry [7]:

    exif_orientation(data) -> int                   the tag 0x0112 of IFD0 of the first Exif APP1 before SOS, 1..8; 0: none
    orient(picture, o) -> picture                   the upright picture of a stored one
    decode(data, fmt, orient=True) -> (status, picture)      numpy_jpeg_decode_ref.decode, upright
    info_row(data, orient) -> list                  the row of info the library gives for the file
    with_exif(stream, o, endian, ...) -> bytes      the stream with a hand-built APP1 behind its SOI
    encode_422(image, quality) -> bytes             a 4:2:2 stream, which numpy_jpeg_ref does not write

Nothing here is taken from the library's source: the walk over the markers is written from ITU T.81 annex B, the TIFF
block from the Exif 2.3 standard, section 4.6.2.
"""
import struct

import numpy as np

import numpy_jpeg_decode_ref as D
import numpy_jpeg_ref as R

EXIF = b"Exif\0\0"
XMP = b"http://ns.adobe.com/xap/1.0/\0<x:xmpmeta xmlns:x='adobe:ns:meta/'/>"


def tiff_orientation(t):
    """of the TIFF block t (the payload behind "Exif\\0\\0"): 1..8, or 0 if it tells none that counts"""
    if len(t) < 8 or t[:4] not in (b"II*\0", b"MM\0*"):
        return 0
    e = "<" if t[:2] == b"II" else ">"
    ifd = struct.unpack_from(e + "I", t, 4)[0]
    if ifd + 2 > len(t):
        return 0
    count = struct.unpack_from(e + "H", t, ifd)[0]
    if ifd + 2 + 12 * count > len(t):
        return 0
    for i in range(count):
        tag, typ, n = struct.unpack_from(e + "HHI", t, ifd + 2 + 12 * i)
        if tag == 0x0112:
            value = struct.unpack_from(e + "H", t, ifd + 2 + 12 * i + 8)[0]
            return value if typ == 3 and n == 1 and 1 <= value <= 8 else 0
    return 0


def exif_orientation(data):
    d = bytes(data)
    n = len(d)
    if n < 4 or d[:2] != b"\xFF\xD8":
        return 0
    p = 2
    while p < n and d[p] == 0xFF:
        while p < n and d[p] == 0xFF:
            p += 1
        if p >= n:
            break
        m = d[p]
        p += 1
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m in (0xD9, 0xDA) or p + 2 > n:
            break
        length = (d[p] << 8) | d[p + 1]
        if length < 2 or p + length > n:
            break
        seg = d[p + 2:p + length]
        p += length
        if m == 0xE1 and seg[:6] == EXIF:
            return tiff_orientation(seg[6:])  # the first Exif segment, whatever it holds
    return 0


def orient(picture, o):
    """O of the table: S the stored h x w (x c) picture"""
    s = np.asarray(picture)
    t = s.swapaxes(0, 1)  # t[y][x] = S[x][y]
    return np.ascontiguousarray({0: s, 1: s, 2: s[:, ::-1], 3: s[::-1, ::-1], 4: s[::-1], 5: t, 6: t[:, ::-1], 7: t[::-1, ::-1], 8: t[::-1]}[o])


_orient = orient


def decode(data, fmt="u8x3", orient=True):
    status, img = D.decode(data, fmt)
    if status == 0 and orient:
        img = _orient(img, exif_orientation(data))
    return status, img


def info_row(data, orient):
    """what info holds for the file (but [6], the count of decodes): entry [7] of the table 1 (orient) or 0"""
    row = D.probe(data).row()
    if orient:
        row[7] = max(exif_orientation(data), 1)
        if row[7] >= 5:
            row[0], row[1] = row[1], row[0]
    return row


def app1(payload):
    return b"\xFF\xE1" + struct.pack(">H", len(payload) + 2) + payload


def exif_payload(o, endian="MM", mark=None, ifd=8, count=None, typ=3, n=1, before=2, after=1):
    """"Exif\\0\\0" and a TIFF block of one IFD: `before` other entries, the orientation o, `after` others.  The knobs: mark
    (the four bytes of the byte order), ifd (the offset written; the IFD itself stays at 8), count (the entry count
    written), typ and n (the orientation entry's type and count)."""
    e = "<" if endian == "II" else ">"
    entry = lambda tag, typ, n, value: struct.pack(e + "HHI", tag, typ, n) + struct.pack(e + "HH", value, 0)  # noqa: E731
    entries = [entry(0x0100 + i, 3, 1, 9) for i in range(before)] + [entry(0x0112, typ, n, o)] + [entry(0x0128 + i, 3, 1, 2) for i in range(after)]
    head = (b"II*\0" if endian == "II" else b"MM\0*") if mark is None else mark
    body = struct.pack(e + "H", len(entries) if count is None else count) + b"".join(entries) + struct.pack(e + "I", 0)
    return EXIF + head + struct.pack(e + "I", ifd) + body


def splice(stream, segments, at=2):
    """the stream with the segments put in at byte `at` (2: behind SOI)"""
    s = bytes(stream)
    assert s[:2] == b"\xFF\xD8"
    return s[:at] + b"".join(segments) + s[at:]


def with_exif(stream, o, endian="MM", **knobs):
    return splice(stream, [app1(exif_payload(o, endian, **knobs))])


def after_sof(stream):
    """the offset just behind the stream's SOF0 segment"""
    s = bytes(stream)
    at = s.index(b"\xFF\xC0")
    return at + 2 + ((s[at + 2] << 8) | s[at + 3])


def encode_422(image, quality):
    """numpy_jpeg_ref's arithmetic and coding for a 4:2:2 stream: MCUs of 16 x 8, two luminance blocks side by side, the
    chrominance the rounded mean of two neighbours"""
    img = np.asarray(image)
    h, w = img.shape[:2]
    pad = np.stack([R._pad(img[..., i], 16, 8) for i in range(3)], axis=-1)
    y, cb, cr = R.ycbcr(pad)
    down = lambda p: (p[:, 0::2] + p[:, 1::2] + 1) >> 1  # noqa: E731
    ql, qc = R.quant_table(R.K1_LUMA, quality), R.quant_table(R.K1_CHROMA, quality)
    yb = R.fdct_quant(R._blocks(y - 128), ql)  # (my, 2 mx, 64)
    my, mx = yb.shape[0], yb.shape[1] // 2
    yb = yb.reshape(my * mx, 2, 64)
    cs = [R.fdct_quant(R._blocks(down(p) - 128), qc).reshape(-1, 1, 64) for p in (cb, cr)]
    stream = R.encode_coefficients(np.concatenate([yb] + cs, axis=1), [0, 0, 1, 2], w, h, quality, R.LAYOUT_444)
    sof = bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    at = stream.index(sof)
    return stream[:at + 1] + b"\x21" + stream[at + 2:]
