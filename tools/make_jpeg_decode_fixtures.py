#!/usr/bin/env python3
"""Regenerate tests/golden/jpeg_decode_kat.npz: foreign JPEG files and their decodes, for the JPEG decoder's tests.

Run in the build container only (needs PIL with libjpeg-turbo; the tests themselves do not):
    python tools/make_jpeg_decode_fixtures.py

The files are PIL's own, of small noisy-ramp pictures.  Per case <name>:
  stream_<name>      the file, uint8
  pil_<name>         PIL's decode of it (H x W for a one-component file, else H x W x 3), uint8; none for the rejects
  names              the accepted cases; rejects: the files the decoder must refuse with status 2
  doc_diff, doc_sha  of tests/golden/doc_image.jpg (the foreign camera file): the restatement's decode
                     (tests/numpy_jpeg_decode_ref.py) MINUS PIL's, int8, and the SHA-256 of PIL's decode.  The picture
                     itself is 1.7 MB; the test rebuilds PIL's decode from the difference and checks it against the hash,
                     so a change of the restatement cannot pass unnoticed.
The accepted cases cover one component, 4:4:4, 4:2:2 and 4:2:0; optimised and Annex K code tables; no DRI, a restart
interval of one and of three MCUs and of one MCU row; sizes that are no multiple of an MCU.  The rejects are a progressive
file, a CMYK file and a file whose frame header says that luminance is sampled 1 x 2 (4:4:0).  PIL writes neither 4:4:0 nor
4:1:1: that file is PIL's 4:2:0 file with the sampling byte of its SOF changed, which is all a refusal on the header needs.
"""
import hashlib
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy_jpeg_decode_ref as D  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "jpeg_decode_kat.npz")
DOC = os.path.join(ROOT, "tests", "golden", "doc_image.jpg")

# name: (width, height, colour, PIL's save options)
CASES = {
    "g_9x7": (9, 7, False, dict(quality=90)),
    "g_17x33_r3": (17, 33, False, dict(quality=75, restart_marker_blocks=3)),
    "g_203x117_opt": (203, 117, False, dict(quality=95, optimize=True)),
    "c444_17x33": (17, 33, True, dict(quality=90, subsampling=0)),
    "c444_203x117_r1": (203, 117, True, dict(quality=85, subsampling=0, restart_marker_blocks=1)),
    "c422_9x7": (9, 7, True, dict(quality=90, subsampling=1)),
    "c422_17x33_r3": (17, 33, True, dict(quality=75, subsampling=1, restart_marker_blocks=3, optimize=True)),
    "c422_203x117_opt": (203, 117, True, dict(quality=95, subsampling=1, optimize=True)),
    "c420_9x7": (9, 7, True, dict(quality=90, subsampling=2)),
    "c420_17x33_r1_opt": (17, 33, True, dict(quality=75, subsampling=2, restart_marker_blocks=1, optimize=True)),
    "c420_203x117": (203, 117, True, dict(quality=95, subsampling=2)),
    "c420_203x117_opt": (203, 117, True, dict(quality=95, subsampling=2, optimize=True)),
    "c420_203x117_rows": (203, 117, True, dict(quality=85, subsampling=2, restart_marker_rows=1)),
}


def textured(w, h, seed, colour):
    """a ramp under noise of +-20"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    ramp = (3 * x + 2 * y) % 256
    if colour:
        ramp = np.stack([ramp, (ramp + 85) % 256, (2 * ramp) % 256], axis=-1)
    return np.clip(ramp + rng.integers(-20, 21, ramp.shape), 0, 255).astype(np.uint8)


def save(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", **kw)
    return buf.getvalue()


def sof(stream):
    """(marker, payload) of the frame header"""
    p = 2
    while True:
        assert stream[p] == 0xFF
        m, n = stream[p + 1], (stream[p + 2] << 8) | stream[p + 3]
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return m, stream[p + 4:p + 2 + n]
        p += 2 + n


def main():
    data, names = {}, []
    for i, (name, (w, h, colour, kw)) in enumerate(CASES.items()):
        stream = save(textured(w, h, 100 + i, colour), **kw)
        dec = np.asarray(Image.open(io.BytesIO(stream)))
        assert dec.shape == ((h, w, 3) if colour else (h, w)) and dec.dtype == np.uint8
        m, f = sof(stream)
        assert m == 0xC0 and (b"\xFF\xDD" in stream) == any(k.startswith("restart") for k in kw), name
        if colour:
            assert f[7] == {0: 0x11, 1: 0x21, 2: 0x22}[kw["subsampling"]], name
        data["stream_" + name] = np.frombuffer(stream, np.uint8)
        data["pil_" + name] = dec
        names.append(name)
        print("%-20s %6d bytes, SOF%d, sampling %02x" % (name, len(stream), m - 0xC0, f[7]))
    rejects = {
        "progressive": save(textured(40, 24, 1, True), quality=85, progressive=True),
        "c440": save(textured(40, 24, 4, True), quality=85, subsampling=2),
    }
    buf = io.BytesIO()
    Image.fromarray(textured(40, 24, 2, True)).convert("CMYK").save(buf, "JPEG", quality=85)
    rejects["cmyk"] = buf.getvalue()
    # PIL writes no 4:4:0 itself: the 4:2:0 file's luminance sampling 2 x 2 becomes 1 x 2 in the frame header (the decoder
    # must refuse the file on its header, whatever the scan holds)
    s = bytearray(rejects["c440"])
    at = s.index(b"\xFF\xC0") + 4 + 7
    assert s[at] == 0x22
    s[at] = 0x12
    rejects["c440"] = bytes(s)
    assert sof(rejects["progressive"])[0] == 0xC2 and sof(rejects["cmyk"])[1][5] == 4
    for name, stream in rejects.items():
        data["stream_" + name] = np.frombuffer(stream, np.uint8)
        print("%-20s %6d bytes (reject)" % (name, len(stream)))
    doc = open(DOC, "rb").read()
    pil = np.asarray(Image.open(io.BytesIO(doc)))
    status, ours = D.decode(doc)
    assert status == 0 and ours.shape == pil.shape == (563, 1000, 3)
    diff = ours.astype(np.int16) - pil.astype(np.int16)
    assert np.abs(diff).max() <= 127
    data["doc_diff"] = diff.astype(np.int8)
    data["doc_sha"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(pil).tobytes()).digest(), np.uint8)
    print("doc_image.jpg: the restatement differs from PIL by at most %d" % np.abs(diff).max())
    data["names"] = np.array(names)
    data["rejects"] = np.array(list(rejects))
    np.savez_compressed(OUT, **data)
    print("wrote", os.path.normpath(OUT), os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    sys.exit(main())
