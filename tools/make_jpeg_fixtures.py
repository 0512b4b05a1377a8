#!/usr/bin/env python3
"""Regenerate tests/golden/jpeg_kat.npz: the known answers of the JPEG encoder's CPU tests.

Run in the build container only (needs PIL; the tests themselves do not):
    python tools/make_jpeg_fixtures.py

Cases: the colour frame 203 x 117 (tests/numpy_jpeg_ref.py: synth_u8, seed 21) in 4:2:0 and 4:4:4 and the gray frame
257 x 131 (seed 12), each at qualities 50, 90 and 95.  Per case <name> = c420 | c444 | g, quality <q>:
  sha_c, sha_g                 SHA-256 of the sources' bytes (the test regenerates the sources and checks them: the
                               frames themselves, noise included, would fill the file on their own)
  stream_<name>_<q>            the reference's stream (tests/numpy_jpeg_ref.py: encode), uint8
  ref_<name>_<q>               float64 [PSNR against the source of PIL's decode of that stream]
  pil_<name>_<q>               float64 [size in bytes, PSNR against the source] of PIL's own encoder at the same quality and
                               layout with optimize=False
  decode_g_95                  PIL's decode of stream_g_95 MINUS the source, as int8: the one decode kept in full (the
                               test recomputes ref_g_95 from it).  Nine decodes are 290 KB even as differences; the file
                               stays under 100 KB, and where PIL is importable the test decodes every stream live.
"""
import hashlib
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy_jpeg_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "jpeg_kat.npz")
QUALITIES = (50, 90, 95)


def main():
    src_c, src_g = R.synth_u8(203, 117, 21, True), R.synth_u8(257, 131, 12, False)
    sha = lambda a: np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)  # noqa: E731
    data = dict(sha_c=sha(src_c), sha_g=sha(src_g))
    for name, img, layout in (("c420", src_c, 0), ("c444", src_c, 1), ("g", src_g, 0)):
        for q in QUALITIES:
            stream = R.encode(img, q, layout)
            dec = np.asarray(Image.open(io.BytesIO(stream)))
            assert dec.shape == img.shape and dec.dtype == np.uint8
            diff = dec.astype(np.int16) - img.astype(np.int16)
            assert np.abs(diff).max() <= 127
            buf = io.BytesIO()
            kw = dict(subsampling=2 if layout == 0 else 0) if img.ndim == 3 else {}
            Image.fromarray(img).save(buf, "JPEG", quality=q, optimize=False, **kw)
            pil = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
            key = "%s_%d" % (name, q)
            data["stream_" + key] = np.frombuffer(stream, np.uint8)
            data["ref_" + key] = np.array([R.psnr(dec, img)], np.float64)
            if key == "g_95":
                data["decode_" + key] = diff.astype(np.int8)
            data["pil_" + key] = np.array([len(buf.getvalue()), R.psnr(pil, img)], np.float64)
            print("%-8s stream %6d  PIL %6d  PSNR %.3f  PIL's %.3f" % (key, len(stream), len(buf.getvalue()), R.psnr(dec, img), R.psnr(pil, img)))
    np.savez_compressed(OUT, **data)
    print("wrote", os.path.normpath(OUT), os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    sys.exit(main())
