#!/usr/bin/env python3
"""Regenerate tests/golden/jpeg_sampling_kat.npz: baseline JPEG files of the samplings that lr_decode_jpeg_device takes with
LR_JPEG_ANY_SAMPLING alone, and PIL's decodes of them.

Run in the build container only (needs PIL with libjpeg-turbo; the tests themselves do not):
    python tools/make_jpeg_sampling_fixtures.py

PIL writes neither 4:4:0 nor 4:1:1, so the files come from the small baseline writer below: any factors of 1, 2, 4, a box
average down to each component's size, and the DCT, quantisation and Huffman coding of tests/numpy_jpeg_ref.py (Annex K
tables) and tests/numpy_jpeg_optimize_ref.py (tables of the file's own symbols).  Per case <name>:
  stream_<name>      the file, uint8
  pil_<name>         PIL's decode of it, H x W x 3 uint8
  names              all cases
Every file is held to what it is meant to be: PIL opens it, and its SOF carries the intended sampling bytes.
The writer itself (coefficients, write, encode) needs no PIL: tests/test_gpu_jpeg_sampling.py makes a 4:4:0 file of a
picture with lines in it with it.
The cases: seven samplings (named by the three components' sampling bytes), each at 9 x 7 (less than one MCU) and at 67 x 35
(ragged on both edges, more than two MCUs each way); restart intervals of 1 MCU, 3 MCUs and one MCU row on 4:4:0 and 4:1:1;
`t440_35x67`, a 4:4:0 file made the way a lossless rotation makes one -- the coefficients, the block grid and the
quantisation tables of one of PIL's 4:2:2 files transposed; `big440`, 320 x 240 noise at quality 95 in 4:4:0, whose scan
is longer than the 32 KiB one workgroup of the decoder's first stage takes.
"""
import io
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy_jpeg_decode_ref as D  # noqa: E402
import numpy_jpeg_optimize_ref as P  # noqa: E402
import numpy_jpeg_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "jpeg_sampling_kat.npz")

# name: the sampling bytes of Y, Cb, Cr
SAMPLINGS = {
    "s12": (0x12, 0x11, 0x11),      # 4:4:0
    "s41": (0x41, 0x11, 0x11),      # 4:1:1
    "s14": (0x14, 0x11, 0x11),
    "s42": (0x42, 0x11, 0x11),
    "s24": (0x24, 0x11, 0x11),      # 10 blocks to the MCU
    "s21x3": (0x21, 0x21, 0x21),    # equal factors that are not 1
    "s22_11_21": (0x22, 0x11, 0x21),  # Cb and Cr differ
}


def textured(w, h, seed):
    """tools/make_jpeg_decode_fixtures.py's picture: a ramp under noise of +-20"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    ramp = (3 * x + 2 * y) % 256
    ramp = np.stack([ramp, (ramp + 85) % 256, (2 * ramp) % 256], axis=-1)
    return np.clip(ramp + rng.integers(-20, 21, ramp.shape), 0, 255).astype(np.uint8)


def coefficients(img, sampling, quality):
    """((n_mcus, blocks per MCU, 64) zig-zag coefficients in coding order, component of each block, [q of Y, q of C] zig-zag)"""
    hv = [(s >> 4, s & 15) for s in sampling]
    hmax, vmax = hv[0]
    pad = np.stack([R._pad(img[..., i], 8 * hmax, 8 * vmax) for i in range(3)], axis=-1)
    H, W = pad.shape[:2]
    my, mx = H // (8 * vmax), W // (8 * hmax)
    qs = [R.quant_table(R.K1_LUMA, quality), R.quant_table(R.K1_CHROMA, quality)]
    parts, comp_of = [], []
    for i, (plane, (h, v)) in enumerate(zip(R.ycbcr(pad), hv)):
        rx, ry = hmax // h, vmax // v
        box = plane.reshape(H // ry, ry, W // rx, rx).sum(axis=(1, 3))
        small = (box + rx * ry // 2) // (rx * ry)
        c = R.fdct_quant(R._blocks(small - 128), qs[min(i, 1)])  # (my v, mx h, 64)
        parts.append(c.reshape(my, v, mx, h, 64).transpose(0, 2, 1, 3, 4).reshape(my * mx, v * h, 64))
        comp_of += [i] * (h * v)
    return np.concatenate(parts, axis=1), comp_of, qs


def write(coefs, comp_of, qs, sampling, w, h, ri=0, optimize=False):
    """the baseline file of the coefficients: SOI, two DQT, SOF0, four DHT, DRI if ri, SOS, the scan, EOI"""
    def interval_starts():
        return range(0, len(coefs), ri if ri else len(coefs))

    if optimize:
        counts = [[[0] * 256, [0] * 256], [[0] * 256, [0] * 256]]
        for m0 in interval_starts():
            pred = [0, 0, 0]
            for m in range(m0, min(len(coefs), m0 + (ri if ri else len(coefs)))):
                for k, comp in enumerate(comp_of):
                    dc, ac = counts[min(comp, 1)]
                    P._block_symbols(coefs[m, k], int(coefs[m, k, 0]) - pred[comp], dc, ac)
                    pred[comp] = int(coefs[m, k, 0])
        tables = [(P.optimal_table(c[0]), P.optimal_table(c[1])) for c in counts]
    else:
        tables = [((R.DC_LUMA_BITS, R.DC_VALS), (R.AC_LUMA_BITS, R.AC_LUMA_VALS)), ((R.DC_CHROMA_BITS, R.DC_VALS), (R.AC_CHROMA_BITS, R.AC_CHROMA_VALS))]
    out = [b"\xFF\xD8"]
    for t, q in enumerate(qs):
        out.append(R._segment(0xDB, bytes([t]) + bytes(np.asarray(q).tolist())))
    sof = bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3])
    for i, s in enumerate(sampling):
        sof += bytes([i + 1, s, min(i, 1)])
    out.append(R._segment(0xC0, sof))
    for t, (dc, ac) in enumerate(tables):
        out.append(R._segment(0xC4, bytes([t]) + bytes(dc[0]) + bytes(dc[1])))
        out.append(R._segment(0xC4, bytes([0x10 | t]) + bytes(ac[0]) + bytes(ac[1])))
    if ri:
        out.append(R._segment(0xDD, ri.to_bytes(2, "big")))
    out.append(R._segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    tabs = [(R.huff_table(*dc), R.huff_table(*ac)) for dc, ac in tables]
    starts = list(interval_starts())
    for i, m0 in enumerate(starts):
        pred, acc, n = [0, 0, 0], 0, 0
        for m in range(m0, starts[i + 1] if i + 1 < len(starts) else len(coefs)):
            for k, comp in enumerate(comp_of):
                dc, ac = tabs[min(comp, 1)]
                a, l = R._encode_block(coefs[m, k], int(coefs[m, k, 0]) - pred[comp], dc, ac)
                pred[comp] = int(coefs[m, k, 0])
                acc, n = (acc << l) | a, n + l
            # the MCU's whole bytes leave the accumulator (a scan without restart markers would make it quadratic)
            out.append((acc >> (n % 8)).to_bytes(n // 8, "big").replace(b"\xFF", b"\xFF\x00"))
            acc, n = acc & ((1 << (n % 8)) - 1), n % 8
        padn = -n % 8
        acc, n = (acc << padn) | ((1 << padn) - 1), n + padn
        out.append(acc.to_bytes(n // 8, "big").replace(b"\xFF", b"\xFF\x00"))
        if i != len(starts) - 1:
            out.append(bytes([0xFF, 0xD0 + (i & 7)]))
    out.append(b"\xFF\xD9")
    return b"".join(out)


def encode(img, sampling, quality, ri=0, optimize=False):
    h, w = img.shape[:2]
    coefs, comp_of, qs = coefficients(img, sampling, quality)
    return write(coefs, comp_of, qs, sampling, w, h, ri, optimize)


def transposed_422(img, quality):
    """PIL's 4:2:2 file of the picture, turned into the 4:4:0 file of the transposed picture without decoding it further than
    its coefficients: every block transposed, the MCU grid transposed, the luminance pair side by side now one above the other
    (the same two blocks in the same order), the quantisation tables transposed"""
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=1)
    info = D.probe(buf.getvalue())
    assert info.status == 0 and info.layout == D.LAYOUT_422
    status, nat = D.coefficients(info, buf.getvalue())  # (n_mcus, 4, 64) natural order
    assert status == 0
    _, _, _, mx, my, comp_of = D.geometry(info)
    t = nat.reshape(my, mx, 4, 8, 8).transpose(1, 0, 2, 4, 3).reshape(mx * my, 4, 64)
    qs = [np.asarray(info.q[i]).reshape(8, 8).T.reshape(64)[R.ZIGZAG] for i in (0, 1)]
    assert (np.asarray(info.q[1]) == np.asarray(info.q[2])).all()
    return write(t[..., R.ZIGZAG], comp_of, qs, (0x12, 0x11, 0x11), info.height, info.width, optimize=True)


def sof(stream):
    at = stream.index(b"\xFF\xC0")
    return stream[at + 4:at + 2 + ((stream[at + 2] << 8) | stream[at + 3])]


def main():
    from PIL import Image

    cases = {}
    for i, (name, s) in enumerate(SAMPLINGS.items()):
        cases["%s_9x7" % name] = (encode(textured(9, 7, 200 + i), s, 90, optimize=bool(i & 1)), s, 9, 7, 0)
        cases["%s_67x35" % name] = (encode(textured(67, 35, 300 + i), s, 85, optimize=not i & 1), s, 67, 35, 0)
    for j, name in enumerate(("s12", "s41")):
        s = SAMPLINGS[name]
        row = -(-67 // (8 * (s[0] >> 4)))
        for k, ri in enumerate((1, 3, row)):
            label = "%s_67x35_%s" % (name, ("r1", "r3", "rows")[k])  # (an MCU row of 4:1:1 is 3 MCUs here as well)
            cases[label] = (encode(textured(67, 35, 400 + 3 * j + k), s, 80, ri, optimize=bool((j + k) & 1)), s, 67, 35, ri)
    cases["t440_35x67"] = (transposed_422(textured(67, 35, 500), 90), SAMPLINGS["s12"], 35, 67, 0)
    noise = np.random.default_rng(600).integers(0, 256, (240, 320, 3), dtype=np.uint8)
    cases["big440"] = (encode(noise, SAMPLINGS["s12"], 95), SAMPLINGS["s12"], 320, 240, 0)
    assert len(cases["big440"][0]) >= 40000, "its parts span two workgroups of the sync stage (256 parts of 128 bytes)"
    data = {}
    for name, (stream, s, w, h, ri) in cases.items():
        f = sof(stream)
        assert f[0] == 8 and (f[1] << 8 | f[2], f[3] << 8 | f[4], f[5]) == (h, w, 3) and (f[7], f[10], f[13]) == s, name
        assert (b"\xFF\xDD" in stream) == bool(ri), name
        dec = np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))
        assert dec.shape == (h, w, 3) and dec.dtype == np.uint8, name
        data["stream_" + name] = np.frombuffer(stream, np.uint8)
        data["pil_" + name] = dec
        print("%-20s %6d bytes, sampling %02x %02x %02x, restart %d" % ((name, len(stream)) + s + (ri,)))
    # the transposed file is the transposed picture: PIL's decode of it against PIL's decode of the 4:2:2 file it was made of
    buf = io.BytesIO()
    Image.fromarray(textured(67, 35, 500)).save(buf, "JPEG", quality=90, subsampling=1)
    upright = np.asarray(Image.open(buf)).astype(int)
    print("t440_35x67 against the transposed decode of its 4:2:2 source: differs by at most %d"
          % np.abs(data["pil_t440_35x67"].astype(int) - upright.swapaxes(0, 1)).max())
    data["names"] = np.array(list(cases))
    np.savez_compressed(OUT, **data)
    print("wrote", os.path.normpath(OUT), os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 1000000


if __name__ == "__main__":
    sys.exit(main())
