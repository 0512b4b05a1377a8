"""Pure-numpy restatement of lr_encode_jpeg_device's stream: the complete baseline JPEG file,
byte for byte.  No PIL, no GPU.  Everything is in integers.

    encode(image_u8, quality, layout) -> bytes      image H x W (one component) or H x W x 3 (c0 red; YCbCr stream)

The stream: SOI, JFIF 1.01 APP0, one DQT segment per table (Annex K tables scaled by the IJG quality rule, zig-zag order),
SOF0, one DHT segment per table (the Annex K tables), DRI, SOS, one interleaved scan with RSTm after every restart
interval but the last, EOI.  A one-component stream carries table 0 only (one DQT, the two luminance DHT).
"""
import numpy as np

LAYOUT_420, LAYOUT_444 = 0, 1

# ITU-T T.81 Annex K.1 (natural order)
K1_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
K1_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99])
# zig-zag position -> natural index (row * 8 + column)
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
# Annex K.3: BITS (codes of length 1..16) and HUFFVAL
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
    0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
    0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5,
    0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25,
    0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA,
    0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4,
    0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]

# The forward DCT's matrix: T[u][x] = round(2^13 * c(u) / 2 * cos((2x + 1) u pi / 16)), c(0) = 1 / sqrt(2), else 1.
# Written out (they are the constants of DESIGN.md): row u is +-DCT_ROWS[u][x] mirrored with the sign (-1)^u.
DCT_HALF = [[2896, 2896, 2896, 2896], [4017, 3406, 2276, 799], [3784, 1567, -1567, -3784], [3406, -799, -4017, -2276],
            [2896, -2896, -2896, 2896], [2276, -4017, 799, 3406], [1567, -3784, 3784, -1567], [799, -2276, 3406, -4017]]
DCT = np.array([r + [(-1) ** u * v for v in reversed(r)] for u, r in enumerate(DCT_HALF)], np.int64)
DCT_ROW_SHIFT = 7  # the row pass keeps 13 - 7 = 6 fractional bits


def restart_interval(width, layout, components):
    """MCUs per restart interval: 96 blocks whatever the width (16 MCUs of 4:2:0, 32 of 4:4:4, 96 of one component)"""
    if components == 1:
        return 96
    return 16 if layout == LAYOUT_420 else 32


def quant_table(base, quality):
    """the IJG rule, in zig-zag order"""
    q = int(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((base[ZIGZAG] * s + 50) // 100, 1, 255).astype(np.int64)


def huff_table(bits, vals):
    """symbol -> (code, length), the canonical codes of Annex C"""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


def ycbcr(rgb):
    """IJG's fixed-point colour rule on an (..., 3) integer array"""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(plane, mw, mh):
    """to whole MCUs by replicating the last column and row"""
    h, w = plane.shape
    H, W = -(-h // mh) * mh, -(-w // mw) * mw
    return np.pad(plane, ((0, H - h), (0, W - w)), mode="edge")


def _blocks(plane):
    """(rows of blocks, columns of blocks, 8, 8)"""
    H, W = plane.shape
    return plane.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)


def fdct_quant(blocks, qzz):
    """blocks (..., 8, 8) of level-shifted samples -> (..., 64) quantised coefficients in zig-zag order"""
    s = blocks.astype(np.int64)
    a = (s @ DCT.T + (1 << (DCT_ROW_SHIFT - 1))) >> DCT_ROW_SHIFT  # row pass: a[y][u]
    b = DCT @ a                                                    # column pass: b[v][u], scale 2^(26 - 7)
    nat = b.reshape(b.shape[:-2] + (64,))[..., ZIGZAG]
    div = qzz << (26 - DCT_ROW_SHIFT)
    q = (np.abs(nat) + (div >> 1)) // div  # half away from zero
    return np.where(nat < 0, -q, q)


def planes(image, layout):
    """the padded, level-shifted component planes and (blocks per MCU, MCU width, MCU height)"""
    img = np.asarray(image)
    assert img.dtype == np.uint8
    if img.ndim == 2:
        return [_pad(img.astype(np.int64), 8, 8) - 128], 1, 8, 8
    assert img.ndim == 3 and img.shape[2] == 3
    if layout == LAYOUT_444:
        y, cb, cr = ycbcr(img)
        return [_pad(p, 8, 8) - 128 for p in (y, cb, cr)], 3, 8, 8
    pad = np.stack([_pad(img[..., i], 16, 16) for i in range(3)], axis=-1)
    y, cb, cr = ycbcr(pad)
    down = lambda p: (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2  # noqa: E731
    return [y - 128, down(cb) - 128, down(cr) - 128], 6, 16, 16


DUMMY = 0x7FFF  # in a block's DC: a 4:2:0 luminance block that lies wholly outside the frame


def coefficients(image, quality, layout):
    """(n_mcus, blocks per MCU, 64) quantised zig-zag coefficients in coding order, and the component of each block.  A 4:2:0
    luminance block whose block column is >= ceil(W / 8) or whose block row is >= ceil(H / 8) holds no pixel of the frame: it
    is DUMMY (DC = DUMMY, AC = 0) and coded as a DC difference of 0 and an end of block, libjpeg's dummy block."""
    ps, bpm, mw, mh = planes(image, layout)
    ql, qc = quant_table(K1_LUMA, quality), quant_table(K1_CHROMA, quality)
    if bpm == 1:
        c = fdct_quant(_blocks(ps[0]), ql)
        return c.reshape(-1, 1, 64), [0]
    if bpm == 3:
        cs = [fdct_quant(_blocks(p), q) for p, q in zip(ps, (ql, qc, qc))]
        return np.stack([c.reshape(-1, 64) for c in cs], axis=1), [0, 1, 2]
    yb = fdct_quant(_blocks(ps[0]), ql)  # (2 my, 2 mx, 64)
    h, w = np.asarray(image).shape[:2]
    yb[-(-h // 8):, :, :] = 0
    yb[-(-h // 8):, :, 0] = DUMMY
    yb[:, -(-w // 8):, :] = 0
    yb[:, -(-w // 8):, 0] = DUMMY
    my, mx = yb.shape[0] // 2, yb.shape[1] // 2
    yb = yb.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my * mx, 4, 64)
    cb = fdct_quant(_blocks(ps[1]), qc).reshape(-1, 1, 64)
    cr = fdct_quant(_blocks(ps[2]), qc).reshape(-1, 1, 64)
    return np.concatenate([yb, cb, cr], axis=1), [0, 0, 0, 0, 1, 2]


def _category(v):
    return int(abs(int(v))).bit_length()


def _encode_block(zz, diff, dc, ac):
    """(bits as an int, their number)"""
    cat = _category(diff)
    acc, n = dc[cat]
    if cat:
        acc = (acc << cat) | (diff if diff >= 0 else diff + (1 << cat) - 1)
        n += cat
    run = 0
    last = 0
    nz = np.flatnonzero(zz[1:]) + 1
    for k in nz.tolist():
        run = k - last - 1
        last = k
        while run >= 16:
            c, l = ac[0xF0]
            acc, n = (acc << l) | c, n + l
            run -= 16
        v = int(zz[k])
        cat = _category(v)
        c, l = ac[(run << 4) | cat]
        acc = (((acc << l) | c) << cat) | (v if v >= 0 else v + (1 << cat) - 1)
        n += l + cat
    if last != 63:
        c, l = ac[0x00]
        acc, n = (acc << l) | c, n + l
    return acc, n


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(width, height, quality, layout, components):
    ql, qc = quant_table(K1_LUMA, quality), quant_table(K1_CHROMA, quality)
    out = b"\xFF\xD8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += _segment(0xDB, bytes([0]) + bytes(ql.tolist()))
    if components == 3:
        out += _segment(0xDB, bytes([1]) + bytes(qc.tolist()))
    sof = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([components])
    if components == 1:
        sof += bytes([1, 0x11, 0])
    else:
        sof += bytes([1, 0x22 if layout == LAYOUT_420 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    out += _segment(0xC0, sof)
    out += _segment(0xC4, bytes([0x00]) + bytes(DC_LUMA_BITS) + bytes(DC_VALS))
    out += _segment(0xC4, bytes([0x10]) + bytes(AC_LUMA_BITS) + bytes(AC_LUMA_VALS))
    if components == 3:
        out += _segment(0xC4, bytes([0x01]) + bytes(DC_CHROMA_BITS) + bytes(DC_VALS))
        out += _segment(0xC4, bytes([0x11]) + bytes(AC_CHROMA_BITS) + bytes(AC_CHROMA_VALS))
    out += _segment(0xDD, restart_interval(width, layout, components).to_bytes(2, "big"))
    if components == 1:
        out += _segment(0xDA, bytes([1, 1, 0x00, 0, 63, 0]))
    else:
        out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def intervals(width, height, layout, components):
    mw = 16 if components == 3 and layout == LAYOUT_420 else 8
    n_mcus = (-(-width // mw)) * (-(-height // mw))
    ri = restart_interval(width, layout, components)
    return -(-n_mcus // ri)


def encode_coefficients(coefs, comp_of, width, height, quality, layout):
    """the complete stream of (n_mcus, blocks per MCU, 64) zig-zag coefficients"""
    components = 1 if len(comp_of) == 1 else 3
    tabs = [(huff_table(DC_LUMA_BITS, DC_VALS), huff_table(AC_LUMA_BITS, AC_LUMA_VALS)),
            (huff_table(DC_CHROMA_BITS, DC_VALS), huff_table(AC_CHROMA_BITS, AC_CHROMA_VALS))]
    ri = restart_interval(width, layout, components)
    out = [header(width, height, quality, layout, components)]
    n_mcus = len(coefs)
    n_int = -(-n_mcus // ri)
    for i in range(n_int):
        pred = [0, 0, 0]
        acc, n = 0, 0
        for m in range(i * ri, min(n_mcus, (i + 1) * ri)):
            for k, comp in enumerate(comp_of):
                zz = coefs[m, k]
                dc, ac = tabs[0 if comp == 0 else 1]
                if int(zz[0]) == DUMMY:  # (the prediction stays what it was)
                    a, l = _encode_block(zz, 0, dc, ac)
                else:
                    a, l = _encode_block(zz, int(zz[0]) - pred[comp], dc, ac)
                    pred[comp] = int(zz[0])
                acc, n = (acc << l) | a, n + l
        padn = -n % 8
        acc, n = (acc << padn) | ((1 << padn) - 1), n + padn
        out.append(acc.to_bytes(n // 8, "big").replace(b"\xFF", b"\xFF\x00"))
        if i != n_int - 1:
            out.append(bytes([0xFF, 0xD0 + (i & 7)]))
    out.append(b"\xFF\xD9")
    return b"".join(out)


def encode(image, quality, layout=LAYOUT_420):
    img = np.asarray(image)
    if not 1 <= int(quality) <= 100:
        raise ValueError("quality is 1..100")
    if img.ndim == 2 and layout != 0:
        raise ValueError("a one-component stream has layout 0")
    h, w = img.shape[:2]
    coefs, comp_of = coefficients(img, quality, layout)
    return encode_coefficients(coefs, comp_of, w, h, quality, layout)


def bound(width, height, components, layout):
    """lr_jpeg_bound"""
    mw = 16 if components == 3 and layout == LAYOUT_420 else 8
    bpm = 1 if components == 1 else (6 if layout == LAYOUT_420 else 3)
    n_mcus = (-(-width // mw)) * (-(-height // mw))
    ri = restart_interval(width, layout, components)
    return 640 + 2 * (-(-n_mcus // ri)) + 416 * n_mcus * bpm


def synth_u8(width, height, seed, colour):
    """an 8-bit frame of librectify_amd.synth.frame: gray, or three frames of seeds seed, seed + 1, seed + 2 as c0, c1, c2"""
    from librectify_amd import synth
    f = lambda s: np.clip(np.floor(synth.frame(width, height, s, noise=0.01).astype(np.float64) * 255.0 + 0.5), 0, 255).astype(np.uint8)  # noqa: E731
    return np.stack([f(seed), f(seed + 1), f(seed + 2)], axis=-1) if colour else f(seed)


def psnr(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    mse = float((d * d).mean())
    return 99.0 if mse == 0 else 10.0 * np.log10(255.0 * 255.0 / mse)
