"""Pure-numpy restatement of lr_decode_jpeg_device: a baseline JPEG stream to pixels, in
integers throughout.  No PIL, no GPU.

    probe(data)                 -> Info (width, height, components, layout, restart interval, status, message, ...)
    decode(data, fmt="u8x3")    -> (status, picture or None)    fmt "u8": the luminance plane, "u8x3": RGB with c0 red

The entropy decoder here is the plain sequential one (it counts MCUs); the device's self-synchronising one arrives at the
same coefficients on every stream whose status is 0, which is what the GPU tests compare.  Everything behind the
coefficients (dequantisation, the inverse DCT, the upsampling, the colour rule) is the rule itself.
"""
import re

import numpy as np

from numpy_jpeg_ref import DCT, ZIGZAG

LAYOUT_420, LAYOUT_444, LAYOUT_422 = 0, 1, 2
OK, NOT_JPEG, UNSUPPORTED, SIZE_MISMATCH, DAMAGED = 0, 1, 2, 3, 4

IDCT_MID_SHIFT = 7      # after the first pass: 13 - 7 = 6 fractional bits stay
IDCT_END_SHIFT = 19     # 6 + 13
COEF_LIMIT = 32767      # |c q| saturates here (legitimate data stays below 2^12)
MID_LIMIT = 65535       # and the first pass's result here (legitimate data stays below 2^15.8)


class Info:
    def __init__(self):
        self.width = self.height = self.components = self.layout = self.restart = 0
        self.status, self.message = NOT_JPEG, "not a JPEG stream"
        self.scan = 0        # offset of the scan's first byte
        self.q = []          # per component: 64 divisors, natural order
        self.dc = []         # per component: (bits, vals)
        self.ac = []
        self.hv = []         # per component: (h, v)

    def row(self):
        return [self.width, self.height, self.components, self.layout, self.restart, self.status, 0, 0]


def probe(data, expect=None):
    """The headers up to SOS.  expect: (width, height) the caller allocated for, or None."""
    d = bytes(data)
    n = len(d)
    info = Info()

    def fail(status, message):
        info.status, info.message = status, message
        return info

    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        return fail(NOT_JPEG, "no SOI")
    qt, ht, sof, p = {}, {}, None, 2
    jfif, adobe = False, None  # a JFIF APP0 was seen; the transform byte of the last Adobe APP14
    while True:
        if p >= n:
            return fail(NOT_JPEG, "truncated before SOS")
        if d[p] != 0xFF:
            return fail(NOT_JPEG, "no marker where one is due")
        while p < n and d[p] == 0xFF:
            p += 1
        if p >= n:
            return fail(NOT_JPEG, "truncated before SOS")
        m = d[p]
        p += 1
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            return fail(NOT_JPEG, "EOI before SOS")
        if p + 2 > n:
            return fail(NOT_JPEG, "truncated before SOS")
        length = (d[p] << 8) | d[p + 1]
        if length < 2 or p + length > n:
            return fail(NOT_JPEG, "truncated before SOS")
        seg = d[p + 2:p + length]
        p += length
        if m == 0xDB:
            s = 0
            while s < len(seg):
                pq, tq = seg[s] >> 4, seg[s] & 15
                if pq != 0:
                    return fail(UNSUPPORTED, "16-bit quantisation table")
                if tq > 3 or s + 65 > len(seg):
                    return fail(NOT_JPEG, "bad DQT")
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = np.frombuffer(seg[s + 1:s + 65], np.uint8)
                qt[tq] = t
                s += 65
        elif m == 0xC4:
            s = 0
            while s < len(seg):
                if s + 17 > len(seg):
                    return fail(NOT_JPEG, "bad DHT")
                tc, th = seg[s] >> 4, seg[s] & 15
                bits = list(seg[s + 1:s + 17])
                cnt = sum(bits)
                if tc > 1 or th > 3 or cnt > 256 or s + 17 + cnt > len(seg):
                    return fail(NOT_JPEG, "bad DHT")
                ht[(tc, th)] = (bits, list(seg[s + 17:s + 17 + cnt]))
                s += 17 + cnt
        elif m == 0xDD:
            if len(seg) != 2:
                return fail(NOT_JPEG, "bad DRI")
            info.restart = (seg[0] << 8) | seg[1]
        elif m in (0xC0, 0xC1):
            if sof is not None:
                return fail(UNSUPPORTED, "more than one frame header")
            if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                return fail(NOT_JPEG, "bad SOF")
            sof = seg
        elif 0xC2 <= m <= 0xCF and m != 0xC8:  # (0xC4 was handled above)
            if m != 0xCC and len(seg) >= 6:  # (the size and the components are told all the same)
                info.height, info.width, info.components = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if m == 0xC2:
                return fail(UNSUPPORTED, "progressive (SOF2)")
            return fail(UNSUPPORTED, "arithmetic, lossless or hierarchical coding (SOF%d)" % (m - 0xC0))
        elif m == 0xE0 and seg[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
            adobe = seg[11]
        elif m == 0xDA:
            break
    if sof is None:
        return fail(NOT_JPEG, "SOS before SOF")
    if sof[0] != 8:
        return fail(UNSUPPORTED, "%d-bit precision" % sof[0])
    info.height, info.width, nc = (sof[1] << 8) | sof[2], (sof[3] << 8) | sof[4], sof[5]
    if info.width < 1 or info.height < 1:
        return fail(UNSUPPORTED, "a size of 0 (DNL)")
    if nc not in (1, 3):
        info.components = nc
        return fail(UNSUPPORTED, "%d components" % nc)
    info.components = nc
    # libjpeg's rule for three components (default_decompress_parms): a JFIF segment says YCbCr; else an Adobe segment
    # decides (transform 0: RGB); else the ids 'R', 'G', 'B' say RGB.  The colour rule here is YCbCr's alone, so an RGB file
    # is refused, not decoded into wrong colours.
    if nc == 3 and not jfif and adobe == 0:
        return fail(UNSUPPORTED, "an RGB file (Adobe segment with transform 0 and no JFIF segment)")
    if nc == 3 and not jfif and adobe is None and [sof[6], sof[9], sof[12]] == [0x52, 0x47, 0x42]:
        return fail(UNSUPPORTED, "an RGB file (component ids 'R', 'G', 'B' and neither a JFIF nor an Adobe segment)")
    comps = [(sof[6 + 3 * i], sof[7 + 3 * i] >> 4, sof[7 + 3 * i] & 15, sof[8 + 3 * i]) for i in range(nc)]
    if nc == 1:
        info.layout = 0
        info.hv = [(1, 1)]
    else:
        hv = [(c[1], c[2]) for c in comps]
        if hv[1] != (1, 1) or hv[2] != (1, 1) or hv[0] not in ((2, 2), (1, 1), (2, 1)):
            return fail(UNSUPPORTED, "sampling other than 4:2:0, 4:4:4, 4:2:2")
        info.layout = {(2, 2): LAYOUT_420, (1, 1): LAYOUT_444, (2, 1): LAYOUT_422}[hv[0]]
        info.hv = hv
    if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
        return fail(NOT_JPEG, "bad SOS")
    if seg[0] != nc:
        return fail(UNSUPPORTED, "a non-interleaved or multi-scan file")
    for i in range(nc):
        cs, tt = seg[1 + 2 * i], seg[2 + 2 * i]
        if cs != comps[i][0]:
            return fail(UNSUPPORTED, "the scan's components are not the frame's, in order")
        td, ta = tt >> 4, tt & 15
        if comps[i][3] not in qt or (0, td) not in ht or (1, ta) not in ht:
            return fail(UNSUPPORTED, "a missing table")
        info.q.append(qt[comps[i][3]])
        info.dc.append(ht[(0, td)])
        info.ac.append(ht[(1, ta)])
    if seg[-3] != 0 or seg[-2] != 63 or seg[-1] != 0:
        return fail(UNSUPPORTED, "a spectral selection or successive approximation")
    info.scan = p
    if expect is not None and (int(expect[0]) != info.width or int(expect[1]) != info.height):
        return fail(SIZE_MISMATCH, "the stream is %d x %d" % (info.width, info.height))
    info.status, info.message = OK, ""
    return info


def geometry(info):
    """(blocks per MCU, MCU width, MCU height, MCUs across, MCUs down, component of each block of an MCU)"""
    if info.components == 1:
        bpm, mw, mh, comp_of = 1, 8, 8, [0]
    elif info.layout == LAYOUT_444:
        bpm, mw, mh, comp_of = 3, 8, 8, [0, 1, 2]
    elif info.layout == LAYOUT_422:
        bpm, mw, mh, comp_of = 4, 16, 8, [0, 0, 1, 2]
    else:
        bpm, mw, mh, comp_of = 6, 16, 16, [0, 0, 0, 0, 1, 2]
    return bpm, mw, mh, -(-info.width // mw), -(-info.height // mh), comp_of


_MARK = re.compile(rb"\xFF+([\x00-\xFE])")
_STUFF = re.compile(rb"\xFF+\x00")


def segments(d, p):
    """The scan from byte p as [(entropy-coded bytes with the stuffed zeros and fill bytes removed, the marker behind
    them)]: up to the first marker that is no RSTm, or the stream's end (then 0xD9)."""
    out, start = [], p
    for m in _MARK.finditer(d, p):
        mk = m.group(1)[0]
        if mk == 0:
            continue
        out.append((_STUFF.sub(b"\xFF", d[start:m.start()]), mk))
        start = m.end()
        if not 0xD0 <= mk <= 0xD7:
            return out
    out.append((_STUFF.sub(b"\xFF", d[start:].rstrip(b"\xFF")), 0xD9))
    return out


def _windows(seg):
    """for every bit position of the segment the 16 bits from it on (zeros behind the end), and the number of bits"""
    bits = np.unpackbits(np.frombuffer(seg, np.uint8)).astype(np.uint32)
    n = len(bits)
    bits = np.concatenate([bits, np.zeros(16, np.uint32)])
    win = np.zeros(n + 1, np.uint32)
    for j in range(16):
        win += bits[j:j + n + 1] << (15 - j)
    return win.tolist(), n


def _lut(bits, vals):
    """16 bits -> (symbol, code length), length 0 where no code begins"""
    sym, length = np.zeros(65536, np.int64), np.zeros(65536, np.int64)
    code, k = 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            if k < len(vals) and code < (1 << n):
                lo = code << (16 - n)
                sym[lo:lo + (1 << (16 - n))] = vals[k]
                length[lo:lo + (1 << (16 - n))] = n
            code += 1
            k += 1
        code <<= 1
    return sym.tolist(), length.tolist()


def coefficients(info, data):
    """(status, (n_mcus, blocks per MCU, 64) int64 coefficients in NATURAL order, the DC being values, not differences)"""
    bpm, mw, mh, mx, my, comp_of = geometry(info)
    n_mcus = mx * my
    out = np.zeros((n_mcus, bpm, 64), np.int64)
    dcs = [_lut(*t) for t in info.dc]
    acs = [_lut(*t) for t in info.ac]
    segs = segments(bytes(data), info.scan)
    ri = info.restart if info.restart else n_mcus
    zigzag = ZIGZAG.tolist()
    if len(segs) != -(-n_mcus // ri):
        return DAMAGED, out  # a missing RSTm, or one too many
    scratch = np.zeros(64, np.int64)
    BAD, SHORT = "bad", "short"

    def block(win, n, pos, comp, blk, pred):
        """one block from bit `pos` of a segment of n bits: (the bit behind it, the DC value); BAD for sixteen bits that are
        no code, a category above 11 or an index beyond 63; SHORT where the segment ends inside the block"""
        dsym, dlen = dcs[comp]
        asym, alen = acs[comp]
        w = win[pos] if pos <= n else 0
        s, l = dsym[w], dlen[w]
        if l == 0:
            return BAD if pos + 16 <= n else SHORT
        pos += l
        if pos > n:
            return SHORT
        if s > 11:
            return BAD
        if pos + s > n:
            return SHORT
        diff = 0
        if s:
            diff = win[pos] >> (16 - s)
            if diff < (1 << (s - 1)):
                diff -= (1 << s) - 1
            pos += s
        pred = (pred + diff + 2 ** 31) % 2 ** 32 - 2 ** 31
        blk[0] = min(max(pred, -32768), 32767)
        z = 1
        while z < 64:
            if pos > n:
                return SHORT
            w = win[pos]
            rs, l = asym[w], alen[w]
            if l == 0:
                return BAD if pos + 16 <= n else SHORT
            pos += l
            if pos > n:
                return SHORT
            run, s = rs >> 4, rs & 15
            if s == 0:
                if run != 15:
                    break
                z += 16
                continue
            z += run
            if z > 63:
                return BAD
            if pos + s > n:
                return SHORT
            v = win[pos] >> (16 - s)
            if v < (1 << (s - 1)):
                v -= (1 << s) - 1
            pos += s
            blk[zigzag[z]] = v
            z += 1
        return BAD if z > 64 else (pos, pred)

    for i, (seg, marker) in enumerate(segs):
        last = i == len(segs) - 1
        if not last and marker != 0xD0 + (i & 7):
            return DAMAGED, out
        win, n = _windows(seg)
        pos = 0
        pred = [0, 0, 0]
        for m in range(i * ri, min(n_mcus, (i + 1) * ri)):
            for k, comp in enumerate(comp_of):
                got = block(win, n, pos, comp, out[m, k], pred[comp])
                if got is BAD or got is SHORT:
                    return DAMAGED, out
                pos, pred[comp] = got
        if not last and n - pos >= 8:
            return DAMAGED, out  # whole bytes of data where the interval's end is due
        if not last and n > pos and win[pos] >> (16 - (n - pos)) != (1 << (n - pos)) - 1:
            # In front of an RSTm the padding is 1-bits (T.81 F.1.2.3).  Only 1-bits are never a code, so only they tell a
            # decoder that starts in the middle of the scan that the interval has ended: any other padding is damage.  In
            # front of EOI any padding is taken (the symbol it begins runs over the end).
            return DAMAGED, out
        if last and block(win, n, pos, comp_of[0], scratch, 0) is not SHORT:
            return DAMAGED, out  # behind the last MCU one more whole block (more MCUs than the frame has), or no code
    return OK, out


def idct(coefs, q):
    """(..., 64) natural-order coefficients and 64 divisors -> (..., 8, 8) samples 0..255"""
    f = np.clip(np.asarray(coefs, np.int64) * np.asarray(q, np.int64), -COEF_LIMIT, COEF_LIMIT)
    f = f.reshape(f.shape[:-1] + (8, 8))                                 # f[v][u]
    a = (f @ DCT + (1 << (IDCT_MID_SHIFT - 1))) >> IDCT_MID_SHIFT        # a[v][x] = sum_u T[u][x] f[v][u]
    a = np.clip(a, -MID_LIMIT, MID_LIMIT)
    assert np.abs(f).max(initial=0) * 21641 < 2 ** 31 and np.abs(a).max(initial=0) * 21641 + (1 << 18) < 2 ** 31
    b = DCT.T @ a                                                        # b[y][x] = sum_v T[v][y] a[v][x]
    return np.clip(((b + (1 << (IDCT_END_SHIFT - 1))) >> IDCT_END_SHIFT) + 128, 0, 255)


def _plane(blocks, bx, by):
    """(by, bx, 8, 8) -> (8 by, 8 bx)"""
    return blocks.reshape(by, bx, 8, 8).transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def component_planes(info, coefs, only_luma=False):
    """the components' planes at their own sizes (luminance w x h; chrominance ceil(w / 2) x ... where subsampled)"""
    bpm, mw, mh, mx, my, comp_of = geometry(info)
    w, h = info.width, info.height
    if info.components == 1:
        return [_plane(idct(coefs[:, 0], info.q[0]), mx, my)[:h, :w]]
    ny = comp_of.count(0)
    hs, vs = (2 if mw == 16 else 1), (2 if mh == 16 else 1)
    yb = idct(coefs[:, :ny], info.q[0]).reshape(my, mx, vs, hs, 8, 8).transpose(0, 2, 1, 3, 4, 5)
    planes = [_plane(yb.reshape(-1, 8, 8), mx * hs, my * vs)[:h, :w]]
    if only_luma:
        return planes
    cw, ch = -(-w // hs), -(-h // vs)
    for c in (1, 2):
        planes.append(_plane(idct(coefs[:, ny + c - 1], info.q[c]), mx, my)[:ch, :cw])
    return planes


def upsample(plane, w, h, hs, vs):
    """centred triangle filters, the edges replicated at the component's own size"""
    p = np.asarray(plane, np.int64)
    ch, cw = p.shape
    if hs == 1 and vs == 1:
        return p
    x = np.arange(w)
    nx = x >> 1
    fx = np.clip(nx + np.where(x & 1, 1, -1), 0, cw - 1)
    if vs == 1:
        return (3 * p[:, nx] + p[:, fx] + 2) >> 2
    y = np.arange(h)
    ny = y >> 1
    fy = np.clip(ny + np.where(y & 1, 1, -1), 0, ch - 1)
    near, far = p[ny], p[fy]
    return (9 * near[:, nx] + 3 * near[:, fx] + 3 * far[:, nx] + far[:, fx] + 8) >> 4


def rgb(y, cb, cr):
    """the IJG fixed-point inverse of the encoder's rule"""
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(data, fmt="u8x3", expect=None):
    """(status, picture or None).  A status of 4 comes with no picture: the device leaves such an extent unspecified."""
    info = probe(data, expect)
    if info.status != OK:
        return info.status, None
    status, coefs = coefficients(info, data)
    if status != OK:
        return status, None
    w, h = info.width, info.height
    planes = component_planes(info, coefs, only_luma=fmt == "u8")
    if fmt == "u8":
        return OK, planes[0].astype(np.uint8)
    if info.components == 1:
        g = planes[0].astype(np.uint8)
        return OK, np.ascontiguousarray(np.stack([g, g, g], axis=-1))
    hs = 1 if info.layout == LAYOUT_444 else 2
    vs = 2 if info.layout == LAYOUT_420 else 1
    cb, cr = (upsample(p, w, h, hs, vs) for p in planes[1:])
    return OK, np.ascontiguousarray(rgb(planes[0].astype(np.int64), cb, cr))
