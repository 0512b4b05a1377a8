"""Pure-numpy restatement of lr_decode_jpeg_device with LR_JPEG_ANY_SAMPLING: a baseline JPEG
stream of any sampling whose factors are 1, 2 or 4 to pixels, in integers throughout.  No PIL, no GPU.

    probe(data, any_sampling=True)              -> Info: numpy_jpeg_decode_ref's, layout being info [3] of the library
    decode(data, fmt="u8x3", any_sampling=True, orient=False) -> (status, picture or None)

The header walk, the entropy decoder, the inverse DCT and the colour rule are numpy_jpeg_decode_ref's; what is written here is
what the option adds: the admission rule, the geometry of ITU T.81 A.1.1 and A.2.3 for arbitrary factors, and the
upsampling rule per axis (ratio 1: the sample; 2: the centred triangle; 4: replication).  On the three layouts that need no
option all of it comes down to numpy_jpeg_decode_ref.decode, byte for byte (tests/test_jpeg_sampling_cpu.py holds it to that).
"""
import numpy as np

import numpy_jpeg_decode_ref as D
import numpy_jpeg_orient_ref as O

OK, UNSUPPORTED = D.OK, D.UNSUPPORTED
ANY_SAMPLING = 0x20000  # LR_JPEG_ANY_SAMPLING
SAMPLING_MESSAGE = "sampling other than 4:2:0, 4:4:4, 4:2:2"


def sof_sampling(d):
    """offset of the first component's sampling byte in the stream's first SOF0/SOF1 segment (the walk of T.81 B.1.1.2: a
    marker, a 16-bit length), or None"""
    p, n = 2, len(d)
    while p + 4 <= n and d[p] == 0xFF:
        while p < n and d[p] == 0xFF:
            p += 1
        if p >= n:
            return None
        m = d[p]
        p += 1
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m in (0xD9, 0xDA) or p + 2 > n:
            return None
        length = (d[p] << 8) | d[p + 1]
        if m in (0xC0, 0xC1):
            return p + 2 + 7 if length >= 8 + 3 * 3 and p + length <= n else None
        p += length
    return None


def admitted(hv):
    """the option's rule for three components' (h, v)"""
    if any(f not in (1, 2, 4) for c in hv for f in c):
        return False
    if any(c[0] > hv[0][0] or c[1] > hv[0][1] for c in hv):
        return False  # the luminance has the largest factors; the ratios are then 1, 2 or 4 of themselves
    return sum(h * v for h, v in hv) <= 10  # T.81 B.2.3


def probe(data, any_sampling=True, expect=None):
    d = bytes(data)
    info = D.probe(d, expect)
    if not any_sampling or info.status != UNSUPPORTED or info.message != SAMPLING_MESSAGE:
        return info
    at = sof_sampling(d)
    hv = [(d[at + 3 * i] >> 4, d[at + 3 * i] & 15) for i in range(3)]
    if not admitted(hv):
        return info
    # every other check is that of a file with these tables and this scan whose header says 4:4:4
    as444 = bytearray(d)
    as444[at] = as444[at + 3] = as444[at + 6] = 0x11
    info = D.probe(bytes(as444), expect)
    info.hv = hv
    if info.status in (OK, D.SIZE_MISMATCH):
        info.layout = d[at]
    return info


def info_row(data, any_sampling=True):
    return probe(data, any_sampling).row()


def geometry(info):
    """numpy_jpeg_decode_ref.geometry for any factors: (blocks per MCU, MCU width, MCU height, MCUs across, MCUs down,
    component of each block of an MCU).  An MCU's blocks come component by component (T.81 A.2.3)."""
    hv = [(1, 1)] if info.components == 1 else info.hv
    comp_of = [i for i, (h, v) in enumerate(hv) for _ in range(h * v)]
    mw, mh = 8 * hv[0][0], 8 * hv[0][1]
    return len(comp_of), mw, mh, -(-info.width // mw), -(-info.height // mh), comp_of


def coefficients(info, data):
    """numpy_jpeg_decode_ref.coefficients, its sequential entropy decoder walking the MCU of `geometry` above"""
    legacy = D.geometry
    D.geometry = geometry
    try:
        return D.coefficients(info, data)
    finally:
        D.geometry = legacy


def component_planes(info, coefs, only_luma=False):
    """the components' planes at their own sizes, ceil(w h_i / Hmax) x ceil(h v_i / Vmax): component i's blocks of an MCU
    are v_i rows of h_i blocks"""
    bpm, mw, mh, mx, my, comp_of = geometry(info)
    hv = [(1, 1)] if info.components == 1 else info.hv
    hmax, vmax = hv[0]
    planes = []
    for i, (h, v) in enumerate(hv[:1] if only_luma else hv):
        first = comp_of.index(i)
        b = D.idct(coefs[:, first:first + h * v], info.q[i]).reshape(my, mx, v, h, 8, 8).transpose(0, 2, 1, 3, 4, 5)
        plane = D._plane(b.reshape(-1, 8, 8), mx * h, my * v)
        planes.append(plane[:-(-info.height * v // vmax), :-(-info.width * h // hmax)])
    return planes


def _axis(n, ratio, size):
    """for the n output samples of one axis: (near index, far index, whether the triangle applies)"""
    x = np.arange(n)
    if ratio == 2:
        near = x >> 1
        return near, np.clip(near + np.where(x & 1, 1, -1), 0, size - 1), True
    near = x >> (2 if ratio == 4 else 0)
    return near, near, False


def upsample(plane, w, h, rx, ry):
    """per axis by its ratio: 1 the sample, 2 the centred triangle (3 near + far, the edges replicated at the component's
    own size), 4 sample x >> 2; the triangle of one axis is taken over the replicated samples of the other"""
    p = np.asarray(plane, np.int64)
    nx, fx, tx = _axis(w, rx, p.shape[1])
    ny, fy, ty = _axis(h, ry, p.shape[0])
    near, far = p[ny], p[fy]
    if tx and ty:
        return (9 * near[:, nx] + 3 * near[:, fx] + 3 * far[:, nx] + far[:, fx] + 8) >> 4
    if tx:
        return (3 * near[:, nx] + near[:, fx] + 2) >> 2
    if ty:
        return (3 * near[:, nx] + far[:, nx] + 2) >> 2
    return near[:, nx]


def decode(data, fmt="u8x3", any_sampling=True, orient=False, expect=None):
    """(status, picture or None), as numpy_jpeg_decode_ref.decode; orient: upright by the file's EXIF orientation"""
    info = probe(data, any_sampling, expect)
    if info.status != OK:
        return info.status, None
    status, coefs = coefficients(info, data)
    if status != OK:
        return status, None
    w, h = info.width, info.height
    planes = component_planes(info, coefs, only_luma=fmt == "u8")
    if fmt == "u8":
        out = planes[0].astype(np.uint8)
    elif info.components == 1:
        out = np.ascontiguousarray(np.stack([planes[0].astype(np.uint8)] * 3, axis=-1))
    else:
        hmax, vmax = info.hv[0]
        cb, cr = (upsample(p, w, h, hmax // ch, vmax // cv) for p, (ch, cv) in zip(planes[1:], info.hv[1:]))
        out = np.ascontiguousarray(D.rgb(planes[0].astype(np.int64), cb, cr))
    return OK, O.orient(out, O.exif_orientation(data)) if orient else out
