"""Pure-numpy restatement of lr_decode_jpeg_device with LR_JPEG_SCALED: a baseline JPEG stream
to the picture at 1/N of its size, N = 1, 2, 4 or 8, in integers throughout.  No PIL, no GPU.

    scaled_size(n, N)                                        -> ceil(n / N)
    probe_row(data, N, any_sampling=True, orient=False)      -> the row of info the library gives for the file at scale N
    average(samples, rx, ry)                                 -> the reduced samples of a plane of whole blocks
    decode(data, N, fmt="u8x3", any_sampling=True, orient=False) -> (status, picture or None)

The header walk, the entropy decoder, the inverse DCT, the upsampling rule and the colour rule are those of
numpy_jpeg_sampling_ref and numpy_jpeg_decode_ref, the orientation numpy_jpeg_orient_ref's; what is written here is what the
option adds.  For component i and each axis on its own, with rho the ratio of the largest sampling factor to the
component's: d = min(N, rho), r = N / d reduces the component's blocks, rho' = rho / d is the upsampling that is left.

    S'[Y][X] = (sum over j < ry, i < rx of S[Y ry + j][X rx + i] + rx ry / 2) >> log2(rx ry)

over the component's UNCROPPED samples (whole blocks, as the transform leaves them), cropped to ceil(cw / rx) x ceil(ch / ry)
afterwards and upsampled by rho' to the reduced picture, ceil(w / N) x ceil(h / N).  N = 1 is numpy_jpeg_sampling_ref.decode.
"""
import numpy as np

import numpy_jpeg_decode_ref as D
import numpy_jpeg_orient_ref as O
import numpy_jpeg_sampling_ref as S

OK = D.OK
SCALED = 0x80000  # LR_JPEG_SCALED
SCALES = (1, 2, 4, 8)


def scaled_size(n, N):
    return -(-n // N)


def probe_row(data, N, any_sampling=True, orient=False):
    """info's row in probe mode with the bit and entry [6] = N: the sizes are the reduced picture's, swapped after the
    reduction for the orientations 5 .. 8"""
    row = S.info_row(data, any_sampling)
    row[0], row[1] = scaled_size(row[0], N), scaled_size(row[1], N)
    if orient:
        row[7] = max(O.exif_orientation(data), 1)
        if row[7] >= 5:
            row[0], row[1] = row[1], row[0]
    return row


def split(N, ratio):
    """(r, rho'): what of the scale reduces the blocks on an axis of this ratio, and the upsampling that is left"""
    d = min(N, ratio)
    return N // d, ratio // d


def padded_planes(info, coefs, only_luma=False):
    """numpy_jpeg_sampling_ref.component_planes without its crop: every component as whole blocks, (8 my v_i, 8 mx h_i)"""
    bpm, mw, mh, mx, my, comp_of = S.geometry(info)
    hv = [(1, 1)] if info.components == 1 else info.hv
    planes = []
    for i, (h, v) in enumerate(hv[:1] if only_luma else hv):
        first = comp_of.index(i)
        b = D.idct(coefs[:, first:first + h * v], info.q[i]).reshape(my, mx, v, h, 8, 8).transpose(0, 2, 1, 3, 4, 5)
        planes.append(D._plane(b.reshape(-1, 8, 8), mx * h, my * v))
    return planes


def average(samples, rx, ry):
    """cells of rx x ry (each 1, 2, 4 or 8; a cell never straddles two blocks) to their rounded means"""
    s = np.asarray(samples, np.int64)
    h, w = s.shape
    assert h % ry == 0 and w % rx == 0
    sums = s.reshape(h // ry, ry, w // rx, rx).sum(axis=(1, 3))
    return (sums + rx * ry // 2) >> (rx * ry).bit_length() - 1


def decode(data, N, fmt="u8x3", any_sampling=True, orient=False):
    assert N in SCALES
    info = S.probe(data, any_sampling)
    if info.status != OK:
        return info.status, None
    status, coefs = S.coefficients(info, data)
    if status != OK:
        return status, None
    w, h = info.width, info.height
    sw, sh = scaled_size(w, N), scaled_size(h, N)
    hv = [(1, 1)] if info.components == 1 else info.hv
    hmax, vmax = hv[0]
    reduced, left = [], []
    for plane, (ch, cv) in zip(padded_planes(info, coefs, only_luma=fmt == "u8"), hv):
        (rx, ux), (ry, uy) = split(N, hmax // ch), split(N, vmax // cv)
        cw_i, ch_i = -(-w * ch // hmax), -(-h * cv // vmax)
        reduced.append(average(plane, rx, ry)[:-(-ch_i // ry), :-(-cw_i // rx)])
        left.append((ux, uy))
    assert reduced[0].shape == (sh, sw) and left[0] == (1, 1)
    if fmt == "u8":
        out = reduced[0].astype(np.uint8)
    elif info.components == 1:
        out = np.ascontiguousarray(np.stack([reduced[0].astype(np.uint8)] * 3, axis=-1))
    else:
        cb, cr = (S.upsample(p, sw, sh, ux, uy) for p, (ux, uy) in zip(reduced[1:], left[1:]))
        out = np.ascontiguousarray(D.rgb(reduced[0].astype(np.int64), cb, cr))
    return OK, O.orient(out, O.exif_orientation(data)) if orient else out
