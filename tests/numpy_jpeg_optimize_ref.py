"""Pure-numpy restatement of lr_encode_jpeg_device's stream with LR_JPEG_OPTIMIZE: the
stream of numpy_jpeg_ref with Huffman tables built from the frame's own symbol statistics, byte for byte.  No PIL, no GPU.

    encode(image_u8, quality, layout) -> bytes

    statistics(coefs, comp_of, ...)   -> [[dc0, ac0], [dc1, ac1]]: counts of the symbols numpy_jpeg_ref would emit
    code_lengths(counts)              -> (sizes before the limit, BITS after it): Annex K.2 with the K.3 adjustment
    optimal_table(counts)             -> (BITS, HUFFVAL)

Everything else -- coefficients, intervals, header layout, markers -- is numpy_jpeg_ref's.
"""
import numpy as np

import numpy_jpeg_ref as ref

LAYOUT_420, LAYOUT_444 = ref.LAYOUT_420, ref.LAYOUT_444


def _block_symbols(zz, diff, dc, ac):
    """counts the symbols ref._encode_block emits for the block"""
    dc[ref._category(diff)] += 1
    last = 0
    for k in (np.flatnonzero(zz[1:]) + 1).tolist():
        run = k - last - 1
        last = k
        ac[0xF0] += run >> 4
        ac[((run & 15) << 4) | ref._category(zz[k])] += 1
    if last != 63:
        ac[0x00] += 1


def statistics(coefs, comp_of, width, layout):
    """[[dc, ac] of table 0, [dc, ac] of table 1]: lists of 256 counts (Python integers: no width to overflow), over all restart
    intervals, the DC prediction reset at every one; a dummy block counts DC category 0 and an EOB"""
    components = 1 if len(comp_of) == 1 else 3
    ri = ref.restart_interval(width, layout, components)
    counts = [[[0] * 256, [0] * 256], [[0] * 256, [0] * 256]]
    pred = [0, 0, 0]
    for m in range(len(coefs)):
        if m % ri == 0:
            pred = [0, 0, 0]
        for k, comp in enumerate(comp_of):
            zz = coefs[m, k]
            dc, ac = counts[0 if comp == 0 else 1]
            if int(zz[0]) == ref.DUMMY:
                _block_symbols(zz, 0, dc, ac)
            else:
                _block_symbols(zz, int(zz[0]) - pred[comp], dc, ac)
                pred[comp] = int(zz[0])
    return counts


def code_sizes(counts):
    """Annex K.2 as the IJG library does it: the code length (up to 32 and beyond) of every symbol and of the 257th
    pseudo-symbol, whose count of 1 keeps the all-ones code from every real symbol.  The two least frequent entries are
    merged (the first the least frequent, the second the least frequent of the others; of equal counts the larger index),
    and every member of both chains gets one more bit."""
    freq = [int(c) for c in counts] + [1]
    assert len(freq) == 257
    size = [0] * 257
    others = [-1] * 257

    def least(skip):
        best = -1
        for i, f in enumerate(freq):
            if f and i != skip and (best < 0 or f <= freq[best]):
                best = i
        return best

    while True:
        c1 = least(-1)
        c2 = least(c1)
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        size[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            size[c1] += 1
        others[c1] = c2  # the chain of c2 is hung behind the chain of c1
        size[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            size[c2] += 1
    return size


def limit_lengths(size):
    """BITS (index 1 .. 16) from the sizes: the K.3 adjustment from the longest length (IJG starts at 32 and gives up on a
    longer one; counts like Fibonacci numbers over 40 symbols, which a large frame can have, need more, and the same step
    serves them) down to 17, then the pseudo-symbol's code leaves the longest length"""
    top = max(32, max(size))
    bits = [0] * (top + 1)
    for s in size:
        if s:
            bits[s] += 1
    for i in range(top, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    return bits[1:17]


def optimal_table(counts):
    """(BITS, HUFFVAL): the symbols that occur, by their length before the limit and within one by ascending value -- the
    IJG order; lengths after the limit follow from BITS"""
    size = code_sizes(counts)
    bits = limit_lengths(size)
    vals = [s for _, s in sorted((size[s], s) for s in range(256) if size[s])]
    assert sum(bits) == len(vals)
    return bits, vals


def header(width, height, quality, layout, components, tables):
    """numpy_jpeg_ref.header with the DHT payloads replaced; tables = [(dc, ac) of table 0, (dc, ac) of table 1], each a
    (BITS, HUFFVAL)"""
    std = ref.header(width, height, quality, layout, components)
    first = std.index(b"\xFF\xC4")
    tail = std.index(b"\xFF\xDD")
    out = std[:first]
    for t in range(2 if components == 3 else 1):
        for cls in (0, 1):
            bits, vals = tables[t][cls]
            out += ref._segment(0xC4, bytes([cls << 4 | t]) + bytes(bits) + bytes(vals))
    return out + std[tail:]


def tables_of(coefs, comp_of, width, layout):
    counts = statistics(coefs, comp_of, width, layout)
    n = 1 if len(comp_of) == 1 else 2
    return counts, [(optimal_table(counts[t][0]), optimal_table(counts[t][1])) for t in range(n)]


def encode_coefficients(coefs, comp_of, width, height, quality, layout):
    components = 1 if len(comp_of) == 1 else 3
    _, tables = tables_of(coefs, comp_of, width, layout)
    tabs = [(ref.huff_table(*dc), ref.huff_table(*ac)) for dc, ac in tables]
    ri = ref.restart_interval(width, layout, components)
    out = [header(width, height, quality, layout, components, tables)]
    n_mcus = len(coefs)
    n_int = -(-n_mcus // ri)
    for i in range(n_int):
        pred = [0, 0, 0]
        acc, n = 0, 0
        for m in range(i * ri, min(n_mcus, (i + 1) * ri)):
            for k, comp in enumerate(comp_of):
                zz = coefs[m, k]
                dc, ac = tabs[0 if comp == 0 else 1]
                if int(zz[0]) == ref.DUMMY:
                    a, l = ref._encode_block(zz, 0, dc, ac)
                else:
                    a, l = ref._encode_block(zz, int(zz[0]) - pred[comp], dc, ac)
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
    coefs, comp_of = ref.coefficients(img, quality, layout)
    return encode_coefficients(coefs, comp_of, w, h, quality, layout)


def bound(width, height, components, layout):
    """lr_jpeg_bound with LR_JPEG_OPTIMIZE: a block is at most 27 + 63 * 26 = 1665 bits, 418 bytes with every byte stuffed"""
    mw = 16 if components == 3 and layout == LAYOUT_420 else 8
    bpm = 1 if components == 1 else (6 if layout == LAYOUT_420 else 3)
    n_mcus = (-(-width // mw)) * (-(-height // mw))
    ri = ref.restart_interval(width, layout, components)
    return 640 + 2 * (-(-n_mcus // ri)) + 418 * n_mcus * bpm
