"""A baseline JPEG stream writer for the decoder's tests: its input is the set of quantised
coefficients, which therefore ARE the expected result of a decode, and a spec that says everything an encoder library
decides for its caller.  Pure Python and numpy; no PIL, no decoder of ours, nothing of the encoder's restatement.

    write(coefs, spec) -> (bytes, Log)

coefs   int array (n_mcus, blocks per MCU, 64), natural order, the DC as values (the writer takes the differences).
spec    a dict:
    width, height
    sof          0xC0 or 0xC1
    components   [dict(id=, hv=<sampling byte>, tq=, td=, ta=)], one or three
    layout       the header, segment by segment, as seg(...) items in file order (default_layout builds the usual one):
                   seg("APP", (n, payload))  seg("COM", payload)  seg("RAW", (marker, payload))
                   seg("DQT", [(tq, 64 divisors in natural order), ...])       one segment, its tables in this order
                   seg("DHT", [(tc, th, (bits, vals)), ...])                   tc 0 DC, 1 AC
                   seg("DRI", value)  seg("SOF")  seg("SOS")
                 every item takes fill=<number of extra 0xFF in front of its marker> and, for APP, COM and RAW,
                 length=<the length field, if not the payload's>.  A table defined twice: the later one holds; the DRI
                 that holds is the last one.  SOS is the last item.
    fill_rst     extra 0xFF in front of RSTm: an int, or {interval index: count}
    fill_eoi     extra 0xFF in front of EOI
    pad_rst      the padding bits in front of RSTm: "ones", "zeros", "alt" (1010...), "alt0" (0101...), or {index: one of them}
    pad_eoi      the same in front of EOI
    eoi          False: no EOI
    tail         bytes behind EOI

Log     positions are bit addresses in the FILE, 8 * byte + bit, the byte being the one that holds the bit (a stuffed zero is
        never one):
    scan         the scan's first byte
    sym_pos, sym_c, sym_z    for every symbol its first bit, the block of the MCU and the zig-zag index it begins at
    sym_val      the first of its extra bits, -1 if it has none
    mcu_pos      for every MCU its first bit
    pad          for every interval (the last one: in front of EOI) the number of padding bits
    end          the byte behind the last entropy-coded byte of each interval (where the fill bytes or the marker begin)
    eoi          the offset of EOI's 0xFF (the first of its fill bytes), or the length of the stream if there is none
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])  # T.81 figure A.6: natural index of zig-zag position k

# T.81 Annex K.3 (typical tables), as (bits, vals)
STD_DC_LUM = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
STD_DC_CHR = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
STD_AC_LUM = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1,
    0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA,
    0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
    0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
    0xFA])
STD_AC_CHR = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19,
    0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8,
    0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4,
    0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
    0xFA])
assert len(STD_AC_LUM[1]) == sum(STD_AC_LUM[0]) == 162 and len(STD_AC_CHR[1]) == sum(STD_AC_CHR[0]) == 162


def table_from_lengths(lengths):
    """(bits, vals) from [(symbol, code length), ...]: the symbols of a length keep the list's order"""
    bits = [0] * 16
    for _, l in lengths:
        assert 1 <= l <= 16
        bits[l - 1] += 1
    return bits, [s for l in range(1, 17) for s, sl in lengths if sl == l]


def codes(table):
    """{symbol: (code, length)} by T.81 Annex C, with what it demands of a table asserted: the lengths fit (a code of
    length l is below 2^l) and no code is all 1-bits"""
    bits, vals = table
    assert len(bits) == 16 and len(vals) == sum(bits) <= 256 and len(set(vals)) == len(vals)
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            assert code < (1 << l) - 1, "a code of length %d does not fit, or is all 1-bits" % l
            out[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


def seg(name, arg=None, fill=0, length=None):
    return dict(name=name, arg=arg, fill=fill, length=length)


def adobe(transform):
    return seg("APP", (14, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, transform])))


def jfif():
    return seg("APP", (0, b"JFIF\0\1\1\0\0\1\0\1\0\0"))


def default_layout(q, dc, ac, ri=0, extra=()):
    """SOI [extra] DQT (one segment per table) SOF DHT (one segment per table) [DRI] SOS; q, dc, ac: {id: table}"""
    out = list(extra)
    out += [seg("DQT", [(i, t)]) for i, t in sorted(q.items())]
    out.append(seg("SOF"))
    out += [seg("DHT", [(0, i, t)]) for i, t in sorted(dc.items())]
    out += [seg("DHT", [(1, i, t)]) for i, t in sorted(ac.items())]
    if ri:
        out.append(seg("DRI", ri))
    return out + [seg("SOS")]


def blocks_of(spec):
    """the component of every block of an MCU (T.81 A.2.3; a one-component scan is not interleaved: one block)"""
    comps = spec["components"]
    if len(comps) == 1:
        return [0]
    return [i for i, c in enumerate(comps) for _ in range((c["hv"] >> 4) * (c["hv"] & 15))]


def mcu_grid(spec):
    """(MCUs across, MCUs down)"""
    comps = spec["components"]
    hmax, vmax = (1, 1) if len(comps) == 1 else (max(c["hv"] >> 4 for c in comps), max(c["hv"] & 15 for c in comps))
    return -(-spec["width"] // (8 * hmax)), -(-spec["height"] // (8 * vmax))


class Log:
    pass


class _Bits:
    def __init__(self, out):
        self.out, self.acc, self.n = out, 0, 0

    def pos(self):
        return 8 * len(self.out) + self.n

    def put(self, value, length):
        self.acc = (self.acc << length) | value
        self.n += length
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def pad(self, how):
        """fills the byte; returns the number of padding bits"""
        k = (8 - self.n) % 8
        if k:
            pattern = {"ones": 0xFF, "zeros": 0, "alt": 0xAA, "alt0": 0x55}[how]
            self.put(pattern >> (8 - k), k)
        return k


def _which(v, i, default):
    if v is None:
        return default
    return v.get(i, default) if isinstance(v, dict) else v


def write(coefs, spec):
    comps = spec["components"]
    comp_of = blocks_of(spec)
    mx, my = mcu_grid(spec)
    coefs = np.asarray(coefs)
    assert coefs.shape == (mx * my, len(comp_of), 64), (coefs.shape, (mx * my, len(comp_of), 64))
    out = bytearray(b"\xFF\xD8")
    qt, ht, ri = {}, {}, 0
    layout = spec["layout"]
    assert layout[-1]["name"] == "SOS" and sum(s["name"] == "SOF" for s in layout) == 1

    def emit(s, marker, payload):
        length = len(payload) + 2 if s["length"] is None else s["length"]
        out.extend(b"\xFF" * (s["fill"] + 1) + bytes([marker, length >> 8, length & 255]) + payload)

    for s in layout:
        name, arg = s["name"], s["arg"]
        if name == "APP":
            emit(s, 0xE0 + arg[0], arg[1])
        elif name == "COM":
            emit(s, 0xFE, arg)
        elif name == "RAW":
            emit(s, arg[0], arg[1])
        elif name == "DQT":
            body = b""
            for tq, table in arg:
                table = np.asarray(table)
                assert table.shape == (64,) and table.min() >= 1 and table.max() <= 255 and 0 <= tq <= 3
                qt[tq] = table
                body += bytes([tq]) + bytes(table[ZIGZAG].tolist())
            emit(s, 0xDB, body)
        elif name == "DHT":
            body = b""
            for tc, th, table in arg:
                assert tc in (0, 1) and 0 <= th <= 3
                ht[(tc, th)] = codes(table)
                body += bytes([(tc << 4) | th]) + bytes(table[0]) + bytes(table[1])
            emit(s, 0xC4, body)
        elif name == "DRI":
            ri = arg
            emit(s, 0xDD, bytes([arg >> 8, arg & 255]))
        elif name == "SOF":
            body = bytes([8, spec["height"] >> 8, spec["height"] & 255, spec["width"] >> 8, spec["width"] & 255, len(comps)])
            for c in comps:
                body += bytes([c["id"], c["hv"], c["tq"]])
            emit(s, spec.get("sof", 0xC0), body)
        elif name == "SOS":
            body = bytes([len(comps)])
            for c in comps:
                assert c["tq"] in qt and (0, c["td"]) in ht and (1, c["ta"]) in ht, "a component's table is not defined in front of SOS"
                body += bytes([c["id"], (c["td"] << 4) | c["ta"]])
            emit(s, 0xDA, body + bytes([0, 63, 0]))
        else:
            raise ValueError(name)

    log = Log()
    log.scan = len(out)
    log.q = [qt[c["tq"]] for c in comps]
    log.ri = ri
    sym_pos, sym_c, sym_z, sym_val, mcu_pos = [], [], [], [], []
    log.pad, log.end = [], []
    dc = [ht[(0, c["td"])] for c in comps]
    ac = [ht[(1, c["ta"])] for c in comps]
    w = _Bits(out)
    zz = coefs[:, :, ZIGZAG].tolist()
    n_mcus = mx * my
    per = ri if ri else n_mcus
    pred = [0, 0, 0]

    def symbol(table, sym, value, size, c, z):
        code, length = table[sym]  # (KeyError: the table has no code for a symbol the coefficients need)
        sym_pos.append(w.pos())
        sym_c.append(c)
        sym_z.append(z)
        w.put(code, length)
        if size:
            sym_val.append(w.pos())
            w.put(value if value >= 0 else value + (1 << size) - 1, size)
        else:
            sym_val.append(-1)

    for m in range(n_mcus):
        if m and m % per == 0:
            i = m // per - 1
            log.pad.append(w.pad(_which(spec.get("pad_rst"), i, "ones")))
            log.end.append(len(out))
            out.extend(b"\xFF" * (_which(spec.get("fill_rst"), i, 0) + 1) + bytes([0xD0 + (i & 7)]))
            pred = [0, 0, 0]
        mcu_pos.append(w.pos())
        for c, comp in enumerate(comp_of):
            blk = zz[m][c]
            diff = blk[0] - pred[comp]
            pred[comp] = blk[0]
            size = abs(diff).bit_length()
            assert size <= 11, "a DC difference beyond category 11"
            symbol(dc[comp], size, diff, size, c, 0)
            last = max([k for k in range(1, 64) if blk[k]], default=0)
            run = 0
            for k in range(1, last + 1):
                v = blk[k]
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    symbol(ac[comp], 0xF0, 0, 0, c, k - run)
                    run -= 16
                size = abs(v).bit_length()
                assert size <= 10, "an AC coefficient beyond category 10"
                symbol(ac[comp], (run << 4) | size, v, size, c, k - run)
                run = 0
            if last < 63:
                symbol(ac[comp], 0x00, 0, 0, c, last + 1)
    log.pad.append(w.pad(spec.get("pad_eoi") or "ones"))
    log.end.append(len(out))
    log.eoi = len(out)
    if spec.get("eoi", True):
        out.extend(b"\xFF" * (spec.get("fill_eoi", 0) + 1) + b"\xD9")
    out.extend(spec.get("tail", b""))
    log.sym_pos, log.sym_c, log.sym_z, log.sym_val = (np.array(a, np.int64) for a in (sym_pos, sym_c, sym_z, sym_val))
    log.mcu_pos = np.array(mcu_pos, np.int64)
    return bytes(out), log
