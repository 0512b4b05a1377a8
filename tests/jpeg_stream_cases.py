"""The streams of tests/test_jpeg_streams_cpu.py and tests/test_gpu_jpeg_streams.py, built symbol by symbol with
tests/jpeg_stream_writer.py.  A case is its coefficients (the truth), its spec, its stream, the writer's log, the status the
decoder owes it, and `reach`: what the case claims to reach, asserted on the log alone (no decoder involved).

    names()          every case's name, in a fixed order
    get(name)        the case, built once
    lane_exit(...)   a sequential model of one lane of the entropy decoder's first launch, for the reach assertions

A case that needs a property takes it from a deterministic construction or a search over seeds; either way `reach` asserts
it.  Every case keeps its dequantised amplitudes within +-300 (the range of test_idct_is_within_one_level_of_float64), except
`dc_category_11`, whose blocks are DC alone (there every inverse transform is the same rounding of DC / 8).
"""
import numpy as np

import jpeg_stream_writer as W

PART, WG = 128, 256 * 128  # bytes of a lane's part and of a workgroup's parts (kernels_jpeg_decode.hip)
OK, UNSUPPORTED, DAMAGED = 0, 2, 4
Q2, Q3 = np.full(64, 2), np.full(64, 3)
DC_LUM, AC_LUM = W.codes(W.STD_DC_LUM), W.codes(W.STD_AC_LUM)


class Case:
    def __init__(self, name, coefs, spec, status=OK, any_sampling=False, reach=None, message=None):
        """message: for a case of status 2, a word that the reason given must hold"""
        self.name, self.coefs, self.spec, self.status, self.any_sampling = name, np.asarray(coefs, np.int64), spec, status, any_sampling
        self.message = message
        self.stream, self.log = W.write(self.coefs, spec)
        self._reach = reach

    def reach(self):
        if self._reach is not None:
            self._reach(self)

    @property
    def scan_bytes(self):
        """the scan's bytes up to EOI (its fill bytes not counted)"""
        return self.log.eoi - self.log.scan

    @property
    def n_parts(self):
        return max(1, -(-(len(self.stream) - self.log.scan) // PART))

    def segments(self):
        """the header as the file has it: [(marker, length field, payload)] from behind SOI up to and with SOS"""
        d, p, out = self.stream, 2, []
        while True:
            assert d[p] == 0xFF
            while d[p] == 0xFF:
                p += 1
            length = (d[p + 1] << 8) | d[p + 2]
            out.append((d[p], length, d[p + 3:p + 1 + length]))
            p += 1 + length
            if out[-1][0] == 0xDA:
                assert p == self.log.scan
                return out

    def tables(self, marker):
        """the tables of the DQT (0xDB) or DHT (0xC4) segments in file order: [(index of the segment, id byte, contents)]"""
        out = []
        for i, (m, _, body) in enumerate(self.segments()):
            s = 0
            while m == marker and s < len(body):
                n = 65 if marker == 0xDB else 17 + sum(body[s + 1:s + 17])
                out.append((i, body[s], body[s + 1:s + n]))
                s += n
        return out

    def sof(self):
        """(index of the segment, marker, [(id, sampling byte, tq)])"""
        for i, (m, _, body) in enumerate(self.segments()):
            if m in (0xC0, 0xC1):
                return i, m, [tuple(body[6 + 3 * k:9 + 3 * k]) for k in range(body[5])]


# ---- specs ----

def gray(w, h, q=Q3, dc=W.STD_DC_LUM, ac=W.STD_AC_LUM, ri=0, cid=1, hv=0x11, extra=(), layout=None, **scan):
    spec = dict(width=w, height=h, components=[dict(id=cid, hv=hv, tq=0, td=0, ta=0)])
    spec["layout"] = layout or W.default_layout({0: q}, {0: dc}, {0: ac}, ri, extra)
    spec.update(scan)
    return spec


def rotated(table, by):
    """the same lengths, other symbols under them"""
    bits, vals = table
    return bits, vals[by:] + vals[:by]


DC_THIRD = W.table_from_lengths([(4, 2), (5, 2), (3, 2), (6, 3), (2, 4), (7, 5), (1, 6), (8, 7), (0, 8), (9, 9), (10, 10), (11, 11)])
THREE_Q = {1: Q3, 2: np.full(64, 5), 3: np.full(64, 7)}
THREE_DC = {3: W.STD_DC_LUM, 0: W.STD_DC_CHR, 2: DC_THIRD}
THREE_AC = {2: W.STD_AC_LUM, 3: W.STD_AC_CHR, 1: rotated(W.STD_AC_LUM, 40)}


def colour(w, h, hv=(0x11, 0x11, 0x11), ids=(1, 2, 3), three=False, sof=0xC0, ri=0, extra=(), layout=None, **scan):
    if three:  # three different table sets, under ids that are not the components' indices
        comps = [dict(id=ids[0], hv=hv[0], tq=1, td=3, ta=2), dict(id=ids[1], hv=hv[1], tq=2, td=0, ta=3), dict(id=ids[2], hv=hv[2], tq=3, td=2, ta=1)]
        tables = (THREE_Q, THREE_DC, THREE_AC)
    else:
        comps = [dict(id=ids[0], hv=hv[0], tq=0, td=0, ta=0), dict(id=ids[1], hv=hv[1], tq=1, td=1, ta=1), dict(id=ids[2], hv=hv[2], tq=1, td=1, ta=1)]
        tables = ({0: Q3, 1: np.full(64, 4)}, {0: W.STD_DC_LUM, 1: W.STD_DC_CHR}, {0: W.STD_AC_LUM, 1: W.STD_AC_CHR})
    spec = dict(width=w, height=h, components=comps, sof=sof)
    spec["layout"] = layout(*tables) if layout else W.default_layout(*tables, ri=ri, extra=extra)
    spec.update(scan)
    return spec


def shape_of(spec):
    mx, my = W.mcu_grid(spec)
    return mx * my, len(W.blocks_of(spec))


def texture(seed, spec, amp=40, keep=0.12, dc=60):
    """sparse random coefficients: |c| <= amp, the DC within +-dc"""
    rng = np.random.default_rng(seed)
    n, bpm = shape_of(spec)
    c = rng.integers(-amp, amp + 1, (n, bpm, 64)) * (rng.random((n, bpm, 64)) < keep)
    c[:, :, 0] = rng.integers(-dc, dc + 1, (n, bpm))
    return c


# ---- steering: a gray scan with the typical tables whose bits land where a case wants them ----

def ac_len(s):
    return AC_LUM[s][1] + s


def plan(rng, bits):
    """sizes s of AC symbols (run 0) whose lengths add up to `bits` exactly; at most 60 of them"""
    out, rem = [], bits
    assert rem == 0 or rem in (3, 4) or rem >= 6
    while rem:
        want = [s for s in range(1, 6) if rem - ac_len(s) in (0, 3, 4) or rem - ac_len(s) >= 6]
        if rem > 7 * (58 - len(out)):
            want = want[-2:]
        s = int(rng.choice(want))
        out.append(s)
        rem -= ac_len(s)
    assert len(out) <= 60
    return out


def block_of(rng, sizes, values=None):
    """a block (natural order) whose AC symbols are (0, s) for the sizes, then EOB; the DC is left 0"""
    zz = np.zeros(64, np.int64)
    for k, s in enumerate(sizes):
        v = int(rng.integers(1 << (s - 1), 1 << s)) * int(rng.choice([-1, 1]))
        zz[1 + k] = values[k] if values and values[k] is not None else v
    blk = np.zeros(64, np.int64)
    blk[W.ZIGZAG] = zz
    return blk


def steered(seed, n_mcus, target_of, tail, q=np.ones(64, np.int64)):
    """A one-row gray picture of random blocks in which one block is rebuilt so that, counted from the scan's first byte, its
    symbols end exactly `tail(rng)[0]` bits in front of bit target_of(log) and are followed by the symbols tail gives as
    (size, value).  Returns (coefs, spec, index of the rebuilt MCU)."""
    spec = gray(8 * n_mcus, 8, q=q)
    coefs = texture(seed, spec)
    rng = np.random.default_rng(seed + 1000)
    _, log = W.write(coefs, spec)
    target = target_of(log)
    m = int(np.searchsorted(log.mcu_pos, target - 70, side="right")) - 1
    assert m >= 1
    before, after = tail(rng)
    sizes = plan(rng, target - int(log.mcu_pos[m]) - DC_LUM[0][1] - before)
    blk = block_of(rng, sizes + [s for s, _ in after], [None] * len(sizes) + [v for _, v in after])
    blk[0] = coefs[m - 1, 0, 0]  # a DC difference of 0
    coefs[m, 0] = blk
    return coefs, spec, m


def edge_case(name, B, mode, seed):
    """mode: "end" a symbol ends exactly on byte B of the scan; "straddle" a code lies across it; "split" a code ends there
    and its extra bits begin behind it; "stuffed" byte B - 1 is a data byte 0xFF and byte B its stuffed zero"""
    tails = {"end": lambda rng: (0, [(2, None)]),
             "straddle": lambda rng: (1, [(1, None)]),
             "split": lambda rng: (AC_LUM[3][1], [(3, None)]),
             "stuffed": lambda rng: (AC_LUM[8][1] + 8, [(8, 255)])}
    n_mcus = max(24, (B + 700) // 20)

    def reach(case):
        log, at = case.log, 8 * (case.log.scan + B)
        i = int(np.searchsorted(log.sym_pos, at, side="right")) - 1  # the symbol that holds, or begins at, bit `at`
        if mode == "end":
            assert log.sym_pos[i] == at
        elif mode == "straddle":
            assert log.sym_pos[i] < at < log.sym_val[i] and (at - log.sym_pos[i]) < 16
        elif mode == "split":
            assert log.sym_val[i] == at
        else:
            assert case.stream[log.scan + B - 1] == 0xFF and case.stream[log.scan + B] == 0
        assert case.scan_bytes > B + 16

    for s in range(seed, seed + 20):  # (a stuffed byte among the steering symbols moves what lies behind it: then the next seed)
        coefs, spec, _ = steered(s, n_mcus, lambda log: 8 * (log.scan + B), tails[mode])
        case = Case(name, coefs, spec, reach=reach)
        try:
            case.reach()
            return case
        except AssertionError:
            continue
    raise AssertionError(name + ": no seed reaches the edge")


def sized_case(name, N, seed):
    """a scan of exactly N bytes up to EOI"""
    def reach(case):
        assert case.scan_bytes == N, (case.scan_bytes, N)
        assert case.n_parts == -(-(N + 2) // PART) == SIZES[N]
        if N in (126, 32766, 65534):
            assert len(case.stream) - case.log.scan == PART * SIZES[N], "the last part, EOI in it, is full"

    if N == 1:
        return Case(name, np.zeros((1, 1, 64)), gray(8, 8), reach=reach)
    for s in range(seed, seed + 20):
        spec = gray(8 * (N // 10 + 40), 8, q=Q2)
        coefs = texture(s, spec)
        _, log = W.write(coefs, spec)
        m = int(np.searchsorted(log.mcu_pos, 8 * (log.scan + N) - 90, side="right")) - 1
        assert 1 <= m < len(coefs) - 1
        rng = np.random.default_rng(s + 1000)
        sizes = plan(rng, 8 * (log.scan + N) - int(log.mcu_pos[m]) - DC_LUM[0][1] - AC_LUM[0][1] - 3)  # EOB, 3 bits of padding
        coefs = coefs[:m + 1]
        coefs[m, 0] = block_of(rng, sizes)
        coefs[m, 0, 0] = coefs[m - 1, 0, 0]
        case = Case(name, coefs, gray(8 * (m + 1), 8, q=Q2), reach=reach)
        if case.scan_bytes == N:
            return case
    raise AssertionError(name + ": no seed gives the size")


# ---- a sequential model of one lane's first decode ----

def decoder_of(table):
    """{(code, length): symbol}"""
    return {v: k for k, v in W.codes(table).items()}


def lane_exit(bits, start, limit, dc, ac, bpm=1):
    """The first launch of the entropy decoder for one lane, on a scan WITHOUT 0xFF bytes (bits: its bits as a string, bit 0
    the scan's first): from the guess (bit `start`, block 0, index 0) symbol by symbol to the first symbol boundary at or
    behind bit `limit`.  Returns (bit, block of the MCU, zig-zag index) there.  Sixteen bits that are no code end the block,
    as in the kernel."""
    pos, c, z = start, 0, 0
    while pos < limit and pos < len(bits):
        table = dc if z == 0 else ac
        sym = None
        for l in range(1, 17):
            sym = table.get((int(bits[pos:pos + l] or "1", 2), l)) if pos + l <= len(bits) else None
            if sym is not None:
                pos += l
                break
        done = False
        if sym is None:
            pos += 16
            done = True
        elif z == 0:
            pos += sym if sym <= 11 else 0
            z = 1
        else:
            run, s = sym >> 4, sym & 15
            if s == 0:
                z += 16 if run == 15 else 0
                done = run != 15 or z >= 64
            else:
                z += run
                if z > 63:
                    done = True
                else:
                    pos += s
                    z += 1
                    done = z == 64
        if done:
            z, c = 0, (c + 1) % bpm
    return pos, c, z


NR_LENGTHS = [(6, 1), (5, 2), (4, 3), (3, 4), (2, 5)]  # size s under a code of 7 - s bits: every symbol is 7 bits
NR_DC = W.table_from_lengths(NR_LENGTHS + [(0, 6)])
NR_AC = W.table_from_lengths(NR_LENGTHS + [(0x00, 6)])
NR_FIRST = 10  # AC coefficients of the first block, which ends in EOB: the symbols behind it begin at bit 7 n - 1


def no_resync_case():
    """Blocks with all 63 AC coefficients, every symbol (code and extra bits) 7 bits, the DC table's codes the AC table's, and
    no run of five 1-bits behind the first block: a lane that starts on a guess reads symbols of 7 bits for ever, at its own
    bit phase -- or, where its phase is the true one (every 7th part), at a zig-zag index that is (53 - NR_FIRST) mod 64
    from the true one.  No guess is ever right, and no lane finds the truth by itself."""
    n_blocks = 1200  # 56 bytes each: more than 65 536 bytes, three workgroups
    rng = np.random.default_rng(77)
    codes = W.codes(NR_AC)
    zz = np.zeros((n_blocks, 64), np.int64)
    tail, pred = "0", 0

    def draw(sign=None):
        nonlocal tail
        for _ in range(200):
            s = int(rng.integers(2, 7))
            v = int(rng.integers(1 << (s - 1), 1 << s)) * (sign or int(rng.choice([-1, 1])))
            code, length = codes[s]
            text = format(code, "0%db" % length) + format(v if v > 0 else v + (1 << s) - 1, "0%db" % s)
            if "11111" not in tail[-4:] + text:
                tail = text
                return v
        raise AssertionError("no symbol without a run of five 1-bits")

    for b in range(n_blocks):
        diff = draw(-1 if pred > 0 else 1)
        pred += diff
        zz[b, 0] = pred
        for k in range(1, 64 if b else 1 + NR_FIRST):
            zz[b, k] = draw()
        if b == 0:
            tail = "0"  # (EOB is 111110)
    coefs = np.zeros((n_blocks, 1, 64), np.int64)
    coefs[:, 0, W.ZIGZAG] = zz
    spec = gray(8 * n_blocks, 8, q=np.ones(64, np.int64), dc=NR_DC, ac=NR_AC)

    def reach(case):
        log, data = case.log, case.stream[case.log.scan:case.log.eoi]
        assert 0xFF not in data and case.n_parts > 2 * 256 and len(data) > 2 * WG
        assert np.all(np.diff(log.mcu_pos)[1:] == 64 * 7), "all 63 AC coefficients, no EOB, 7 bits a symbol"
        bits = "".join(format(b, "08b") for b in data)
        dc, ac = decoder_of(NR_DC), decoder_of(NR_AC)
        missed = []
        for i in range(1, len(data) // PART):
            limit = 8 * PART * (i + 1)
            j = int(np.searchsorted(log.sym_pos, 8 * log.scan + limit))
            truth = (int(log.sym_pos[j]) - 8 * log.scan, 0, int(log.sym_z[j])) if j < len(log.sym_pos) else None
            missed.append(lane_exit(bits, 8 * PART * i, limit, dc, ac) != truth)
        assert missed[0] and missed[1], "lanes 1 and 2 do not resynchronise"
        assert np.mean(missed) >= 0.9, np.mean(missed)
        case.missed = float(np.mean(missed))

    return Case("no_resync", coefs, spec, reach=reach)


# ---- the cases ----

BUILDERS = {}


def case(fn):
    BUILDERS[fn.__name__] = lambda: fn(fn.__name__)
    return fn


for _B, _tag in ((PART * 3, "part"), (WG, "workgroup")):
    for _k, _mode in enumerate(("end", "straddle", "split", "stuffed")):
        BUILDERS["edge_%s_%s" % (_tag, _mode)] = (lambda B=_B, mode=_mode, n="edge_%s_%s" % (_tag, _mode), k=_k: edge_case(n, B, mode, 100 * k + B % 97))
# with EOI's two bytes: 1, 1 (one full part), 2, 2, 256 (one full workgroup), 257, 257, 512 (two full ones), 513 parts
SIZES = {1: 1, 126: 1, 128: 2, 129: 2, 32766: 256, 32768: 257, 32769: 257, 65534: 512, 65537: 513}
for _N in SIZES:
    BUILDERS["scan_of_%d_bytes" % _N] = (lambda N=_N: sized_case("scan_of_%d_bytes" % N, N, N % 89))
BUILDERS["no_resync"] = no_resync_case

ONE_DC = W.table_from_lengths([(0, 1)])
ONE_AC = W.table_from_lengths([(0x00, 1)])


@case
def ri_1_constant(name):
    """2 bits to the MCU: a byte and an RSTm, 42 markers to a part, 300 of them"""
    def reach(c):
        assert set(np.diff(c.log.mcu_pos).tolist()) == {24} and c.stream.count(b"\xFF\xD7") >= 37

    return Case(name, np.zeros((301, 1, 64)), gray(8 * 43, 8 * 7, dc=ONE_DC, ac=ONE_AC, ri=1), reach=reach)


def intervals_case(name, w, h, ri, count, seed=5, **kw):
    def reach(c):
        n = shape_of(c.spec)[0]
        assert -(-n // min(ri, n)) == count and len(c.log.pad) == count
        scan = c.stream[c.log.scan:]
        found = [scan[i + 1] - 0xD0 for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
        assert found == [i & 7 for i in range(count - 1)], "the RSTm of the scan, their numbers wrapping from 7 to 0"

    spec = gray(w, h, ri=ri, **kw)
    return Case(name, texture(seed, spec), spec, reach=reach)


BUILDERS["intervals_63"] = lambda: intervals_case("intervals_63", 8 * 21, 8 * 6, 2, 63)       # 126 MCUs
BUILDERS["intervals_64"] = lambda: intervals_case("intervals_64", 8 * 16, 8 * 8, 2, 64)       # 128 MCUs
BUILDERS["intervals_9"] = lambda: intervals_case("intervals_9", 8 * 9, 8 * 3, 3, 9)
BUILDERS["intervals_17"] = lambda: intervals_case("intervals_17", 8 * 17, 8 * 2, 2, 17)
BUILDERS["ri_above_the_mcu_count"] = lambda: intervals_case("ri_above_the_mcu_count", 40, 24, 16, 1)
BUILDERS["ri_65535"] = lambda: intervals_case("ri_65535", 40, 24, 65535, 1)
BUILDERS["ri_not_a_row"] = lambda: intervals_case("ri_not_a_row", 8 * 7, 8 * 5, 4, 9)        # 35 MCUs: 8 of 4 and one of 3
BUILDERS["interval_of_257"] = lambda: intervals_case("interval_of_257", 8 * 257, 16, 257, 2)
BUILDERS["interval_of_1000"] = lambda: intervals_case("interval_of_1000", 8 * 250, 40, 1000, 2)


def dri_layout(front, behind=()):
    """DRI segments in front of DQT and SOF, and behind SOF and DHT (in front of SOS)"""
    layout = W.default_layout({0: Q3}, {0: W.STD_DC_LUM}, {0: W.STD_AC_LUM}, extra=[W.seg("DRI", v) for v in front])
    return layout[:-1] + [W.seg("DRI", v) for v in behind] + layout[-1:]


def dri_case(name, ri, count, front, behind=()):
    """35 MCUs; ri is the interval that holds: the last DRI's"""
    case = intervals_case(name, 8 * 7, 8 * 5, ri, count, layout=dri_layout(front, behind))
    counted = case._reach

    def reach(c):
        counted(c)
        marks = [m for m, _, _ in c.segments()]
        sof = marks.index(0xC0)
        assert [(m == 0xDD) for m in marks[:sof]].count(True) == len(front) and marks[sof:].count(0xDD) == len(behind)
        assert [(b[0] << 8) | b[1] for m, _, b in c.segments() if m == 0xDD] == list(front) + list(behind)
        assert c.log.ri == (list(front) + list(behind))[-1]

    case._reach = reach
    return case


BUILDERS["dri_twice"] = lambda: dri_case("dri_twice", 4, 9, [7], [4])  # the second one behind SOF: it overrides across the frame header
BUILDERS["dri_0_behind_dri_5"] = lambda: dri_case("dri_0_behind_dri_5", 35, 1, [5, 0])
BUILDERS["dri_in_front_of_sof"] = lambda: dri_case("dri_in_front_of_sof", 4, 9, [4])
BUILDERS["dri_behind_sof"] = lambda: dri_case("dri_behind_sof", 4, 9, [], [4])


@case
def dc_category_11(name):
    """DC differences of +-2047: the predictor runs to 2047, to -2047 and back (the blocks are DC alone, q = 1)"""
    dc = [0, 2047, 0, -2047, 0, 2047, 2047, 0, -2047, -2047, 0, 1024, -1023, 1024]
    coefs = np.zeros((len(dc), 1, 64), np.int64)
    coefs[:, 0, 0] = dc

    def reach(c):
        assert (np.abs(np.diff(dc)) >= 1024).sum() >= 10 and max(dc) == 2047 and min(dc) == -2047

    return Case(name, coefs, gray(8 * 7, 16, q=np.ones(64, np.int64)), reach=reach)


def fill_case(name, count):
    def reach(c):
        assert c.stream.count(b"\xFF" * (count + 1) + b"\xD1") == 1 and c.stream.endswith(b"\xFF" * (count + 1) + b"\xD9")

    spec = gray(8 * 7, 8 * 5, ri=4, fill_rst=count, fill_eoi=count)
    return Case(name, texture(8, spec), spec, reach=reach)


for _n in (1, 2, 200):
    BUILDERS["fill_bytes_%d" % _n] = lambda n=_n: fill_case("fill_bytes_%d" % n, n)


@case
def dc_table_of_one_code(name):
    spec = gray(40, 24, dc=ONE_DC)
    coefs = texture(3, spec)
    coefs[:, :, 0] = 0

    def reach(c):
        dc = [t for _, tid, t in c.tables(0xC4) if tid >> 4 == 0]
        assert len(dc) == 1 and list(dc[0][:16]) == [1] + [0] * 15, "one code, of length 1"

    return Case(name, coefs, spec, reach=reach)


SIXTEEN_AC = W.table_from_lengths([(0x00, 1), (0x01, 2), (0x02, 3), (0x03, 4), (0x11, 5), (0x04, 6), (0x12, 7), (0x21, 8), (0x05, 9), (0x31, 10),
                                   (0xF0, 11), (0x13, 12), (0x41, 13), (0x22, 14), (0x06, 15), (0x51, 16)])


@case
def codes_of_all_sixteen_lengths(name):
    spec = gray(8 * 6, 8 * 4, ac=SIXTEEN_AC)
    rng = np.random.default_rng(16)
    n = shape_of(spec)[0]
    zz = np.zeros((n, 64), np.int64)
    for b in range(n):
        k = 1
        for sym in rng.permutation([0x01, 0x02, 0x03, 0x11, 0x04, 0x12, 0x21, 0x05, 0x31, 0xF0, 0x13, 0x41, 0x22, 0x06, 0x51]):
            run, s = int(sym) >> 4, int(sym) & 15
            k += run if s else 0
            if s:
                zz[b, k] = int(rng.integers(1 << (s - 1), 1 << s)) * int(rng.choice([-1, 1]))
                k += 1
            else:
                k += 16  # (ZRL: sixteen zeros, the coefficient behind them follows)
        zz[b, 0] = rng.integers(-50, 51)
    coefs = np.zeros((n, 1, 64), np.int64)
    coefs[:, 0, W.ZIGZAG] = zz

    def reach(c):
        used = set()
        lut = W.codes(SIXTEEN_AC)
        for b in range(n):
            run = 0
            for k in range(1, 64):
                v = int(zz[b, k])
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    used.add(lut[0xF0][1])
                    run -= 16
                used.add(lut[(run << 4) | abs(v).bit_length()][1])
                run = 0
            used.add(lut[0][1])
        assert used == set(range(1, 17)), sorted(used)

    return Case(name, coefs, spec, reach=reach)


def one_dht(q, dc, ac):
    """two DQT in one segment behind SOF, every DHT in one segment"""
    items = sorted(q.items())
    return [W.seg("DQT", items[:1]), W.seg("SOF"), W.seg("DQT", items[1:]),
            W.seg("DHT", [(0, i, t) for i, t in sorted(dc.items())] + [(1, i, t) for i, t in sorted(ac.items())]), W.seg("SOS")]


def tables_twice(q, dc, ac):
    """every table sent with other contents first (under the same id), then as it holds"""
    wrong = [W.seg("DQT", [(i, np.full(64, 9)) for i in q]), W.seg("DHT", [(0, i, W.STD_DC_CHR if dc[i] is not W.STD_DC_CHR else W.STD_DC_LUM) for i in dc]),
             W.seg("DHT", [(1, i, rotated(W.STD_AC_CHR, 7)) for i in ac])]
    return wrong + W.default_layout(q, dc, ac)


def three_sets(c, hv):
    """SOF1; the components' tables, as they hold at SOS, differ pairwise in all three kinds and lie under ids that are not
    the components' indices"""
    at, marker, comps = c.sof()
    assert marker == 0xC1 and [s for _, s, _ in comps] == list(hv)
    held = {}
    for marker_t in (0xDB, 0xC4):
        for _, tid, body in c.tables(marker_t):
            held[(marker_t, tid)] = body  # (the later one holds)
    sos = c.segments()[-1][2]
    for kind, ids in (("q", [(0xDB, tq) for _, _, tq in comps]), ("dc", [(0xC4, sos[2 + 2 * k] >> 4) for k in range(3)]),
                      ("ac", [(0xC4, 0x10 | (sos[2 + 2 * k] & 15)) for k in range(3)])):
        assert len({held[i] for i in ids}) == 3, kind + ": three different tables"
        assert [i[1] & 15 for i in ids] != [0, 1, 2]


@case
def colour_444_three_table_sets(name):
    spec = colour(8 * 5 + 3, 8 * 3 + 1, three=True, sof=0xC1, layout=one_dht)

    def reach(c):
        three_sets(c, (0x11, 0x11, 0x11))
        at = c.sof()[0]
        dht, dqt = c.tables(0xC4), c.tables(0xDB)
        assert len(dht) == 6 and len({i for i, _, _ in dht}) == 1 and dht[0][0] > at, "every DHT in one segment, behind SOF"
        assert [i > at for i, _, _ in dqt] == [False, True, True] and dqt[1][0] == dqt[2][0], "two DQT in one segment, behind SOF"

    return Case(name, texture(44, spec, amp=25, dc=30), spec, reach=reach)


@case
def colour_420_three_table_sets(name):
    spec = colour(16 * 4 + 5, 16 * 3 + 2, hv=(0x22, 0x11, 0x11), three=True, sof=0xC1, layout=tables_twice)

    def reach(c):
        three_sets(c, (0x22, 0x11, 0x11))
        for marker in (0xDB, 0xC4):
            sent = {}
            for _, tid, body in c.tables(marker):
                sent.setdefault(tid, []).append(body)
            assert all(len(v) == 2 and v[0] != v[1] for v in sent.values()), "every table sent twice, with other contents first"
        assert len({i for i, _, _ in c.tables(0xC4)}) == 8, "and the tables that hold in a segment each"

    return Case(name, texture(42, spec, amp=25, dc=30), spec, reach=reach)


@case
def sampling_of_ten_blocks(name):
    spec = colour(32 * 3 + 7, 16 * 2 + 3, hv=(0x42, 0x11, 0x11), three=True, sof=0xC1)

    def reach(c):
        three_sets(c, (0x42, 0x11, 0x11))
        assert c.coefs.shape[1] == 10

    return Case(name, texture(10, spec, amp=25, dc=30), spec, any_sampling=True, reach=reach)


def header_case(name, extra, seed=6, reach=None, **kw):
    spec = gray(40, 24, extra=extra, **kw)
    return Case(name, texture(seed, spec), spec, reach=reach)


def exif(o):
    """an Exif APP1 whose IFD0 holds the orientation alone (big endian)"""
    tiff = b"MM\0*\0\0\0\x08" + b"\0\x01" + b"\x01\x12\0\x03\0\0\0\x01" + bytes([0, o, 0, 0]) + b"\0\0\0\0"
    return W.seg("APP", (1, b"Exif\0\0" + tiff))


def lengths_are(marks):
    def reach(c):
        assert [(m, n) for m, n, _ in c.segments() if m in (0xFE,) or 0xE1 <= m <= 0xEF] == marks
    return reach


@case
def segments_of_length_2(name):
    return header_case(name, [W.seg("COM", b""), W.seg("APP", (5, b""))], reach=lengths_are([(0xFE, 2), (0xE5, 2)]))


@case
def segments_of_length_65535(name):
    """(the COM's payload is full of SOS and EOI markers)"""
    return header_case(name, [W.seg("COM", b"\xFF\xDA\xFF\xD9" * 16383 + b"x"), W.jfif(), W.seg("APP", (7, bytes(range(256)) * 255 + bytes(253)))],
                       reach=lengths_are([(0xFE, 65535), (0xE7, 65535)]))


@case
def app1_that_is_not_exif_first(name):
    def reach(c):
        app1 = [b for m, _, b in c.segments() if m == 0xE1]
        assert len(app1) == 2 and not app1[0].startswith(b"Exif") and app1[1].startswith(b"Exif\0\0")

    return header_case(name, [W.jfif(), W.seg("APP", (1, b"http://ns.adobe.com/xap/1.0/\0<x/>")), exif(6)], reach=reach)


def ids_are(ids):
    def reach(c):
        assert [i for i, _, _ in c.sof()[2]] == list(ids)
        assert list(c.segments()[-1][2][1:1 + 2 * len(ids):2]) == list(ids), "and in SOS"
    return reach


@case
def component_id_0(name):
    return header_case(name, [], cid=0, reach=ids_are([0]))


@case
def fill_bytes_between_segments(name):
    fills = [1, 3, 1, 2, 40, 1]
    layout = [W.seg("APP", (0, b"JFIF\0\1\1\0\0\1\0\1\0\0"), fill=1), W.seg("DQT", [(0, Q3)], fill=3), W.seg("SOF", fill=1), W.seg("DHT", [(0, 0, W.STD_DC_LUM)], fill=2),
              W.seg("DHT", [(1, 0, W.STD_AC_LUM)], fill=40), W.seg("SOS", fill=1)]

    def reach(c):
        marks = [m for m, _, _ in c.segments()]
        plain = sum(4 + len(b) for _, _, b in c.segments())
        assert marks == [0xE0, 0xDB, 0xC0, 0xC4, 0xC4, 0xDA] and c.log.scan == 2 + plain + sum(fills)
        assert b"\xFF" * 41 + b"\xC4" in c.stream[:c.log.scan]

    return header_case(name, [], layout=layout, reach=reach)


@case
def component_ids_0_1_2(name):
    spec = colour(24, 16, ids=(0, 1, 2), extra=[W.jfif()])
    return Case(name, texture(12, spec, amp=25, dc=30), spec, reach=ids_are((0, 1, 2)))


@case
def component_ids_10_20_30(name):
    spec = colour(24, 16, ids=(10, 20, 30), extra=[W.jfif()])
    return Case(name, texture(13, spec, amp=25, dc=30), spec, reach=ids_are((10, 20, 30)))


@case
def one_component_sampled_2x2(name):
    """a one-component scan is not interleaved, whatever its sampling byte says: ceil(w / 8) x ceil(h / 8) blocks"""
    spec = gray(8 * 3 + 2, 8 * 3 + 1, hv=0x22)

    def reach(c):
        assert c.sof()[2] == [(1, 0x22, 0)] and c.coefs.shape == (16, 1, 64) and len(c.log.mcu_pos) == 16

    return Case(name, texture(22, spec), spec, reach=reach)


@case
def noise_behind_eoi(name):
    tail = np.random.default_rng(1).integers(0, 256, 1024, dtype=np.uint8).tobytes()

    def reach(c):
        assert c.stream[c.log.eoi:c.log.eoi + 2] == b"\xFF\xD9" and c.stream[c.log.eoi + 2:] == tail and c.n_parts > 8

    return header_case(name, [], tail=tail, reach=reach)


@case
def a_second_stream_behind_eoi(name):
    other = header_case("other", [], seed=99)

    def reach(c):
        assert c.stream[c.log.eoi:c.log.eoi + 4] == b"\xFF\xD9\xFF\xD8" and c.stream.endswith(other.stream) and other.stream.count(b"\xFF\xDA") == 1
        assert not np.array_equal(other.coefs, c.coefs)

    return header_case(name, [], tail=other.stream, reach=reach)


@case
def no_eoi(name):
    def reach(c):
        assert c.log.eoi == len(c.stream) and b"\xFF\xD9" not in c.stream[c.log.scan:]

    return Case(name, texture(6, gray(40, 24)), gray(40, 24, eoi=False), reach=reach)


# padding: k bits of it in front of one RSTm (the others 1-bits), and in front of EOI

def padded(name, where, how, k):
    """the seed is searched so that the padding in question is k bits"""
    status = DAMAGED if where == "rst" and not (how == "alt" and k == 1) else OK  # (one bit of 1010... is a 1-bit)
    for seed in range(400):
        spec = gray(8 * 8, 8, ri=1)
        coefs = texture(seed, spec, keep=0.08)
        _, log = W.write(coefs, spec)
        at = 3 if where == "rst" else len(log.pad) - 1
        if log.pad[at] == k:
            spec = gray(8 * 8, 8, ri=1, **({"pad_rst": {at: how}} if where == "rst" else {"pad_eoi": how}))

            def reach(c):
                assert c.log.pad[at] == k
                byte = c.stream[c.log.end[at] - 1 - (c.stream[c.log.end[at] - 1] == 0 and c.stream[c.log.end[at] - 2] == 0xFF)]
                want = {"zeros": 0, "alt": 0xAA >> (8 - k), "ones": (1 << k) - 1}[how]
                assert byte & ((1 << k) - 1) == want

            return Case(name, coefs, spec, status=status, reach=reach)
    raise AssertionError(name)


for _where in ("rst", "eoi"):
    for _how in ("zeros", "alt"):
        for _k in range(1, 8):
            BUILDERS["padding_%s_%s_%d" % (_where, _how, _k)] = (lambda w=_where, h=_how, k=_k: padded("padding_%s_%s_%d" % (w, h, k), w, h, k))


@case
def padding_zeros_in_front_of_every_rst(name):
    spec = gray(8 * 8, 8 * 4, ri=1, pad_rst="zeros", pad_eoi="zeros")

    def reach(c):
        assert set(c.log.pad[:-1]) >= set(range(1, 8))

    return Case(name, texture(4, spec, keep=0.08), spec, status=DAMAGED, reach=reach)


# RGB files: refused, with the reason

# libjpeg's order (default_decompress_parms): a JFIF segment says YCbCr; else an Adobe segment decides; else the ids

def colour_marks(jfif, adobe, ids=(1, 2, 3)):
    """reach: whether the file has a JFIF APP0, the transform bytes of its Adobe APP14 segments, the ids"""
    def reach(c):
        segs = c.segments()
        assert any(m == 0xE0 and b.startswith(b"JFIF\0") for m, _, b in segs) == jfif
        assert [b[11] for m, _, b in segs if m == 0xEE and b.startswith(b"Adobe")] == adobe
        assert [i for i, _, _ in c.sof()[2]] == list(ids)
    return reach


@case
def rgb_by_adobe_transform_0(name):
    spec = colour(24, 16, extra=[W.adobe(0)])
    return Case(name, texture(31, spec, amp=25, dc=30), spec, status=UNSUPPORTED, message="RGB", reach=colour_marks(False, [0]))


@case
def rgb_by_component_ids(name):
    spec = colour(24, 16, ids=(ord("R"), ord("G"), ord("B")))
    return Case(name, texture(32, spec, amp=25, dc=30), spec, status=UNSUPPORTED, message="RGB", reach=colour_marks(False, [], (0x52, 0x47, 0x42)))


@case
def ycbcr_with_adobe_transform_1(name):
    spec = colour(24, 16, extra=[W.adobe(1)])
    return Case(name, texture(33, spec, amp=25, dc=30), spec, reach=colour_marks(False, [1]))


@case
def ids_r_g_b_under_jfif_are_ycbcr(name):
    spec = colour(24, 16, ids=(ord("R"), ord("G"), ord("B")), extra=[W.jfif()])
    return Case(name, texture(34, spec, amp=25, dc=30), spec, reach=colour_marks(True, [], (0x52, 0x47, 0x42)))


@case
def jfif_wins_over_adobe_transform_0(name):
    """both segments: YCbCr for libjpeg, which asks for the JFIF segment first"""
    spec = colour(24, 16, extra=[W.jfif(), W.adobe(0)])
    return Case(name, texture(35, spec, amp=25, dc=30), spec, reach=colour_marks(True, [0]))


@case
def ids_r_g_b_under_adobe_transform_1_are_ycbcr(name):
    spec = colour(24, 16, ids=(ord("R"), ord("G"), ord("B")), extra=[W.adobe(1)])
    return Case(name, texture(36, spec, amp=25, dc=30), spec, reach=colour_marks(False, [1], (0x52, 0x47, 0x42)))


_cache = {}


def names():
    return list(BUILDERS)


def get(name):
    if name not in _cache:
        _cache[name] = BUILDERS[name]()
        assert _cache[name].name == name
    return _cache[name]


# ---- the expected picture: the writer's coefficients through the second source's back half ----

_expected = {}


def header(case):
    """the second source's reading of the headers, with the WRITER's divisors in place of the ones it picked"""
    import numpy_jpeg_decode_ref as D
    import numpy_jpeg_sampling_ref as S

    info = S.probe(case.stream) if case.any_sampling else D.probe(case.stream)
    assert info.status == OK, (case.name, info.message)
    info.q = list(case.log.q)
    return info


def expected(case, fmt):
    """"u8" the luminance, "u8x3" RGB: computed once per (case, format), read-only"""
    import numpy_jpeg_decode_ref as D
    import numpy_jpeg_sampling_ref as S

    key = (case.name, fmt)
    if key not in _expected:
        info = header(case)
        planes = (S if case.any_sampling else D).component_planes(info, case.coefs, only_luma=fmt == "u8" or info.components == 1)
        y = planes[0].astype(np.uint8)
        if fmt == "u8":
            out = y
        elif info.components == 1:
            out = np.stack([y, y, y], axis=-1)
        elif case.any_sampling:
            hmax, vmax = info.hv[0]
            cb, cr = (S.upsample(p, info.width, info.height, hmax // h, vmax // v) for p, (h, v) in zip(planes[1:], info.hv[1:]))
            out = D.rgb(planes[0].astype(np.int64), cb, cr)
        else:
            hs, vs = (1 if info.layout == D.LAYOUT_444 else 2), (2 if info.layout == D.LAYOUT_420 else 1)
            cb, cr = (D.upsample(p, info.width, info.height, hs, vs) for p in planes[1:])
            out = D.rgb(planes[0].astype(np.int64), cb, cr)
        out = np.ascontiguousarray(out)
        out.setflags(write=False)
        _expected[key] = out
    return _expected[key]


def expected_from_headers_of(case):
    """the luminance of a case that the decoder refuses for its scan (status 4): its headers are sound"""
    import numpy_jpeg_decode_ref as D

    info = D.probe(case.stream)
    assert info.status == OK
    info.q = list(case.log.q)
    return D.component_planes(info, case.coefs, only_luma=True)[0].astype(np.uint8)
