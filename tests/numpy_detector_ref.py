"""A SECOND, independent restatement of the detector rows of the path -- filter (A2), direction bins and the dilated
masks (A3-A4), seeds (A5-A6), flood (A7-A8) and the weighted line fit (A9) -- in float64 NumPy, written from the
reference's text: filter.cpp:29-43 (maximum_filter), :46-62 (binary_dilate), :65-98 (taps and conv_2d, a correlation
with a 2-px zero border), :101-153 (flood), :161-195 (find_peaks); line_detector.cpp:66-89, 92-122, 126-182, 185-251
(directions, min seed value, component order, COMPONENT_MIN_SIZE); geometry.cpp:20-61 (weighted PCA fit).  The taps
come from the formula itself in float64 (no separable form, no fused chains), the 2x2 from numpy.linalg.eigh, sums are
NumPy's.  The oracle (oracle/rectify_oracle.cpp) and the kernels share one canonical arithmetic; this file shares
nothing with either and does not load the oracle, so agreement with it is not the same reading twice.  Test
infrastructure only.

Two uses:
* `find_line_segments(img, tolerance)`: the detector end to end in float64 (pinned to the reference's own 848 golden
  rows by tests/test_detector_second_source_cpu.py).
* `check_stages(frame, img, st)`: a stage-by-stage check of a fp32 implementation (the kernels, or the oracle).  Each
  stage after the filter takes the implementation's own output of the stage before as its input, so rounding never
  carries from one stage to the next.  Every binary decision on a float is three-valued -- sure yes, sure no, or
  ambiguous: within a relative EPS of its threshold or of the competing value.  EPS = 2^-20 is 16 fp32 ulps, wider
  than any canonical expression's error and too narrow to hide a semantic error.
"""
import collections

import numpy as np

EPS = 2.0 ** -20
N_BINS = 8                    # line_detector.cpp:203
EDGE_KERNEL_SIZE = 2          # config.h
EDGE_KERNEL_SIGMA = 1.0
SEED_DIST = 2
SEED_RATIO = 0.95
TRACE_TOLERANCE = 0.25
COMPONENT_MIN_SIZE = 5
LINE_MIN_LENGTH = 5.0
LINE_MAX_ERR = 2.0


def _fail(frame, stage, msg):
    raise AssertionError("[%s] %s: %s" % (frame, stage, msg))


def _first(mask):
    """(row, col) of the first True pixel in row-major order"""
    return tuple(int(v) for v in np.argwhere(mask)[0])


# ---------------------------------------------------------------------------------------------------------------------
# A2: the filter

def gauss_deriv_kernel(size=EDGE_KERNEL_SIZE, sigma=EDGE_KERNEL_SIGMA, dir_x=True):
    """filter.cpp:65-78: H(i, j) = z / (2 pi sigma^4) * exp(-(x^2 + y^2) / (2 sigma^2)), x = j - size, y = i - size"""
    t = np.arange(-size, size + 1, dtype=np.float64)
    y, x = np.meshgrid(t, t, indexing="ij")
    z = x if dir_x else y
    return z / (2.0 * np.pi * sigma ** 4) * np.exp(-(x * x + y * y) / (2.0 * sigma * sigma))


def conv_2d(img, H):
    """filter.cpp:81-98: out(i + nr/2, j + nc/2) = sum(block(i, j, nr, nc) * H), zero elsewhere"""
    img = np.asarray(img, np.float64)
    h, w = img.shape
    nr, nc = H.shape
    out = np.zeros((h, w))
    if h < nr or w < nc:
        return out
    acc = np.zeros((h - nr + 1, w - nc + 1))
    for a in range(nr):
        for b in range(nc):
            acc += H[a, b] * img[a: a + h - nr + 1, b: b + w - nc + 1]
    out[nr // 2: nr // 2 + h - nr + 1, nc // 2: nc // 2 + w - nc + 1] = acc
    return out


def gradients(img):
    """line_detector.cpp:41-49: dx, dy, and the scale sum_ab |H_ab| |I(y+a, x+b)| of each of them"""
    Hx, Hy = gauss_deriv_kernel(dir_x=True), gauss_deriv_kernel(dir_x=False)
    a = np.abs(np.asarray(img, np.float64))
    return conv_2d(img, Hx), conv_2d(img, Hy), conv_2d(a, np.abs(Hx)), conv_2d(a, np.abs(Hy))


# ---------------------------------------------------------------------------------------------------------------------
# A3-A4: direction planes, bins, dilated masks

def bin_trig():
    theta = np.arange(N_BINS) * np.pi / N_BINS  # line_detector.cpp:144
    return np.sin(theta), np.cos(theta)


def responses(dx, dy):
    """line_detector.cpp:142-146: plane b = |dx sin(theta_b) + dy cos(theta_b)|, shape (8, h, w)"""
    s, c = bin_trig()
    dx = np.asarray(dx, np.float64)
    dy = np.asarray(dy, np.float64)
    return np.abs(dx[None] * s[:, None, None] + dy[None] * c[:, None, None])


def grad_bin(R):
    """line_detector.cpp:152-156: the first bin whose response is strictly above all before it; an all-zero pixel gets
    bin 0 (the reference leaves it uninitialised, :128; DESIGN 3.3 makes it 0), as numpy's argmax does"""
    return np.argmax(R, axis=0)


def binary_dilate(m):
    """filter.cpp:46-62: 3x3 maximum, 1-px zero border"""
    h, w = m.shape
    out = np.zeros((h, w), bool)
    if h < 3 or w < 3:
        return out
    acc = np.zeros((h - 2, w - 2), bool)
    for a in range(3):
        for b in range(3):
            acc |= m[a: a + h - 2, b: b + w - 2] != 0
    out[1:-1, 1:-1] = acc
    return out


def dilate_bits(bits):
    """bitwise OR of a 3x3 neighbourhood, 1-px zero border: the eight dilations of bin == b at once"""
    h, w = bits.shape
    out = np.zeros((h, w), np.uint8)
    if h < 3 or w < 3:
        return out
    acc = np.zeros((h - 2, w - 2), np.uint8)
    for a in range(3):
        for b in range(3):
            acc |= bits[a: a + h - 2, b: b + w - 2]
    out[1:-1, 1:-1] = acc
    return out


def tie_bits(R):
    """bit b set iff plane b is within a relative EPS of the pixel's largest response (bin 0 alone where all are 0)"""
    best = R.max(axis=0)
    tie = R >= best * (1.0 - EPS)
    bits = np.zeros(best.shape, np.uint8)
    for b in range(N_BINS):
        bits |= (tie[b].astype(np.uint8) << b)
    bits[best == 0] = 1
    return bits


def _popcount8(v):
    v = v.astype(np.uint8)
    return sum(((v >> b) & 1) for b in range(8))


# ---------------------------------------------------------------------------------------------------------------------
# A5-A6: seeds

def maximum_filter(img, size=SEED_DIST):
    """filter.cpp:29-43: n x n maximum, zero on a border of `size`"""
    h, w = img.shape
    n = 2 * size + 1
    out = np.zeros((h, w))
    if h < n or w < n:
        return out
    acc = np.full((h - n + 1, w - n + 1), -np.inf)
    for a in range(n):
        for b in range(n):
            acc = np.maximum(acc, img[a: a + h - n + 1, b: b + w - n + 1])
    out[size: size + h - n + 1, size: size + w - n + 1] = acc
    return out


def find_peaks(mag, min_value, size=SEED_DIST):
    """filter.cpp:161-195: (max_im == image) && (image > min_value), sorted by value, largest first (ties: row-major,
    the order the reference's loop finds them in; its std::sort leaves them unspecified)"""
    peaks = (maximum_filter(mag, size) == mag) & (mag > min_value)
    idx = np.flatnonzero(peaks)
    return idx[np.argsort(-mag.ravel()[idx], kind="stable")]


# ---------------------------------------------------------------------------------------------------------------------
# A7-A8: the flood

def flood_all(h, w, seed_idx, seed_bin, seed_val, tolerance, dx, dy, mask_bits, decide=None):
    """line_detector.cpp:92-122 with filter.cpp:101-153, seeds in their order.  A seed claims the 8-connected set of
    unvisited, non-border pixels whose masked response in the seed's bin is > (1 - tolerance) * seed_val and that
    contains the seed, so the order in which the BFS queue visits pixels does not change which pixels it claims (a
    pixel that fails the test stays unvisited, as in the reference).

    decide(k, i, r, thr, scale) -> None for a sure decision, or the decision to take for an ambiguous pixel (then it is
    counted).  Returns the label image (claiming seed index or -1) and the number of decisions taken from `decide`."""
    N = h * w
    visited = bytearray(N)
    for j in range(w):
        visited[j] = visited[(h - 1) * w + j] = 1
    for i in range(h):
        visited[i * w] = visited[i * w + w - 1] = 1
    dxl = np.asarray(dx, np.float64).ravel().tolist()
    dyl = np.asarray(dy, np.float64).ravel().tolist()
    ml = np.asarray(mask_bits, np.uint8).ravel().tolist()
    st, ct = bin_trig()
    label = [-1] * N
    offs = (-1, 1, w, -w, -w - 1, -w + 1, w - 1, w + 1)  # filter.cpp:130-137 (8-connected)
    n_taken = 0
    for k, (s0, b) in enumerate(zip(seed_idx, seed_bin)):
        s0, b = int(s0), int(b)
        if visited[s0]:
            continue
        s, c, bit = float(st[b]), float(ct[b]), 1 << b
        thr = (1.0 - tolerance) * float(seed_val[k])
        q = collections.deque([s0])
        while q:
            i = q.popleft()
            if visited[i]:
                continue
            a, e = dxl[i] * s, dyl[i] * c
            r = abs(a + e) if ml[i] & bit else 0.0
            yes = r > thr
            if decide is not None and r > 0.0:
                d = decide(k, i, r, thr, abs(a) + abs(e))
                if d is not None:
                    yes = d
                    n_taken += 1
            if yes:
                visited[i] = 1
                label[i] = k
                for o in offs:
                    if not visited[i + o]:
                        q.append(i + o)
    return np.array(label, np.int32).reshape(h, w), n_taken


# ---------------------------------------------------------------------------------------------------------------------
# A9: the weighted PCA fit

def fit_components(label, seed_bin, dx, dy):
    """line_detector.cpp:66-89 + geometry.cpp:20-61 for every flood of more than COMPONENT_MIN_SIZE pixels, in seed
    order.  Pixel values are the seed bin's response (a claimed pixel is inside its mask).  Returns per component:
    seed, n, endpoints (x1, y1, x2, y2) with the major axis signed so that its row component >= its col component,
    weight, err, centroid (x, y), axis (d_r, d_c), relative eigen-gap and extent (largest coordinate + 1)."""
    h, w = label.shape
    lab = label.ravel()
    idx = np.flatnonzero(lab >= 0)
    k = lab[idx]
    counts = np.bincount(k, minlength=len(seed_bin)) if len(k) else np.zeros(len(seed_bin), np.int64)
    comps = np.flatnonzero(counts > COMPONENT_MIN_SIZE)
    keep = counts[k] > COMPONENT_MIN_SIZE
    idx, k = idx[keep], k[keep]
    nc = len(comps)
    out = dict(seed=comps, n=counts[comps])
    if nc == 0:
        for key in ("x1", "y1", "x2", "y2", "weight", "err", "cx", "cy", "d_r", "d_c", "gap", "extent"):
            out[key] = np.zeros(0)
        return out
    ci = np.searchsorted(comps, k)
    order = np.argsort(ci, kind="stable")
    idx, ci = idx[order], ci[order]
    starts = np.searchsorted(ci, np.arange(nc))
    r = (idx // w).astype(np.float64)
    c = (idx % w).astype(np.float64)
    st, ct = bin_trig()
    b = np.asarray(seed_bin)[comps][ci]
    val = np.abs(np.asarray(dx, np.float64).ravel()[idx] * st[b] + np.asarray(dy, np.float64).ravel()[idx] * ct[b])
    S = np.bincount(ci, val, nc)
    wn = val / S[ci]                                               # weights sum to 1
    a_r = np.bincount(ci, wn * r, nc)
    a_c = np.bincount(ci, wn * c, nc)
    cr, cc = r - a_r[ci], c - a_c[ci]
    cov = np.empty((nc, 2, 2))
    cov[:, 0, 0] = np.bincount(ci, wn * cr * cr, nc)
    cov[:, 0, 1] = cov[:, 1, 0] = np.bincount(ci, wn * cr * cc, nc)
    cov[:, 1, 1] = np.bincount(ci, wn * cc * cc, nc)
    lam, vec = np.linalg.eigh(cov)                                  # ascending: column 1 is the major axis
    d = vec[:, :, 1].copy()
    flip = d[:, 0] < d[:, 1]
    d[flip] *= -1.0
    nv = vec[:, :, 0]
    t = cr * d[ci, 0] + cc * d[ci, 1]
    t0 = np.minimum.reduceat(t, starts)
    t1 = np.maximum.reduceat(t, starts)
    out.update(
        x1=a_c + d[:, 1] * t0, y1=a_r + d[:, 0] * t0, x2=a_c + d[:, 1] * t1, y2=a_r + d[:, 0] * t1,
        weight=S / counts[comps],
        err=np.bincount(ci, np.abs(cr * nv[ci, 0] + cc * nv[ci, 1]), nc) / counts[comps],
        cx=a_c, cy=a_r, d_r=d[:, 0], d_c=d[:, 1],
        gap=np.where(lam[:, 1] > 0, (lam[:, 1] - lam[:, 0]) / np.where(lam[:, 1] > 0, lam[:, 1], 1.0), 0.0),
        extent=np.maximum.reduceat(np.maximum(r, c), starts) + 1.0,
    )
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the detector end to end

def find_line_segments(img, tolerance=TRACE_TOLERANCE):
    """line_detector.cpp:185-251 in float64; returns records as dicts of arrays (x1, y1, x2, y2, weight, err)"""
    img = np.asarray(img, np.float64)
    h, w = img.shape
    dx, dy, _, _ = gradients(img)
    R = responses(dx, dy)
    b = grad_bin(R)
    masks = np.zeros((h, w), np.uint8)
    for k in range(N_BINS):
        masks |= binary_dilate(b == k).astype(np.uint8) << k
    mag = np.hypot(dx, dy)
    seeds = find_peaks(mag, mag.max() * (1.0 - SEED_RATIO))
    sb = b.ravel()[seeds]
    sval = R.reshape(N_BINS, -1)[sb, seeds]
    label, _ = flood_all(h, w, seeds, sb, sval, tolerance, dx, dy, masks)
    return fit_components(label, sb, dx, dy)


def filter_lines(f, min_length):
    """interface.cpp:27-32: length > max(min_length, LINE_MIN_LENGTH) and err < LINE_MAX_ERR"""
    length = np.hypot(f["x2"] - f["x1"], f["y2"] - f["y1"])
    keep = (length > max(min_length, LINE_MIN_LENGTH)) & (f["err"] < LINE_MAX_ERR)
    return {k: (v[keep] if isinstance(v, np.ndarray) and len(v) == len(keep) else v) for k, v in f.items()}


# ---------------------------------------------------------------------------------------------------------------------
# stage-by-stage checks of an fp32 implementation

def check_filter(frame, img, dx, dy):
    """|dev - f64| <= 2^-20 * sum_ab |H_ab| |I(y+a, x+b)| everywhere; the 2-px border is exactly 0.0.

    The bound: an fp32 form of the 25-term correlation rounds about nine partial sums (the separable form: two
    differences or sums and their products in the row pass, as many in the column pass), each by at most 2^-24 of
    the magnitude of the terms it has gathered, which is at most sum |H| |I|; and it uses four rounded tap factors
    (d1, d2, g1, g2, each within about an ulp of the formula), a product of two of which is each tap.  That is some
    13 ulps of sum |H| |I|; 16 (EPS) is the bound."""
    h, w = img.shape
    fx, fy, sx, sy = gradients(img)
    for name, dev, ref, scale in (("dx", dx, fx, sx), ("dy", dy, fy, sy)):
        dev = np.asarray(dev, np.float64)
        border = np.ones((h, w), bool)
        border[2:h - 2, 2:w - 2] = False
        bad = border & (dev != 0.0)
        if bad.any():
            p = _first(bad)
            _fail(frame, "filter " + name, "border pixel %s is %r, not 0.0" % (p, dev[p]))
        bad = ~(np.abs(dev - ref) <= EPS * scale)
        if bad.any():
            p = _first(bad)
            _fail(frame, "filter " + name, "%d pixels off, first %s: dev %r f64 %r bound %r" % (
                bad.sum(), p, dev[p], ref[p], EPS * scale[p]))


def check_dmask(frame, dx, dy, dmask):
    """required <= dmask <= allowed bitwise: `required` ORs the bins of the 3x3 neighbours whose tie set is one bin,
    `allowed` adds the whole tie set of every other neighbour; 1-px zero border"""
    bits = tie_bits(responses(dx, dy))
    single = _popcount8(bits) == 1
    required = dilate_bits(np.where(single, bits, 0).astype(np.uint8))
    allowed = dilate_bits(bits)
    dm = np.asarray(dmask, np.uint8)
    bad = (required & ~dm) != 0
    if bad.any():
        p = _first(bad)
        _fail(frame, "dmask", "%d pixels miss a required bin, first %s: dev %#04x required %#04x" % (bad.sum(), p, dm[p], required[p]))
    bad = (dm & ~allowed) != 0
    if bad.any():
        p = _first(bad)
        _fail(frame, "dmask", "%d pixels carry a bin no neighbour can have, first %s: dev %#04x allowed %#04x" % (
            bad.sum(), p, dm[p], allowed[p]))
    return bits


def check_maxmag(frame, dx, dy, maxmag):
    m = float(np.hypot(np.asarray(dx, np.float64), np.asarray(dy, np.float64)).max())
    if not abs(float(maxmag) - m) <= EPS * m:
        _fail(frame, "maxmag", "dev %r f64 %r" % (float(maxmag), m))
    return m


def seed_sets(dx, dy, maxmag64):
    """Three-valued peak test of filter.cpp:161-195 on hypot(dx, dy) (float64 of the device's dx, dy): a pixel is a
    sure seed if it exceeds 0.05 max by more than EPS and every other pixel of its 5x5 window by more than EPS or
    equals it exactly (same |dx|, |dy| pair: the fp32 magnitudes are then equal too, the reference's `max_im == img`
    tie); a sure non-seed if a neighbour exceeds it by more than EPS or it is below the threshold by more than EPS.
    Returns (sure, ambiguous, mag)."""
    dx = np.asarray(dx, np.float64)
    dy = np.asarray(dy, np.float64)
    h, w = dx.shape
    mag = np.hypot(dx, dy)
    lo, hi = np.minimum(np.abs(dx), np.abs(dy)), np.maximum(np.abs(dx), np.abs(dy))
    thr = maxmag64 * (1.0 - SEED_RATIO)
    thr_yes = mag > thr * (1.0 + EPS)
    thr_maybe = mag >= thr * (1.0 - EPS)
    sure = np.zeros((h, w), bool)
    maybe = np.zeros((h, w), bool)
    n = 2 * SEED_DIST + 1
    if h >= n and w >= n:
        sl = (slice(SEED_DIST, h - SEED_DIST), slice(SEED_DIST, w - SEED_DIST))
        m0, lo0, hi0 = mag[sl], lo[sl], hi[sl]
        all_yes = np.ones(m0.shape, bool)
        any_no = np.zeros(m0.shape, bool)
        for a in range(n):
            for b in range(n):
                if a == SEED_DIST and b == SEED_DIST:
                    continue
                win = (slice(a, a + h - n + 1), slice(b, b + w - n + 1))
                mn = mag[win]
                same = (lo[win] == lo0) & (hi[win] == hi0)
                all_yes &= (m0 > mn * (1.0 + EPS)) | same
                any_no |= (mn > m0 * (1.0 + EPS)) & ~same
        sure[sl] = all_yes
        maybe[sl] = ~any_no
    sure_all = sure & thr_yes
    amb = maybe & thr_maybe & ~sure_all
    return sure_all, amb, mag


def check_seeds(frame, dx, dy, bits, maxmag64, seed_idx, seed_bin, seed_thr):
    """sure <= device set <= sure + ambiguous; order non-increasing in f64 magnitude up to EPS; each seed's bin in its
    tie set; seed_thr within EPS of 0.75 * the f64 response of that bin at the seed.  Returns the ambiguous count."""
    h, w = np.asarray(dx).shape
    sure, amb, mag = seed_sets(dx, dy, maxmag64)
    seed_idx = np.asarray(seed_idx, np.int64)
    dev = np.zeros(h * w, bool)
    if len(seed_idx):
        if seed_idx.min() < 0 or seed_idx.max() >= h * w:
            _fail(frame, "seeds", "seed index out of the frame")
        dev[seed_idx] = True
        if len(np.unique(seed_idx)) != len(seed_idx):
            _fail(frame, "seeds", "a pixel is a seed twice")
    dev = dev.reshape(h, w)
    miss = sure & ~dev
    if miss.any():
        p = _first(miss)
        _fail(frame, "seeds", "%d sure seeds missing, first %s (mag %r)" % (miss.sum(), p, mag[p]))
    extra = dev & ~(sure | amb)
    if extra.any():
        p = _first(extra)
        _fail(frame, "seeds", "%d seeds that cannot be, first %s (mag %r)" % (extra.sum(), p, mag[p]))
    m = mag.ravel()[seed_idx]
    bad = np.flatnonzero(m[1:] > m[:-1] * (1.0 + EPS))
    if len(bad):
        i = int(bad[0])
        _fail(frame, "seed order", "seed %d (mag %r) before seed %d (mag %r)" % (i, m[i], i + 1, m[i + 1]))
    sb = np.asarray(seed_bin, np.int64)
    if len(sb) and (sb.min() < 0 or sb.max() >= N_BINS):
        _fail(frame, "seed bins", "bin out of range")
    inset = (bits.ravel()[seed_idx] >> sb.astype(np.uint8)) & 1
    bad = np.flatnonzero(inset == 0)
    if len(bad):
        i = int(bad[0])
        _fail(frame, "seed bins", "seed %d at %s has bin %d, tie set %#04x" % (i, divmod(int(seed_idx[i]), w), sb[i], bits.ravel()[seed_idx[i]]))
    R = responses(dx, dy).reshape(N_BINS, -1)
    want = (1.0 - TRACE_TOLERANCE) * R[sb, seed_idx] if len(sb) else np.zeros(0)
    bad = np.flatnonzero(~(np.abs(np.asarray(seed_thr, np.float64) - want) <= EPS * want))
    if len(bad):
        i = int(bad[0])
        _fail(frame, "seed thresholds", "seed %d: dev %r f64 %r" % (i, float(seed_thr[i]), want[i]))
    return int((amb & dev).sum()), int(amb.sum())


def check_labels(frame, dx, dy, dmask, seed_idx, seed_bin, label):
    """Floods of the device's seeds in their order over the device's dx, dy and dilated mask.  A pixel whose masked
    response is within a relative EPS of the flood's threshold (relative to the threshold plus the magnitudes the
    response is formed from) takes the device's decision -- is its label this seed? -- and is counted.  The label image
    must be equal everywhere.  Returns the count of decisions taken from the device."""
    h, w = np.asarray(dx).shape
    dev = np.asarray(label, np.int32)
    devl = dev.ravel()
    R = responses(dx, dy).reshape(N_BINS, -1)
    sb = np.asarray(seed_bin, np.int64)
    sval = R[sb, np.asarray(seed_idx, np.int64)] if len(sb) else np.zeros(0)

    def decide(k, i, r, thr, scale):
        if abs(r - thr) <= EPS * (thr + scale):
            return bool(devl[i] == k)
        return None

    mine, n_taken = flood_all(h, w, seed_idx, sb, sval, TRACE_TOLERANCE, dx, dy, dmask, decide)
    bad = mine != dev
    if bad.any():
        p = _first(bad)
        _fail(frame, "labels", "%d pixels differ, first %s: dev %d f64 %d" % (bad.sum(), p, dev[p], mine[p]))
    return n_taken


def check_segments(frame, dx, dy, label, seed_bin, lines):
    """Components are the floods of more than 5 px in seed order, fitted in float64.

    Endpoints within 0.01 px + 2^-20 n extent.  The bound: an fp32 sum of n terms is within (n - 1) 2^-24 of the sum
    of their magnitudes, whatever the order; the centroid's terms are coordinates (at most `extent`, the largest
    coordinate + 1) times weights that sum to 1, the covariance's and the projections' are bounded by extent^2 and
    extent, and an endpoint chains a few such sums -- 16 times one sum's bound covers them; 0.01 px is the reference's
    own printing precision (pin 2).  weight within relative 1e-5, group_id -1, err within 1e-4 + 2^-20 extent: err is a
    mean of |centred coordinate . normal|, and an fp32 centred coordinate carries a few ulps of the largest coordinate
    (a 9-px component on an exact line 2000 px from the origin has err 1.2e-4 in fp32, 0 in float64).  The orientation rule
    (the row component of p1 -> p2 is >= its col component) is asserted where |d_r - d_c| > 1e-4, the
    endpoints are compared unordered elsewhere.  A component whose relative eigen-gap is below 1e-3 has no defined
    axis: only its weight, and that its centroid lies on the segment's line, are checked."""
    f = fit_components(np.asarray(label), np.asarray(seed_bin), dx, dy)
    n = len(f["seed"])
    if len(lines) != n:
        _fail(frame, "segments", "%d records, %d components" % (len(lines), n))
    L = {k: np.asarray(lines[k], np.float64) for k in ("x1", "y1", "x2", "y2", "weight", "err")}
    gid = np.asarray(lines["group_id"])
    n_undefined = 0
    for i in range(n):
        tol = 0.01 + EPS * float(f["n"][i]) * float(f["extent"][i])
        where = "record %d (seed %d, %d px)" % (i, f["seed"][i], f["n"][i])
        if gid[i] != -1:
            _fail(frame, "segments", "%s: group_id %d" % (where, gid[i]))
        if not abs(L["weight"][i] - f["weight"][i]) <= 1e-5 * f["weight"][i]:
            _fail(frame, "segments", "%s: weight %r f64 %r" % (where, L["weight"][i], f["weight"][i]))
        p1, p2 = np.array([L["x1"][i], L["y1"][i]]), np.array([L["x2"][i], L["y2"][i]])
        if f["gap"][i] < 1e-3:
            n_undefined += 1
            q = np.array([f["cx"][i], f["cy"][i]])
            v = p2 - p1
            nv = float(np.hypot(*v))
            dist = float(np.hypot(*(q - p1))) if nv == 0 else abs(v[0] * (q - p1)[1] - v[1] * (q - p1)[0]) / nv
            if not dist <= tol:
                _fail(frame, "segments", "%s (no defined axis): centroid %.4f px off the line (tol %.4f)" % (where, dist, tol))
            continue
        etol = 1e-4 + EPS * float(f["extent"][i])
        if not abs(L["err"][i] - f["err"][i]) <= etol:
            _fail(frame, "segments", "%s: err %r f64 %r (tol %r)" % (where, L["err"][i], f["err"][i], etol))
        r1, r2 = np.array([f["x1"][i], f["y1"][i]]), np.array([f["x2"][i], f["y2"][i]])
        ordered = max(np.abs(p1 - r1).max(), np.abs(p2 - r2).max())
        if abs(f["d_r"][i] - f["d_c"][i]) > 1e-4:
            dv = p2 - p1  # (x, y) = (col, row)
            if dv[1] < dv[0] and np.hypot(*dv) > 0:
                _fail(frame, "segments", "%s: p1 -> p2 = %s has row component < col component" % (where, dv))
            off = ordered
        else:
            off = min(ordered, max(np.abs(p1 - r2).max(), np.abs(p2 - r1).max()))
        if not off <= tol:
            _fail(frame, "segments", "%s: endpoints %s %s, f64 %s %s (off %.5f, tol %.5f)" % (where, p1, p2, r1, r2, off, tol))
    return n_undefined


def check_stages(frame, img, st, check_flood=True):
    """All stage-chained rules on one frame.  st: dx, dy, dmask (before the flood), maxmag, seed_idx, seed_bin,
    seed_thr, label, lines -- one implementation's fp32 outputs.  Returns the ambiguity counts."""
    dx = np.asarray(st["dx"], np.float32)
    dy = np.asarray(st["dy"], np.float32)
    check_filter(frame, np.asarray(img, np.float32), dx, dy)
    bits = check_dmask(frame, dx, dy, st["dmask"])
    m64 = check_maxmag(frame, dx, dy, st["maxmag"])
    amb_seeds, amb_px = check_seeds(frame, dx, dy, bits, m64, st["seed_idx"], st["seed_bin"], st["seed_thr"])
    out = dict(seeds=len(st["seed_idx"]), ambiguous_seed_px=amb_px, seeds_taken_from_device=amb_seeds)
    if not check_flood:
        return out
    taken = check_labels(frame, dx, dy, st["dmask"], st["seed_idx"], st["seed_bin"], st["label"])
    labelled = int((np.asarray(st["label"]) >= 0).sum())
    if taken > 1e-4 * max(labelled, 1) and taken > 0:
        _fail(frame, "labels", "%d of %d labelled pixels decided by the device (> 1e-4)" % (taken, labelled))
    out.update(labelled=labelled, flood_px_taken_from_device=taken)
    out["no_axis_components"] = check_segments(frame, dx, dy, st["label"], st["seed_bin"], st["lines"])
    out["components"] = len(st["lines"])
    return out
