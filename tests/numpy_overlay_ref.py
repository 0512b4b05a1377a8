"""Second source of the lines picture (lr_draw_lines_device): the rule of DESIGN.md section 3 in NumPy int64, written as
the demo's loop (autorectify.cpp:89-109) -- segment after segment, each one painted over what is there.  No tiles, no bins,
no search for the highest index: a later segment simply overwrites an earlier one.

The rule, for a pixel (x, y) and a segment with truncated endpoints (X1, Y1), (X2, Y2):
    p = (x - X1, y - Y1), d = (X2 - X1, Y2 - Y1), dd = d.d, t = p.d, c = p.x d.y - p.y d.x
    stroke: 4 |p|^2 <= 9 if t <= 0; else 4 |p - d|^2 <= 9 if t >= dd; else 4 c^2 <= 9 dd
    discs:  |p|^2 <= 25 or |p - d|^2 <= 25
int64 holds every product once the stroke's last case is entered only where |c| <= 3 max(|d.x|, |d.y|); that this early
reject changes nothing is checked against Python's unbounded integers by covered_python (tests/test_overlay_cpu.py)."""
import numpy as np

# (c0, c1, c2), c0 red: the demo's palette (autorectify.cpp:75-87, BGR) in this project's channel order
PALETTE = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 255, 255), (255, 0, 255), (255, 255, 0),
           (128, 0, 0), (0, 128, 0), (0, 0, 128), (0, 128, 128), (128, 0, 128), (128, 128, 0)]
UNGROUPED = (255, 255, 255)
MAX_COORD = 2 ** 24
REACH = 5  # the disc's radius


def colour(group_id):
    g = int(group_id)
    return UNGROUPED if g < 0 else PALETTE[g % 12]


def _truncate(v):
    """int(v) as the demo's cv::Point(int(x), int(y)): toward zero; None for what is not drawn"""
    if not np.isfinite(v):
        return None
    t = int(v)  # Python truncates toward zero, exactly
    return t if abs(t) <= MAX_COORD else None


def endpoints(line, H=None):
    """(X1, Y1, X2, Y2) of one LINE_DTYPE record, or None if the segment is not drawn.  With H every endpoint goes through
    it first, in float64, every product and sum rounded on its own."""
    pts = [(float(line["x1"]), float(line["y1"])), (float(line["x2"]), float(line["y2"]))]
    if H is not None:
        h = [float(v) for v in np.asarray(H, np.float64).reshape(9)]
        with np.errstate(all="ignore"):
            den = [np.float64(h[6]) * x + np.float64(h[7]) * y + np.float64(h[8]) for x, y in pts]
            if not ((den[0] > 0 and den[1] > 0) or (den[0] < 0 and den[1] < 0)):
                return None
            pts = [((np.float64(h[0]) * x + np.float64(h[1]) * y + np.float64(h[2])) / dn,
                    (np.float64(h[3]) * x + np.float64(h[4]) * y + np.float64(h[5])) / dn) for (x, y), dn in zip(pts, den)]
    out = [_truncate(v) for p in pts for v in p]
    return None if any(v is None for v in out) else tuple(out)


def shape_mask(xs, ys, seg, discs=True, stroke=True):
    """the rule on int64 grids xs, ys (broadcastable) for truncated endpoints seg: a boolean mask"""
    X1, Y1, X2, Y2 = seg
    px, py = xs.astype(np.int64) - X1, ys.astype(np.int64) - Y1
    dx, dy = np.int64(X2 - X1), np.int64(Y2 - Y1)
    qx, qy = px - dx, py - dy
    dd = dx * dx + dy * dy
    covered = np.zeros(np.broadcast(px, py).shape, bool)
    if stroke:
        t = px * dx + py * dy
        c = px * dy - py * dx
        near = np.abs(c) <= 3 * max(abs(int(dx)), abs(int(dy)))  # the early reject: 4 c^2 <= 9 dd needs |c| <= 1.5 |d|
        cs = np.where(near, c, 0)
        covered |= np.where(t <= 0, 4 * (px * px + py * py) <= 9,
                            np.where(t >= dd, 4 * (qx * qx + qy * qy) <= 9, near & (4 * cs * cs <= 9 * dd)))
    if discs:
        covered |= (px * px + py * py <= 25) | (qx * qx + qy * qy <= 25)
    return covered


def covered_python(x, y, seg, discs=True, stroke=True):
    """the rule for one pixel in Python's unbounded integers, without the early reject"""
    X1, Y1, X2, Y2 = (int(v) for v in seg)
    px, py, dx, dy = int(x) - X1, int(y) - Y1, X2 - X1, Y2 - Y1
    qx, qy = px - dx, py - dy
    dd, t, c = dx * dx + dy * dy, px * dx + py * dy, px * dy - py * dx
    hit = False
    if stroke:
        if t <= 0:
            hit = 4 * (px * px + py * py) <= 9
        elif t >= dd:
            hit = 4 * (qx * qx + qy * qy) <= 9
        else:
            hit = 4 * c * c <= 9 * dd
    if discs:
        hit = hit or px * px + py * py <= 25 or qx * qx + qy * qy <= 25
    return hit


def draw(image, lines, H=None, discs=True, stroke=True, with_owner=False):
    """The lines picture of an 8-bit frame (H x W gray, every pixel v as (v, v, v), or H x W x 3, copied) -- or, for the
    in-place call, of the destination as it is.  lines: a LINE_DTYPE array; discs / stroke: parts of the shape to paint
    (both, as the library does; the flags exist for the tests of the rule).  Returns H x W x 3 uint8 and, with_owner,
    the int64 index of the segment that owns each pixel (-1: the background)."""
    img = np.asarray(image)
    assert img.dtype == np.uint8 and (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3))
    out = np.repeat(img[:, :, None], 3, axis=2) if img.ndim == 2 else img.copy()
    h, w = out.shape[:2]
    owner = np.full((h, w), -1, np.int64)
    for i, line in enumerate(lines):  # the demo's loop: every segment paints over the ones before it
        seg = endpoints(line, H)
        if seg is None:
            continue
        X1, Y1, X2, Y2 = seg
        x_lo, x_hi = max(min(X1, X2) - REACH, 0), min(max(X1, X2) + REACH, w - 1)
        y_lo, y_hi = max(min(Y1, Y2) - REACH, 0), min(max(Y1, Y2) + REACH, h - 1)
        if x_lo > x_hi or y_lo > y_hi:
            continue
        xs = np.arange(x_lo, x_hi + 1, dtype=np.int64)[None, :]
        ys = np.arange(y_lo, y_hi + 1, dtype=np.int64)[:, None]
        m = shape_mask(xs, ys, seg, discs, stroke)
        out[y_lo:y_hi + 1, x_lo:x_hi + 1][m] = colour(line["group_id"])
        owner[y_lo:y_hi + 1, x_lo:x_hi + 1][m] = i
    return (out, owner) if with_owner else out
