"""lr_pack_tensor_device on the GPU against its NumPy second source (tests/numpy_tensor_ref.py), byte for byte.

Shapes.  The kernel cuts a slot, by absolute address, into chunks of 16 bytes (4 f32 or 8 half elements), takes 256 chunks
(4 KB) a step and 2048 chunks (32 KB) a tile, and launches at most 2048 workgroups, each of which then loops over tiles.  So
beside the slots 1 x 1, 5 x 7, 17 x 65 and 33 x 130 there is 129 x 131: odd in both directions, more than one step in every
dtype, more than one tile with three channels or f32 (and just over one with one channel of 2 bytes), and there is one
tensor of more than 2048 tiles (64 MB), and one whose last slot lies beyond 4 GiB.  Every destination starts 4, 8 or 12 bytes
off a multiple of 16, and with an odd element count in a slot the half-element slots start 2 bytes off a multiple of 4.
"""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import numpy_tensor_ref as ref
from test_tensor_cpu import IMAGENET_MEAN, IMAGENET_STD, TIE_SCALE

pytestmark = pytest.mark.gpu

SENTINEL = 0xA7
GUARD = 64
PIX_U8, PIX_U8X3, PIX_F32 = 0, 1, 2
TENSOR = 0x10000
ELEM = {"f32": 4, "f16": 2, "bf16": 2}


@pytest.fixture(scope="module")
def L():
    import librectify_amd as L
    from librectify_amd import build

    build.build(verbose=False)
    L.lib()
    return L


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    c.set_seed(0)
    yield c
    c.close()


def P(a):
    return a.ctypes.data_as(C.c_void_p)


def picture(w, h, channels, seed):
    """all 256 levels in every channel: a 16 x 16 ramp, tiled, through a permutation per channel"""
    base = (np.arange(h)[:, None] % 16) * 16 + (np.arange(w)[None, :] % 16)
    planes = [np.random.RandomState(seed + c).permutation(256).astype(np.uint8)[base] for c in range(channels)]
    return planes[0] if channels == 1 else np.ascontiguousarray(np.stack(planes, axis=2))


def placements(H, W):
    """(w, h, left, top): the whole slot; 1 x 1 in each corner; odd left and top with pad on all four sides; as wide as the
    slot but shorter; as tall as the slot but narrower"""
    out = [(W, H, 0, 0), (1, 1, 0, 0), (1, 1, W - 1, 0), (1, 1, 0, H - 1), (1, 1, W - 1, H - 1)]
    if W >= 4 and H >= 4:
        left, top = (3 if W >= 8 else 1), (5 if H >= 12 else 1)
        out.append((W - left - 2, H - top - 1, left, top))
    if H >= 2:
        out.append((W, H // 2, 0, (H - H // 2) // 2 | 1 if H >= 5 else 1))
    if W >= 2:
        out.append((W // 2, H, 1, 0))
    seen = []
    for p in out:
        assert p[0] >= 1 and p[1] >= 1 and p[2] + p[0] <= W and p[3] + p[1] <= H, p
        if p not in seen:
            seen.append(p)
    return seen


def lay_sources(pics, bpp, seed):
    """the pictures in one region of random bytes, at odd byte offsets and with padded rows: (region, [(offset, row_bytes)])"""
    rng = np.random.RandomState(seed)
    where, end = [], 0
    for k, p in enumerate(pics):
        row = p.shape[1] * bpp + (0, 1, 5, 3)[k % 4]
        off = (end + 2 * (k % 3)) | 1
        where.append((off, row))
        end = off + row * p.shape[0]
    region = rng.randint(0, 256, end + 7).astype(np.uint8)
    for p, (off, row) in zip(pics, where):
        rows = np.lib.stride_tricks.as_strided(region[off:], (p.shape[0], p.shape[1] * bpp), (row, 1))
        rows[:] = p.reshape(p.shape[0], -1)
    return region, where


def spec_kwargs(L, spec, fmt):
    C_ = spec.channels(fmt)
    return dict(size=spec.size, dtype=spec.dtype, layout=spec.layout, scale=spec.scale[:C_], bias=spec.bias[:C_], pad=spec.pad[:C_],
                swap=spec.bgr, gray3=spec.gray3)


def pack_and_check(L, ctx, fmt, spec, n, frames, misalign=4, seed=1):
    """frames: (slot, w, h, left, top).  One call into a sentinel-filled destination that starts `misalign` bytes into its
    allocation; every named slot equals the reference, every other byte keeps the sentinel."""
    bpp = 3 if fmt == PIX_U8X3 else 1
    pics = [picture(w, h, bpp, seed + 10 * k) for k, (_, w, h, _, _) in enumerate(frames)]
    region, where = lay_sources(pics, bpp, seed)
    table = np.array([[w, h, off, row, slot, left, top, 0] for (slot, w, h, left, top), (off, row) in zip(frames, where)], np.float64)
    shape = spec.shape(n, fmt)
    slot_bytes = int(np.prod(shape[1:])) * ELEM[spec.dtype]
    total = n * slot_bytes
    want = np.full(misalign + total + GUARD, SENTINEL, np.uint8)
    kw = spec_kwargs(L, spec, fmt)
    for (slot, _, _, left, top), p in zip(frames, pics):
        want[misalign + slot * slot_bytes: misalign + (slot + 1) * slot_bytes] = ref.slot(p, left, top, **kw).reshape(-1).view(np.uint8)
    d_src = ctx.device_upload(region)
    d_dst = ctx.device_upload(np.full(len(want), SENTINEL, np.uint8))
    try:
        ctx.pack_tensor_device(d_src, len(region), fmt, table, spec, n, d_dst + misalign, total)
        got = ctx.device_download(d_dst, (len(want),), np.uint8)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first differing byte %d of %d (slot %d)" % (bad[0] - misalign, total, (bad[0] - misalign) // slot_bytes)


SHAPES = [(1, 1), (5, 7), (17, 65), (33, 130), (129, 131)]
SOURCES = [("u8", False), ("u8x3", False), ("u8x3", True), ("gray3", False), ("gray3", True)]  # (source, swap): swap where C = 3
COMBOS = [(s, sw, d, l) for (s, sw), d, l in itertools.product(SOURCES, ("f32", "f16", "bf16"), ("nchw", "nhwc"))]


def pair_shapes():
    """Two shapes per combination, not all five: the two that the combination's (dtype, layout) has met least so far.  Every
    shape still meets every dtype and both layouts (asserted), twice."""
    met = {(s, d, l): 0 for s in range(len(SHAPES)) for d in ELEM for l in ("nchw", "nhwc")}
    cases = []
    for source, swap, dtype, layout in COMBOS:
        for s in sorted(range(len(SHAPES)), key=lambda s: (met[(s, dtype, layout)], s))[:2]:
            met[(s, dtype, layout)] += 1
            cases.append((source, swap, dtype, layout, SHAPES[s]))
    assert min(met.values()) >= 2
    return cases


@pytest.mark.parametrize("source, swap, dtype, layout, size", pair_shapes())
def test_byte_for_byte_against_the_second_source(L, ctx, source, swap, dtype, layout, size):
    fmt = PIX_U8X3 if source == "u8x3" else PIX_U8
    spec = L.TensorSpec(size, dtype, layout, mean=IMAGENET_MEAN, std=IMAGENET_STD, pad=(3, 120, 255), bgr=swap, gray3=source == "gray3")
    places = placements(*size)
    frames = [(k, w, h, left, top) for k, (w, h, left, top) in enumerate(places)]
    k = COMBOS.index((source, swap, dtype, layout))
    pack_and_check(L, ctx, fmt, spec, len(frames), frames, misalign=4 * (1 + k % 3), seed=k)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_five_frames_at_unordered_slots_of_seven(L, ctx, dtype):
    """slots 1 and 4 are named by no frame: they and the 64 bytes behind the tensor keep the sentinel (pack_and_check)"""
    H, W = 17, 65
    spec = L.TensorSpec((H, W), dtype, "nchw", mean=IMAGENET_MEAN, std=IMAGENET_STD, pad=(9, 8, 7))
    frames = [(5, W, H, 0, 0), (0, 33, 9, 3, 5), (6, 1, 1, W - 1, H - 1), (2, W, 8, 0, 3), (3, 20, H, 45, 0)]
    pack_and_check(L, ctx, PIX_U8X3, spec, 7, frames, misalign=12)
    pack_and_check(L, ctx, PIX_U8, L.TensorSpec((H, W), dtype, "nhwc", pad=200), 7, frames, misalign=8)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_the_tie_scale_and_a_pad_per_channel(L, ctx, dtype):
    """the scale of tests/test_tensor_cpu.py, whose levels are exact ties in float16 and bfloat16, both ways"""
    for layout in ("nchw", "nhwc"):
        spec = L.TensorSpec((33, 130), dtype, layout, scale=TIE_SCALE, bias=0.0, pad=(1, 128, 254))
        pack_and_check(L, ctx, PIX_U8X3, spec, 2, [(1, 130, 33, 0, 0), (0, 64, 16, 33, 9)], misalign=4)
    spec = L.TensorSpec((17, 65), dtype, scale=(TIE_SCALE, -TIE_SCALE, 2 * TIE_SCALE), bias=(0.0, 1.0, -1.0), pad=(13, 26, 52), gray3=True, bgr=True)
    pack_and_check(L, ctx, PIX_U8, spec, 1, [(0, 64, 16, 1, 1)], misalign=8)


def test_more_tiles_than_workgroups(L, ctx):
    """2049 x 2731 x 3 f32 is 67 MB: 2050 tiles of 32 KB for 2048 workgroups, so some take a second tile"""
    H, W = 2049, 2731
    spec = L.TensorSpec((H, W), "f32", "nchw", mean=IMAGENET_MEAN, std=IMAGENET_STD, pad=(1, 2, 3))
    pic = picture(1999, 1501, 3, 5)
    got = ctx.pack_tensor([pic], spec)
    assert got.shape == (1, 3, H, W) and got.dtype == np.float32
    left, top = ref.place((H, W), (1999, 1501))
    want = ref.slot(pic, left, top, **spec_kwargs(L, spec, PIX_U8X3))
    assert np.array_equal(got[0].view(np.uint32), want.view(np.uint32))


def good_call(L, ctx):
    """a small valid call and everything a refusal varies: (buffers, arguments, call)"""
    H, W, n = 5, 7, 3
    pics = [picture(7, 5, 3, 1), picture(3, 2, 3, 2)]
    region, where = lay_sources(pics, 3, 3)
    table = np.array([[7, 5, where[0][0], where[0][1], 2, 0, 0, 0], [3, 2, where[1][0], where[1][1], 0, 1, 2, 0]], np.float64)
    total = n * 3 * H * W * 2
    return dict(H=H, W=W, n=n, pics=pics, region=region, table=table, total=total)


def test_refusals_leave_the_destination_as_it_was(L, ctx):
    g = good_call(L, ctx)
    H, W, n, total = g["H"], g["W"], g["n"], g["total"]
    lib = L.lib()
    d_src = ctx.device_upload(g["region"])
    d_dst = ctx.device_upload(np.full(total + GUARD, SENTINEL, np.uint8))
    spec = L.TensorSpec((H, W), "f16", pad=(1, 2, 3))
    kw = spec_kwargs(L, spec, PIX_U8X3)
    want = np.full(total + GUARD, SENTINEL, np.uint8)
    slot_bytes = total // n
    want[2 * slot_bytes: 3 * slot_bytes] = ref.slot(g["pics"][0], 0, 0, **kw).reshape(-1).view(np.uint8)
    want[:slot_bytes] = ref.slot(g["pics"][1], 1, 2, **kw).reshape(-1).view(np.uint8)

    def call(table=g["table"], batch=2, fmt=PIX_U8X3, bits=TENSOR, src=d_src, src_bytes=len(g["region"]), dst=d_dst, dst_bytes=total,
             args=True, frames=True, unused=(0, 0, 0, 0, 0, 0), **fields):
        table = np.ascontiguousarray(table, np.float64)
        a = spec.args(table, n)
        if not frames:
            a.frames = None
        for k, v in fields.items():
            if k in ("scale", "bias", "pad"):
                setattr(a, k, (C.c_double * 3)(*v))
            else:
                setattr(a, k, v)
        w_, h_, srow, ow, oh, drow = unused
        return lib.lr_warp_perspective_device(ctx._h, C.c_void_p(src), src_bytes, batch, w_, h_, srow, fmt | bits,
                                              C.cast(C.byref(a), C.c_void_p) if args else None, C.c_void_p(dst), dst_bytes, ow, oh, drow)

    def valid():
        assert lib.lr_memcpy_h2d(ctx._h, C.c_void_p(d_dst), P(np.full(total + GUARD, SENTINEL, np.uint8)), total + GUARD) == 0
        assert call() == 0, lib.lr_last_error().decode()
        np.testing.assert_array_equal(ctx.device_download(d_dst, (total + GUARD,), np.uint8), want)
        assert lib.lr_memcpy_h2d(ctx._h, C.c_void_p(d_dst), P(np.full(total + GUARD, SENTINEL, np.uint8)), total + GUARD) == 0

    def row(b, k, v):
        t = g["table"].copy()
        t[b, k] = v
        return dict(table=t)

    inf, nan = float("inf"), float("nan")
    refusals = {
        "null source": dict(src=None), "null destination": dict(dst=None), "null lr_tensor_args": dict(args=False), "null frame table": dict(frames=False),
        "batch 0": dict(batch=0), "batch above n": dict(table=np.concatenate([g["table"]] * 2), batch=4),
        "n 0": dict(n=0), "height 0": dict(height=0), "width 0": dict(width=0), "height -1": dict(height=-1),
        "tensor beyond dst_bytes": dict(dst_bytes=total - 1), "tensor beyond 2^53": dict(n=2 ** 31 - 1, height=2 ** 30, width=2 ** 30, dst_bytes=2 ** 62),
        "dtype 3": dict(dtype=3), "dtype -1": dict(dtype=-1), "layout 2": dict(layout=2), "flag 4": dict(flags=4),
        "gray3 with u8x3": dict(flags=2), "swap with one channel": dict(fmt=PIX_U8, flags=1),
        "f32 source": dict(fmt=PIX_F32), "format 7": dict(fmt=7),
        "scale inf": dict(scale=(1.0, inf, 1.0)), "bias nan": dict(bias=(0.0, 0.0, nan)),
        "a level overflows f16": dict(scale=(1.0, 300.0, 1.0)), "a level overflows f32": dict(dtype=0, scale=(1e300, 1.0, 1.0), dst_bytes=2 * total),
        "pad 0.5": dict(pad=(0.5, 0.0, 0.0)), "pad 256": dict(pad=(0.0, 256.0, 0.0)), "pad -1": dict(pad=(0.0, 0.0, -1.0)), "pad nan": dict(pad=(nan, 0.0, 0.0)),
        "width 0 in the table": row(1, 0, 0), "width above the slot's": row(1, 0, W + 1), "height 0 in the table": row(1, 1, 0), "height 2.5": row(1, 1, 2.5),
        "offset -1": row(1, 2, -1), "offset nan": row(0, 2, nan), "stride below a row": row(0, 3, 20), "slot n": row(1, 4, n), "slot -1": row(1, 4, -1),
        "left + width above the slot's": row(1, 5, W - 2), "top + height above the slot's": row(1, 6, H - 1), "left -1": row(1, 5, -1), "reserved 1": row(0, 7, 1),
        "picture beyond src_bytes": dict(src_bytes=int(g["table"][1, 2] + g["table"][1, 3] + 3 * 3) - 1), "two frames in one slot": row(1, 4, 2),
        "regions overlap": dict(dst=d_src + 64, src_bytes=len(g["region"]), dst_bytes=total, src=d_src),
        "destination 2 bytes off": dict(dst=d_dst + 2),
        "width argument": dict(unused=(1, 0, 0, 0, 0, 0)), "height argument": dict(unused=(0, 1, 0, 0, 0, 0)), "source stride argument": dict(unused=(0, 0, 1, 0, 0, 0)),
        "out_width argument": dict(unused=(0, 0, 0, 1, 0, 0)), "out_height argument": dict(unused=(0, 0, 0, 0, 1, 0)), "destination stride argument": dict(unused=(0, 0, 0, 0, 0, 1)),
    }
    for name, bit in (("PREPARE", 0x100), ("PACKED", 0x200), ("RAGGED", 0x800), ("LINES", 0x1000), ("JPEG", 0x2000), ("JPEG_DECODE", 0x4000), ("CUBIC", 0x8000),
                      ("BORDER", 0x40000), ("LENS", 0x100000), ("LENS and LENS_MODEL", 0x900000), ("AREA", 0x400000), ("an unknown bit", 0x2000000)):
        refusals["together with " + name] = dict(bits=TENSOR | bit)
    # (the region of the overlap case has to hold the tensor for the overlap to be what is refused)
    assert len(g["region"]) >= 64
    try:
        valid()
        for name, kwargs in refusals.items():
            assert call(**kwargs) != 0, name
            assert lib.lr_last_error().decode(), name
            got = ctx.device_download(d_dst, (total + GUARD,), np.uint8)
            assert (got == SENTINEL).all(), name
            src_now = ctx.device_download(d_src, (len(g["region"]),), np.uint8)
            np.testing.assert_array_equal(src_now, g["region"], name)
            valid()  # the next good call on the same context
        assert call(**row(1, 5, W - 2)) != 0
        assert "frame 1" in lib.lr_last_error().decode() and "[5]" in lib.lr_last_error().decode()  # the frame and the entry
        ctx.trim()
        valid()
        ctx.trim()
        valid()
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)


def test_pack_tensor_round_trip_and_its_refusals(L, ctx):
    spec = L.TensorSpec((33, 130), "bf16", "nhwc", mean=IMAGENET_MEAN, std=IMAGENET_STD, pad=(0, 10, 20), place="topleft")
    pics = [picture(130, 33, 3, 1), None, picture(17, 9, 3, 2)]
    got = ctx.pack_tensor(pics, spec)
    assert got.shape == (3, 33, 130, 3) and got.dtype == np.uint16
    kw = spec_kwargs(L, spec, PIX_U8X3)
    np.testing.assert_array_equal(got[0], ref.slot(pics[0], 0, 0, **kw))
    np.testing.assert_array_equal(got[1], ref.slot_of_pad(3, (33, 130), "bf16", "nhwc", spec.scale, spec.bias, spec.pad))
    np.testing.assert_array_equal(got[2], ref.slot(pics[2], 0, 0, **kw))
    center = L.TensorSpec((33, 130), "f32", gray3=True, pad=(5, 6, 7))
    gray = picture(17, 9, 1, 3)
    got = ctx.pack_tensor([gray], center)
    assert got.shape == (1, 3, 33, 130) and got.dtype == np.float32
    np.testing.assert_array_equal(got[0], ref.slot(gray, 56, 12, **spec_kwargs(L, center, PIX_U8)))
    np.testing.assert_array_equal(ctx.pack_tensor([None], center, fmt=PIX_U8)[0], ref.slot_of_pad(3, (33, 130), "f32", "nchw", center.scale, center.bias, center.pad))
    for bad in ([], [picture(131, 33, 3, 1)], [picture(4, 4, 3, 1), picture(4, 4, 1, 1)], [None], [np.zeros((4, 4), np.float32)]):
        with pytest.raises(ValueError):
            ctx.pack_tensor(bad, spec)
    with pytest.raises(ValueError):
        ctx.pack_tensor([gray], spec, out=np.zeros((1, 33, 130, 1), np.uint16))  # (no device tensor)


def test_the_torch_hand_over():
    """out= a torch tensor on the device: written in place, nothing downloaded by the call.  In a process of its own, because
    torch has to be imported BEFORE the library is loaded, as bench.py imports it (loaded after it, torch finds no device):
    tests/tensor_torch_child.py."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tensor_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TORCH_HAND_OVER_OK" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_a_slot_beyond_four_gib(L, ctx):
    """700 slots of 1024 x 1024 x 3 bf16 are 4.4 GB; only slots 0 and 699 are named, the latter at a byte offset above 2^32"""
    n, H, W = 700, 1024, 1024
    spec = L.TensorSpec((H, W), "bf16", "nchw", mean=IMAGENET_MEAN, std=IMAGENET_STD, pad=(3, 120, 255))
    slot_bytes = 3 * H * W * 2
    assert (n - 1) * slot_bytes > 2 ** 32
    pics = [picture(1000, 777, 3, 1), picture(1024, 1024, 3, 2)]
    region = np.concatenate([p.reshape(-1) for p in pics])
    table = L.tensor_table(np.array([[1000, 777], [1024, 1024]]), np.array([[0, 3000], [pics[0].nbytes, 3072]]), np.array([n - 1, 0]), spec)
    d_src = ctx.device_upload(region)
    d_dst = C.c_void_p()
    sentinel = np.full(slot_bytes, SENTINEL, np.uint8)
    try:
        L._check(L.lib().lr_device_malloc(ctx._h, n * slot_bytes, C.byref(d_dst)))
        for s in (0, 1, n - 2, n - 1):
            L._check(L.lib().lr_memcpy_h2d(ctx._h, C.c_void_p(d_dst.value + s * slot_bytes), P(sentinel), slot_bytes))
        ctx.pack_tensor_device(d_src, len(region), PIX_U8X3, table, spec, n, d_dst.value, n * slot_bytes)
        got = {s: ctx.device_download(d_dst.value + s * slot_bytes, (3, H, W), np.uint16) for s in (0, 1, n - 2, n - 1)}
    finally:
        ctx.device_free(d_src)
        if d_dst.value:
            ctx.device_free(d_dst.value)
    kw = spec_kwargs(L, spec, PIX_U8X3)
    for s, p in ((n - 1, pics[0]), (0, pics[1])):
        np.testing.assert_array_equal(got[s], ref.slot(p, *ref.place((H, W), (p.shape[1], p.shape[0])), **kw), str(s))
    for s in (1, n - 2):
        assert (got[s].view(np.uint8) == SENTINEL).all(), s


# ---- rectify_batch(tensor=) ----

def gray_frame(w, h, seed):
    from librectify_amd import synth

    return np.clip(synth.frame(w, h, seed) * 255.0, 0, 255).astype(np.uint8)


def check_tensor_results(L, ctx, frames, results, tensor, spec, jpeg, plain, none_at=()):
    """frame by frame: results[b][:-1] is rectify's with the frame's own bound; slot b is the reference's pack of the picture
    that jpeg=None returns; the tensor map takes the picture's corners in the slot where the warp's map takes them"""
    H, W = spec.size
    assert len(results) == len(frames) and tensor.shape == spec.shape(len(frames), PIX_U8)
    kw = spec_kwargs(L, spec, PIX_U8)
    for b, f in enumerate(frames):
        got = results[b]
        assert len(got) == 4
        if b in none_at:
            assert got[2] is None and got[3] is None
            np.testing.assert_array_equal(tensor[b], ref.slot_of_pad(1, (H, W), spec.dtype, spec.layout, spec.scale, spec.bias, spec.pad))
            continue
        _, M, size = L.rectification_homography(got[1], 3.0)
        N = L.fit_box(size, (W, H))
        exp = ctx.rectify(f, out_max_size=N, jpeg=jpeg)
        assert len(exp) == 3 and got[0].tobytes() == exp[0].tobytes() and bytes(got[1]) == bytes(exp[1])
        if jpeg is None:
            np.testing.assert_array_equal(got[2], exp[2])
        else:
            assert got[2] == exp[2]
        pic = plain[b]
        assert pic.shape[0] <= H and pic.shape[1] <= W
        left, top = ref.place((H, W), (pic.shape[1], pic.shape[0]), spec.place)
        np.testing.assert_array_equal(tensor[b], ref.slot(pic, left, top, **kw))
        _, M2, size2, _ = L.shrink_homography(None, M, size, N)
        assert size2 == (pic.shape[1], pic.shape[0]) and got[3].shape == (3, 3) and got[3].dtype == np.float64
        for x, y in ((0, 0), (size2[0] - 1, 0), (0, size2[1] - 1), (size2[0] - 1, size2[1] - 1)):
            a, c = got[3] @ [left + x, top + y, 1.0], M2 @ [x, y, 1.0]
            np.testing.assert_allclose(a[:2] / a[2], c[:2] / c[2], rtol=1e-12, atol=1e-9)


def test_rectify_batch_into_a_tensor(L, ctx, monkeypatch):
    """Four small frames of two shapes.  Frame 2 is flat and has no segments: its transform is the identity, so its picture is
    the frame itself, bounded like the others (a frame without segments still has a homography).  Frame 3's transform is
    replaced by one with three collinear corners, as tests/test_gpu_rectify_batch.py does it: no homography, `warped` None, a
    map of None and a slot of nothing but pad."""
    frames = [gray_frame(320, 240, 41), gray_frame(300, 200, 42), np.full((240, 320), 128, np.uint8), gray_frame(320, 240, 43)]
    spec = L.TensorSpec((96, 160), "f16", mean=0.45, std=0.225, pad=7)
    marked = ctx.rectify(frames[3])[0].tobytes()
    assert len(ctx.rectify(frames[2])[0]) == 0 and len(marked) > 0
    flat = L.ImageTransform()
    flat.width, flat.height = 320, 240
    flat.top_left, flat.top_right, flat.bottom_left, flat.bottom_right = [L.Point(x, y, 0.0) for x, y in ((0, 0), (160, 120), (320, 240), (320, 0))]
    real = L.compute_rectification_transform
    monkeypatch.setattr(L, "compute_rectification_transform",
                        lambda lines, w, h, cfg=None: flat if np.ascontiguousarray(lines, L.LINE_DTYPE).tobytes() == marked else real(lines, w, h, cfg))
    today = ctx.rectify_batch(frames)
    assert today[3][2] is None and all(len(r) == 3 for r in today)
    results, tensor = ctx.rectify_batch(frames, tensor=spec)
    plain = [r[2] for r in results]
    check_tensor_results(L, ctx, frames, results, tensor, spec, None, plain, none_at=(3,))
    assert plain[2].shape == (96, 129)  # (the flat frame: 320 x 240 into 160 x 96 is fit_box's N = 129)
    results, tensor_j = ctx.rectify_batch(frames, tensor=spec, jpeg=90)
    check_tensor_results(L, ctx, frames, results, tensor_j, spec, 90, plain, none_at=(3,))
    np.testing.assert_array_equal(tensor_j, tensor)
    # one shape: the packed warp's path
    same = [frames[0], frames[2], frames[3]]
    results, tensor_s = ctx.rectify_batch(np.stack(same), tensor=spec)
    check_tensor_results(L, ctx, same, results, tensor_s, spec, None, [plain[0], plain[2], None], none_at=(2,))
    # one frame
    (lines, t, pic, tmap), one = ctx.rectify(frames[1], tensor=spec)
    np.testing.assert_array_equal(pic, plain[1])
    np.testing.assert_array_equal(one[0], tensor[1])
    # without tensor=: what the calls return today
    again = ctx.rectify_batch(frames)
    for g, w_ in zip(again, today):
        assert len(g) == 3 and g[0].tobytes() == w_[0].tobytes() and bytes(g[1]) == bytes(w_[1])
        assert (g[2] is None and w_[2] is None) or np.array_equal(g[2], w_[2])
    monkeypatch.undo()
    for g, f in zip(ctx.rectify_batch(frames[:3], jpeg=90), frames[:3]):
        e = ctx.rectify(f, jpeg=90)
        assert len(g) == 3 and g[0].tobytes() == e[0].tobytes() and bytes(g[1]) == bytes(e[1]) and g[2] == e[2]
    with pytest.raises(ValueError, match="out_max_size"):
        ctx.rectify_batch(frames, tensor=spec, out_max_size=64)
    with pytest.raises(ValueError, match="tensor"):
        ctx.rectify_batch(frames, tensor_out=tensor)


def test_rectify_files_into_a_tensor(L, ctx):
    """JPEG files in: decoded, rectified, bounded, packed (and encoded) without a pixel crossing the link"""
    frames = [gray_frame(320, 240, 41), gray_frame(300, 200, 42), np.full((240, 320), 128, np.uint8)]
    data = [ctx.encode_jpeg(f, 95) for f in frames]
    decoded = [ctx.decode_jpeg(d, L.PIX_U8) for d in data]
    spec = L.TensorSpec((160, 96), "bf16", "nhwc", mean=0.45, std=0.225, pad=200, place="topleft")
    results, tensor = ctx.rectify_batch(data, tensor=spec)
    plain = [r[2] for r in results]
    check_tensor_results(L, ctx, decoded, results, tensor, spec, None, plain)
    results, tensor_j = ctx.rectify_batch(data, tensor=spec, jpeg=90)
    check_tensor_results(L, ctx, decoded, results, tensor_j, spec, 90, plain)
    np.testing.assert_array_equal(tensor_j, tensor)
    today = ctx.rectify_batch(data, jpeg=90)
    for g, f in zip(today, decoded):
        e = ctx.rectify(f, jpeg=90)
        assert len(g) == 3 and g[0].tobytes() == e[0].tobytes() and bytes(g[1]) == bytes(e[1]) and g[2] == e[2]
