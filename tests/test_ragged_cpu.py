"""CPU-only checks of the mixed-size batch's host side: the LR_WARP_RAGGED option and lr_frame in the header and in the
Python mirror, ragged_table (the layout lr_warp_perspective_device takes with LR_WARP_RAGGED), and that the feature added
no export and no environment variable."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OUT_SIZES = [(1, 1), (63, 17), (64, 16), (65, 17), (400, 300), (7, 2), (1, 33)]
SOURCES = [(1, 1, 0, 1), (257, 131, 3, 260), (64, 16, 40000, 64), (65, 17, 50001, 70), (5, 7, 60000, 5), (130, 40, 70000, 133),
           (257, 131, 3, 260)]


def _header():
    return open(os.path.join(ROOT, "include", "librectify_amd.h")).read()


def _maps(n):
    return np.random.default_rng(5).normal(size=(n, 3, 3))


def test_header_and_python_agree_on_the_ragged_option():
    import librectify_amd as L

    header = _header()
    m = re.search(r"enum\s+(\w+)\s*\{\s*LR_WARP_RAGGED\s*=\s*(0x[0-9A-Fa-f]+|\d+)\s*\}", header)
    assert m, "LR_WARP_RAGGED is the one enumerator of an enum of its own"
    assert m.group(1) not in ("lr_warp_option", "lr_warp_layout", "lr_frames_option", "lr_pixel_format")
    assert int(m.group(2), 0) == 0x800 == L.WARP_RAGGED
    assert L.WARP_RAGGED & (L.WARP_PREPARE | L.WARP_PACKED | 0xFF) == 0
    # the options the header had keep their lines
    assert re.search(r"enum\s+lr_warp_option\s*\{\s*LR_WARP_PREPARE\s*=\s*0x100\s*\}", header)
    assert re.search(r"enum\s+lr_warp_layout\s*\{\s*LR_WARP_PACKED\s*=\s*0x200\s*\}", header)
    assert re.search(r"enum\s+lr_frames_option\s*\{\s*LR_FRAMES_U8\s*=\s*0x100,\s*LR_FRAMES_U8X3\s*=\s*0x200,\s*LR_FRAMES_F32\s*=\s*0x300\s*\}", header)


def test_frame_mirrors_lr_frame():
    import librectify_amd as L

    assert C.sizeof(L.Frame) == 24
    assert [getattr(L.Frame, f).offset for f in ("data", "width", "height", "stride", "min_length")] == [0, 8, 12, 16, 20]
    assert [f[0] for f in L.Frame._fields_] == ["data", "width", "height", "stride", "min_length"]
    line = r"typedef\s+struct\s+lr_frame\s*\{\s*const\s+void\s*\*\s*data;\s*int32_t\s+width,\s*height,\s*stride;\s*float\s+min_length;\s*\}\s*lr_frame;"
    assert re.search(line, _header())
    f = L.Frame(0x1234, 640, 480, 650, -1.0)
    assert (f.data, f.width, f.height, f.stride, f.min_length) == (0x1234, 640, 480, 650, -1.0)


@pytest.mark.parametrize("bpp,out_bpp", [(1, None), (3, None), (4, None), (1, 4), (3, 4), (4, 4)])
@pytest.mark.parametrize("align", [1, 4, 64])
def test_ragged_table_layout(bpp, out_bpp, align):
    import librectify_amd as L

    obpp = bpp if out_bpp is None else out_bpp
    sources = [(w, h, off * (4 if bpp == 4 else 1), (row * bpp + 3) // 4 * 4 if bpp == 4 else row * bpp) for w, h, off, row in SOURCES]
    Ms = _maps(len(SOURCES))
    if obpp == 4 and align % 4:
        with pytest.raises(ValueError):
            L.ragged_table(Ms, OUT_SIZES, sources, bpp, out_bpp, align)
        return
    table, total = L.ragged_table(Ms, OUT_SIZES, sources, bpp, out_bpp, align)
    assert table.shape == (len(SOURCES), 18) and table.dtype == np.float64 and table.flags["C_CONTIGUOUS"]
    # the packed table's thirteen columns, for the outputs' bytes per pixel
    packed, packed_total = L.warp_table(Ms, OUT_SIZES, obpp, align)
    np.testing.assert_array_equal(table[:, :13], packed)
    assert total == packed_total and isinstance(total, int)
    np.testing.assert_array_equal(table[:, 13:17], np.array(sources, np.float64))
    assert (table[:, 17] == 0).all()
    off, row = table[:, 11].astype(np.int64), table[:, 12].astype(np.int64)
    assert (off % align == 0).all() and (row % align == 0).all()
    end = off + (table[:, 10].astype(np.int64) - 1) * row + table[:, 9].astype(np.int64) * obpp
    assert off[0] == 0 and (off[1:] >= end[:-1]).all() and total == int(end[-1])


def test_ragged_table_without_maps_and_default_alignment():
    import librectify_amd as L

    table, total = L.ragged_table(None, [(3, 2), (5, 5)], [(10, 8, 1, 11), (5, 5, 100, 7)], 1, out_bpp=4)
    np.testing.assert_array_equal(table[:, :9], np.tile(np.eye(3).reshape(-1), (2, 1)))
    np.testing.assert_array_equal(table[:, 9:], [[3, 2, 0, 12, 10, 8, 1, 11, 0], [5, 5, 24, 20, 5, 5, 100, 7, 0]])
    assert total == 24 + 4 * 20 + 20


def test_ragged_table_rejects_bad_input():
    import librectify_amd as L

    ok = _maps(2)
    sizes = [(5, 3), (2, 2)]
    src = [(10, 8, 0, 10), (6, 6, 100, 8)]
    nan = ok.copy()
    nan[1, 2, 0] = np.nan
    bad = [
        dict(Ms=ok.reshape(2, 9)), dict(Ms=nan), dict(out_sizes=sizes[:1]), dict(out_sizes=[(5, 0), (2, 2)]),
        dict(out_sizes=[(5.5, 3), (2, 2)]), dict(sources=src[:1]), dict(sources=[(10, 8, 0), (6, 6, 100)]),
        dict(sources=[(0, 8, 0, 10), (6, 6, 100, 8)]), dict(sources=[(10, -1, 0, 10), (6, 6, 100, 8)]),
        dict(sources=[(10, 8, -1, 10), (6, 6, 100, 8)]), dict(sources=[(10, 8, 0, 9), (6, 6, 100, 8)]),
        dict(sources=[(10.5, 8, 0, 11), (6, 6, 100, 8)]), dict(sources=[(10, 8, 0, 29), (6, 6, 100, 24)], bpp=3),
        dict(bpp=2), dict(bpp=0), dict(out_bpp=2), dict(align=0), dict(align=2.5), dict(out_bpp=4, align=2),
        dict(bpp=4, sources=[(2, 2, 2, 8), (2, 2, 100, 8)]), dict(bpp=4, sources=[(2, 2, 0, 10), (2, 2, 100, 8)]),
        dict(sources=[(10, 8, 2 ** 53, 10), (6, 6, 100, 8)]),
    ]
    for k, change in enumerate(bad):
        kw = dict(Ms=ok, out_sizes=sizes, sources=src, bpp=1, out_bpp=None, align=4)
        kw.update(change)
        with pytest.raises(ValueError):
            L.ragged_table(**kw)
            pytest.fail("case %d was accepted" % k)
    L.ragged_table(ok, sizes, src, 1)
    L.ragged_table(ok, sizes, [(2, 2, 0, 8), (2, 2, 100, 12)], 4, align=8)
    L.ragged_table(None, sizes, src, 1, out_bpp=4)


def test_the_feature_adds_no_export_and_no_environment_variable():
    import librectify_amd as L
    from librectify_amd import build

    import test_boundary_cpu as B

    build.build(verbose=False)
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    # (61: the sixty of this feature's day and lr_set_flood_schedule, the flood's schedule hook)
    assert len(exported) == 61 == len(L.EXPORTS) and exported == sorted(L.EXPORTS)
    csrc = os.path.join(ROOT, "librectify_amd", "csrc")
    read = set()
    for name in os.listdir(csrc):
        read |= set(re.findall(r'getenv\("LIBRECTIFY_([A-Z0-9_]+)"', open(os.path.join(csrc, name)).read()))
    assert read == B.ENV_NAMES
    for name in ("warp_perspective_ragged_device", "prepare_ragged_device", "find_line_segment_groups_frames_device",
                 "rectify_frames_device", "rectify_batch"):
        assert callable(getattr(L.Context, name))
