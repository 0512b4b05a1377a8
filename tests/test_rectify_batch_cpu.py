"""CPU-only checks of the packed warp's host side: warp_table (the layout lr_warp_perspective_device takes with
LR_WARP_PACKED), the option's value in the header, and that the feature added no export and no environment variable."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [(1, 1), (63, 17), (64, 16), (65, 17), (400, 300), (7, 2), (1, 33)]


def _maps(n):
    rng = np.random.default_rng(3)
    return rng.normal(size=(n, 3, 3))


def _extents(table, bpp):
    """[first byte, end) of every frame, as the library computes them"""
    ow, oh, off, row = (table[:, k].astype(np.int64) for k in (9, 10, 11, 12))
    return off, off + (oh - 1) * row + ow * bpp


@pytest.mark.parametrize("bpp", [1, 3, 4])
@pytest.mark.parametrize("align", [1, 4, 3, 64, 256])
def test_warp_table_layout(bpp, align):
    import librectify_amd as L

    if bpp == 4 and align % 4:
        with pytest.raises(ValueError):
            L.warp_table(_maps(len(SIZES)), SIZES, bpp, align)
        return
    Ms = _maps(len(SIZES))
    table, total = L.warp_table(Ms, SIZES, bpp, align)
    assert table.shape == (len(SIZES), 13) and table.dtype == np.float64 and table.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(table[:, :9], Ms.reshape(-1, 9))
    assert [(int(r[9]), int(r[10])) for r in table] == SIZES
    assert (table[:, 9:] == np.floor(table[:, 9:])).all()
    off, end = _extents(table, bpp)
    row = table[:, 12].astype(np.int64)
    assert (off % align == 0).all() and (row % align == 0).all()
    assert (row >= table[:, 9].astype(np.int64) * bpp).all() and (row < table[:, 9].astype(np.int64) * bpp + align).all()
    # frame order, no overlap, no more than the alignment between neighbours, and the end is the last frame's
    assert off[0] == 0 and (off[1:] >= end[:-1]).all() and (off[1:] < end[:-1] + align).all()
    assert total == int(end[-1]) and isinstance(total, int)


def test_warp_table_default_alignment_is_four():
    import librectify_amd as L

    table, total = L.warp_table(_maps(2), [(5, 3), (2, 2)], 3)
    np.testing.assert_array_equal(table[:, 9:], [[5, 3, 0, 16], [2, 2, 48, 8]])
    assert total == 48 + 8 + 6
    one, total = L.warp_table(np.eye(3), [(10, 4)], 1, align=1)  # a single 3x3 map is a batch of one
    np.testing.assert_array_equal(one[0, 9:], [10, 4, 0, 10])
    assert total == 40


def test_warp_table_rejects_bad_input():
    import librectify_amd as L

    ok = _maps(2)
    sizes = [(5, 3), (2, 2)]
    nan, inf = ok.copy(), ok.copy()
    nan[1, 2, 0] = np.nan
    inf[0, 0, 0] = -np.inf
    bad = [
        (ok.reshape(2, 9), sizes, 1, 4), (ok[:, :2], sizes, 1, 4), (ok, sizes[:1], 1, 4), (ok, [(5, 3, 1), (2, 2, 1)], 1, 4),
        (ok, [(5, 0), (2, 2)], 1, 4), (ok, [(5, 3), (-2, 2)], 3, 4), (ok, [(5.5, 3), (2, 2)], 1, 4),
        (nan, sizes, 1, 4), (inf, sizes, 4, 4),
        (ok, sizes, 1, 0), (ok, sizes, 3, -4), (ok, sizes, 1, 2.5), (ok, sizes, 4, 2), (ok, sizes, 4, 6), (ok, sizes, 4, 1),
        (ok, sizes, 2, 4), (ok, sizes, 0, 4),
    ]
    for k, (Ms, sz, bpp, align) in enumerate(bad):
        with pytest.raises(ValueError):
            L.warp_table(Ms, sz, bpp, align)
            pytest.fail("case %d was accepted" % k)
    L.warp_table(ok, sizes, 4, 8)
    L.warp_table(ok, sizes, 3, 1)


def test_header_and_python_agree_on_the_packed_option():
    import librectify_amd as L

    header = open(os.path.join(ROOT, "include", "librectify_amd.h")).read()
    m = re.search(r"enum\s+\w+\s*\{[^}]*\bLR_WARP_PACKED\s*=\s*(0x[0-9A-Fa-f]+|\d+)\s*[,}]", header)
    assert m and int(m.group(1), 0) == 0x200 == L.WARP_PACKED
    assert L.WARP_PACKED & 0xFF == 0 and L.WARP_PACKED & L.WARP_PREPARE == 0
    # the option the header had keeps its line
    assert re.search(r"enum\s+lr_warp_option\s*\{\s*LR_WARP_PREPARE\s*=\s*0x100\s*\}", header)


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
    for name in ("rectify_batch", "rectify_batch_device", "warp_perspective_packed_device"):
        assert callable(getattr(L.Context, name))
