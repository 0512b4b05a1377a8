"""Rectified images without a GPU: the demo's homography through the C ABI, the warp's second source against the
reference's own rectified picture (doc/image.jpg_warp.jpg), and the recipe's --warp without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import numpy_warp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def L():
    import librectify_amd as L
    from librectify_amd import build

    build.build(verbose=False)
    L.lib()
    return L


def transform(L, corners, width, height):
    t = L.ImageTransform()
    t.width, t.height = width, height
    t.top_left, t.top_right, t.bottom_left, t.bottom_right = [L.Point(float(x), float(y), 0.0) for x, y in corners]
    return t


def golden_transform(L):
    rows = [[float(v) for v in line.split(",")] for line in open(os.path.join(G, "doc_warp_tform.csv"))]
    return transform(L, [r[:2] for r in rows[:4]], 1000, 563)


def test_homography_of_the_golden_transform(L):
    t = golden_transform(L)
    H, M, size = L.rectification_homography(t, 3.0)
    assert size == (1132, 594)  # the size of doc/image.jpg_warp.jpg
    assert H[2, 2] == 1.0
    # the shifted corners as the demo computes them, in float
    c = t.as_array()[:4, :2]
    f = np.float32
    lo, hi = c.min(axis=0), c.max(axis=0)
    size = np.minimum(hi - lo, np.array([1000, 563], f) * f(3.0))
    origin = (hi + lo) / f(2) - f(0.5) * size
    for (sx, sy), target in zip([(0, 0), (1000, 0), (0, 563), (1000, 563)], (c - origin).astype(np.float64)):
        p = H @ np.array([sx, sy, 1.0])
        np.testing.assert_allclose(p[:2] / p[2], target, atol=1e-6, rtol=0)
    np.testing.assert_allclose(M @ H, np.eye(3), atol=1e-12, rtol=0)


def test_homography_crops_a_wide_transform_about_its_centre(L):
    # corners spread over 5x the frame's width: the output is int(3 * w) wide, centred on the bounding box
    t = transform(L, [(-1000, 0), (1500, 10), (-900, 480), (1400, 470)], 500, 480)
    H, M, (w, h) = L.rectification_homography(t, 3.0)
    assert (w, h) == (1500, 480)
    p = H @ np.array([0.0, 0.0, 1.0])
    # the bounding box's centre (250, 240) lands on the output's centre (750, 240): x0 = 250 - 750 = -500
    np.testing.assert_allclose(p[:2] / p[2], [-1000 + 500, 0.0], atol=1e-6)
    _, _, (w2, h2) = L.rectification_homography(t, 2.0)
    assert (w2, h2) == (1000, 480)
    np.testing.assert_allclose(M @ H, np.eye(3), atol=1e-12)


@pytest.mark.parametrize(
    "corners,clip,why",
    [
        ([(float("nan"), 0), (10, 0), (0, 10), (10, 10)], 3.0, "not finite"),
        ([(0, 0), (float("inf"), 0), (0, 10), (10, 10)], 3.0, "not finite"),
        ([(0, 0), (10, 0), (0, 10), (10, 10)], 0.0, "clip"),
        ([(0, 0), (10, 0), (0, 10), (10, 10)], -1.0, "clip"),
        ([(0, 0), (10, 0), (0, 10), (10, 10)], float("nan"), "clip"),
        ([(0, 0), (0.5, 0), (0, 10), (0.5, 10)], 3.0, "smaller than one pixel"),
        ([(0, 0), (10, 0), (0, 0.25), (10, 0.25)], 3.0, "smaller than one pixel"),
        ([(0, 0), (10, 0), (20, 0), (10, 10)], 3.0, "singular"),
        ([(0, 0), (10, 10), (5, 5), (0, 20)], 3.0, "singular"),
    ],
)
def test_homography_errors(L, corners, clip, why):
    t = transform(L, corners, 10, 10)
    H = np.zeros(9)
    w, h = C.c_int(-1), C.c_int(-1)
    rc = L.lib().lr_rectification_homography(C.byref(t), clip, H.ctypes.data_as(C.c_void_p), None, C.byref(w), C.byref(h))
    assert rc != 0
    assert why in L.lib().lr_last_error().decode()
    assert (w.value, h.value) == (-1, -1) and not H.any()


def test_homography_accepts_null_outputs(L):
    t = golden_transform(L)
    assert L.lib().lr_rectification_homography(C.byref(t), 3.0, None, None, None, None) == 0
    assert L.lib().lr_rectification_homography(None, 3.0, None, None, None, None) != 0


def _stats(a, b):
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    return d.mean(), np.percentile(d, 99)


def test_second_source_reproduces_the_reference_rectified_picture(L):
    """The demo warped the colour frame with OpenCV and wrote a JPEG; its luma against the warp of our luma by the
    same M: JPEG noise only (mean 0.73, p99 4).  The pin is sharp: half a pixel, one pixel or nearest-neighbour
    sampling each miss it by a wide margin."""
    _, M, (w, h) = L.rectification_homography(golden_transform(L), 3.0)
    src = np.load(os.path.join(G, "doc_image_gray.npy"))
    gold = np.load(os.path.join(G, "doc_warp_gray.npz"))["gray"]
    assert gold.shape == (h, w)
    mean, p99 = _stats(R.warp(src, M, w, h), gold)
    assert mean <= 1.0 and p99 <= 5, (mean, p99)

    def shifted(dx, dy):
        return np.array([[1, 0, dx], [0, 1, dy], [0, 0, 1.0]]) @ M

    for Mv in (shifted(0.5, 0.5), shifted(1.0, 0.0), shifted(0.0, 1.0)):
        mean, p99 = _stats(R.warp(src, Mv, w, h), gold)
        assert mean > 1.0 or p99 > 5, (mean, p99)
    X, Y = R.fixed_coords(M, w, h)
    nx, ny = (X + 16) >> 5, (Y + 16) >> 5
    ok = (nx >= 0) & (nx < src.shape[1]) & (ny >= 0) & (ny < src.shape[0])
    nearest = np.where(ok, src[np.clip(ny, 0, src.shape[0] - 1), np.clip(nx, 0, src.shape[1] - 1)], 0)
    mean, p99 = _stats(nearest, gold)
    assert mean > 1.0 or p99 > 5, (mean, p99)


def test_second_source_edge_conventions():
    """What the canonical arithmetic says in the corners of its definition: identity = copy, W0 == 0 on a row takes
    source pixel (0, 0), a NaN coordinate is outside, u8 rounding and f32 weights."""
    src = (np.arange(35, dtype=np.int64).reshape(5, 7) * 7 % 256).astype(np.uint8)
    np.testing.assert_array_equal(R.warp(src, np.eye(3), 7, 5), src)
    f = np.random.default_rng(1).random((5, 7), dtype=np.float32)
    np.testing.assert_array_equal(R.warp(f, np.eye(3), 7, 5), f)
    # W0 = y - 2: zero on row 2, where every pixel takes the value of source pixel (0, 0)
    M = np.array([[1.0, 0, 0], [0, 1, 0], [0, 1, -2]])
    out = R.warp(src, M, 7, 5)
    assert (out[2] == src[0, 0]).all()
    # half a pixel to the right: (a + b + 1) // 2 rounding of the 5-bit weights
    Mh = np.array([[1.0, 0, 0.5], [0, 1, 0], [0, 0, 1]])
    out = R.warp(src, Mh, 7, 5)
    exp = (src[:, :-1].astype(int) * 512 + src[:, 1:].astype(int) * 512 + 512) >> 10
    np.testing.assert_array_equal(out[:, :-1], exp)
    np.testing.assert_array_equal(out[:, -1], (src[:, -1].astype(int) * 512 + 512) >> 10)
    # a tiny W0: 32 / W0 overflows, 0 * inf is NaN (INT_MIN), 1 * inf is INT_MAX: all outside
    Mt = np.array([[1.0, 0, 0], [0, 1, 0], [0, 0, 1e-320]])
    X, Y = R.fixed_coords(Mt, 3, 2)
    assert X[0, 0] == -2**31 and X[0, 1] == 2**31 - 1 and Y[1, 0] == 2**31 - 1
    assert not R.warp(src, Mt, 3, 2).any()


def test_recipe_with_warp_and_no_gpu_writes_the_csv_files_and_fails(tmp_path, L):
    exe = str(tmp_path / "rectify_recipe")
    lib_dir = os.path.join(ROOT, "librectify_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "rectify_recipe.cpp"),
                           "-I", os.path.join(ROOT, "include"), "-L", lib_dir, "-l:librectify_amd.so",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    a = np.load(os.path.join(G, "doc_image_gray.npy"))
    pgm = str(tmp_path / "doc.pgm")
    with open(pgm, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (a.shape[1], a.shape[0]) + a.tobytes())
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe, pgm, str(tmp_path / "out"), "--warp"], text=True, capture_output=True, env=env)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert "warp" in r.stderr and "failed" in r.stderr
    assert open(str(tmp_path / "out_lines.csv")).read() == ""
    assert open(str(tmp_path / "out_tform.csv")).read().split() == ["0,0", "1000,0", "0,563", "1000,563", "1,0,0", "0,1,0"]
    assert not os.path.exists(str(tmp_path / "out_warp.pgm"))
