"""The JPEG encoder without a GPU: tests/numpy_jpeg_ref.py (the second source the GPU is compared with, byte for byte) against
the known answers of tests/golden/jpeg_kat.npz (tools/make_jpeg_fixtures.py: its streams, PIL's decode of them, PIL's own
encoder's size and PSNR), the two yardsticks, jpeg_table and jpeg_bound, and the recipe's --jpeg without a device.

The yardsticks' cases and bounds: the synth.frame-derived colour frame 203 x 117 in both layouts and the gray frame
257 x 131 at qualities 50, 90 and 95; PIL's decode of the reference's stream is at most 0.1 dB below PIL's own encoder at
the same quality and layout (optimize=False), and len(stream) - 3 * intervals <= 1.01 * PIL's size (the 3 bytes per
interval are the marker and padding that PIL's stream does not have).  Recorded: -0.015 .. +0.031 dB and 0.986 .. 0.999."""
import hashlib
import io
import os
import subprocess

import numpy as np
import pytest

import numpy_jpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
CASES = [(name, q) for name in ("c420", "c444", "g") for q in (50, 90, 95)]


@pytest.fixture(scope="module")
def kat():
    return dict(np.load(os.path.join(G, "jpeg_kat.npz")))


@pytest.fixture(scope="module")
def sources(kat):
    src = dict(c=R.synth_u8(203, 117, 21, True), g=R.synth_u8(257, 131, 12, False))
    for k, a in src.items():
        assert hashlib.sha256(a.tobytes()).digest() == kat["sha_" + k].tobytes(), "the regenerated source %s is the fixture's" % k
    return src


def case(sources, name):
    return sources[name[0]], (1 if name == "c444" else 0)


@pytest.mark.parametrize("name,q", CASES)
def test_reference_reproduces_the_fixture_streams(kat, sources, name, q):
    img, layout = case(sources, name)
    assert R.encode(img, q, layout) == kat["stream_%s_%d" % (name, q)].tobytes()


def test_the_kept_decode_gives_the_recorded_psnr(kat, sources):
    dec = sources["g"].astype(np.int16) + kat["decode_g_95"]
    assert dec.min() >= 0 and dec.max() <= 255
    assert abs(R.psnr(dec, sources["g"]) - float(kat["ref_g_95"][0])) < 1e-9


@pytest.mark.parametrize("name,q", CASES)
def test_quality_yardstick(kat, name, q):
    ours, pil = float(kat["ref_%s_%d" % (name, q)][0]), float(kat["pil_%s_%d" % (name, q)][1])
    print("%s q%d: PIL's decode of the reference's stream %.3f dB, PIL's own encoder %.3f dB" % (name, q, ours, pil))
    assert ours >= pil - 0.1


@pytest.mark.parametrize("name,q", CASES)
def test_size_yardstick(kat, sources, name, q):
    img, layout = case(sources, name)
    stream = kat["stream_%s_%d" % (name, q)]
    n = R.intervals(img.shape[1], img.shape[0], layout, 1 if img.ndim == 2 else 3)
    assert stream.tobytes().count(b"\xFF\xD0") + sum(stream.tobytes().count(bytes([0xFF, 0xD0 + m])) for m in range(1, 8)) >= n - 1
    pil = float(kat["pil_%s_%d" % (name, q)][0])
    print("%s q%d: %d bytes in %d intervals, PIL %d: %.4f" % (name, q, len(stream), n, pil, (len(stream) - 3 * n) / pil))
    assert len(stream) - 3 * n <= 1.01 * pil


@pytest.mark.parametrize("name,q", CASES)
def test_live_decode_with_pil(kat, sources, name, q):
    Image = pytest.importorskip("PIL.Image")
    img, _ = case(sources, name)
    dec = np.asarray(Image.open(io.BytesIO(kat["stream_%s_%d" % (name, q)].tobytes())))
    assert dec.shape == img.shape and dec.dtype == np.uint8
    assert abs(R.psnr(dec, img) - float(kat["ref_%s_%d" % (name, q)][0])) <= 0.1


def test_stream_structure():
    img = R.synth_u8(70, 50, 5, True)
    s = R.encode(img, 80, 0)
    assert s[:4] == b"\xFF\xD8\xFF\xE0" and s[6:11] == b"JFIF\x00" and s[11:13] == b"\x01\x01" and s[-2:] == b"\xFF\xD9"
    assert len(R.header(70, 50, 80, 0, 3)) == 629 and len(R.header(70, 50, 80, 0, 1)) == 334
    dri = s.index(b"\xFF\xDD")
    assert s[dri + 2:dri + 6] == b"\x00\x04\x00\x10", "DRI: 16 MCUs of 4:2:0"
    assert R.restart_interval(70, 1, 3) == 32 and R.restart_interval(70, 0, 1) == 96
    # the IJG quality rule
    assert R.quant_table(R.K1_LUMA, 50).tolist() == R.K1_LUMA[R.ZIGZAG].tolist()
    assert set(R.quant_table(R.K1_LUMA, 100).tolist()) == {1} and R.quant_table(R.K1_CHROMA, 1).max() == 255
    assert R.quant_table(R.K1_LUMA, 75)[0] == 8 and R.quant_table(R.K1_LUMA, 25)[0] == 32
    # RSTm cycle 0..7 and come after every interval but the last
    big = R.encode(R.synth_u8(256, 200, 6, False), 60, 0)
    scan = big[big.index(b"\xFF\xDA"):]
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert marks == [0xD0 + (i & 7) for i in range(R.intervals(256, 200, 0, 1) - 1)] and len(marks) == 8
    # 4:2:0 luminance blocks wholly outside the frame are dummies
    coefs, _ = R.coefficients(R.synth_u8(17, 8, 7, True), 90, 0)
    assert coefs.shape == (2, 6, 64) and (coefs[:, 2:4, 0] == R.DUMMY).all() and (coefs[1, 1, 0] == R.DUMMY)
    assert (coefs[0, :2, 0] != R.DUMMY).all() and coefs[1, 0, 0] != R.DUMMY and (coefs[:, 4:, 0] != R.DUMMY).all()


def adversarial_frames():
    """what makes a stream long: noise, and blocks alternating 0 and 255, at quality 100"""
    rng = np.random.default_rng(11)
    by, bx = np.mgrid[0:5, 0:7]
    checks = np.kron(((by + bx) & 1) * 255, np.ones((8, 8), np.int64)).astype(np.uint8)
    pixel_checks = (((np.mgrid[0:33, 0:17][0] + np.mgrid[0:33, 0:17][1]) & 1) * 255).astype(np.uint8)
    gray = [rng.integers(0, 256, (33, 17), dtype=np.uint8), checks, pixel_checks, rng.integers(0, 2, (16, 16), dtype=np.uint8) * 255]
    return gray + [np.stack([g, np.roll(g, 1, axis=1), 255 - g], axis=-1) for g in gray]


def test_jpeg_bound_holds_on_adversarial_blocks():
    import librectify_amd as L

    for img in adversarial_frames():
        h, w = img.shape[:2]
        for layout in ((0,) if img.ndim == 2 else (0, 1)):
            fmt = L.PIX_U8 if img.ndim == 2 else L.PIX_U8X3
            bound = L.jpeg_bound(w, h, fmt, layout)
            assert bound == R.bound(w, h, 1 if img.ndim == 2 else 3, layout)
            for q in (100, 1):
                assert len(R.encode(img, q, layout)) <= bound
    assert L.jpeg_bound(1, 1, L.PIX_U8, 0) == 640 + 2 + 416 and L.jpeg_bound(17, 9, L.PIX_U8X3, 0) == 640 + 2 + 416 * 12
    assert L.jpeg_bound(17, 9, L.PIX_U8X3, 1) == 640 + 2 + 416 * 18 and L.jpeg_bound(65535, 65535, L.PIX_U8, 0) > 2 ** 34
    for bad in ((0, 5, L.PIX_U8, 0), (5, 65536, L.PIX_U8, 0), (5, 5, L.PIX_F32, 0), (5, 5, L.PIX_U8, 1), (5, 5, L.PIX_U8X3, 2)):
        assert L.jpeg_bound(*bad) == 0


def test_jpeg_table():
    import librectify_amd as L

    t = L.jpeg_table([(203, 117), (64, 16)], [(5, 610), (80000, 192)], [(9000, 500), (0, 9000)], [95, 10], [0, 1])
    assert t.dtype == np.float64 and t.shape == (2, 8)
    np.testing.assert_array_equal(t, [[203, 117, 5, 610, 9000, 500, 95, 0], [64, 16, 80000, 192, 0, 9000, 10, 1]])
    np.testing.assert_array_equal(L.jpeg_table([(3, 2)], [(0, 9)], [(0, 0)], 50), [[3, 2, 0, 9, 0, 0, 50, 0]])
    good = dict(sizes=[(3, 2), (4, 4)], sources=[(0, 9), (18, 12)], outputs=[(0, 100), (100, 100)], quality=90, layout=0)
    for bad in (dict(sizes=[(0, 2), (4, 4)]), dict(sizes=[(3, 65536), (4, 4)]), dict(sizes=[(3.5, 2), (4, 4)]), dict(sizes=[]),
                dict(sources=[(-1, 9), (18, 12)]), dict(sources=[(0, 9)]), dict(outputs=[(0, 100), (99, 100)]),
                dict(outputs=[(0, 2 ** 53 + 2), (2 ** 54, 1)]), dict(quality=0), dict(quality=101), dict(quality=[90, 90, 90]),
                dict(quality=90.5), dict(layout=2), dict(layout=-1), dict(layout=[0, 1, 0])):
        kw = dict(good)
        kw.update(bad)
        with pytest.raises(ValueError):
            L.jpeg_table(**kw)
    assert "lr_encode_jpeg_device" not in L.EXPORTS and L.WARP_JPEG == 0x2000
    assert L.WARP_JPEG & (L.WARP_PREPARE | L.WARP_PACKED | L.WARP_RAGGED | L.WARP_LINES | 0x400 | 0x10000 | (1 << 30) | 0xFF) == 0


def test_recipe_with_jpeg_and_no_gpu_writes_the_csv_files_and_fails(tmp_path):
    from librectify_amd import build

    build.build(verbose=False)
    exe = str(tmp_path / "rectify_recipe")
    lib_dir = os.path.join(ROOT, "librectify_amd")
    src = os.path.join(ROOT, "examples", "rectify_recipe.cpp")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Wextra", "-Werror", src, "-I", os.path.join(ROOT, "include"),
                           "-L", lib_dir, "-l:librectify_amd.so", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    usage = subprocess.run([exe], text=True, capture_output=True)
    assert usage.returncode == 2 and "--jpeg Q" in usage.stderr
    a = np.load(os.path.join(G, "doc_image_gray.npy"))[:200, :300]
    pgm = str(tmp_path / "doc.pgm")
    with open(pgm, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (a.shape[1], a.shape[0]) + a.tobytes())
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    for q in ("0", "101", "x"):
        r = subprocess.run([exe, pgm, str(tmp_path / "bad"), "--jpeg", q], text=True, capture_output=True, env=env)
        assert r.returncode == 2 and "unknown or incomplete option" in r.stderr
    r = subprocess.run([exe, pgm, str(tmp_path / "out"), "--jpeg", "90", "--lines"], text=True, capture_output=True, env=env)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert "failed" in r.stderr and "unknown or incomplete option" not in r.stderr
    assert len(open(str(tmp_path / "out_tform.csv")).read().split()) == 6
    assert not os.path.exists(str(tmp_path / "out_warp.jpg")) and not os.path.exists(str(tmp_path / "out_warp_lines.jpg"))
