"""The detector rows (A2-A9) against a second, independent source: tests/numpy_detector_ref.py, a float64 NumPy
restatement written from the reference's text.  Here it checks the oracle stage by stage (each stage fed with the
oracle's fp32 output of the stage before), and it is pinned on its own to the reference's 848 golden rows, so that a
misreading the oracle and the kernels share shows up.  CPU only; tests/test_gpu_detector_second_source.py holds the
kernels to the same rules."""
import os

import numpy as np
import pytest

import numpy_detector_ref as N
import oracle_lib as O
from test_oracle_pins import _golden_hits, _golden_lines

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def oracle_stages(img):
    """the oracle's fp32 stage outputs in the layout check_stages takes (the device's buffers)"""
    img = np.ascontiguousarray(img, np.float32)
    h, w = img.shape
    f = O.filter_stage(img, planes=True)
    s = O.find_seeds(f["mag"], f["bin"])
    r = O.find_line_segments(img)
    thr = (np.float32(0.75) * f["planes"][s["bins"], s["rows"], s["cols"]]).astype(np.float32)
    return dict(dx=f["dx"], dy=f["dy"], dmask=f["dmask"], maxmag=f["mag"].max(), seed_idx=s["rows"] * w + s["cols"],
                seed_bin=s["bins"], seed_thr=thr, label=r["label"], lines=r["lines"])


def _frames():
    from librectify_amd import synth

    out = {c: np.load(os.path.join(G, c + ".npz"))["image"] for c in ("synth_96x64_s11", "synth_257x131_s12", "synth_320x240_s13")}
    out["noiseless 200x150"] = synth.frame(200, 150, 21, bars=12, noise=0.0)
    out["few grey levels 180x140"] = (np.round(synth.frame(180, 140, 7, bars=8) * 16) / np.float32(16)).astype(np.float32)
    return out


FRAMES = _frames()


@pytest.mark.parametrize("name", list(FRAMES))
def test_oracle_stages_against_the_second_source(name):
    img = FRAMES[name]
    counts = N.check_stages(name, img, oracle_stages(img))
    assert counts["components"] > 10, counts
    print(name, counts)
    if name.startswith("synth_"):  # noisy frames: no decision is left to the implementation
        assert counts["seeds_taken_from_device"] == 0 and counts["flood_px_taken_from_device"] == 0, counts


def test_second_source_alone_reproduces_the_golden_rows():
    """The float64 detector end to end, unchained, on the reference's doc image at TRACE_TOLERANCE 0.3 and
    filter_lines(10): >= 700 of the 848 golden rows within 0.01 px (pin 2's gate; the oracle reaches 713)."""
    gray = np.load(os.path.join(G, "doc_image_gray.npy"))
    img = gray.astype(np.float32) / np.float32(256.0)
    f = N.filter_lines(N.find_line_segments(img, tolerance=0.3), 10.0)
    lines = np.zeros(len(f["x1"]), [("x1", "f8"), ("y1", "f8"), ("x2", "f8"), ("y2", "f8")])
    for k in ("x1", "y1", "x2", "y2"):
        lines[k] = f[k]
    hits = int(_golden_hits(lines, _golden_lines()[:, :4]).sum())
    print("second source: %d of 848 golden rows" % hits)
    assert hits >= 700, hits


def test_the_checks_fail_on_a_wrong_stage():
    """each stage check fires on an output that is wrong by more than its bound (and names the frame and stage)"""
    img = FRAMES["synth_257x131_s12"]
    base = oracle_stages(img)

    def broken(**kw):
        st = dict(base)
        st.update(kw)
        return st

    dx = base["dx"].copy()
    dx.flat[np.abs(dx).argmax()] *= np.float32(1.0 + 2.0 ** -12)
    dm = base["dmask"].copy()
    dm[base["dmask"] != 0] = 0  # dilation dropped
    idx = base["seed_idx"].copy()
    idx[[0, 1]] = idx[[1, 0]]
    lab = base["label"].copy()
    lab[lab == lab.max()] = -1
    lines = base["lines"].copy()
    lines["weight"][3] *= np.float32(1.0001)
    for kw, stage in [(dict(dx=dx), "filter dx"), (dict(dmask=dm), "dmask"), (dict(maxmag=base["maxmag"] * np.float32(1.001)), "maxmag"),
                      (dict(seed_idx=idx), "seed"), (dict(seed_thr=base["seed_thr"] * np.float32(1.0001)), "seed thresholds"),
                      (dict(label=lab), "labels"), (dict(lines=lines), "segments")]:
        with pytest.raises(AssertionError, match=r"\[257x131\] %s" % stage):
            N.check_stages("257x131", img, broken(**kw))
