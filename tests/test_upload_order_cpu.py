"""The host upload path (csrc/upload.hip, ctx_find_groups_host in frame.hip, the lane loop of batch.hip) against a model
of the HIP runtime on the CPU.

That code decides correctness by ORDER -- which thread enqueues what, on which stream, behind which event -- and a GPU
shows an ordering error only when the timing is unlucky.  Here the whole library is compiled host-only and linked with
tests/cxx/model_hip (streams as in-order op lists, events, a registry of every allocation) and the harness
tests/cxx/upload_order_main.cpp, which drives the C ABI on frames whose every pixel encodes (frame, row, column) and checks,
when the model executes a filter launch, that the rows the launch reads have arrived.

Three builds (plain, address + undefined sanitizers, thread sanitizer), three schedules: ops run when enqueued (eager), only
when a synchronising call forces them (lazy), or on a worker per stream with seeded pauses (threaded, under the thread
sanitizer, where a missing stream dependency is a data race).  Everything is a stand-alone program; nothing is loaded into
Python.

Then the test shows that each check fires: copies of upload.hip and frame.hip with ONE statement taken out must fail the
harness, with the violated rule named.
"""
import concurrent.futures
import os
import re
import shutil
import subprocess
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "librectify_amd", "csrc")
CXX = os.path.join(ROOT, "tests", "cxx")


def _tool(name):
    for cand in (shutil.which(name), os.path.join("/opt/rocm/bin", name), os.path.join("/opt/rocm/lib/llvm/bin", name)):
        if cand and os.path.exists(cand):
            return cand
    return None


HIPCC = _tool("hipcc")
CLANGXX = _tool("amdclang++") or _tool("clang++")
pytestmark = pytest.mark.skipif(HIPCC is None or CLANGXX is None, reason="hipcc / clang++ of ROCm not found: the host-only build needs them")

VARIANTS = {
    "plain": [],
    "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
    "tsan": ["-fsanitize=thread", "-fno-omit-frame-pointer"],
}
MAX_COMPILES = 8

# Slowest single run of the harness, measured on a 16-core box: 13.7 s (the thread-sanitizer build under the threaded schedule,
# all groups of one process; the plain build takes 1.4 s).  Ten times that.
RUN_TIMEOUT_S = 137
# Slowest compile step measured there: 4.1 s (that is a whole variant, nineteen units eight at a time, so an upper bound for
# one unit; a link takes under a second).  Ten times that.
COMPILE_TIMEOUT_S = 41

# What a process of the harness runs.  The library reads LIBRECTIFY_UPLOAD_BAND_KB and LIBRECTIFY_REGISTER_FRAMES once per
# process: the two settings of each are two processes.
GROUPS_BANDS = "single,slow,seq,consecutive,crew,batch,batchfail"
GROUPS_WHOLE = "single,seq,consecutive,big,crew,batch,batchfail"
PROCESSES = [
    ("bands64-noregister", {"LIBRECTIFY_UPLOAD_BAND_KB": "64", "LIBRECTIFY_REGISTER_FRAMES": "0"}, GROUPS_BANDS),
    ("default-register4", {"LIBRECTIFY_REGISTER_FRAMES": "4"}, GROUPS_WHOLE),
]


def _sources(csrc):
    return sorted(f for f in os.listdir(csrc) if f.endswith(".hip") or f.endswith(".cpp"))


def _run(cmd, timeout):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stdout
    return r.stdout


def _compile_lib_unit(src_path, obj, flags, include_dir):
    _run([HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g1", "-I", include_dir, "-I", CSRC]
         + [a for f in flags for a in ("-Xarch_host", f)] + ["-c", src_path, "-o", obj], COMPILE_TIMEOUT_S)
    return obj


class Build:
    """The host-only objects of one variant, cached for the module; link() makes a harness from them, with some units
    replaced by objects compiled from changed copies of their sources."""

    def __init__(self, work, variant):
        self.dir = os.path.join(work, variant)
        self.flags = VARIANTS[variant]
        os.makedirs(self.dir, exist_ok=True)
        units = _sources(CSRC)
        self.objs = {}
        t0 = time.time()
        with concurrent.futures.ThreadPoolExecutor(MAX_COMPILES) as pool:
            jobs = {u: pool.submit(_compile_lib_unit, os.path.join(CSRC, u), os.path.join(self.dir, u + ".o"), self.flags, CSRC) for u in units}
            # the model (plain C++ against HIP's own header) and the harness (which reads the library's internal headers)
            model = pool.submit(_run, [CLANGXX, "-std=c++17", "-O1", "-g1", "-D__HIP_PLATFORM_AMD__", "-I", self._hip_include(), "-I", CXX] + self.flags
                                + ["-c", os.path.join(CXX, "model_hip", "model_hip.cpp"), "-o", os.path.join(self.dir, "model_hip.o")], COMPILE_TIMEOUT_S)
            harness = pool.submit(_compile_lib_unit, os.path.join(CXX, "upload_order_main.cpp"), os.path.join(self.dir, "upload_order_main.o"), self.flags, CXX)
            for u, j in jobs.items():
                self.objs[u] = j.result()
            model.result()
            harness.result()
        self.compile_s = time.time() - t0

    @staticmethod
    def _hip_include():
        return os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "include")

    def link(self, name, replaced=None):
        """replaced: {unit name: path of its changed source}"""
        exe = os.path.join(self.dir, name)
        if not replaced and os.path.exists(exe):
            return exe
        objs = dict(self.objs)
        for unit, src in (replaced or {}).items():
            objs[unit] = _compile_lib_unit(src, os.path.join(self.dir, name + "." + unit + ".o"), self.flags, CSRC)
        # every kernel file refers to the device code object the offload build would have embedded: words of nothing here
        undefined = _run(["nm", "-u"] + list(objs.values()), 60)
        blobs = sorted(set(re.findall(r"\b(__hip_fatbin_[0-9a-f]+)\b", undefined)))
        stub = os.path.join(self.dir, name + ".fatbin_stubs.c")
        with open(stub, "w") as f:
            f.write("".join("const unsigned long long %s[4] = {0, 0, 0, 0};\n" % b for b in blobs))
        _run([CLANGXX] + self.flags + ["-x", "c", stub, "-x", "none"] + list(objs.values())
             + [os.path.join(self.dir, "model_hip.o"), os.path.join(self.dir, "upload_order_main.o"), "-lpthread", "-o", exe], COMPILE_TIMEOUT_S)
        return exe


_T_MODULE = time.time()
_builds = {}
_slowest = {"run": 0.0}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("upload_order"))
    yield d
    print("\nupload-order module: %.1f s in all; slowest harness run %.1f s; builds %s" % (
        time.time() - _T_MODULE, _slowest["run"], ", ".join("%s %.1f s" % (k, b.compile_s) for k, b in _builds.items())))


def build(work, variant):
    if variant not in _builds:
        _builds[variant] = Build(work, variant)
    return _builds[variant]


def harness(exe, schedule, seed, groups, env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("LIBRECTIFY_")}
    e.update(env or {})
    e["TSAN_OPTIONS"] = "halt_on_error=0 exitcode=66 second_deadlock_stack=1"
    e["ASAN_OPTIONS"] = "detect_leaks=1 exitcode=67"
    e["UBSAN_OPTIONS"] = "print_stacktrace=1"
    t0 = time.time()
    r = subprocess.run([exe, schedule, str(seed), groups], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=RUN_TIMEOUT_S, env=e)
    _slowest["run"] = max(_slowest["run"], time.time() - t0)
    return r


def check_clean(r):
    tail = "\n".join(r.stdout.splitlines()[-5:]) + "\n" + r.stderr[-6000:]
    assert r.returncode == 0, tail
    assert r.stdout.splitlines()[-1] == "ok", tail
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, tail
    assert "model_hip:" not in r.stderr, tail


def check_coverage(r):
    """A run that checked nothing cannot pass: every single-frame case with more than one upload band has more than one
    checked filter launch where the filter follows the bands, and every batch case checked `batch` launches."""
    singles = batches = 0
    for line in r.stdout.splitlines():
        if not line.startswith("case "):
            continue
        kv = dict(p.split("=", 1) for p in line.split()[2:] if "=" in p)
        name = line.split()[1]
        assert all(int(t) >= 0 for t in kv["trace"].split(",") if t != "-"), line
        if name in ("single", "slow", "seq"):
            singles += 1
            assert int(kv["launches"]) >= 1 and int(kv["rows"]) >= int(kv["h"]), line
            assert sum(int(t) for t in kv["trace"].split(",")) > int(kv["bands"]), line
            if int(kv["follow"]) and int(kv["bands"]) > 1:
                assert int(kv["launches"]) > 1, line
        elif name in ("batch", "batchfail-next", "batchfail-warm", "batchfail-register"):
            batches += 1
            assert int(kv["rc"]) == 0 and int(kv["checked"]) == int(kv["batch"]), line
            assert int(kv["rows"]) == int(kv["batch"]) * int(kv["h"]), line
    return singles, batches


@pytest.mark.parametrize("variant", ["plain", "asan"])
@pytest.mark.parametrize("schedule", ["eager", "lazy"])
@pytest.mark.parametrize("process", [0, 1])
def test_unmodified_tree_under_the_deterministic_schedules(work, variant, schedule, process):
    name, env, groups = PROCESSES[process]
    exe = build(work, variant).link("upload_order")
    r = harness(exe, schedule, 1, groups, env)
    check_clean(r)
    singles, batches = check_coverage(r)
    # 3 formats x 8 heights x 3 strides x pageable / page-locked x 3 thread counts, and the sequence's frames
    assert singles >= 432 + 28, singles
    # 4 layouts x 3 lane counts x 2 frame sizes, and the calls around the failure paths
    assert batches >= 24 + 2 * 6, batches
    if process == 0:  # 64 KB bands: f32 at w = 256 and u8 at w = 1024 have 64 rows to a band, so h = 65 has two
        assert re.search(r"case single fmt=f32 w=256 h=65 stride=256 pinned=0 threads=2 follow=1 bands=2 launches=2 ", r.stdout), r.stdout[:2000]
        assert re.search(r"case single fmt=u8 w=1024 h=193 stride=1024 pinned=1 threads=1 follow=1 bands=4 launches=4 ", r.stdout)
    else:  # 2048 x 1025 f32 without the knob: three 4 MB bands through upload_rows
        assert re.search(r"case big fmt=f32 w=2048 h=1025 .* bands=3 launches=1 rows=1025 ", r.stdout)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])  # (three seeds to each of the two processes)
def test_unmodified_tree_threaded_under_the_thread_sanitizer(work, seed):
    name, env, groups = PROCESSES[seed % 2]
    exe = build(work, "tsan").link("upload_order")
    r = harness(exe, "threaded", seed * 7919, groups, env)
    check_clean(r)
    check_coverage(r)


# ---- each check fires: one statement out, the harness must fail and name the rule ---------------------------------------------

BANDS = {"LIBRECTIFY_UPLOAD_BAND_KB": "64", "LIBRECTIFY_REGISTER_FRAMES": "0"}
REGISTER = {"LIBRECTIFY_REGISTER_FRAMES": "4"}
MUTANTS = {
    # the second staging fill of a slot runs under the first frame's pending transfers
    "ensure_frame_slot-event-synchronize": (
        "upload.hip", "    LR_HIP(hipEventSynchronize(c->ev_up[slot]));\n", "",
        "lazy", "consecutive", BANDS, ["source-changed"]),
    # the filter is launched over rows whose band has not arrived
    "filter_after_band-wait-event": (
        "frame.hip", "        LR_HIP(hipStreamWaitEvent(c->stream, c->band_ev[(size_t)k], 0));\n", "",
        "lazy", "single", BANDS, ["filter-rows"]),
    # hipStreamWaitEvent before the band's record was enqueued: no wait at all (the helpers are made slower than the driver)
    "ready-spin": (
        "frame.hip", "while ((r = ready[(size_t)k].load(std::memory_order_acquire)) == 0) {", "while ((r = ready[(size_t)k].load(std::memory_order_acquire)) == 0 && false) {",
        "lazy", "slow", BANDS, ["filter-rows"]),
    # a lane filters its slot without waiting for the frame's transfer
    "batch-ready-wait-event": (
        "upload.hip", "    if (hipStreamWaitEvent(lane_stream, c->ring_ev[(size_t)slot], 0) != hipSuccess) {\n        set_error(\"hipStreamWaitEvent failed\");\n        return 1;\n    }\n", "",
        "lazy", "batch", REGISTER, ["filter-rows"]),
    # after an error the call returns (and unregisters the caller's pages) with transfers of the caller's frames pending
    "batch-close-stream-synchronize": (
        "upload.hip", "    (void)hipStreamSynchronize(c->copy_stream);  // (after an error: nothing may still read the caller's frames)\n", "",
        "lazy", "batchfail", REGISTER, ["caller-memory-pending", "unregister-pending"]),
}


def mutate(tmp_path, unit, old, new):
    text = open(os.path.join(CSRC, unit)).read()
    assert text.count(old) == 1, "%s: the statement of this mutant occurs %d times in the source, not once:\n%s" % (unit, text.count(old), old)
    path = str(tmp_path / unit)
    with open(path, "w") as f:
        f.write(text.replace(old, new))
    return path


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_a_missing_statement_fails_the_harness_with_the_rule_named(work, tmp_path, mutant):
    unit, old, new, schedule, groups, env, rules = MUTANTS[mutant]
    exe = build(work, "plain").link("mutant_" + mutant, {unit: mutate(tmp_path, unit, old, new)})
    r = harness(exe, schedule, 1, groups, env)
    assert r.returncode == 1 and r.stdout.splitlines()[-1].startswith("FAILED"), r.stdout[-2000:] + r.stderr[-4000:]
    named = set(re.findall(r"^model_hip: \[([a-z-]+)\]", r.stderr, re.M))
    assert named & set(rules), (named, rules)
    # ... and the same groups pass on the unchanged sources
    check_clean(harness(build(work, "plain").link("upload_order"), schedule, 1, groups, env))
    # The threaded schedule sees it as well: the missing dependency is a data race under the thread sanitizer (or, where the
    # workers' pauses fall that way, the same rule).
    exe = build(work, "tsan").link("mutant_" + mutant, {unit: mutate(tmp_path, unit, old, new)})
    r = harness(exe, "threaded", 1, groups, env)
    named = set(re.findall(r"^model_hip: \[([a-z-]+)\]", r.stderr, re.M))
    assert r.returncode != 0 and ("ThreadSanitizer: data race" in r.stderr or named & set(rules)), r.stdout[-1000:] + r.stderr[-4000:]


def test_the_last_band_statement_is_redundant(work, tmp_path):
    """`if (k == n_bands - 1) by_end = band_rows;` in filter_after_band cannot be killed: the loop in front of it takes band
    rows while min(h - 1, filter_band_last_row(by)) <= last_row, and for the last upload band last_row is h - 1, so the loop
    itself runs to band_rows.  The harness counts, per frame, how often every band row is filtered (exactly once); without
    the statement it prints the same launches and rows, line for line."""
    old = "        if (k == n_bands - 1) by_end = band_rows;\n"
    exe = build(work, "plain").link("mutant_last_band", {"frame.hip": mutate(tmp_path, "frame.hip", old, "")})
    r = harness(exe, "lazy", 1, "single,seq", BANDS)
    check_clean(r)
    ref = harness(build(work, "plain").link("upload_order"), "lazy", 1, "single,seq", BANDS)
    check_clean(ref)
    assert r.stdout == ref.stdout
