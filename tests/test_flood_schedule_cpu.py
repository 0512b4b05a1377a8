"""The flood's schedule hook (lr_set_flood_schedule) without a GPU: the Python statement of its permutation
(librectify_amd.flood_schedule_perm; csrc/common.h states it for the device) is a bijection for every length, is neither the
identity nor the reversal from eight entries on, and changes with the round and with the seed; the entry is declared in the
header and let through by the linker's export list."""
import fnmatch
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 0 .. 3: no multiplier but 1; 63 / 64 / 65 and 255 / 256 / 257: around a wavefront and a workgroup of the order kernel, powers
# of two (half the residues share a factor with n) and odd neighbours; 1 514 and 40 611: the seed counts of the 333x190 random
# frame and of a 4K bench frame (40 611 = 3 * 13 537)
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1514, 40611)
SEEDS = (0, 1, 2, 0xDEADBEEF)
ROUNDS = (0, 1, 2, 7)


@pytest.fixture(scope="module")
def perm():
    from librectify_amd import flood_schedule_perm

    return flood_schedule_perm


@pytest.mark.parametrize("n", LENGTHS)
def test_the_permutation_is_a_bijection(perm, n):
    for seed in SEEDS:
        for rnd in ROUNDS:
            p = perm(n, seed, rnd)
            assert len(p) == n and sorted(p) == list(range(n)), (n, seed, rnd)


def test_the_permutation_is_a_bijection_for_every_small_length(perm):
    """every length up to 130 (all the small cases of the multiplier's search: primes, powers of two, 6, products of small
    primes), two seeds, two rounds"""
    for n in range(131):
        for seed in (0, 3):
            for rnd in (0, 5):
                assert sorted(perm(n, seed, rnd)) == list(range(n)), (n, seed, rnd)


@pytest.mark.parametrize("n", [n for n in LENGTHS if n >= 8] + [8, 9, 10, 12])
def test_it_is_neither_the_identity_nor_the_reversal(perm, n):
    for seed in SEEDS:
        for rnd in ROUNDS:
            p = perm(n, seed, rnd)
            assert p != list(range(n)) and p != list(range(n - 1, -1, -1)), (n, seed, rnd)
            # ... nor a rotation of either: neighbours in the new list were not neighbours in the old one
            assert (p[1] - p[0]) % n not in (1, n - 1), (n, seed, rnd)


@pytest.mark.parametrize("n", (64, 257, 1514, 40611))
def test_it_changes_with_the_round_and_with_the_seed(perm, n):
    by_round = [tuple(perm(n, 1, r)) for r in range(6)]
    assert len(set(by_round)) == len(by_round), n
    by_seed = [tuple(perm(n, s, 2)) for s in range(6)]
    assert len(set(by_seed)) == len(by_seed), n
    assert perm(n, 5, 3) == perm(n, 5, 3)


def test_the_python_statement_is_the_headers(perm, tmp_path):
    """The C++ statement (csrc/common.h: flood_schedule_coeffs, flood_schedule_perm -- the functions the order kernel calls),
    compiled for the host into a small program, prints the permutation of every length of this module for two (seed, round)
    pairs; the Python statement gives the same lists."""
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "perm.cpp"
    src.write_text("""
#include <cstdio>
#include <cstdlib>
#include "common.h"
int main(int argc, char** argv) {
    const uint32_t n = (uint32_t)std::strtoul(argv[1], nullptr, 0), seed = (uint32_t)std::strtoul(argv[2], nullptr, 0),
                   rnd = (uint32_t)std::strtoul(argv[3], nullptr, 0);
    uint32_t a = 0, b = 0;
    lramd::flood_schedule_coeffs(seed, rnd, n, &a, &b);
    for (uint32_t i = 0; i < n; ++i) std::printf("%u\\n", lramd::flood_schedule_perm(i, a, b, n));
    return 0;
}
""")
    exe = tmp_path / "perm"
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "librectify_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True, capture_output=True)
    for n in LENGTHS + (5, 6, 7, 8, 12):
        for seed, rnd in ((0, 0), (0xDEADBEEF, 7)):
            out = subprocess.run([str(exe), str(n), str(seed), str(rnd)], check=True, capture_output=True, text=True).stdout
            assert [int(v) for v in out.split()] == perm(n, seed, rnd), (n, seed, rnd)


def test_the_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "librectify_amd.h")).read()
    assert re.search(r"^void\s+lr_set_flood_schedule\s*\(\s*lr_context\s*\*\s*ctx\s*,\s*int\s+order\s*,\s*uint32_t\s+seed\s*,\s*int\s+width\s*\)\s*;",
                     header, flags=re.M)
    exports = open(os.path.join(ROOT, "librectify_amd", "csrc", "exports.map")).read()
    exports = re.sub(r"/\*.*?\*/", "", exports, flags=re.S)
    glob_part = exports[exports.index("global:") + len("global:"):exports.index("local:")]
    patterns = [p.strip() for p in glob_part.split(";") if p.strip()]
    assert any(fnmatch.fnmatchcase("lr_set_flood_schedule", p) for p in patterns), patterns
    import librectify_amd as L

    assert "lr_set_flood_schedule" in L.EXPORTS
    assert callable(getattr(L.Context, "set_flood_schedule"))
    api = open(os.path.join(ROOT, "librectify_amd", "csrc", "api.cpp")).read()
    assert re.search(r"\bvoid\s+lr_set_flood_schedule\s*\(", api)
