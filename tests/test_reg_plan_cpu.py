"""The page-registration plan of batch calls on host frames (csrc/reg_plan.h) on its own: a stand-alone C++ program
compares it with a brute-force restatement of its rules (CPU only, no HIP)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_registration_plan_equals_its_brute_force_restatement(tmp_path):
    exe = str(tmp_path / "reg_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cxx", "reg_plan_check.cpp"),
                           "-I", os.path.join(ROOT, "librectify_amd", "csrc"), "-o", exe])
    r = subprocess.run([exe], text=True, capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "ok 11 cases 39 frames"
