"""GAUSSIAN_BLUR and ADJUST_HUE of the photometric chains on the host -- the planner's masks (llcomp_amd/csrc/photo_plan.cpp), the rule's
functions (photo_rule.hpp) and llcomp_mi_photo_reference -- as a stand-alone program under AddressSanitizer and UBSan.  Host code only:
no GPU, and nothing of it runs inside this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_photo_area_ops_under_sanitizers(tmp_path):
    """tests/helpers/photo_area_check.cpp: 2 channel counts x 100 seeded rounds of 1 to 3 groups of up to 5000 x 5000 whose chains mix
    the two ops with the pointwise family (the record of every step, the blur in it, is that of the chains), then 2 x 150 rounds of the
    reference on such chains with every buffer on the heap at its exact size (out of place, in place, op by op), the rule's functions
    at the ends of their domains, and the refusals with the output untouched"""
    exe = str(tmp_path / "photo_area_check")
    csrc = os.path.join(ROOT, "llcomp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "helpers", "photo_area_check.cpp"), os.path.join(csrc, "photo_plan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, rounds = out.stdout.split()
    assert word == "ok" and int(rounds) == 2 * 100 + 2 * 150
