"""ADJUST_SHARPNESS of the photometric chains on the host -- the planner's band, halo and chunk arithmetic (llcomp_amd/csrc/photo_plan.cpp),
the rule's functions (photo_rule.hpp) and llcomp_mi_photo_reference -- as a stand-alone program under AddressSanitizer and UBSan.  Host
code only: no GPU, and nothing of it runs inside this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_photo_sharpness_under_sanitizers(tmp_path):
    """tests/helpers/photo_sharp_check.cpp: 2 channel counts x 400 seeded rounds of 1 to 3 groups of up to 5000 x 5000 under staging
    bounds below, at and above the largest view -- every planned chunk with its halo areas within the bound, a single view always
    planned, every address of a view, a saved row and a halo area inside stage_bytes -- then 2 x 150 rounds of the reference on chains
    with the op, every buffer on the heap at its exact size (out of place, in place, op by op, against the window summed by hand), the
    named worst cases, the rule's functions and the refusals with the output untouched"""
    exe = str(tmp_path / "photo_sharp_check")
    csrc = os.path.join(ROOT, "llcomp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "helpers", "photo_sharp_check.cpp"), os.path.join(csrc, "photo_plan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, rounds = out.stdout.split()
    assert word == "ok" and int(rounds) == 2 * 400 + 2 * 150
