"""The host planner of the photometric chains (llcomp_amd/csrc/photo_plan.cpp) and the rule's host functions (photo_rule.hpp) as a
stand-alone program under AddressSanitizer and UBSan.  Host code only: no GPU, and nothing of it runs inside this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_photo_plan_and_reference_under_sanitizers(tmp_path):
    """tests/helpers/photo_plan_check.cpp: 2 channel counts x 3 staging bounds x 100 seeded rounds of 1 to 4 groups whose chains lie in
    heap arrays of exactly n_views chains -- the block put into a heap buffer of exactly its size and within the bound the staging buffer
    is sized by, every chunk within the staging bound, the step masks those of the chains -- then 200 rounds of the reference with
    every buffer on the heap at its exact size (out of place, in place, op by op), and the refusals"""
    exe = str(tmp_path / "photo_plan_check")
    csrc = os.path.join(ROOT, "llcomp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "helpers", "photo_plan_check.cpp"), os.path.join(csrc, "photo_plan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, rounds = out.stdout.split()
    assert word == "ok" and int(rounds) == 2 * 3 * 100 + 2 * 100
