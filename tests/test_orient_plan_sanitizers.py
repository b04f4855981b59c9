"""The host half of the batch orientation (llcomp_amd/csrc/orient_plan.cpp) and the rule's host functions (orient_rule.hpp) as a
stand-alone program under AddressSanitizer and UBSan.  Host code only: no GPU, and nothing of it runs inside this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_orient_plan_and_reference_under_sanitizers(tmp_path):
    """tests/helpers/orient_plan_check.cpp: 3 kinds of codes (all zero, all one code, drawn) x (n = 1, 2 and 65535 + 50 seeded sizes)
    with the codes in heap arrays of exactly n bytes -- the table lists the oriented samples and nothing else, within the bound the
    codec sizes its buffer by -- then 4 dtypes x 2 layouts x 50 rounds of the reference with every buffer on the heap at its exact
    size (out of place and in place, on arbitrary bit patterns) against the rule pixel by pixel, the fundamental domains of every code
    on every shape up to 9 x 9 (their pixels and the images of those are every pixel that moves, once), and the refusals"""
    exe = str(tmp_path / "orient_plan_check")
    csrc = os.path.join(ROOT, "llcomp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "helpers", "orient_plan_check.cpp"), os.path.join(csrc, "orient_plan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, rounds = out.stdout.split()
    assert word == "ok" and int(rounds) == 3 * (3 + 50) + 4 * 2 * 50
