"""The host planner of the batch mixing (llcomp_amd/csrc/mix_plan.cpp) and the rule's host functions (mix_rule.hpp) as a stand-alone
program under AddressSanitizer and UBSan.  Host code only: no GPU, and nothing of it runs inside this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mix_plan_and_reference_under_sanitizers(tmp_path):
    """tests/helpers/mix_plan_check.cpp: 4 kinds of permutation x (7 sizes around the segment length and at the limit + 100 seeded
    rounds) with the records in heap arrays of exactly n records and the plan written into arrays of exactly n and n + 1 entries --
    every segment within the segment length, every saved head where its reader looks for it, the table in a heap buffer of exactly its
    size -- then 4 dtypes x 2 layouts x 50 rounds of the reference with every buffer on the heap at its exact size (out of place and in
    place, on arbitrary bit patterns), the roundings at their ties, and the refusals"""
    exe = str(tmp_path / "mix_plan_check")
    csrc = os.path.join(ROOT, "llcomp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "helpers", "mix_plan_check.cpp"), os.path.join(csrc, "mix_plan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, rounds = out.stdout.split()
    assert word == "ok" and int(rounds) == 4 * (7 + 100) + 4 * 2 * 50
