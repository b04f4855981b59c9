"""The host planner of the windowed decodes (llcomp_amd/csrc/windows_plan.cpp: the regions, resized and views plans, and the layout and
bounds of the one copy each call stages) as a stand-alone program under AddressSanitizer and UBSan.  Host code only: no GPU, and nothing
of it runs inside this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plans_layout_and_refusals_under_sanitizers(tmp_path):
    """tests/helpers/windows_plan_check.cpp: five shapes x 200 seeded rounds of 1 to 6 frames -- every table entry and resample entry in
    range and the classes tiling the table; the block put into a heap buffer of exactly its size, its offsets aligned and the whole copy
    within stage_bound plus the call's tables bound -- and where the gather's arrays, the block and photometric chains behind it sit
    (tests/helpers/copy_layout_check.hpp: with and without a gather, with and without chains); a resized plan equal to the views plan of one view per frame; every refusal's status"""
    exe = str(tmp_path / "windows_plan_check")
    csrc = os.path.join(ROOT, "llcomp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "helpers", "windows_plan_check.cpp"), os.path.join(csrc, "container.cpp"),
                           os.path.join(csrc, "windows_plan.cpp"), os.path.join(csrc, "resize_plan.cpp"), os.path.join(csrc, "photo_plan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, rounds = out.stdout.split()
    assert word == "ok" and int(rounds) == 1000
