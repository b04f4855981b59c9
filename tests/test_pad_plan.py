"""The host planner of the padded calls (llcomp_amd/csrc/windows_plan.cpp: padded_setup, padded_views_setup; resize_plan.cpp: the folded
weights) as a stand-alone program under AddressSanitizer and UBSan.  Host code only: no GPU, and nothing of it runs inside this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_padded_plans_windows_bounds_and_refusals_under_sanitizers(tmp_path):
    """tests/helpers/pad_plan_check.cpp: five geometries x 160 seeded rounds over the four pad modes, fills and 1 to 6 frames -- every
    source rectangle inside the image; the windows, classes and boxes those of the unpadded plan and of llcomp_mi_resized_regions_plan for
    the source rectangles; no tap, bias or fill offset outside its array; the block put into a heap buffer of exactly its size and the
    whole copy within stage_bound plus the padded tables bound, also for Lanczos rectangles at the pad limit, and with photometric
    chains behind the block (tests/helpers/copy_layout_check.hpp); a views plan's unions the
    bounding boxes of its views' source rectangles and llcomp_mi_views_plan's for them; every refusal's status"""
    exe = str(tmp_path / "pad_plan_check")
    csrc = os.path.join(ROOT, "llcomp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "helpers", "pad_plan_check.cpp"), os.path.join(csrc, "container.cpp"),
                           os.path.join(csrc, "windows_plan.cpp"), os.path.join(csrc, "resize_plan.cpp"), os.path.join(csrc, "photo_plan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, rounds = out.stdout.split()
    assert word == "ok" and int(rounds) == 800
