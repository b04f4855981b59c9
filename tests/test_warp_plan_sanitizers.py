"""The host planner of the warped views (llcomp_amd/csrc/warp_plan.cpp) and the rule's host functions (warp_rule.hpp) as a stand-alone
program under AddressSanitizer and UBSan.  Host code only: no GPU, and nothing of it runs inside this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_warp_plan_and_reference_under_sanitizers(tmp_path):
    """tests/helpers/warp_plan_check.cpp: five shapes x 120 seeded rounds of 1 to 3 groups of affine views -- every entry's source
    rectangle inside its frame's box, the index tables in range, the block put into a heap buffer of exactly its size and within the
    bound the staging buffer is sized by, the whole copy's offsets with and without a gather and photometric chains
    (tests/helpers/copy_layout_check.hpp) within the bounds the entry points pass on, the public plan equal to the decode's, a refusal after good views -- then the reference and
    the source rectangle on the corner cases (1 x 1 and 1 x N images, the identity, pure scales, views wholly outside) with every
    buffer on the heap at its exact size, and the limits"""
    exe = str(tmp_path / "warp_plan_check")
    csrc = os.path.join(ROOT, "llcomp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "helpers", "warp_plan_check.cpp"), os.path.join(csrc, "container.cpp"),
                           os.path.join(csrc, "windows_plan.cpp"), os.path.join(csrc, "resize_plan.cpp"), os.path.join(csrc, "warp_plan.cpp"), os.path.join(csrc, "photo_plan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, rounds = out.stdout.split()
    assert word == "ok" and int(rounds) == 5 * 120 + 6 * 3 * 5 * 8
