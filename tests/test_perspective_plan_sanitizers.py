"""The host planner of the perspective views (llcomp_amd/csrc/warp_plan.cpp) and the rule's host functions (warp_rule.hpp) as a
stand-alone program under AddressSanitizer and UBSan.  Host code only: no GPU, and nothing of it runs inside this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_perspective_plan_and_reference_under_sanitizers(tmp_path):
    """tests/helpers/perspective_plan_check.cpp: four shapes x 100 seeded rounds of 1 to 3 groups of perspective views -- every fifth
    with 1 x 1 outputs, every thirteenth with every view empty -- each entry's source rectangle inside its frame's box, the tail's block
    put into a heap buffer of exactly its size and within the bound the staging buffer is sized by, the whole copy's offsets
    (tests/helpers/copy_layout_check.hpp), the public plan equal to the decode's, a refusal after good views; a group of 65535 views
    and the refusal of 65536; then the reference and the source rectangle on the corner cases (1 x 1 and 1 x N images and outputs, the
    identity, strong denominators, views wholly outside) with every buffer on the heap at its exact size; and coefficients at the
    limits: refused at them, planned and run just inside, denominators down to 2^-40 included"""
    exe = str(tmp_path / "perspective_plan_check")
    csrc = os.path.join(ROOT, "llcomp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "helpers", "perspective_plan_check.cpp"), os.path.join(csrc, "container.cpp"),
                           os.path.join(csrc, "windows_plan.cpp"), os.path.join(csrc, "resize_plan.cpp"), os.path.join(csrc, "warp_plan.cpp"),
                           os.path.join(csrc, "photo_plan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, rounds = out.stdout.split()
    assert word == "ok" and int(rounds) == 4 * 100 + 1 + 6 * 3 * 5 * 8 + 7
