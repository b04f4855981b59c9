"""The label targets (llcomp_amd/csrc/label_targets_rule.hpp, label_targets.cpp) as a stand-alone program under AddressSanitizer and
UBSan.  Host code only: no GPU, and nothing of it runs inside this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_label_targets_units_under_sanitizers(tmp_path):
    """tests/helpers/label_targets_check.cpp walks k_label_targets' workgroups, threads and units on the host through a memory that
    checks every access -- map reads inside the maps, 16-byte accesses aligned and whole inside their buffer, every output byte written
    exactly once and nothing outside, the slots of the workgroup's arrays inside their LDS sizes -- and compares with
    llcomp_mi_label_targets_reference and with a value worked out pixel by pixel: the six kinds and element sizes for both map sizes
    x 5 pixel counts around a segment x every map offset of a 16-byte unit x 3 output offsets (three samples, the middle one with an
    empty list and no planes, ids that differ in the high byte only), lists of 1, 256, 257, 1024, 1025 and 4096 ids, plane counts of
    1, a chunk, a chunk + 1 and 4096, the table within the bound the codec sizes its buffer by, and the refusals"""
    exe = str(tmp_path / "label_targets_check")
    csrc = os.path.join(ROOT, "llcomp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "helpers", "label_targets_check.cpp"), os.path.join(csrc, "label_targets.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, rounds = out.stdout.split()
    assert word == "ok" and int(rounds) == 6 * 5 * (16 + 8) * 3 + (6 * 4 - 4 * 2) + 4 * 4
