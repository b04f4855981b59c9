"""The label boxes of listed ids (llcomp_amd/csrc/label_boxes_rule.hpp, label_lists.hpp, label_boxes.cpp) as a stand-alone program under
AddressSanitizer and UBSan.  Host code only: no GPU, and nothing of it runs inside this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_label_boxes16_units_under_sanitizers(tmp_path):
    """tests/helpers/label_boxes16_check.cpp walks k_label_boxes16's workgroups and threads on the host through a memory that checks
    every access -- reads inside the maps, 16-byte reads aligned and whole inside the batch, record slots inside the list's capacity and
    the call's records -- and compares with llcomp_mi_label_boxes16_reference and with a count pixel by pixel: 7 widths x 5 heights
    around a band x the 8 even byte offsets of the maps (three samples, the middle one with an empty list, ids that differ in the high
    byte only), lists of 1, 256, 257, 1024, 1025, 4095 and 4096 ids at two offsets for the three capacities, the table within the bound
    the codec sizes its buffer by, and the refusals; and k_label_boxes' workgroups on byte maps against llcomp_mi_label_boxes_reference,
    the same 7 widths x 5 heights x all 16 byte offsets of the maps"""
    exe = str(tmp_path / "label_boxes16_check")
    csrc = os.path.join(ROOT, "llcomp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "helpers", "label_boxes16_check.cpp"), os.path.join(csrc, "label_boxes.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, rounds = out.stdout.split()
    assert word == "ok" and int(rounds) == 7 * 5 * 8 + 7 * 2 + 7 * 5 * 16
