"""The host half of the batch copy-paste by 16-bit ids (llcomp_amd/csrc/paste_plan.cpp) and the kernel's own unit decisions
(paste_rule.hpp with 2-byte mask pixels, on compose_rule.hpp) as a stand-alone program under AddressSanitizer and UBSan.  Host code only: no
GPU, and nothing of it runs inside this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_paste16_plan_and_unit_decisions_under_sanitizers(tmp_path):
    """tests/helpers/paste_check.cpp, run as `paste_check 16`, walks k_paste16's workgroups and threads on the host through a memory that checks every access
    -- reads inside the src or the mask batch, writes inside the dst batch, 16-byte accesses aligned, a selected dst element written
    exactly once and any other never -- and compares with llcomp_mi_paste16_reference bit for bit: 4 dtypes x 2 layouts x every even
    byte offset 0..14 of the mask x every offset of dst that the element allows (576 drawn calls whose batches end where their arrays
    end, the maps their own source half the time where the shapes allow), 96 drawn calls on shapes around the tile's borders, 4 dtypes
    x 2 layouts x all 16 x 16 pairs of sx and dx with one-row pieces of 1, 7, 8, 9, 15, 16, 17 and 33 pixels (2048), 2 calls with 256
    pieces on one dst sample, the plan's CSR and the table within the bound the codec sizes its buffer by, in every one of them, and
    the refusals"""
    exe = str(tmp_path / "paste_check")
    csrc = os.path.join(ROOT, "llcomp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "helpers", "paste_check.cpp"), os.path.join(csrc, "paste_plan.cpp")])
    out = subprocess.run([exe, "16"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, rounds = out.stdout.split()
    assert word == "ok" and int(rounds) == 2 * 8 * (16 + 8 + 8 + 4) + 8 * 12 + 8 * 256 + 2
