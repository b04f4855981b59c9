"""The host half of the batch copy-paste (llcomp_amd/csrc/paste_plan.cpp) and the kernel's own unit decisions (paste_rule.hpp on
compose_rule.hpp) as a stand-alone program under AddressSanitizer and UBSan.  Host code only: no GPU, and nothing of it runs inside this
process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_paste_plan_and_unit_decisions_under_sanitizers(tmp_path):
    """tests/helpers/paste_check.cpp, run as `paste_check 8`, walks k_paste's workgroups and threads on the host through a memory that checks every access
    -- reads inside the src or the mask batch, writes inside the dst batch, 16-byte accesses aligned, a selected dst element written
    exactly once and any other never -- and compares with llcomp_mi_paste_reference bit for bit: 4 dtypes x 2 layouts x every byte
    offset 0..15 of src x of dst that the element allows, the mask's offset drawn (800 drawn calls, the U8 c = 1 ones with the mask as
    its own src half the time), 96 drawn calls on shapes around the tile's borders, 4 dtypes x 2 layouts x all 16 x 16 pairs of sx and
    dx with one-row pieces of 1, 15, 16, 17 and 33 pixels (2048), 2 calls with 256 pieces on one dst sample, the plan's CSR and the
    table within the bound the codec sizes its buffer by, in every one of them, and the refusals"""
    exe = str(tmp_path / "paste_check")
    csrc = os.path.join(ROOT, "llcomp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "helpers", "paste_check.cpp"), os.path.join(csrc, "paste_plan.cpp")])
    out = subprocess.run([exe, "8"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, rounds = out.stdout.split()
    assert word == "ok" and int(rounds) == 2 * (256 + 64 + 64 + 16) + 8 * 12 + 8 * 256 + 2
