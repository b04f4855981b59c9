"""The batch copy-paste by ids of 3 and 4 bytes (llcomp_amd/csrc/paste_rule.hpp with MB 3 and 4, paste_plan.cpp) as a stand-alone
program under AddressSanitizer and UBSan.  Host code only: no GPU, and nothing of it runs inside this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wide_paste_plan_and_unit_decisions_under_sanitizers(tmp_path):
    """tests/helpers/wide_paste_check.cpp walks k_paste<3, ES>'s and k_paste<4, ES>'s workgroups and threads on the host through a memory
    that checks every access -- reads inside the src or the mask batch, writes inside the dst batch, 16-byte accesses aligned, 4-byte
    mask pixels at multiples of 4, the mask never written, a selected dst element written exactly once and any other never -- and
    compares with llcomp_mi_paste32_reference bit for bit.  MB 3: 4 dtypes x 2 layouts x every byte offset 0..15 of the mask x every
    offset of dst that the element allows (1152 drawn calls whose batches end where their arrays end, the maps their own source half
    the time where the shapes allow, VALUE and VALUE_PIXEL pieces, windows that pass the top id).  MB 4: the same at the offsets 0, 4, 8
    and 12 (288).  Both: 4 dtypes x 2 layouts x all 16 x 16 pairs of sx and dx with one-row pieces of 1, 5, 6, 7, 15, 16, 17 and 33
    pixels (2048), 2 calls with 256 pieces on one dst sample, the table within the bound the codec sizes its buffer by, and the
    refusals, the 8- and 16-bit calls' of flag bits above bit 0 among them."""
    exe = str(tmp_path / "wide_paste_check")
    csrc = os.path.join(ROOT, "llcomp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "helpers", "wide_paste_check.cpp"), os.path.join(csrc, "paste_plan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, rounds = out.stdout.split()
    assert word == "ok" and int(rounds) == (2 * 16 * (16 + 8 + 8 + 4) + 8 * 256 + 2) + (2 * 4 * (16 + 8 + 8 + 4) + 8 * 256 + 2)
