"""The batch alpha paste (llcomp_amd/csrc/alpha_rule.hpp, alpha_plan.cpp) as a stand-alone program under AddressSanitizer and UBSan.
Host code only: no GPU, and nothing of it runs inside this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_alpha_paste_plan_and_unit_walks_under_sanitizers(tmp_path):
    """tests/helpers/alpha_paste_check.cpp walks k_alpha_paste<AB, DT>'s workgroups and threads on the host through a memory that checks
    every access -- reads inside the src, the alpha or the dst batch, writes inside dst, 16-byte accesses aligned, src and alpha never
    written, every byte of dst written at most once and only by the thread that owns its (row, unit), an element
    no piece reaches never written -- and compares with llcomp_mi_alpha_paste_reference bit for bit.  4 dtypes x 2 layouts x every byte
    offset 0..15 of src and of dst that the element allows (800 drawn calls, alpha_px_bytes 1..4 with every alpha_byte in turn, the
    alpha at drawn byte offsets, the batch its own alpha half the time where the shapes allow); 4 dtypes x 2 layouts x the 10 alpha
    formats on a tile and five pixels by the tile's rows and three, pieces across every border (80); 2 calls with 256 pieces on one dst
    sample; OVER at all 4 x 4 offsets of src and dst that are multiples of 4, among PASTE and VALUE pieces, with a matte and with the
    RGBA batch as its own alpha (32)."""
    exe = str(tmp_path / "alpha_paste_check")
    csrc = os.path.join(ROOT, "llcomp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "helpers", "alpha_paste_check.cpp"), os.path.join(csrc, "alpha_plan.cpp"),
                           os.path.join(csrc, "paste_plan.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, rounds = out.stdout.split()
    assert word == "ok" and int(rounds) == 2 * (256 + 64 + 64 + 16) + 80 + 2 + 32
