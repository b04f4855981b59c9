"""The plain-C++ pieces every host call goes through (llcomp_amd/csrc/container.cpp: covered_span; host_result.hpp: HostOut and
with_overflow_retry) as a stand-alone program under AddressSanitizer, LeakSanitizer and UBSan.  Host code only: no GPU, and nothing of
it runs inside this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_span_output_and_retry_under_sanitizers(tmp_path):
    """tests/helpers/host_result_check.cpp: covered_span against a brute-force sum for every tile box of 19x13x3 in 8x4 planes, 100x44x3
    in 32x16 interleaved, 300x12x3 in 64x1 planes, one tile and one pixel (60 + 60 + 1170 + 1 + 1 boxes), each also with the payload cut
    at the span's end, inside it, before it and to nothing, the container in a heap buffer of exactly its size; a legacy stream;
    HostOut with a caller's buffer of n and n - 1 bytes, n = 0, an allocation committed and one abandoned (the leak check is the
    assertion); with_overflow_retry's five cases by call count and capacities -- the only place its second attempt runs"""
    exe = str(tmp_path / "host_result_check")
    csrc = os.path.join(ROOT, "llcomp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "helpers", "host_result_check.cpp"), os.path.join(csrc, "container.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, boxes = out.stdout.split()
    assert word == "ok" and int(boxes) == 1292
