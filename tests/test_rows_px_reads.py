"""The row encoder of planar 1-row slices reads the caller's pixel batch itself, one dword per sample where that dword stays inside
the batch and the pixel's bytes alone where it would not (geometry.hpp: rows_px_dwords, rows_px_tail).  A device buffer of exactly
the batch's size may end on a page boundary, so no read may pass it -- which a GPU test cannot see (allocators leave slack behind a
block).  The kernel's load schedule is checked here instead, on the host, against the batch's size for 1..4 channels."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_encoder_pixel_reads_stay_inside_the_batch(tmp_path):
    exe = str(tmp_path / "rows_px_reads_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "llcomp_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "helpers", "rows_px_reads_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, geometries, lanes, byte_reads = out.stdout.split()
    assert word == "ok" and int(geometries) >= 3000 and int(lanes) >= 1000000 and int(byte_reads) > 0
