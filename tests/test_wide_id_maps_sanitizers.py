"""The label boxes and the label targets of id maps of 3 and 4 bytes per pixel (llcomp_amd/csrc/batch_chunk.hpp, label_boxes_rule.hpp,
label_lists.hpp, label_targets_rule.hpp, label_boxes.cpp, label_targets.cpp) as a stand-alone program under AddressSanitizer and UBSan.
Host code only: no GPU, and nothing of it runs inside this process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wide_id_map_units_under_sanitizers(tmp_path):
    """tests/helpers/wide_ids_check.cpp walks the workgroups and threads of k_label_boxes32 and k_label_targets32 on the host through a
    memory that checks every access -- reads inside the maps, 16-byte reads aligned and whole inside the batch, 4-byte pixels read at
    multiples of 4, the maps never written, every pixel of a band in exactly one run of its own id, every output byte written exactly
    once, slots inside the workgroup's arrays -- and compares with llcomp_mi_label_boxes32_reference, llcomp_mi_label_targets32_reference
    and values worked out pixel by pixel.  Boxes: 8 widths x 5 heights around a band x every byte offset 0..15 of a 3-byte map and the
    offsets 0, 4, 8, 12 of a 4-byte map (three samples, the middle one with an empty list, ids that differ in byte 2 or 3 only, ids 0,
    0xFFFFFF and 0xFFFFFFFF listed and present, the maps ending where their array ends).  Lists of 1, 256, 257, 1024, 1025 and 4096 ids
    through boxes and targets for both widths.  Targets: 7 kinds and dtypes x 5 pixel counts around a segment x the same offsets.  The
    tables within the bounds the codec sizes its buffers by, and the refusals, the 16-bit struct's of map_bytes 3 and 4 among them."""
    exe = str(tmp_path / "wide_ids_check")
    csrc = os.path.join(ROOT, "llcomp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "helpers", "wide_ids_check.cpp"), os.path.join(csrc, "label_boxes.cpp"),
                           os.path.join(csrc, "label_targets.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, rounds = out.stdout.split()
    assert word == "ok" and int(rounds) == 8 * 5 * (16 + 4) + 2 * 6 * 2 + 7 * 5 * (16 + 4)
