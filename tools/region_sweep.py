#!/usr/bin/env python3
"""Region decode against a full decode of the same batch (DESIGN.md "Region decode"): device-resident batches of 16 frames of 4K RGB8
(nat / mid / g3 content from the seeded generators of bench.make_frames), three slicings, five rectangles from 64x64 to the whole
frame.  Per case: the median over the repeats of Codec.decode_region ms and of Codec.decode ms, the covered slices per frame, and
the region's output MPix/s.  Every shape is warmed up first; the two calls alternate their order from repeat to repeat; timing is
hipEvents on the stream with a synchronise behind each call.  Every region output is checked against the same rectangle of the full
decode.  The payload comes from the HIP encoder (bit-exact with the oracle: tests/test_gpu_parity.py).

    python tools/region_sweep.py [out.txt] [--reps N] [--tag TEXT]      # on a GPU box; one JSON line per case
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, W, H, C = 16, 3840, 2160, 3
SLICINGS = [(64, 64, False), (128, 128, True), (480, 1, True)]
REGIONS = [(64, 64), (256, 256), (1024, 1024), (1920, 1080), (W, H)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    import numpy as np
    import torch

    import bench
    import llcomp_amd as mi

    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            print(line, file=out, flush=True)

    emit({"tool": "region_sweep", "tag": a.tag, "frames": FRAMES, "w": W, "h": H, "c": C, "reps": a.reps, "device": torch.cuda.get_device_name(0)})
    st = torch.cuda.current_stream()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        ev0.record(st)
        fn()
        ev1.record(st)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    for content in ("nat", "mid", "g3"):
        d_img = torch.from_numpy(bench.make_frames(content, FRAMES, 0, distinct=4)).cuda()
        for tw, th, planar in SLICINGS:
            codec = mi.Codec(FRAMES, W, H, C, tw, th, planar, device=0)
            codec.prepare(encode=True, decode=True, region=True)
            cap = min(codec.max_payload_bytes, 2 * d_img.numel() + 64 * codec.n_slices + 4096)
            d_pay = torch.empty(cap, dtype=torch.uint8, device="cuda")
            d_len = torch.empty(codec.n_slices, dtype=torch.int32, device="cuda")
            d_tot = torch.zeros(1, dtype=torch.int64, device="cuda")
            d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
            codec.encode(d_img.data_ptr(), d_pay.data_ptr(), cap, d_len.data_ptr(), d_tot.data_ptr(), d_st.data_ptr(), st.cuda_stream)
            torch.cuda.synchronize()
            assert int(d_st.item()) == 0
            total = int(d_tot.item())
            d_full = torch.empty_like(d_img)

            def full():
                codec.decode(d_pay.data_ptr(), total, d_len.data_ptr(), d_full.data_ptr(), d_st.data_ptr(), st.cuda_stream)

            for _ in range(2):
                full()
            torch.cuda.synchronize()
            assert int(d_st.item()) == 0 and torch.equal(d_full, d_img)
            for rw, rh in REGIONS:
                x, y = min(1000, W - rw), min(500, H - rh)  # (not tile-aligned unless it is the whole frame)
                d_out = torch.empty((FRAMES, rh, rw, C), dtype=torch.uint8, device="cuda")

                def region():
                    codec.decode_region(d_pay.data_ptr(), total, d_len.data_ptr(), x, y, rw, rh, d_out.data_ptr(), d_st.data_ptr(), st.cuda_stream)

                for _ in range(2):
                    region()
                torch.cuda.synchronize()
                assert int(d_st.item()) == 0 and torch.equal(d_out, d_img[:, y:y + rh, x:x + rw]), (content, tw, th, rw, rh)
                t_reg, t_full = [], []
                for r in range(a.reps):
                    if r % 2 == 0:
                        t_reg.append(timed(region))
                        t_full.append(timed(full))
                    else:
                        t_full.append(timed(full))
                        t_reg.append(timed(region))
                assert int(d_st.item()) == 0
                (_, n_cov) = mi.region_plan(W, H, C, tw, th, planar, x, y, rw, rh)
                ms_r, ms_f = float(np.median(t_reg)), float(np.median(t_full))
                emit({"content": content, "slicing": f"{tw}x{th}{'p' if planar else 'i'}", "region": f"{rw}x{rh}", "x": x, "y": y,
                      "covered_slices_per_frame": n_cov, "slices_per_frame": codec.n_slices // FRAMES,
                      "family": "".join(k[0] for k in ("rows", "lds_table", "bank_cache") if codec.region_family(x, y, rw, rh)[k]) or "-",
                      "region_ms": round(ms_r, 3), "full_ms": round(ms_f, 3), "region_over_full": round(ms_r / ms_f, 3),
                      "region_mpix_s": round(FRAMES * rw * rh / ms_r / 1e3, 1), "region_ms_min": round(min(t_reg), 3), "full_ms_min": round(min(t_full), 3)})
                del d_out
            codec.close()
            del d_pay, d_len, d_full
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
