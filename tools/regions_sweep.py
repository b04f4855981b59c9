#!/usr/bin/env python3
"""Regions decode (a random crop of one size per frame, DESIGN.md "Region decode") against the two ways a caller had before it: a full
decode of the batch plus a torch crop per frame, and a loop of one-frame region decodes (one launch chain per frame).  Device-resident
batches of 16 frames of 4K RGB8 (nat = photo-like, g3 = noise, from the seeded generators of bench.make_frames), 480x1 planar and 64x64
interleaved slices, 224x224 and 512x512 crops at seeded random offsets.  4K at 64x64 has two classes (2160 % 64 != 0): its crops are
measured once with every window above the last tile row (one class) and once with half the frames' windows in it (two classes).

Per case: the median over the repeats of each of the three, in ms, and the classes of the call.  Every variant is warmed up first;
the three rotate their order from repeat to repeat; timing is hipEvents on the stream with a synchronise behind each call.  Every
output is checked against the crops of the source frames.  The payload comes from the HIP encoder (bit-exact with the oracle:
tests/test_gpu_parity.py).

    python tools/regions_sweep.py [out.jsonl] [--reps N] [--tag TEXT]      # on a GPU box; one JSON line per case
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, W, H, C = 16, 3840, 2160, 3
SLICINGS = [(480, 1, True), (64, 64, False)]
CROPS = [224, 512]


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

    emit({"tool": "regions_sweep", "tag": a.tag, "frames": FRAMES, "w": W, "h": H, "c": C, "reps": a.reps, "device": torch.cuda.get_device_name(0)})
    st = torch.cuda.current_stream()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        ev0.record(st)
        fn()
        ev1.record(st)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    rng = np.random.default_rng(224)
    for content in ("nat", "g3"):
        d_img = torch.from_numpy(bench.make_frames(content, FRAMES, 0, distinct=4)).cuda()
        for tw, th, planar in SLICINGS:
            codec = mi.Codec(FRAMES, W, H, C, tw, th, planar, device=0)
            one = mi.Codec(1, W, H, C, tw, th, planar, device=0)
            codec.prepare(encode=True, decode=True, region=True, regions=True)
            one.prepare(encode=False, decode=True, region=True)
            cap = min(codec.max_payload_bytes, 2 * d_img.numel() + 64 * codec.n_slices + 4096)
            d_pay = torch.empty(cap, dtype=torch.uint8, device="cuda")
            d_len = torch.empty(codec.n_slices, dtype=torch.int32, device="cuda")
            d_tot = torch.zeros(1, dtype=torch.int64, device="cuda")
            d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
            codec.encode(d_img.data_ptr(), d_pay.data_ptr(), cap, d_len.data_ptr(), d_tot.data_ptr(), d_st.data_ptr(), st.cuda_stream)
            torch.cuda.synchronize()
            assert int(d_st.item()) == 0
            total = int(d_tot.item())
            spf = codec.n_slices // FRAMES
            lens = d_len.cpu().numpy().astype(np.int64)
            frame_off = np.concatenate([[0], np.cumsum(lens.reshape(FRAMES, spf).sum(axis=1))])
            d_full = torch.empty_like(d_img)
            for r in CROPS:
                ty = th if th > 1 else 1
                last_row0 = (H - 1) // ty * ty  # the first pixel row of the last tile row
                kinds = [("random", None)]
                if H % ty:
                    kinds = [("1class", False), ("2class", True)]
                for kind, bottom in kinds:
                    xs = rng.integers(0, W - r + 1, size=FRAMES)
                    if bottom is None:
                        ys = rng.integers(0, H - r + 1, size=FRAMES)
                    else:  # windows clear of the last tile row, and (2 classes) every other frame's crop at the bottom edge
                        ys = rng.integers(0, max(1, last_row0 - 2 * ty - r), size=FRAMES)
                        if bottom:
                            ys[1::2] = H - r
                    xy = np.stack([xs, ys], axis=1).astype(np.uint32)
                    n_classes = mi.regions_plan(W, H, C, tw, th, planar, r, r, xy)[1]
                    want = torch.stack([d_img[f, int(y):int(y) + r, int(x):int(x) + r] for f, (x, y) in enumerate(xy)])
                    d_out = torch.empty((FRAMES, r, r, C), dtype=torch.uint8, device="cuda")

                    def regions():
                        codec.decode_regions(d_pay.data_ptr(), total, d_len.data_ptr(), xy, r, r, d_out.data_ptr(), d_st.data_ptr(), st.cuda_stream)

                    def full_crop():
                        codec.decode(d_pay.data_ptr(), total, d_len.data_ptr(), d_full.data_ptr(), d_st.data_ptr(), st.cuda_stream)
                        torch.stack([d_full[f, int(y):int(y) + r, int(x):int(x) + r] for f, (x, y) in enumerate(xy)], out=d_out)

                    def loop():
                        for f, (x, y) in enumerate(xy):
                            one.decode_region(d_pay.data_ptr() + int(frame_off[f]), int(frame_off[f + 1] - frame_off[f]), d_len.data_ptr() + 4 * f * spf,
                                              int(x), int(y), r, r, d_out[f].data_ptr(), d_st.data_ptr(), st.cuda_stream)

                    variants = [("regions", regions), ("full_crop", full_crop), ("loop", loop)]
                    for _, fn in variants:
                        d_out.zero_()
                        fn()
                        fn()
                        torch.cuda.synchronize()
                        assert int(d_st.item()) == 0 and torch.equal(d_out, want), (content, tw, th, r, kind)
                    times = {name: [] for name, _ in variants}
                    for rep in range(a.reps):
                        k = rep % len(variants)
                        for name, fn in variants[k:] + variants[:k]:
                            times[name].append(timed(fn))
                    assert int(d_st.item()) == 0
                    med = {name: float(np.median(t)) for name, t in times.items()}
                    emit({"content": content, "slicing": f"{tw}x{th}{'p' if planar else 'i'}", "crop": f"{r}x{r}", "offsets": kind,
                          "classes": n_classes, "families": ["".join(k[0] for k in ("rows", "lds_table", "bank_cache") if f[k]) or "-"
                                                             for f in codec.regions_family(xy, r, r)],
                          "regions_ms": round(med["regions"], 3), "full_crop_ms": round(med["full_crop"], 3), "loop_ms": round(med["loop"], 3),
                          "regions_over_full_crop": round(med["regions"] / med["full_crop"], 3), "regions_over_loop": round(med["regions"] / med["loop"], 3),
                          "regions_ms_min": round(min(times["regions"]), 3), "full_crop_ms_min": round(min(times["full_crop"]), 3),
                          "loop_ms_min": round(min(times["loop"]), 3)})
                    del d_out, want
            codec.close()
            one.close()
            del d_pay, d_len, d_full
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
