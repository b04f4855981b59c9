#!/usr/bin/env python3
"""What the photometric chains cost on top of the views call they follow, on one batch and one set of views:

    P  Codec.decode_views            2 views of 224 x 224 and 8 of 96 x 96 per frame (a multi-crop), bilinear, float16 CHW normalised
    J  ... with photo=               ColorJitter without hue + RandomGrayscale on every view: brightness, contrast, color, grayscale
    R  ... with photo=               a RandAugment-style pair on every view: solarize, equalize
    D  ... with photo=               the DINO global-view chain on every view: brightness, contrast, color, adjust_hue, grayscale,
                                     gaussian_blur with radius 1.0
    S  ... with photo=               J's chain and adjust_sharpness with factor 1.8 behind it: S - J is the sharpness step
    B  ... with photo=               J's chain and gaussian_blur with radius 1.0 behind it: B - J is the blur step, S's yardstick

on frames of 3840 x 2160 x 3 in 64 x 64 tiles.  All of them decode the same unions and resample the same views; P writes the formatted
output from the vertical pass, the others write U8 HWC into the staging buffer and run their chains from there.  The calls alternate
P, J, R, D, S, B, P, J, ...; each is timed with the host clock from the call to the end of a stream synchronise (what a caller waits for) and
with device events around it (what the GPU does).  A second pass with the codec's profiling on gives the split of a call: slot 5 the
slice decoder, slot 6 the inverse model with the crops, the resample passes and the chains.

    python tools/ubench/photo_views.py [--frames 16] [--calls 12] [--out FILE]

Needs a GPU; there is no fallback."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

JITTER = [("brightness", 1.2), ("contrast", 0.8), ("color", 1.3), ("grayscale", None)]
RANDAUG = [("solarize", 128), ("equalize", None)]
DINO = [("brightness", 1.2), ("contrast", 0.8), ("color", 1.3), ("adjust_hue", 0.05), ("grayscale", None), ("gaussian_blur", 1.0)]
SHARP = JITTER + [("adjust_sharpness", 1.8)]
BLUR = JITTER + [("gaussian_blur", 1.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--tile", type=int, default=64)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import llcomp_amd as mi
    from llcomp_amd import synth

    assert mi.device_count() >= 1 and torch.cuda.is_available(), "needs a GPU"
    frames, w, h, c = a.frames, a.width, a.height, 3
    rng = np.random.default_rng(a.seed)
    base = torch.from_numpy(synth.gen_nat(w, h, c)).cuda()
    px = torch.stack([torch.roll(base, shifts=(37 * f, 91 * f), dims=(0, 1)) for f in range(frames)]).contiguous()
    codec = mi.Codec(frames, w, h, c, a.tile, a.tile, True, device=0)
    cap = 2 * px.numel()
    pay = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
    lens = torch.empty(codec.n_slices, dtype=torch.int32, device="cuda")
    tot = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    codec.encode(px.data_ptr(), pay.data_ptr(), cap, lens.data_ptr(), tot.data_ptr(), st.data_ptr(), s)
    torch.cuda.synchronize()
    assert int(st.item()) == 0, "encode failed"
    nbytes = int(tot.item())

    def crops(n, lo, hi):
        """n RandomResizedCrop-like rectangles per frame, lo..hi of the frame's area"""
        out = []
        for f in range(frames):
            for _ in range(n):
                area = rng.uniform(lo, hi) * w * h
                ratio = np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
                rw, rh = min(w, int(round((area * ratio) ** 0.5))), min(h, int(round((area / ratio) ** 0.5)))
                out.append((f, int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1)), rw, rh, int(rng.integers(0, 2))))
        return out

    big, small = crops(2, 0.05, 0.2), crops(8, 0.01, 0.05)
    fmt = dict(dtype="float16", layout="chw", scale=True, mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
    o_big = torch.empty((len(big), c, 224, 224), dtype=torch.float16, device="cuda")
    o_small = torch.empty((len(small), c, 96, 96), dtype=torch.float16, device="cuda")

    def groups(photo):
        return [mi.ViewGroup(big, 224, 224, o_big.data_ptr(), filter="bilinear", photo=photo, **fmt),
                mi.ViewGroup(small, 96, 96, o_small.data_ptr(), filter="bilinear", photo=photo, **fmt)]

    legs = {"P": groups(None), "J": groups(JITTER), "R": groups(RANDAUG), "D": groups(DINO), "S": groups(SHARP), "B": groups(BLUR)}

    def call(which):
        codec.decode_views(pay.data_ptr(), nbytes, lens.data_ptr(), legs[which], st.data_ptr(), s)

    order = list(legs) * (a.warmup + a.calls)
    wall, dev = {k: [] for k in legs}, {k: [] for k in legs}
    for i, which in enumerate(order):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        call(which)
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        assert int(st.item()) == 0
        if i >= len(legs) * a.warmup:
            wall[which].append((t1 - t0) * 1e3)
            dev[which].append(e0.elapsed_time(e1))
    split = {}
    codec.set_profiling(True)
    for which in legs:
        codec.get_profile()
        for _ in range(3):
            call(which)
        torch.cuda.synchronize()
        split[which] = [v / 3 for v in codec.get_profile()[0].values()]
    codec.set_profiling(False)
    codec.close()

    med = statistics.median

    def row(label, t, note=""):
        return (f"  {label:<34}" + "".join(f"{med(t[k]):10.3f}  " for k in legs) + " " +
                "".join(f"{med(t[k]) / med(t['P']):6.3f}   " for k in list(legs)[1:]) + note)

    lines = [
        "Photometric chains on top of the views call (tools/ubench/photo_views.py)",
        f"  {frames} frames of {w} x {h} x {c}, {a.tile} x {a.tile} tiles planar; per frame 2 views of 224 x 224 and 8 of 96 x 96 "
        f"({len(big) + len(small)} views), bilinear, float16 CHW normalised",
        "  P = decode_views; J = the same with brightness, contrast, color, grayscale on every view; R = with solarize, equalize on every view;",
        "  D = with brightness, contrast, color, adjust_hue, grayscale, gaussian_blur(1.0) on every view;",
        "  S = J's chain and adjust_sharpness(1.8) on every view; B = J's chain and gaussian_blur(1.0) on every view",
        f"  run order: {' '.join(order[:len(legs) * a.warmup])} (warm-up, not counted) then {' '.join(legs)} x {a.calls}",
        "",
        "  ms per call                         P (plain)   J (jitter)  R (randaug)     D (dino)    S (sharp)     B (blur)     J / P    R / P    D / P    S / P    B / P",
        row("host clock, call to synchronise", wall, f"(median of {a.calls})"),
        row("device events around the call", dev),
        "  min / max of the host clock       " + "    ".join(f"{min(wall[k]):.3f} / {max(wall[k]):.3f}" for k in legs),
        f"  the last op's step, device events: sharpness S - J = {med(dev['S']) - med(dev['J']):.3f} ms, blur B - J = {med(dev['B']) - med(dev['J']):.3f} ms",
        "",
        "  the codec's profile, ms per call (3 calls each, profiling on): slot 4 locate + copy, 5 slice decoder, 6 inverse model + crops + resample + chains, 7 clear",
    ] + ["    " + k + "  " + "  ".join(f"[{i}] {split[k][i]:.3f}" for i in range(4, 8)) for k in legs]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
