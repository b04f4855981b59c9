#!/usr/bin/env python3
"""A/B of the perspective views against the views call, on one batch and one set of boxes:

    A  Codec.decode_perspective_views   10 views of 224 x 224 per frame, distorted as torchvision's RandomPerspective(0.5) distorts, bilinear
    B  Codec.decode_views               the same views' SOURCE RECTANGLES (llcomp_mi_perspective_source_rect), resized to 224 x 224, bilinear

on 32 frames of 3840 x 2160 x 3 in 64 x 64 tiles.  Both decode the same unions -- the windows, classes and boxes are the same plan -- so
the difference is the tail (one gather launch with two binary64 divisions per pixel against two resample passes through the rows'
buffer) and the host's planning (the rectangles are a bound: a pixel wider than the exact box).  A view is a 224 x 224 square of the
frame whose corners are sent to endpoints drawn as torchvision's RandomPerspective.get_params draws them for distortion_scale.  The calls
alternate A, B, A, B, ...; each is timed with the host clock from the call to the end of a stream synchronise (what a caller waits for)
and with device events around it (what the GPU does).  A second pass with the codec's profiling on gives the split of a call: slot 5 the
slice decoder, slot 6 the inverse model with the crops and the tail.

    python tools/ubench/perspective_views.py [--frames 32] [--views 10] [--calls 12] [--first A|B] [--out FILE]

Needs a GPU; there is no fallback."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--tile", type=int, default=64)
    ap.add_argument("--views", type=int, default=10)
    ap.add_argument("--side", type=int, default=224)
    ap.add_argument("--distortion", type=float, default=0.5)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--first", choices=("A", "B"), default="A", help="which call opens every pair")
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import llcomp_amd as mi
    from llcomp_amd import synth

    assert mi.device_count() >= 1 and torch.cuda.is_available(), "needs a GPU"
    frames, w, h, c, side = a.frames, a.width, a.height, 3, a.side
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

    warp, rect = [], []
    half, d = side // 2, a.distortion
    for f in range(frames):
        for _ in range(a.views):
            # torchvision's get_params on a side x side image: every corner moves inwards by up to distortion * side / 2
            tl = (int(rng.integers(0, int(d * half) + 1)), int(rng.integers(0, int(d * half) + 1)))
            tr = (int(rng.integers(side - int(d * half) - 1, side)), int(rng.integers(0, int(d * half) + 1)))
            br = (int(rng.integers(side - int(d * half) - 1, side)), int(rng.integers(side - int(d * half) - 1, side)))
            bl = (int(rng.integers(0, int(d * half) + 1)), int(rng.integers(side - int(d * half) - 1, side)))
            x0, y0 = rng.uniform(side, w - 2 * side), rng.uniform(side, h - 2 * side)
            start = [(x0, y0), (x0 + side - 1, y0), (x0 + side - 1, y0 + side - 1), (x0, y0 + side - 1)]
            m = mi.perspective_coeffs(start, [tl, tr, br, bl])
            (x, y, rw, rh), empty = mi.perspective_source_rect(w, h, m, "bilinear", side, side)
            assert not empty
            warp.append((f, *m))
            rect.append((f, x, y, rw, rh))
    n = len(warp)
    out_a = torch.empty((n, side, side, c), dtype=torch.uint8, device="cuda")
    out_b = torch.empty((n, side, side, c), dtype=torch.uint8, device="cuda")
    ga = [mi.PerspectiveGroup(warp, side, side, out_a.data_ptr(), filter="bilinear")]
    gb = [mi.ViewGroup(rect, side, side, out_b.data_ptr(), filter="bilinear")]
    uni_a = mi.perspective_views_plan(w, h, c, a.tile, a.tile, True, frames, ga)[0]
    uni_b = mi.views_plan(w, h, c, a.tile, a.tile, True, frames, gb)[0]
    assert np.array_equal(uni_a, uni_b), "the two calls must decode the same unions"
    plan_ms = {}
    for which, fn, g in (("A", mi.perspective_views_plan, ga), ("B", mi.views_plan, gb)):
        t0 = time.perf_counter()
        for _ in range(5):
            fn(w, h, c, a.tile, a.tile, True, frames, g)
        plan_ms[which] = (time.perf_counter() - t0) * 1e3 / 5

    def call(which):
        if which == "A":
            codec.decode_perspective_views(pay.data_ptr(), nbytes, lens.data_ptr(), ga, st.data_ptr(), s)
        else:
            codec.decode_views(pay.data_ptr(), nbytes, lens.data_ptr(), gb, st.data_ptr(), s)

    order = (["A", "B"] if a.first == "A" else ["B", "A"]) * (a.warmup + a.calls)
    wall, dev = {"A": [], "B": []}, {"A": [], "B": []}
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
        if i >= 2 * a.warmup:
            wall[which].append((t1 - t0) * 1e3)
            dev[which].append(e0.elapsed_time(e1))
    split = {}
    codec.set_profiling(True)
    for which in ("A", "B"):
        codec.get_profile()
        for _ in range(3):
            call(which)
        torch.cuda.synchronize()
        ms = list(codec.get_profile()[0].values())
        split[which] = [v / 3 for v in ms]
    codec.set_profiling(False)
    codec.close()

    med = lambda v: statistics.median(v)
    lines = [
        "Perspective views against the views call on the same boxes (tools/ubench/perspective_views.py)",
        f"  {frames} frames of {w} x {h} x {c}, {a.tile} x {a.tile} tiles planar, {a.views} views of {side} x {side} per frame ({n} views), "
        f"distortion {a.distortion} as RandomPerspective draws it, bilinear, u8 HWC",
        f"  A = decode_perspective_views, B = decode_views on the views' source rectangles; largest union {int(uni_a[:, 2].max())} x {int(uni_a[:, 3].max())}, "
        f"largest source rectangle {max(r[3] for r in rect)} x {max(r[4] for r in rect)}",
        f"  run order: {' '.join(order[:2 * a.warmup])} (warm-up, not counted) then {' '.join(order[2 * a.warmup:])}",
        "",
        "  ms per call                         A (persp.)   B (views)   A / B",
        f"  host clock, call to synchronise   {med(wall['A']):10.3f}  {med(wall['B']):10.3f}  {med(wall['A']) / med(wall['B']):6.3f}   (median of {a.calls})",
        f"  device events around the call     {med(dev['A']):10.3f}  {med(dev['B']):10.3f}  {med(dev['A']) / med(dev['B']):6.3f}",
        f"  min / max of the host clock       {min(wall['A']):.3f} / {max(wall['A']):.3f}    {min(wall['B']):.3f} / {max(wall['B']):.3f}",
        f"  the plan alone, on the host        {plan_ms['A']:10.3f}  {plan_ms['B']:10.3f}           (perspective_views_plan / views_plan, Python wrapper included)",
        "",
        "  the codec's profile, ms per call (3 calls each, profiling on): slot 4 locate + copy, 5 slice decoder, 6 inverse model + crops + tail, 7 clear",
        "    A  " + "  ".join(f"[{i}] {split['A'][i]:.3f}" for i in range(4, 8)),
        "    B  " + "  ".join(f"[{i}] {split['B'][i]:.3f}" for i in range(4, 8)),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
