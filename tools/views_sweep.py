#!/usr/bin/env python3
"""Views decode (several views of each frame in one call, each frame decoded once: DESIGN.md "Several views of each frame") against the
only way a caller had before it, and against the floor it cannot beat.  Multi-crop rectangles as SwAV / DINO draw them: per frame 2
"global" views (RandomResizedCrop scale (0.4, 1)) to 224 x 224 and 8 "local" views (scale (0.05, 0.4)) to 96 x 96, every other view
mirrored, from a seeded generator.  Device-resident batches of 16 frames of 4K RGB8 (nat = photo-like, g3 = noise, from the seeded
generators of bench.make_frames), 480x1 planar and 64x64 interleaved slices.

The legs:
    views       Codec.decode_views, one call: two groups (32 views to 224 x 224, 128 views to 96 x 96)
    ten_calls   the same ten views per frame through ten Codec.decode_resized_regions calls on the same codec (view j of every frame per call)
    union       Codec.decode_resized_regions once on the frames' union rectangles (views_plan): what the views call decodes, with one
                resample per frame instead of ten -- the floor

Per case: the median over the repeats of each leg, in ms.  Every leg is warmed up first; the legs rotate their order from repeat to
repeat; timing is hipEvents on the stream with a synchronise behind each leg.  Every output of the views call is checked once, byte for
byte, against the ten-call leg's.

    python tools/views_sweep.py [out.jsonl] [--reps N] [--tag TEXT] [--quick]    # on a GPU box; one JSON line per case

--quick: one case (nat, 480x1p), the views leg alone, a few calls: for a kernel trace.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAMES, W, H, C = 16, 3840, 2160, 3
SLICINGS = [(480, 1, True), (64, 64, False)]
GLOBAL, LOCAL = (2, 224, (0.4, 1.0)), (8, 96, (0.05, 0.4))  # (views per frame, output side, RandomResizedCrop scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tag", default="")
    ap.add_argument("--quick", action="store_true", help="one case (nat, 480x1p), the views call only: for a kernel trace")
    a = ap.parse_args()
    import numpy as np
    import torch

    import bench
    import llcomp_amd as mi
    from resize_spec import random_resized_crop

    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            print(line, file=out, flush=True)

    emit({"tool": "views_sweep", "tag": a.tag, "frames": FRAMES, "w": W, "h": H, "c": C, "views_per_frame": [GLOBAL[:2], LOCAL[:2]], "reps": a.reps,
          "device": torch.cuda.get_device_name(0)})
    st = torch.cuda.current_stream()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        ev0.record(st)
        fn()
        ev1.record(st)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    rng = np.random.default_rng(2240096)
    for content in (("nat",) if a.quick else ("nat", "g3")):
        d_img = torch.from_numpy(bench.make_frames(content, FRAMES, 0, distinct=4)).cuda()
        for tw, th, planar in (SLICINGS[:1] if a.quick else SLICINGS):
            codec = mi.Codec(FRAMES, W, H, C, tw, th, planar, device=0)
            codec.prepare(encode=True, decode=True, region=True, regions=True, resized=True, views=True)
            cap = min(codec.max_payload_bytes, 2 * d_img.numel() + 64 * codec.n_slices + 4096)
            d_pay = torch.empty(cap, dtype=torch.uint8, device="cuda")
            d_len = torch.empty(codec.n_slices, dtype=torch.int32, device="cuda")
            d_tot = torch.zeros(1, dtype=torch.int64, device="cuda")
            d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
            codec.encode(d_img.data_ptr(), d_pay.data_ptr(), cap, d_len.data_ptr(), d_tot.data_ptr(), d_st.data_ptr(), st.cuda_stream)
            torch.cuda.synchronize()
            assert int(d_st.item()) == 0
            total = int(d_tot.item())
            # view j of frame f: rect[kind][j][f]; a group lists its views j-major, so its output is [j][f], as the ten calls write theirs
            kinds = []
            for n, side, scale in (GLOBAL, LOCAL):
                rects = np.array([[random_resized_crop(rng, W, H, scale=scale) for _ in range(FRAMES)] for _ in range(n)], np.uint32)
                flags = np.array([[(j + f) % 2 for f in range(FRAMES)] for j in range(n)], np.uint8)
                d_new = torch.empty((n, FRAMES, side, side, C), dtype=torch.uint8, device="cuda")
                d_old = torch.empty_like(d_new)
                views = [(f,) + tuple(int(v) for v in rects[j, f]) + (int(flags[j, f]),) for j in range(n) for f in range(FRAMES)]
                kinds.append((n, side, rects, flags, d_new, d_old, views))
            groups = [mi.ViewGroup(k[6], k[1], k[1], k[4].data_ptr()) for k in kinds]
            uni, win, n_used, n_classes = mi.views_plan(W, H, C, tw, th, planar, FRAMES, groups)
            assert n_used == FRAMES
            d_uni = torch.empty((FRAMES, GLOBAL[1], GLOBAL[1], C), dtype=torch.uint8, device="cuda")

            def views_call():
                codec.decode_views(d_pay.data_ptr(), total, d_len.data_ptr(), groups, d_st.data_ptr(), st.cuda_stream)

            def ten_calls():
                for n, side, rects, flags, _, d_old, _ in kinds:
                    for j in range(n):
                        codec.decode_resized_regions(d_pay.data_ptr(), total, d_len.data_ptr(), rects[j], side, side, d_old[j].data_ptr(),
                                                     d_st.data_ptr(), flags=flags[j], stream=st.cuda_stream)

            def union():
                codec.decode_resized_regions(d_pay.data_ptr(), total, d_len.data_ptr(), uni, GLOBAL[1], GLOBAL[1], d_uni.data_ptr(), d_st.data_ptr(),
                                             stream=st.cuda_stream)

            legs = [("views", views_call)] if a.quick else [("views", views_call), ("ten_calls", ten_calls), ("union", union)]
            for k in kinds:
                k[4].zero_()
                k[5].fill_(1)
            for name, fn in legs:
                fn()
                fn()
                torch.cuda.synchronize()
                assert int(d_st.item()) == 0, name
            if not a.quick:
                for k in kinds:
                    assert torch.equal(k[4], k[5]), "a view differs from the per-view path"
            times = {name: [] for name, _ in legs}
            for rep in range(a.reps):
                r = rep % len(legs)
                for name, fn in legs[r:] + legs[:r]:
                    times[name].append(timed(fn))
            assert int(d_st.item()) == 0
            med = {name: float(np.median(t)) for name, t in times.items()}
            area = lambda r: float((r[..., 2].astype(np.float64) * r[..., 3]).mean()) / (W * H)  # noqa: E731
            rec = {"content": content, "slicing": f"{tw}x{th}{'p' if planar else 'i'}", "classes": n_classes,
                   "largest_union": [int(uni[:, 2].max()), int(uni[:, 3].max())], "mean_union_area": round(area(uni), 3),
                   "mean_global_area": round(area(kinds[0][2]), 3), "mean_local_area": round(area(kinds[1][2]), 3)}
            rec.update({f"{name}_ms": round(m, 3) for name, m in med.items()})
            rec.update({f"{name}_min_max_ms": [round(float(min(t)), 3), round(float(max(t)), 3)] for name, t in times.items()})
            if not a.quick:
                rec.update({"views_over_ten_calls": round(med["views"] / med["ten_calls"], 3), "views_over_union": round(med["views"] / med["union"], 3)})
            emit(rec)
            codec.close()
            del d_pay, d_len, d_uni, kinds, groups
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
