#!/usr/bin/env python3
"""Resized regions decode (a rectangle of its own size per frame, resampled to one output shape: RandomResizedCrop, DESIGN.md "Crops of
different sizes, resized to one shape") against the two ways a caller had before it: a full decode of the batch plus a torch crop and
interpolate(mode="bilinear", antialias=True) per frame on the GPU, and a loop of one-frame region decodes plus the same interpolate.  Also
measured: decode_regions of the same batch at the largest rectangle's size (what the new call decodes), to show what the resampling adds.
Device-resident batches of 16 frames of 4K RGB8 (nat = photo-like, g3 = noise, from the seeded generators of bench.make_frames), 480x1
planar and 64x64 interleaved slices, 224x224 output, rectangles drawn like torchvision's RandomResizedCrop (scale (0.08, 1), ratio
(3/4, 4/3)) from a seeded generator, every other frame mirrored.

Per case: the median over the repeats of each path, in ms.  Every variant is warmed up first; the paths rotate their order from repeat to
repeat; timing is hipEvents on the stream with a synchronise behind each call.  The new call's first frame is checked byte for byte against
the numpy statement of the rule (tests/resize_spec.py); the torch paths are checked to agree with it within 1 LSB.

    python tools/resized_regions_sweep.py [out.jsonl] [--reps N] [--tag TEXT] [--quick]    # on a GPU box; one JSON line per case

With --filter NAME[,NAME...] (or "all") the tool measures the new call alone, per filter (bilinear, nearest, box, hamming, bicubic,
lanczos), on the same four cases and rectangles, the filters in rotating order from repeat to repeat.  Per case and filter: the median,
the smallest and the largest of the repeats, and the largest K.  Frame 0 of each is checked byte for byte against the rule restated in
tests/resize_filters_spec.py.  --quick with --filter: one case (for a kernel trace of one filter).
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
OW = OH = 224


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tag", default="")
    ap.add_argument("--quick", action="store_true", help="one case (nat, 480x1p), the new call only: for a kernel trace")
    ap.add_argument("--filter", default="", help="comma-separated filters, or 'all': the new call alone, per filter")
    a = ap.parse_args()
    if a.filter:
        return filter_sweep(a)
    import numpy as np
    import torch
    import torch.nn.functional as F

    import bench
    import llcomp_amd as mi
    from resize_spec import random_resized_crop, resize

    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            print(line, file=out, flush=True)

    emit({"tool": "resized_regions_sweep", "tag": a.tag, "frames": FRAMES, "w": W, "h": H, "c": C, "out": [OW, OH], "reps": a.reps,
          "device": torch.cuda.get_device_name(0)})
    st = torch.cuda.current_stream()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        ev0.record(st)
        fn()
        ev1.record(st)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    def interp(crop, flip):  # [rh, rw, c] u8 on the GPU -> [OH, OW, c] u8, torch's antialiased bilinear
        x = crop.permute(2, 0, 1)[None].float()
        y = F.interpolate(x, size=(OH, OW), mode="bilinear", align_corners=False, antialias=True)
        y = y.round_().clamp_(0, 255).to(torch.uint8)[0].permute(1, 2, 0)
        return y.flip(1) if flip else y

    rng = np.random.default_rng(224)
    for content in (("nat",) if a.quick else ("nat", "g3")):
        d_img = torch.from_numpy(bench.make_frames(content, FRAMES, 0, distinct=4)).cuda()
        for tw, th, planar in (SLICINGS[:1] if a.quick else SLICINGS):
            codec = mi.Codec(FRAMES, W, H, C, tw, th, planar, device=0)
            one = mi.Codec(1, W, H, C, tw, th, planar, device=0)
            codec.prepare(encode=True, decode=True, region=True, regions=True, resized=True)
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
            rects = np.array([random_resized_crop(rng, W, H) for _ in range(FRAMES)], np.uint32)
            flags = np.array([f % 2 for f in range(FRAMES)], np.uint8)
            wmax, hmax = int(rects[:, 2].max()), int(rects[:, 3].max())
            xy_max = np.stack([np.minimum(rects[:, 0], W - wmax), np.minimum(rects[:, 1], H - hmax)], axis=1).astype(np.uint32)
            n_classes = mi.resized_regions_plan(W, H, C, tw, th, planar, rects)[1]
            d_out = torch.empty((FRAMES, OH, OW, C), dtype=torch.uint8, device="cuda")
            d_box = torch.empty((FRAMES, hmax, wmax, C), dtype=torch.uint8, device="cuda")
            d_one = torch.empty((hmax * wmax * C,), dtype=torch.uint8, device="cuda")

            def resized():
                codec.decode_resized_regions(d_pay.data_ptr(), total, d_len.data_ptr(), rects, OW, OH, d_out.data_ptr(), d_st.data_ptr(),
                                             flags=flags, stream=st.cuda_stream)

            def regions_max():
                codec.decode_regions(d_pay.data_ptr(), total, d_len.data_ptr(), xy_max, wmax, hmax, d_box.data_ptr(), d_st.data_ptr(), st.cuda_stream)

            def full_interp():
                codec.decode(d_pay.data_ptr(), total, d_len.data_ptr(), d_full.data_ptr(), d_st.data_ptr(), st.cuda_stream)
                for f, (x, y, rw, rh) in enumerate(rects.tolist()):
                    d_out[f] = interp(d_full[f, y:y + rh, x:x + rw], flags[f] & 1)

            def loop_interp():
                for f, (x, y, rw, rh) in enumerate(rects.tolist()):
                    one.decode_region(d_pay.data_ptr() + int(frame_off[f]), int(frame_off[f + 1] - frame_off[f]), d_len.data_ptr() + 4 * f * spf,
                                      x, y, rw, rh, d_one.data_ptr(), d_st.data_ptr(), st.cuda_stream)
                    d_out[f] = interp(d_one[:rh * rw * C].view(rh, rw, C), flags[f] & 1)

            variants = [("resized", resized)] if a.quick else [("resized", resized), ("regions_max", regions_max), ("full_interp", full_interp),
                                                                ("loop_interp", loop_interp)]
            x0, y0, rw0, rh0 = rects[0].tolist()
            spec0 = resize(mi, d_img[0, y0:y0 + rh0, x0:x0 + rw0].cpu().numpy(), OW, OH, False)
            for name, fn in variants:
                d_out.zero_()
                fn()
                fn()
                torch.cuda.synchronize()
                assert int(d_st.item()) == 0, name
                if name == "resized":
                    assert np.array_equal(d_out[0].cpu().numpy(), spec0)
                elif name != "regions_max":
                    assert np.abs(d_out[0].cpu().numpy().astype(int) - spec0.astype(int)).max() <= 1, name
            times = {name: [] for name, _ in variants}
            for rep in range(a.reps):
                k = rep % len(variants)
                for name, fn in variants[k:] + variants[:k]:
                    times[name].append(timed(fn))
            assert int(d_st.item()) == 0
            med = {name: float(np.median(t)) for name, t in times.items()}
            rec = {"content": content, "slicing": f"{tw}x{th}{'p' if planar else 'i'}", "classes": n_classes, "largest": [wmax, hmax],
                   "mean_rect": [round(float(rects[:, 2].mean()), 1), round(float(rects[:, 3].mean()), 1)]}
            rec.update({f"{name}_ms": round(m, 3) for name, m in med.items()})
            if not a.quick:
                rec.update({"resized_over_regions_max": round(med["resized"] / med["regions_max"], 3),
                            "resized_over_full_interp": round(med["resized"] / med["full_interp"], 3),
                            "resized_over_loop_interp": round(med["resized"] / med["loop_interp"], 3)})
            emit(rec)
            codec.close()
            one.close()
            del d_pay, d_len, d_full, d_out, d_box, d_one
            torch.cuda.empty_cache()
    if out:
        out.close()


def filter_sweep(a):
    """--filter: the resized call per filter"""
    import numpy as np
    import torch

    import bench
    import llcomp_amd as mi
    import resize_filters_spec as spec
    from resize_spec import random_resized_crop

    names = list(mi.FILTER_NAMES) if a.filter == "all" else [n.strip().lower() for n in a.filter.split(",")]
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            print(line, file=out, flush=True)

    emit({"tool": "resized_regions_sweep --filter", "tag": a.tag, "frames": FRAMES, "w": W, "h": H, "c": C, "out": [OW, OH], "reps": a.reps,
          "filters": names, "device": torch.cuda.get_device_name(0)})
    st = torch.cuda.current_stream()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        ev0.record(st)
        fn()
        ev1.record(st)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    rng = np.random.default_rng(224)
    for content in (("nat",) if a.quick else ("nat", "g3")):
        d_img = torch.from_numpy(bench.make_frames(content, FRAMES, 0, distinct=4)).cuda()
        for tw, th, planar in (SLICINGS[:1] if a.quick else SLICINGS):
            codec = mi.Codec(FRAMES, W, H, C, tw, th, planar, device=0)
            codec.prepare(encode=True, decode=True, region=True, regions=True, resized=True)
            cap = min(codec.max_payload_bytes, 2 * d_img.numel() + 64 * codec.n_slices + 4096)
            d_pay = torch.empty(cap, dtype=torch.uint8, device="cuda")
            d_len = torch.empty(codec.n_slices, dtype=torch.int32, device="cuda")
            d_tot = torch.zeros(1, dtype=torch.int64, device="cuda")
            d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
            codec.encode(d_img.data_ptr(), d_pay.data_ptr(), cap, d_len.data_ptr(), d_tot.data_ptr(), d_st.data_ptr(), st.cuda_stream)
            torch.cuda.synchronize()
            assert int(d_st.item()) == 0
            total = int(d_tot.item())
            rects = np.array([random_resized_crop(rng, W, H) for _ in range(FRAMES)], np.uint32)
            flags = np.array([f % 2 for f in range(FRAMES)], np.uint8)
            d_out = torch.empty((FRAMES, OH, OW, C), dtype=torch.uint8, device="cuda")
            x0, y0, rw0, rh0 = rects[0].tolist()
            crop0 = d_img[0, y0:y0 + rh0, x0:x0 + rw0].cpu().numpy()

            def call(code):
                codec.decode_resized_regions(d_pay.data_ptr(), total, d_len.data_ptr(), rects, OW, OH, d_out.data_ptr(), d_st.data_ptr(),
                                             flags=flags, stream=st.cuda_stream, filter=code)

            codes = [mi.filter_code(n) for n in names]
            for code in codes:
                d_out.zero_()
                call(code)
                call(code)
                torch.cuda.synchronize()
                assert int(d_st.item()) == 0 and np.array_equal(d_out[0].cpu().numpy(), spec.resize(crop0, OW, OH, code, False)), code
            times = {code: [] for code in codes}
            for rep in range(a.reps):
                k = rep % len(codes)
                for code in codes[k:] + codes[:k]:
                    times[code].append(timed(lambda: call(code)))
            for name, code in zip(names, codes):
                kmax = max(mi.resize_weights(int(r[2]), OW, code)[1].shape[1] for r in rects)
                emit({"content": content, "slicing": f"{tw}x{th}{'p' if planar else 'i'}", "filter": name, "kx_max": int(kmax),
                      "largest": [int(rects[:, 2].max()), int(rects[:, 3].max())], "resized_ms": round(float(np.median(times[code])), 3),
                      "min_ms": round(float(min(times[code])), 3), "max_ms": round(float(max(times[code])), 3)})
            codec.close()
            del d_pay, d_len, d_out
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
