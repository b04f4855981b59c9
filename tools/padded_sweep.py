#!/usr/bin/env python3
"""Padded crops (rectangles that leave the image: DESIGN.md "Crops that leave the image") against what they stand beside: the existing
resized call on the same frames' SOURCE rectangles -- it decodes the same windows with the same kernels, so the padded call should cost
the same -- and the way a caller had before: a full decode of the batch plus torch's pad, crop and interpolate per frame.

Device-resident batches of 16 frames of 4K RGB8 (nat = photo-like, g3 = noise, bench.make_frames), 480x1 planar and 64x64 interleaved
slices, 224x224 output, bilinear.  Rectangles are drawn like torchvision's RandomResizedCrop from a seeded generator and every other one
is then moved past an edge of the image by up to 10 % of that side; every other frame is mirrored.  Legs, per case:
    padded_<mode>   the padded call, per pad mode (constant with a NULL fill)
    padded_fill     the padded call, constant with fill (124, 116, 104): the kernels' bias forms
    source          the EXISTING decode_resized_regions on the source rectangles of the mode "edge"
    torch_<mode>    full decode + torch.nn.functional.pad + crop + interpolate(antialias=True), for the modes torch has (no "symmetric")
Per leg the median, the smallest and the largest of the repeats in ms; the legs rotate their order from repeat to repeat, so the padded
legs and `source` alternate.  Timing is hipEvents on the stream with a synchronise behind each call.  A frame whose rectangle leaves the
image is checked byte for byte against np.pad + the rule restated in tests/resize_filters_spec.py for every padded leg; the torch legs
are checked to agree within 1 LSB.

    python tools/padded_sweep.py [out.jsonl] [--reps N] [--tag TEXT] [--quick]    # on a GPU box; one JSON line per case
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
FILL = (124, 116, 104)
TORCH_MODE = {"constant": "constant", "edge": "replicate", "reflect": "reflect"}


def shifted(rng, rect, f):
    """every other rectangle past an edge by 1 px .. 10 % of that side: left, right, top, bottom in turn"""
    x, y, rw, rh = rect
    if f % 2 == 0:
        return x, y, rw, rh
    side = (f // 2) % 4
    d = int(rng.integers(1, (W if side < 2 else H) // 10 + 1))
    if side == 0:
        return -d, y, rw, rh
    if side == 1:
        return W - rw + d, y, rw, rh
    if side == 2:
        return x, -d, rw, rh
    return x, H - rh + d, rw, rh


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tag", default="")
    ap.add_argument("--quick", action="store_true", help="one case (nat, 480x1p), no torch legs")
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F

    import bench
    import llcomp_amd as mi
    import resize_filters_spec as spec
    from resize_spec import random_resized_crop

    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            print(line, file=out, flush=True)

    emit({"tool": "padded_sweep", "tag": a.tag, "frames": FRAMES, "w": W, "h": H, "c": C, "out": [OW, OH], "reps": a.reps, "fill": FILL,
          "device": torch.cuda.get_device_name(0)})
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
            rects = np.array([shifted(rng, random_resized_crop(rng, W, H), f) for f in range(FRAMES)], np.int64)
            flags = np.array([f % 2 for f in range(FRAMES)], np.uint8)
            source = mi.padded_regions_plan(W, H, rects, "edge")
            d_out = torch.empty((FRAMES, OH, OW, C), dtype=torch.uint8, device="cuda")
            d_full = torch.empty_like(d_img)

            def padded(mode, fill=None):
                codec.decode_resized_regions(d_pay.data_ptr(), total, d_len.data_ptr(), rects, OW, OH, d_out.data_ptr(), d_st.data_ptr(),
                                             flags=flags, stream=st.cuda_stream, pad_mode=mode, fill=fill)

            def on_source():
                codec.decode_resized_regions(d_pay.data_ptr(), total, d_len.data_ptr(), source, OW, OH, d_out.data_ptr(), d_st.data_ptr(),
                                             flags=flags, stream=st.cuda_stream)

            def torch_chain(mode):
                codec.decode(d_pay.data_ptr(), total, d_len.data_ptr(), d_full.data_ptr(), d_st.data_ptr(), st.cuda_stream)
                for f, (x, y, rw, rh) in enumerate(rects.tolist()):
                    pl, pr, pt, pb = max(-x, 0), max(x + rw - W, 0), max(-y, 0), max(y + rh - H, 0)
                    img = d_full[f].permute(2, 0, 1)[None].float()
                    if pl or pr or pt or pb:
                        img = F.pad(img, (pl, pr, pt, pb), mode=TORCH_MODE[mode])
                    crop = img[:, :, y + pt:y + pt + rh, x + pl:x + pl + rw]
                    v = F.interpolate(crop, size=(OH, OW), mode="bilinear", align_corners=False, antialias=True)
                    v = v.round_().clamp_(0, 255).to(torch.uint8)[0].permute(1, 2, 0)
                    d_out[f] = v.flip(1) if flags[f] & 1 else v

            variants = [(f"padded_{m}", (lambda m=m: padded(m))) for m in mi.PAD_NAMES]
            variants += [("padded_fill", lambda: padded("constant", FILL)), ("source", on_source)]
            if not a.quick:
                variants += [(f"torch_{m}", (lambda m=m: torch_chain(m))) for m in TORCH_MODE]
            # frame 1 leaves the image by its left edge
            x1, y1, rw1, rh1 = rects[1].tolist()
            img1 = d_img[1].cpu().numpy()
            pads = ((max(-y1, 0), max(y1 + rh1 - H, 0)), (max(-x1, 0), max(x1 + rw1 - W, 0)), (0, 0))

            def spec1(mode, fill):
                if mode == "constant":
                    big = np.empty((H + sum(pads[0]), W + sum(pads[1]), C), np.uint8)
                    big[:] = np.asarray(fill if fill is not None else (0, 0, 0), np.uint8)
                    big[pads[0][0]:pads[0][0] + H, pads[1][0]:pads[1][0] + W] = img1
                else:
                    big = np.pad(img1, pads, mode=mode)
                crop = big[y1 + pads[0][0]:y1 + pads[0][0] + rh1, x1 + pads[1][0]:x1 + pads[1][0] + rw1]
                return spec.resize(crop, OW, OH, spec.BILINEAR, True)

            for name, fn in variants:
                d_out.zero_()
                fn()
                fn()
                torch.cuda.synchronize()
                assert int(d_st.item()) == 0, name
                got = d_out[1].cpu().numpy()
                kind, _, mode = name.partition("_")
                if kind == "padded":
                    want = spec1("constant", FILL) if mode == "fill" else spec1(mode, None)
                    assert np.array_equal(got, want), name
                elif kind == "torch":
                    assert np.abs(got.astype(int) - spec1(mode, None).astype(int)).max() <= 1, name
            codec.counters(reset=True)
            padded("constant", FILL)
            bias_launches = codec.counters()["bias_launches"]
            times = {name: [] for name, _ in variants}
            for rep in range(a.reps):
                k = rep % len(variants)
                for name, fn in variants[k:] + variants[:k]:
                    times[name].append(timed(fn))
            assert int(d_st.item()) == 0
            rec = {"content": content, "slicing": f"{tw}x{th}{'p' if planar else 'i'}", "leaving": int((source != rects).any(axis=1).sum()),
                   "largest_source": [int(source[:, 2].max()), int(source[:, 3].max())], "bias_launches_per_call": int(bias_launches)}
            for name, t in times.items():
                rec[f"{name}_ms"] = [round(float(np.median(t)), 3), round(float(min(t)), 3), round(float(max(t)), 3)]
            med = {name: float(np.median(t)) for name, t in times.items()}
            rec["padded_edge_over_source"] = round(med["padded_edge"] / med["source"], 3)
            rec["padded_fill_over_source"] = round(med["padded_fill"] / med["source"], 3)
            if not a.quick:
                rec["padded_edge_over_torch_edge"] = round(med["padded_edge"] / med["torch_edge"], 3)
            emit(rec)
            codec.close()
            del d_pay, d_len, d_full, d_out
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
