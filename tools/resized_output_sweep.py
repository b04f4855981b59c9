#!/usr/bin/env python3
"""Resized regions decode in an output format (DESIGN.md "Float and normalised outputs"): the _ex call writing a model's input directly
against the u8 call followed by torch's ToTensor() + Normalize() chain on the GPU.  Per case:
  (a) f32_chw   decode_resized_regions(dtype="float32", layout="chw", scale=True, mean/std = ImageNet's)
  (b) bf16_chw  the same in bfloat16
  (c) u8_torch  the u8 call, then permute, float, div(255), sub(mean), div(std), contiguous on the same stream (baseline of (a));
      u8_torch_bf16 adds .to(torch.bfloat16) (baseline of (b))
  (d) u8        the u8 call alone
Device-resident batches of 16 frames of 4K RGB8 (nat = photo-like, g3 = noise, from the seeded generators of bench.make_frames), 480x1
planar and 64x64 interleaved slices, 224x224 output, rectangles drawn like torchvision's RandomResizedCrop from a seeded generator, every
other frame mirrored.

Per case: the median over the repeats of each path, in ms; every variant is warmed up first, the paths rotate their order from repeat to
repeat, timing is hipEvents on the stream with a synchronise behind each call.  Checked: (d)'s first frame byte for byte against the numpy
statement of the resampling rule (tests/resize_spec.py); (a) and (b), the whole batch, bit for bit against output_table over (d)'s bytes;
(c) against (a) -- reported as the number of elements that differ, since torch on the GPU may divide by a scalar as a multiply by its
reciprocal.

    python tools/resized_output_sweep.py [out.jsonl] [--reps N] [--tag TEXT] [--quick]    # on a GPU box; one JSON line per case
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
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tag", default="")
    ap.add_argument("--quick", action="store_true", help="one case (nat, 480x1p), (a) and (d) only: for a kernel trace")
    a = ap.parse_args()
    import numpy as np
    import torch

    import bench
    import llcomp_amd as mi
    from resize_spec import random_resized_crop, resize

    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            print(line, file=out, flush=True)

    emit({"tool": "resized_output_sweep", "tag": a.tag, "frames": FRAMES, "w": W, "h": H, "c": C, "out": [OW, OH], "reps": a.reps,
          "device": torch.cuda.get_device_name(0)})
    st = torch.cuda.current_stream()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        ev0.record(st)
        fn()
        ev1.record(st)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    norm = dict(scale=True, mean=MEAN, std=STD)
    t_f32 = mi.output_table(C, "float32", **norm)
    t_bf16 = mi.output_table(C, "bfloat16", **norm)
    d_mean = torch.tensor(MEAN, dtype=torch.float32, device="cuda").view(1, C, 1, 1)
    d_std = torch.tensor(STD, dtype=torch.float32, device="cuda").view(1, C, 1, 1)
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
            d_u8 = torch.empty((FRAMES, OH, OW, C), dtype=torch.uint8, device="cuda")
            d_f32 = torch.empty((FRAMES, C, OH, OW), dtype=torch.float32, device="cuda")
            d_bf16 = torch.empty((FRAMES, C, OH, OW), dtype=torch.bfloat16, device="cuda")
            res = {}

            def call(ptr, **kw):
                codec.decode_resized_regions(d_pay.data_ptr(), total, d_len.data_ptr(), rects, OW, OH, ptr, d_st.data_ptr(), flags=flags,
                                             stream=st.cuda_stream, **kw)

            def u8():
                call(d_u8.data_ptr())

            def f32_chw():
                call(d_f32.data_ptr(), dtype="float32", layout="chw", **norm)

            def bf16_chw():
                call(d_bf16.data_ptr(), dtype="bfloat16", layout="chw", **norm)

            def chain():
                call(d_u8.data_ptr())
                return d_u8.permute(0, 3, 1, 2).float().div(255).sub(d_mean).div(d_std).contiguous()

            def u8_torch():
                res["c"] = chain()

            def u8_torch_bf16():
                res["c_bf16"] = chain().to(torch.bfloat16)

            variants = [("f32_chw", f32_chw), ("u8", u8)] if a.quick else [("f32_chw", f32_chw), ("bf16_chw", bf16_chw), ("u8_torch", u8_torch),
                                                                        ("u8_torch_bf16", u8_torch_bf16), ("u8", u8)]
            for name, fn in variants:
                fn()
                fn()
                torch.cuda.synchronize()
                assert int(d_st.item()) == 0, name
            # checks: (d) against the rule, (a) / (b) bit for bit against the table over (d), (c) against (a)
            u8()
            torch.cuda.synchronize()
            h_u8 = d_u8.cpu().numpy()
            x0, y0, rw0, rh0 = rects[0].tolist()
            assert np.array_equal(h_u8[0], resize(mi, d_img[0, y0:y0 + rh0, x0:x0 + rw0].cpu().numpy(), OW, OH, False))
            placed = lambda t: np.ascontiguousarray(np.stack([t[ch][h_u8[..., ch]] for ch in range(C)], axis=-1).transpose(0, 3, 1, 2))
            f32_chw()
            torch.cuda.synchronize()
            assert np.array_equal(d_f32.cpu().numpy().view(np.uint32), placed(t_f32).view(np.uint32))
            rec = {"content": content, "slicing": f"{tw}x{th}{'p' if planar else 'i'}",
                   "mean_rect": [round(float(rects[:, 2].mean()), 1), round(float(rects[:, 3].mean()), 1)]}
            if not a.quick:
                bf16_chw()
                torch.cuda.synchronize()
                assert np.array_equal(d_bf16.view(torch.int16).cpu().numpy().view(np.uint16), placed(t_bf16))
                u8_torch()
                u8_torch_bf16()
                torch.cuda.synchronize()
                rec["torch_f32_elements_differing"] = int((res["c"] != d_f32).sum().item())
                rec["torch_f32_max_abs_diff"] = float((res["c"] - d_f32).abs().max().item())
                rec["torch_bf16_elements_differing"] = int((res["c_bf16"] != d_bf16).sum().item())
            times = {name: [] for name, _ in variants}
            for rep in range(a.reps):
                k = rep % len(variants)
                for name, fn in variants[k:] + variants[:k]:
                    times[name].append(timed(fn))
            assert int(d_st.item()) == 0
            med = {name: float(np.median(t)) for name, t in times.items()}
            rec.update({f"{name}_ms": round(m, 3) for name, m in med.items()})
            rec["f32_chw_minus_u8_ms"] = round(med["f32_chw"] - med["u8"], 3)
            if not a.quick:
                rec.update({"f32_chw_over_u8_torch": round(med["f32_chw"] / med["u8_torch"], 3),
                            "bf16_chw_over_u8_torch_bf16": round(med["bf16_chw"] / med["u8_torch_bf16"], 3)})
            emit(rec)
            codec.close()
            del d_pay, d_len, d_u8, d_f32, d_bf16, res
            torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
