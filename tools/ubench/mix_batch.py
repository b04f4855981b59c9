#!/usr/bin/env python3
"""What the batch mixing costs against the torch expressions a user writes today, on one batch in HBM:

    roll   MixUp, partner i - 1   Codec.mix_batch   vs   x.roll(1, 0).mul(1.0 - lam).add_(x.mul(lam))          (torchvision)
    flip   MixUp, partner n-1-i   Codec.mix_batch   vs   x.mul_(lam).add_(x.flip(0).mul_(1.0 - lam))           (timm)
    cut    CutMix, one box of a   Codec.mix_batch   vs   o = x.clone(); o[..., y1:y2, x1:x2] = x.roll(1, 0)[..., y1:y2, x1:x2]
           quarter of the area
    erase  RandomErasing alone,   Codec.mix_batch   vs   for i: x[i][..., y:y+h, x:x+w] = v                     (per sample, as in the recipes)
           a rectangle per sample

on 256 x 3 x 224 x 224 in float16 and float32, CHW.  Each torch expression runs on the same buffer with its allocations included: they
are what a user pays today.  Every leg is timed with device events around it, after a warm-up, `--calls` times, the legs alternating;
the table has the median, the least and the most, the GB/s of 2 * n * E * esize bytes (one read and one write of the batch: what a
MixUp has to move, and more than a CutMix or an erase has to) and torch's time over ours.

--segments: the same legs on builds of the library with other segment lengths (make -C llcomp_amd/csrc mixseg builds
libllcomp_mi_seg<S>.so), each in a process of its own, one after the other: the roll legs are the ones the length changes.

    python tools/ubench/mix_batch.py [--n 256] [--calls 20] [--segments 2,4,16,32,64] [--out FILE]

Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
LAM = 0.3712345678901234


def measure(a):
    """the legs on the library this process loads -> {"segment": S, "rows": [[dtype, leg, ours ms list, torch ms list], ...]}"""
    import torch

    import llcomp_amd as mi

    assert mi.device_count() >= 1 and torch.cuda.is_available(), "needs a GPU"
    n, c, h, w = a.n, 3, a.side, a.side
    codec = mi.Codec(1, 64, 64, c, device=0)
    s = torch.cuda.current_stream().cuda_stream
    box = (w // 4, h // 4, w // 2, h // 2)
    g = torch.Generator().manual_seed(a.seed)
    rects = []
    for _ in range(n):  # RandomErasing's default scale: 2 % to 33 % of the area
        area = (0.02 + 0.31 * float(torch.rand((), generator=g))) * w * h
        rw = max(1, min(w, int(round(area ** 0.5))))
        rh = max(1, min(h, int(round(area / rw))))
        rects.append((int(torch.randint(0, w - rw + 1, (), generator=g)), int(torch.randint(0, h - rh + 1, (), generator=g)), rw, rh))
    rows = []
    for dtype in ("float16", "float32"):
        tdt = getattr(torch, dtype)
        x0 = torch.randn((n, c, h, w), generator=g).to(tdt).cuda()
        x = x0.clone()
        v = torch.zeros(c, dtype=tdt, device="cuda")[:, None, None]
        recs = {"roll": mi.mix_samples(n, "roll", LAM), "flip": mi.mix_samples(n, "flip", LAM), "cut": mi.mix_samples(n, "roll", boxes=box),
                "erase": mi.mix_samples(n, erase=rects)}

        def ours(leg):
            codec.mix_batch(x.data_ptr(), n, w, h, recs[leg], dtype=dtype, layout="chw", stream=s)

        def theirs(leg):
            if leg == "roll":
                return x.roll(1, 0).mul(1.0 - LAM).add_(x.mul(LAM))
            if leg == "flip":
                return x.mul_(LAM).add_(x.flip(0).mul_(1.0 - LAM))
            if leg == "cut":
                o = x.clone()
                o[..., box[1]:box[1] + box[3], box[0]:box[0] + box[2]] = x.roll(1, 0)[..., box[1]:box[1] + box[3], box[0]:box[0] + box[2]]
                return o
            for i, (rx, ry, rw, rh) in enumerate(rects):
                x[i][..., ry:ry + rh, rx:rx + rw] = v
            return x

        times = {(leg, who): [] for leg in recs for who in ("ours", "torch")}
        for it in range(a.warmup + a.calls):
            for leg in recs:
                for who, f in (("ours", ours), ("torch", theirs)):
                    x.copy_(x0)  # (a blend of blends would drift; the copy is outside the events)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    keep = f(leg)
                    e1.record()
                    torch.cuda.synchronize()
                    del keep
                    if it >= a.warmup:
                        times[(leg, who)].append(e0.elapsed_time(e1))
        for leg in recs:
            rows.append([dtype, leg, times[(leg, "ours")], times[(leg, "torch")]])
    codec.close()
    return {"segment": mi.mix_segment(), "rows": rows}


def table(res, a):
    esize = {"float16": 2, "float32": 4}
    out = [f"  segment length {res['segment']}",
           "    dtype    leg      ours ms: median (min .. max)     GB/s     torch ms: median (min .. max)    torch / ours"]
    for dtype, leg, ours, torch_ms in res["rows"]:
        mo, mt = statistics.median(ours), statistics.median(torch_ms)
        gbs = 2 * a.n * 3 * a.side * a.side * esize[dtype] / (mo * 1e-3) / 1e9
        out.append(f"    {dtype:<8} {leg:<6} {mo:9.3f} ({min(ours):.3f} .. {max(ours):.3f}) {gbs:9.0f}    {mt:9.3f} ({min(torch_ms):.3f} .. {max(torch_ms):.3f})"
                   f"   {mt / mo:8.2f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--side", type=int, default=224)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--segments", default="")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="(internal) measure on the library LLCOMP_MI_LIB names and print JSON")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(measure(a)))
        return
    results = [measure(a)] if not a.segments else []
    for seg in [v for v in a.segments.split(",") if v]:  # a process each: a process loads one library
        lib = os.path.join(ROOT, "llcomp_amd", f"libllcomp_mi_seg{int(seg)}.so")
        env = dict(os.environ, LLCOMP_MI_LIB=lib if os.path.exists(lib) else os.path.join(ROOT, "llcomp_amd", "libllcomp_mi.so"))
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--n", str(a.n), "--side", str(a.side), "--calls", str(a.calls), "--warmup",
               str(a.warmup), "--seed", str(a.seed)]
        done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        if done.returncode != 0:
            sys.exit(f"segment {seg}: the child ended with {done.returncode}\n{done.stdout}\n{done.stderr}")
        results.append(json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    lines = ["Batch mixing against torch's expressions (tools/ubench/mix_batch.py)",
             f"  {a.n} x 3 x {a.side} x {a.side}, CHW; device events around each leg, {a.warmup} warm-up rounds, then {a.calls} rounds, the legs alternating;",
             "  GB/s of 2 * n * E * esize bytes over our median"]
    for res in results:
        lines += table(res, a)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
