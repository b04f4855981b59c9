#!/usr/bin/env python3
"""What the batch orientation costs on one batch in HBM, every code, against two yardsticks of torch's on the same batch in the same run:

    expr   torch's own OUT-OF-PLACE expression for the code, its allocation included: what a user pays today for ONE orientation of
           the whole batch (a code per sample would cost them masked indexing on top)
             flip_left_right  x.flip(-1)             rotate_90   torch.rot90(x, 1, (-2, -1)).contiguous()
             flip_top_bottom  x.flip(-2)             rotate_270  torch.rot90(x, 3, (-2, -1)).contiguous()
             rotate_180       x.flip(-2, -1)         transpose   x.transpose(-1, -2).contiguous()
                                                     transverse  x.transpose(-1, -2).flip(-2, -1).contiguous()
           (on the HWC batch the two spatial axes are 1 and 2, not the last two)
    copy   y.copy_(x) of the batch into a buffer that exists: one read and one write per element, the floor for anything that moves
           every element once

on 256 x 3 x 224 x 224 as float16 CHW and as uint8 HWC, every sample under the same code (Codec.orient_batch takes a code per sample at
the same price).  Every leg is timed with device events around it, after a warm-up, `--calls` times, the legs alternating; the table
has the median, the least and the most of each, the GB/s of 2 * n * E * esize bytes over our median, and both yardsticks over ours.
The spread of the copy leg, whose work never changes, is the run-to-run spread to read the other columns against.

    python tools/ubench/orient_batch.py [--n 256] [--side 224] [--calls 20] [--out FILE]

Needs a GPU; there is no fallback."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def expression(torch, x, code, ay, ax):
    if code == 1:
        return x.flip(ax)
    if code == 2:
        return x.flip(ay)
    if code == 3:
        return torch.rot90(x, 1, (ay, ax)).contiguous()
    if code == 4:
        return x.flip(ay, ax)
    if code == 5:
        return torch.rot90(x, 3, (ay, ax)).contiguous()
    if code == 6:
        return x.transpose(ay, ax).contiguous()
    return x.transpose(ay, ax).flip(ay, ax).contiguous()


def measure(a):
    """-> [[format, code name, ours ms list, expr ms list, copy ms list], ...]"""
    import torch

    import llcomp_amd as mi

    assert mi.device_count() >= 1 and torch.cuda.is_available(), "needs a GPU"
    n, c, side = a.n, 3, a.side
    codec = mi.Codec(1, 64, 64, c, device=0)
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(a.seed)
    rows = []
    for dtype, layout in (("float16", "chw"), ("uint8", "hwc")):
        shape = (n, c, side, side) if layout == "chw" else (n, side, side, c)
        ay, ax = (2, 3) if layout == "chw" else (1, 2)
        if dtype == "uint8":
            x = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).cuda()
        else:
            x = torch.randn(shape, generator=g).to(getattr(torch, dtype)).cuda()
        y = torch.empty_like(x)
        # what is timed is also right: every code against torch's expression, once
        for code in range(1, 8):
            z = x.clone()
            codec.orient_batch(z.data_ptr(), n, side, side, code, dtype=dtype, layout=layout, stream=s)
            assert torch.equal(z.view(torch.uint8 if dtype == "uint8" else torch.int16),
                               expression(torch, x, code, ay, ax).view(torch.uint8 if dtype == "uint8" else torch.int16)), (dtype, layout, code)
            del z
        legs = {"ours": lambda code: codec.orient_batch(x.data_ptr(), n, side, side, code, dtype=dtype, layout=layout, stream=s),
                "expr": lambda code: expression(torch, x, code, ay, ax), "copy": lambda code: y.copy_(x)}
        times = {(code, who): [] for code in range(1, 8) for who in legs}
        for it in range(a.warmup + a.calls):
            for code in range(1, 8):
                for who, f in legs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    keep = f(code)
                    e1.record()
                    torch.cuda.synchronize()
                    del keep
                    if it >= a.warmup:
                        times[(code, who)].append(e0.elapsed_time(e1))
        for code in range(1, 8):
            rows.append([f"{dtype} {layout}", mi.ORIENT_NAMES[code]] + [times[(code, who)] for who in ("ours", "expr", "copy")])
    codec.close()
    return rows


def table(rows, a):
    esize = {"float16 chw": 2, "uint8 hwc": 1}

    def span(v):
        return f"{statistics.median(v):7.3f} ({min(v):.3f} .. {max(v):.3f})"

    out = ["  format       code             ours ms: median (min .. max)   GB/s   expr ms: median (min .. max)   copy ms: median (min .. max)  expr/ours copy/ours"]
    for fmt, name, ours, expr, copy in rows:
        mo = statistics.median(ours)
        gbs = 2 * a.n * 3 * a.side * a.side * esize[fmt] / (mo * 1e-3) / 1e9
        out.append(f"  {fmt:<12} {name:<16} {span(ours)} {gbs:7.0f}   {span(expr)}   {span(copy)}   {statistics.median(expr) / mo:7.2f} {statistics.median(copy) / mo:8.2f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--side", type=int, default=224)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["Batch orientation against torch's out-of-place expressions and a plain copy_ (tools/ubench/orient_batch.py)",
             f"  {a.n} x 3 x {a.side} x {a.side}; device events around each leg, {a.warmup} warm-up rounds, then {a.calls} rounds, the legs alternating;",
             "  GB/s of 2 * n * E * esize bytes over our median; ours is in place, expr allocates its result, copy writes a buffer that exists"]
    lines += table(measure(a), a)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
