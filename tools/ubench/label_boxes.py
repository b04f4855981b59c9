#!/usr/bin/env python3
"""What the label boxes cost in HBM, against two yardsticks on the same maps in the same run:

    read   maps.sum(): one pass over the bytes, the floor for anything that has to see every pixel
    expr   a torch loop over the ids present, which is what a user writes today (masks_to_boxes' expressions per id and sample, batched
           over the samples): any() over rows and columns, argmax of the first and the last set position, and the sum

    blobs   256 maps of 448 x 448 of blobs (blocks of 32 x 32 pixels of one of 8 ids)
    one_id  256 maps of 448 x 448 of ONE id: every run of every lane updates the same record in LDS

Every leg is timed with device events around it, after a warm-up, `--calls` times, the legs alternating; the table has the median, the
least and the most of each, the GB/s of the map bytes over our median, and both yardsticks over ours.

    python tools/ubench/label_boxes.py [--samples 256] [--side 448] [--calls 20] [--out FILE]

Needs a GPU; there is no fallback."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def expression(maps):
    """-> {id: (count [n], x0, y0, x1, y1)} for the ids present"""
    import torch

    n, h, w = maps.shape
    out = {}
    for m in torch.unique(maps).tolist():
        eq = maps == m
        cols, rows = eq.any(1), eq.any(2)
        x0, y0 = cols.int().argmax(1), rows.int().argmax(1)
        x1, y1 = w - cols.flip(1).int().argmax(1), h - rows.flip(1).int().argmax(1)
        out[m] = (eq.sum((1, 2)), x0, y0, x1, y1)
    return out


def measure(a):
    import torch

    import llcomp_amd as mi

    assert mi.device_count() >= 1 and torch.cuda.is_available(), "needs a GPU"
    n, s = a.samples, a.side
    codec = mi.Codec(1, 64, 64, 3, device=0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(a.seed)
    blocks = torch.randint(0, 8, (n, (s + 31) // 32, (s + 31) // 32), generator=g, dtype=torch.uint8)
    workloads = [("blobs", blocks.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :s, :s].contiguous().cuda()),
                 ("one_id", torch.full((n, s, s), 9, dtype=torch.uint8).cuda())]
    boxes = torch.empty(n * 256 * 20, dtype=torch.uint8).cuda()
    rows = []
    for name, maps in workloads:
        def ours():
            codec.label_boxes(maps.data_ptr(), n, s, s, boxes.data_ptr(), stream=st)

        # what is timed is also right: ours against torch's loop, once
        ours()
        torch.cuda.synchronize()
        got = boxes.cpu().numpy().view(mi.LABEL_BOX_DTYPE).reshape(n, 256)
        want = expression(maps)
        for m, cols in want.items():
            present = cols[0].cpu().numpy() > 0
            for field, col in zip(("count", "x0", "y0", "x1", "y1"), cols):
                assert np.array_equal(got[present, m][field], col.cpu().numpy()[present]), (name, m, field)
        assert int(got["count"].sum()) == n * s * s
        legs = {"ours": ours, "read": lambda: maps.sum(), "expr": lambda: expression(maps)}
        times = {who: [] for who in legs}
        for it in range(a.warmup + a.calls):
            for who, f in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    times[who].append(e0.elapsed_time(e1))
        rows.append([name, len(want), maps.numel()] + [times[who] for who in ("ours", "read", "expr")])
    codec.close()
    return rows


def table(rows):
    def span(v):
        return f"{statistics.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})"

    out = ["  workload  ids  ours ms: median (min .. max)    GB/s   read ms: median (min .. max)     expr ms: median (min .. max)  read/ours expr/ours"]
    for name, ids, nbytes, ours, read, expr in rows:
        mo = statistics.median(ours)
        out.append(f"  {name:<8} {ids:4d} {span(ours)} {nbytes / (mo * 1e-3) / 1e9:7.0f}   {span(read)}   {span(expr)}   "
                   f"{statistics.median(read) / mo:7.2f} {statistics.median(expr) / mo:8.2f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--side", type=int, default=448)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["Label boxes against one pass over the bytes and a torch loop over the ids present (tools/ubench/label_boxes.py)",
             f"  {a.samples} maps of {a.side} x {a.side}; device events around each leg, {a.warmup} warm-up rounds, then {a.calls} rounds, the legs alternating;",
             "  GB/s of the map bytes over our median"]
    lines += table(measure(a))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
