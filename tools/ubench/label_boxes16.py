#!/usr/bin/env python3
"""What the label boxes of listed ids cost in HBM, against two yardsticks on the same content in the same run:

    u8     label_boxes of this same build on the same maps narrowed to bytes (the ids are below 256): half the map bytes, no search,
           all 256 records per map
    expr   a torch loop over the listed ids that are present on the u16 data, which is what a user writes today (masks_to_boxes'
           expressions per id, batched over the samples)

    blobs   256 maps of 448 x 448 uint16 of blobs (blocks of 32 x 32 pixels of one of 8 ids)

once with lists of 8 ids per sample (capacity 256) and once with lists of 1024 (capacity 1024; the 8 present ids among them).  Every
leg is timed with device events around it, after a warm-up, `--calls` times, the legs alternating; the table has the median, the least
and the most of each, the GB/s of the u16 map bytes over our median, and both yardsticks over ours.  Our leg includes the host's check
of the lists and the table's copy; the lists' arrays are built once, ahead.

    python tools/ubench/label_boxes16.py [--samples 256] [--side 448] [--calls 20] [--listed 8,1024] [--out FILE]

Needs a GPU; there is no fallback."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def expression(maps, ids):
    """maps: int32 copies are not made -- int16 bits of the u16 maps; -> {id: (count [n], x0, y0, x1, y1)} for the listed ids present"""
    import torch

    n, h, w = maps.shape
    present = set((torch.unique(maps).int() & 0xFFFF).tolist())
    out = {}
    for m in ids:
        if m not in present:
            continue
        eq = maps == (m - 65536 if m >= 32768 else m)
        cols, rows = eq.any(1), eq.any(2)
        x0, y0 = cols.int().argmax(1), rows.int().argmax(1)
        x1, y1 = w - cols.flip(1).int().argmax(1), h - rows.flip(1).int().argmax(1)
        out[m] = (eq.sum((1, 2)), x0, y0, x1, y1)
    return out


def measure(a):
    import ctypes as C

    import torch

    import llcomp_amd as mi

    assert mi.device_count() >= 1 and torch.cuda.is_available(), "needs a GPU"
    n, s = a.samples, a.side
    codec = mi.Codec(1, 64, 64, 3, device=0)
    L = mi._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(a.seed)
    blocks = torch.randint(0, 8, (n, (s + 31) // 32, (s + 31) // 32), generator=g, dtype=torch.uint8)
    narrow = blocks.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :s, :s].contiguous().cuda()
    maps = narrow.to(torch.int16).contiguous()  # (ids below 256: the same bits as uint16)
    boxes8 = torch.empty(n * 256 * 20, dtype=torch.uint8).cuda()
    rows = []
    for per_sample in a.listed:
        ids = list(range(per_sample))
        flat = np.tile(np.arange(per_sample, dtype=np.uint16), n)
        first = (np.arange(n + 1, dtype=np.uint32) * per_sample).astype(np.uint32)
        boxes = torch.empty(n * per_sample * 20, dtype=torch.uint8).cuda()

        def ours():
            rc = L.llcomp_mi_codec_label_boxes16(codec._h, maps.data_ptr(), n, s, s, flat.ctypes.data, first.ctypes.data, boxes.data_ptr(), C.c_void_p(st))
            assert rc == mi.OK

        def u8():
            codec.label_boxes(narrow.data_ptr(), n, s, s, boxes8.data_ptr(), stream=st)

        # what is timed is also right: ours against torch's loop and against the 8-bit call, once
        ours()
        u8()
        torch.cuda.synchronize()
        got = boxes.cpu().numpy().view(mi.LABEL_BOX_DTYPE).reshape(n, per_sample)
        got8 = boxes8.cpu().numpy().view(mi.LABEL_BOX_DTYPE).reshape(n, 256)
        assert np.array_equal(got[:, :min(per_sample, 256)], got8[:, :min(per_sample, 256)])
        want = expression(maps, ids)
        for m, cols in want.items():
            present = cols[0].cpu().numpy() > 0
            for field, col in zip(("count", "x0", "y0", "x1", "y1"), cols):
                assert np.array_equal(got[present, m][field], col.cpu().numpy()[present]), (per_sample, m, field)
        assert int(got["count"].sum()) == n * s * s
        legs = {"ours": ours, "u8": u8, "expr": lambda: expression(maps, ids)}
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
        rows.append([per_sample, len(want), maps.numel() * 2] + [times[who] for who in ("ours", "u8", "expr")])
    codec.close()
    return rows


def table(rows):
    def span(v):
        return f"{statistics.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})"

    out = ["  listed present  ours ms: median (min .. max)    GB/s   u8 ms: median (min .. max)       expr ms: median (min .. max)  ours/u8 expr/ours"]
    for listed, ids, nbytes, ours, u8, expr in rows:
        mo = statistics.median(ours)
        out.append(f"  {listed:6d} {ids:7d} {span(ours)} {nbytes / (mo * 1e-3) / 1e9:7.0f}   {span(u8)}   {span(expr)}   "
                   f"{mo / statistics.median(u8):7.2f} {statistics.median(expr) / mo:8.2f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--side", type=int, default=448)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--listed", type=lambda v: [int(x) for x in v.split(",")], default=[8, 1024], help="ids listed per sample, one run each")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["Label boxes of listed ids against the 8-bit call on the narrowed maps and a torch loop over the listed ids present (tools/ubench/label_boxes16.py)",
             f"  {a.samples} uint16 maps of {a.side} x {a.side}; device events around each leg, {a.warmup} warm-up rounds, then {a.calls} rounds, the legs alternating;",
             "  GB/s of the uint16 map bytes over our median; ours includes the host's check of the lists and the table's copy"]
    lines += table(measure(a))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
