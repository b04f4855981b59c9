#!/usr/bin/env python3
"""What the label boxes of listed ids cost on id maps of 3 and 4 bytes per pixel, against two yardsticks on the same content in the same
run:

    u16    label_boxes16 of this same build on the same blobs with 16-bit ids (id k of the blobs is k there and WIDE * (k + 1) in the
           wide maps): two thirds or half of the map bytes, eight pixels to a unit
    expr   a torch loop over the listed ids that are present on an int32 copy of the maps, which is what a user writes today
           (masks_to_boxes' expressions per id, batched over the samples)

    blobs   256 maps of 448 x 448 of blobs (blocks of 32 x 32 pixels of one of 8 ids), the shape of tools/ubench/label_boxes16.py

once with lists of 8 ids per sample (capacity 256) and once with lists of 1024 (capacity 1024; the 8 present ids among them).  Every
leg is timed with device events around it, after a warm-up, `--calls` times, the legs alternating; the table has the median, the least
and the most of each, the GB/s of the map's bytes over the median, and the ratios wide / u16 and expr / wide.  Our legs include the
host's check of the lists and the table's copy; the lists' arrays are built once, ahead.

    python tools/ubench/label_boxes32.py [--samples 256] [--side 448] [--calls 20] [--listed 8,1024] [--out FILE]

Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WIDE = 0x010203  # id k of the blobs is WIDE * (k + 1): three different bytes, above 65535


def expression(maps, ids):
    """maps int32 [n, h, w] -> {id: (count [n], x0, y0, x1, y1)} for the listed ids present"""
    import torch

    n, h, w = maps.shape
    present = set(torch.unique(maps).tolist())
    out = {}
    for m in ids:
        if m not in present:
            continue
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
    L = mi._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(a.seed)
    blocks = torch.randint(0, 8, (n, (s + 31) // 32, (s + 31) // 32), generator=g, dtype=torch.uint8)
    narrow = blocks.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :s, :s].contiguous()
    maps16 = narrow.to(torch.int16).contiguous().cuda()
    maps4 = ((narrow.to(torch.int32) + 1) * WIDE).contiguous().cuda()
    maps3 = maps4.view(torch.uint8).view(n, s, s, 4)[..., :3].contiguous()
    rows = []
    for per_sample in a.listed:
        listed = np.concatenate([WIDE * (np.arange(8, dtype=np.int64) + 1), 5 + 7 * np.arange(per_sample - 8, dtype=np.int64)])  # (5 + 7 j is no multiple of WIDE below 1024 ids)
        order = np.argsort(listed)
        flat = np.tile(listed[order].astype(np.uint32), n)
        flat16 = np.tile(np.arange(per_sample, dtype=np.uint16), n)
        first = (np.arange(n + 1, dtype=np.uint32) * per_sample).astype(np.uint32)
        boxes = {k: torch.empty(n * per_sample * 20, dtype=torch.uint8).cuda() for k in ("u16", "w3", "w4")}

        def wide(mb, maps, out):
            def call():
                rc = L.llcomp_mi_codec_label_boxes32(codec._h, maps.data_ptr(), mb, n, s, s, flat.ctypes.data, first.ctypes.data, out.data_ptr(), C.c_void_p(st))
                assert rc == mi.OK
            return call

        def u16():
            rc = L.llcomp_mi_codec_label_boxes16(codec._h, maps16.data_ptr(), n, s, s, flat16.ctypes.data, first.ctypes.data, boxes["u16"].data_ptr(), C.c_void_p(st))
            assert rc == mi.OK

        legs = {"w3": wide(3, maps3, boxes["w3"]), "w4": wide(4, maps4, boxes["w4"]), "u16": u16, "expr": lambda: expression(maps4, listed[order].tolist())}
        # what is timed is also right: the three calls against each other and against torch's loop, once
        for who in ("w3", "w4", "u16"):
            legs[who]()
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy().view(mi.LABEL_BOX_DTYPE).reshape(n, per_sample) for k, v in boxes.items()}
        at = np.argsort(order)[:8]  # where the 8 present ids stand in the sorted list
        assert np.array_equal(got["w3"], got["w4"]) and np.array_equal(got["w3"][:, at], got["u16"][:, :8])
        want = expression(maps4, listed[order].tolist())
        for k in range(8):
            cols = want.get(WIDE * (k + 1))
            if cols is None:
                continue
            present = cols[0].cpu().numpy() > 0
            for field, col in zip(("count", "x0", "y0", "x1", "y1"), cols):
                assert np.array_equal(got["w3"][present, at[k]][field], col.cpu().numpy()[present]), (per_sample, k, field)
        assert int(got["w3"]["count"].sum()) == n * s * s
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
        rows.append([per_sample, n * s * s, times])
    codec.close()
    return rows


def table(rows):
    def span(v):
        return f"{statistics.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})"

    out = ["  listed  leg   ms: median (min .. max)       GB/s  leg/u16 expr/leg"]
    for listed, pixels, times in rows:
        m16, mexpr = statistics.median(times["u16"]), statistics.median(times["expr"])
        for who, mb in (("u16", 2), ("w3", 3), ("w4", 4)):
            m = statistics.median(times[who])
            out.append(f"  {listed:6d}  {who:4s} {span(times[who])} {mb * pixels / (m * 1e-3) / 1e9:7.0f} {m / m16:8.2f} {mexpr / m:8.2f}")
        out.append(f"  {listed:6d}  expr {span(times['expr'])}")
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
    lines = ["Label boxes of listed ids on 3- and 4-byte id maps against the 16-bit call on the same blobs and a torch loop over the listed ids present (tools/ubench/label_boxes32.py)",
             f"  {a.samples} maps of {a.side} x {a.side}; device events around each leg, {a.warmup} warm-up rounds, then {a.calls} rounds, the legs alternating;",
             "  GB/s of the leg's own map bytes over its median; our legs include the host's check of the lists and the table's copy"]
    lines += table(measure(a))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
