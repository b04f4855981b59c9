#!/usr/bin/env python3
"""What the label targets cost on id maps of 3 and 4 bytes per pixel, one row per map_bytes, against two yardsticks on the same content
in the same run:

    mb 2   label_targets of this same build on the same blobs with 16-bit ids (id k of the blobs is k there and WIDE * (k + 1) in the
           wide maps)
    expr   the torch expression that yields the same tensor from an int32 copy of the maps.  lut[map] needs a table of 2^24 or 2^32
           entries for wide ids, so the expression is a search: j = torch.bucketize(map, ids); torch.where(ids[j] == map, values[j],
           default) -- and for PLANES the comparison with torch.arange(K) behind it

    blobs   256 maps of 448 x 448 of blobs (blocks of 32 x 32 pixels of one of 8 ids), the shape of tools/ubench/label_targets.py

The legs: INDEX int64 with lists of 8 ids; PLANES float16 with K = 19; INDEX int64 with lists of 1024 ids (capacity 1024; the 8 present
ids among them).  Every leg is timed with device events around it, after a warm-up, `--calls` times, the legs alternating; the table
has the median, the least and the most of each, the GB/s of the output bytes over the median, and the ratios to the 16-bit row and to
the expression.  Our legs include the host's check of the lists and the table's copy; the lists' arrays are built once, ahead.

    python tools/ubench/label_targets32.py [--samples 256] [--side 448] [--calls 20] [--out FILE]

Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

K = 19
WIDE = 0x010203  # id k of the blobs is WIDE * (k + 1): three different bytes, above 65535


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
    planes_of = torch.arange(K, device="cuda").view(1, K, 1, 1)
    rows = []
    for leg, per_sample, planar in (("index i64, 8 ids", 8, False), ("planes f16 K=19", 8, True), ("index i64, 1024 ids", 1024, False)):
        listed = np.concatenate([WIDE * (np.arange(8, dtype=np.int64) + 1), 5 + 7 * np.arange(per_sample - 8, dtype=np.int64)])
        order = np.argsort(listed)
        class_of = ((np.arange(per_sample) * 7 + 1) % K).astype(np.int32)  # (of the listed id's index before the sort)
        first = (np.arange(n + 1, dtype=np.uint32) * per_sample).astype(np.uint32)
        plane_first = (np.arange(n + 1, dtype=np.uint32) * K).astype(np.uint32)
        keep = {2: (np.tile(np.arange(per_sample, dtype=np.uint16), n), np.tile(class_of, n)),
                4: (np.tile(listed[order].astype(np.uint32), n), np.tile(class_of[order], n))}
        kw = dict(kind=mi.TARGET_PLANES, dtype=mi.DTYPE_F16, on_bits=0x3C00) if planar else dict(kind=mi.TARGET_INDEX, dtype=mi.TARGET_I64)
        shape, tdt = ((n * K, s, s), torch.float16) if planar else ((n, s, s), torch.int64)
        outs = {mb: torch.empty(shape, dtype=tdt, device="cuda") for mb in (2, 3, 4)}
        ids_dev = torch.from_numpy(listed[order].astype(np.int32)).cuda()
        vals_dev = torch.from_numpy(class_of[order].astype(np.int64)).cuda()

        def ours(mb, maps):
            flat, values = keep[2 if mb == 2 else 4]
            struct = mi._lib.LabelTargets if mb == 2 else mi._lib.LabelTargets32
            t = struct(struct_size=C.sizeof(struct), map_bytes=mb, default_value=-1, ids=flat.ctypes.data, values=values.ctypes.data, first=first.ctypes.data,
                       plane_first=plane_first.ctypes.data, **kw)
            call = L.llcomp_mi_codec_label_targets if mb == 2 else L.llcomp_mi_codec_label_targets32

            def run():
                rc = call(codec._h, maps.data_ptr(), n, s, s, C.byref(t), outs[mb].data_ptr(), C.c_void_p(st))
                assert rc == mi.OK
            return run

        def expr():
            j = torch.bucketize(maps4, ids_dev).clamp_(max=per_sample - 1)
            v = torch.where(ids_dev[j] == maps4, vals_dev[j], -1)
            return (v[:, None] == planes_of).to(torch.float16) if planar else v

        legs = {"mb 2": ours(2, maps16), "mb 3": ours(3, maps3), "mb 4": ours(4, maps4), "expr": expr}
        # what is timed is also right: the three calls against each other and against the expression, once
        for who in ("mb 2", "mb 3", "mb 4"):
            legs[who]()
        torch.cuda.synchronize()
        want = expr()
        assert torch.equal(outs[3].view(want.shape), want) and torch.equal(outs[4], outs[3]) and torch.equal(outs[2], outs[3]), leg
        del want
        times = {who: [] for who in legs}
        for it in range(a.warmup + a.calls):
            for who, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                r = fn()
                e1.record()
                torch.cuda.synchronize()
                del r
                if it >= a.warmup:
                    times[who].append(e0.elapsed_time(e1))
        rows.append([leg, outs[3].numel() * outs[3].element_size(), times])
        del outs
        torch.cuda.empty_cache()
    codec.close()
    return rows


def table(rows):
    def span(v):
        return f"{statistics.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})"

    out = ["  leg                  map_bytes  out MB  ms: median (min .. max)       GB/s  row/mb 2 expr/row"]
    for leg, nbytes, times in rows:
        m2, mexpr = statistics.median(times["mb 2"]), statistics.median(times["expr"])
        for who in ("mb 2", "mb 3", "mb 4"):
            m = statistics.median(times[who])
            out.append(f"  {leg:20s} {who[3:]:>9s} {nbytes / 1e6:7.0f} {span(times[who])} {nbytes / (m * 1e-3) / 1e9:7.0f} {m / m2:9.2f} {mexpr / m:8.2f}")
        out.append(f"  {leg:20s}      expr {nbytes / 1e6:7.0f} {span(times['expr'])}")
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
    lines = ["Label targets on 3- and 4-byte id maps against the 16-bit row on the same blobs and the torch expression that yields the same tensor (tools/ubench/label_targets32.py)",
             f"  {a.samples} maps of {a.side} x {a.side}; device events around each leg, {a.warmup} warm-up rounds, then {a.calls} rounds, the legs alternating;",
             "  GB/s of the output bytes over the row's median; our legs include the host's check of the lists and the table's copy"]
    lines += table(measure(a))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
