#!/usr/bin/env python3
"""What the label targets cost in HBM, against two yardsticks on the same content in the same run:

    expr    the torch expression that yields the same tensor, which is what a user writes today:
              INDEX    lut[map.long()]
              PLANES   (lut[map.long()][:, None] == torch.arange(K).view(1, K, 1, 1)).to(dtype)
              masks    map[:, None] == ids[:, :, None, None]
    floor   out.zero_() on the same output plus a read of the maps (a sum): what a kernel that writes every byte once cannot beat

    blobs   256 maps of 448 x 448 of blobs (blocks of 32 x 32 pixels of one of 8 ids), as uint8 and as uint16

The legs: INDEX int64 with lists of 8 ids; PLANES float16 with K = 19; PLANES uint8 with 8 instance masks per sample; INDEX int64 with
lists of 1024 ids (uint16 maps only: capacity 1024; the 8 present ids among them).  Every leg is timed with device events around it,
after a warm-up, `--calls` times, ours, expr and floor alternating; the table has the median, the least and the most of each, the GB/s
of the output bytes over our median, and both yardsticks over ours.  Our leg includes the host's check of the lists and the table's
copy; the lists' arrays are built once, ahead.

    python tools/ubench/label_targets.py [--samples 256] [--side 448] [--calls 20] [--out FILE]

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
    narrow = blocks.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :s, :s].contiguous().cuda()
    wide = narrow.to(torch.int16).contiguous()  # (ids below 256: the same bits as uint16)
    class_of = (np.arange(1024) * 7 + 1) % K  # id -> class
    lut = torch.from_numpy(class_of.astype(np.int64)).cuda()
    planes_of = torch.arange(K, device="cuda").view(1, K, 1, 1)
    rows = []
    for name, maps in (("u8", narrow), ("u16", wide)):
        legs = [("index i64", 8, dict(kind=mi.TARGET_INDEX, dtype=mi.TARGET_I64), torch.int64, n, lambda: lut[maps.long()]),
                ("planes f16 K=19", 8, dict(kind=mi.TARGET_PLANES, dtype=mi.DTYPE_F16, on_bits=0x3C00), torch.float16, n * K,
                 lambda: (lut[maps.long()][:, None] == planes_of).to(torch.float16)),
                ("8 masks u8", 8, dict(kind=mi.TARGET_PLANES, dtype=mi.DTYPE_U8, on_bits=1, default_value=-1), torch.uint8, n * 8, None)]
        if name == "u16":
            legs.append(("index i64, 1024 ids", 1024, dict(kind=mi.TARGET_INDEX, dtype=mi.TARGET_I64), torch.int64, n, lambda: lut[maps.long()]))
        for leg, per_sample, kw, tdt, planes, expr in legs:
            masks = leg.startswith("8 masks")
            flat = np.tile(np.arange(per_sample, dtype=np.uint16), n)
            values = np.tile(np.arange(per_sample, dtype=np.int32) if masks else class_of[:per_sample].astype(np.int32), n)
            first = (np.arange(n + 1, dtype=np.uint32) * per_sample).astype(np.uint32)
            per = 8 if masks else K
            plane_first = (np.arange(n + 1, dtype=np.uint32) * per).astype(np.uint32)
            f = dict(struct_size=C.sizeof(mi._lib.LabelTargets), map_bytes=maps.element_size(), default_value=int(class_of[0]), on_bits=0, off_bits=0,
                     ids=flat.ctypes.data, values=values.ctypes.data, first=first.ctypes.data, plane_first=plane_first.ctypes.data)
            f.update(kw)
            t = mi._lib.LabelTargets(**f)
            out = torch.empty((planes, s, s), dtype=tdt, device="cuda")
            ids_dev = torch.arange(8, device="cuda", dtype=maps.dtype).view(1, 8, 1, 1)
            if masks:
                expr = lambda: maps[:, None] == ids_dev  # noqa: E731

            def ours():
                rc = L.llcomp_mi_codec_label_targets(codec._h, maps.data_ptr(), n, s, s, C.byref(t), out.data_ptr(), C.c_void_p(st))
                assert rc == mi.OK

            def floor():
                out.zero_()
                return maps.sum()

            # what is timed is also right: ours against the expression, once
            ours()
            torch.cuda.synchronize()
            want = expr()
            assert torch.equal(out.view(want.shape) if not masks else out.view(want.shape).bool(), want), (name, leg)
            del want
            times = {who: [] for who in ("ours", "expr", "floor")}
            for it in range(a.warmup + a.calls):
                for who, fn in (("ours", ours), ("expr", expr), ("floor", floor)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    r = fn()
                    e1.record()
                    torch.cuda.synchronize()
                    del r
                    if it >= a.warmup:
                        times[who].append(e0.elapsed_time(e1))
            rows.append([name, leg, out.numel() * out.element_size(), times["ours"], times["expr"], times["floor"]])
            del out
            torch.cuda.empty_cache()
    codec.close()
    return rows


def table(rows):
    def span(v):
        return f"{statistics.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})"

    out = ["  maps leg                  out MB  ours ms: median (min .. max)    GB/s   expr ms: median (min .. max)      floor ms: median (min .. max)  expr/ours ours/floor"]
    for name, leg, nbytes, ours, expr, floor in rows:
        mo = statistics.median(ours)
        out.append(f"  {name:4s} {leg:20s} {nbytes / 1e6:7.0f} {span(ours)} {nbytes / (mo * 1e-3) / 1e9:7.0f}   {span(expr)}   {span(floor)}   "
                   f"{statistics.median(expr) / mo:8.2f} {mo / statistics.median(floor):9.2f}")
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
    lines = ["Label targets against the torch expression that yields the same tensor and against out.zero_() plus a read of the maps (tools/ubench/label_targets.py)",
             f"  {a.samples} maps of {a.side} x {a.side}, uint8 and uint16; device events around each leg, {a.warmup} warm-up rounds, then {a.calls} rounds, the legs alternating;",
             "  GB/s of the output bytes over our median; ours includes the host's check of the lists and the table's copy"]
    lines += table(measure(a))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
