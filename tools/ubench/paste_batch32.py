#!/usr/bin/env python3
"""What the batch copy-paste by ids of 3 and 4 bytes costs, against two yardsticks on the same pieces in the same run:

    u16      paste_batch16 of this same build on the same blobs with 16-bit ids (id k of the blobs): one window, one piece per sample
    expr     torch's where per sample on an int32 copy of the maps, which is what a user writes today:
               sel = torch.isin(map[s], ids);  dst[d] = torch.where(sel, src[s], dst[d])

    copy_paste  Simple Copy-Paste on 256 samples of 3 x 448 x 448: one full-size rectangle per sample from the sample behind it, which
                selects half of the 8 ids of an id map of blobs (blocks of 32 x 32 pixels of one id), the shape of
                tools/ubench/paste_batch16.py.  The wide ids are "dense", 0x010200 + k -- one window, one piece per sample, as the 16-bit
                leg -- or "sparse", 0x010203 * (k + 1), as RGB ids are: one piece per id, four per sample.

on float16 CHW and uint8 HWC.  Every leg is timed with device events around it, after a warm-up, `--calls` times, the legs alternating;
the table has the median, the least and the most of each, the leg over the 16-bit call and torch's loop over the leg.  Our legs include
the host's plan and the table's copy; the pieces' ctypes tables are built once, ahead.

    python tools/ubench/paste_batch32.py [--samples 256] [--side 448] [--calls 20] [--out FILE]

Needs a GPU; there is no fallback."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WIDE = {"dense": lambda k: 0x010200 + k, "sparse": lambda k: 0x010203 * (k + 1)}


def expression(dst, src, maps, tuples, layout):
    """torch's loop: dst [n, c, h, w] or [n, h, w, c] in place; maps int32 [n, h, w]"""
    import torch

    for d, s, dx, dy, sx, sy, w, h, ids in tuples:
        sel = torch.isin(maps[s, sy:sy + h, sx:sx + w], torch.tensor(ids, dtype=torch.int32, device=dst.device))
        if layout == "chw":
            dst[d, :, dy:dy + h, dx:dx + w] = torch.where(sel, src[s, :, sy:sy + h, sx:sx + w], dst[d, :, dy:dy + h, dx:dx + w])
        else:
            dst[d, dy:dy + h, dx:dx + w, :] = torch.where(sel[..., None], src[s, sy:sy + h, sx:sx + w, :], dst[d, dy:dy + h, dx:dx + w, :])
    return dst


def measure(a):
    """-> [[format, ids, pieces, dst bytes, {leg: ms list}], ...]"""
    import torch

    import llcomp_amd as mi

    assert mi.device_count() >= 1 and torch.cuda.is_available(), "needs a GPU"
    c, n, s = 3, a.samples, a.side
    codec = mi.Codec(1, 64, 64, c, device=0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(a.seed)
    blocks = torch.randint(0, 8, (n, (s + 31) // 32, (s + 31) // 32), generator=g, dtype=torch.uint8)
    narrow = blocks.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :s, :s].contiguous()
    mask16 = narrow.to(torch.int16).contiguous().cuda()
    chosen = [1, 3, 4, 6]
    tuples16 = [(i, (i + 1) % n, 0, 0, 0, 0, s, s, chosen) for i in range(n)]
    pieces16 = mi.paste_pieces16(tuples16)
    rows = []
    for kind, wide in WIDE.items():
        lut = torch.tensor([wide(k) for k in range(8)], dtype=torch.int32)
        maps4 = lut[narrow.long()].contiguous().cuda()
        maps3 = maps4.view(torch.uint8).view(n, s, s, 4)[..., :3].contiguous()
        tuples = [(i, (i + 1) % n, 0, 0, 0, 0, s, s, [wide(k) for k in chosen]) for i in range(n)]
        pieces = {3: mi.paste_pieces32(tuples, 3), 4: mi.paste_pieces32(tuples, 4)}
        for dtype, layout in (("float16", "chw"), ("uint8", "hwc")):
            tdt = getattr(torch, dtype)
            bits = torch.uint8 if dtype == "uint8" else torch.int16
            shape = (n, c, s, s) if layout == "chw" else (n, s, s, c)
            if dtype == "uint8":
                src, dst0 = (torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).cuda() for _ in range(2))
            else:
                src, dst0 = (torch.randn(shape, generator=g).to(tdt).cuda() for _ in range(2))

            def wide_leg(mb, maps):
                def run(dst):
                    codec.paste_batch32(src.data_ptr(), maps.data_ptr(), mb, n, s, s, dst.data_ptr(), n, s, s, pieces[mb], dtype=dtype, layout=layout, stream=st)
                    return dst
                return run

            def u16(dst):
                codec.paste_batch16(src.data_ptr(), mask16.data_ptr(), n, s, s, dst.data_ptr(), n, s, s, pieces16, dtype=dtype, layout=layout, stream=st)
                return dst

            w3, w4 = wide_leg(3, maps3), wide_leg(4, maps4)
            # what is timed is also right: the three calls against torch's loop, once
            want = expression(dst0.clone(), src, maps4, tuples, layout).view(bits)
            for f in (w3, w4, u16):
                assert torch.equal(f(dst0.clone()).view(bits), want), (kind, dtype, layout)
            dst = dst0.clone()
            legs = {"u16": lambda: u16(dst), "w3": lambda: w3(dst), "w4": lambda: w4(dst), "expr": lambda: expression(dst, src, maps4, tuples, layout)}
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
            rows.append([f"{dtype} {layout}", kind, len(pieces[3]), dst.numel() * dst.element_size(), times])
            del src, dst0, dst
    codec.close()
    return rows


def table(rows):
    def span(v):
        return f"{statistics.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})"

    out = ["  format       ids    pieces  dst MB  leg   ms: median (min .. max)      leg/u16 expr/leg"]
    for fmt, kind, pieces, nbytes, times in rows:
        m16, mexpr = statistics.median(times["u16"]), statistics.median(times["expr"])
        for who in ("u16", "w3", "w4"):
            m = statistics.median(times[who])
            out.append(f"  {fmt:<12} {kind:<6} {pieces:6d} {nbytes / 1e6:7.0f}  {who:4s} {span(times[who])} {m / m16:8.2f} {mexpr / m:8.2f}")
        out.append(f"  {fmt:<12} {kind:<6} {'':6s} {nbytes / 1e6:7.0f}  expr {span(times['expr'])}")
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
    lines = ["Batch copy-paste by ids of 3 and 4 bytes against the 16-bit call on the same blobs and torch's where per sample (tools/ubench/paste_batch32.py)",
             f"  {a.samples} samples of 3 x {a.side} x {a.side}, one full-size rectangle per sample; device events around each leg, {a.warmup} warm-up rounds, then",
             f"  {a.calls} rounds, the legs alternating; our legs include the host's plan and the table's copy"]
    lines += table(measure(a))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
