#!/usr/bin/env python3
"""What the batch copy-paste by 16-bit ids costs in HBM, against two yardsticks on the same pieces in the same run:

    u8       paste_batch of this same build on the same content with the id maps narrowed to bytes (the ids are below 256): half the
             mask bytes, no window base
    expr     torch's where per piece on the u16 maps, which is what a user writes today:
               d = mask[s, sy:sy+h, sx:sx+w] - base;  sel = (d >= 0) & (d < 256) & lut[d];  dst[d, :, ys, xs] = torch.where(sel, src, dst)

    copy_paste  Simple Copy-Paste on 256 samples of 3 x 448 x 448: one full-size piece per sample from the sample behind it, which
                selects half of the 8 ids of a uint16 id map of blobs (blocks of 32 x 32 pixels of one id)

on float16 CHW and uint8 HWC.  Every leg is timed with device events around it, after a warm-up, `--calls` times, the legs alternating;
the table has the median, the least and the most of each, ours over the 8-bit call and torch's loop over ours.  Our legs include the
host's plan and the table's copy; the pieces' ctypes tables are built once, ahead.

    python tools/ubench/paste_batch16.py [--samples 256] [--side 448] [--calls 20] [--out FILE]

Needs a GPU; there is no fallback."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def expression(dst, src, mask, tuples, layout):
    """torch's loop: dst [n, c, h, w] or [n, h, w, c] in place; mask: the u16 maps' bits as int16"""
    import torch

    for d, s, dx, dy, sx, sy, w, h, ids in tuples:
        base = min(ids)
        lut = torch.zeros(256, dtype=torch.bool, device=dst.device)
        lut[torch.tensor([m - base for m in ids], device=dst.device)] = True
        off = (mask[s, sy:sy + h, sx:sx + w].int() & 0xFFFF) - base
        sel = (off >= 0) & (off < 256) & lut[off.clamp(0, 255).long()]
        if layout == "chw":
            dst[d, :, dy:dy + h, dx:dx + w] = torch.where(sel, src[s, :, sy:sy + h, sx:sx + w], dst[d, :, dy:dy + h, dx:dx + w])
        else:
            dst[d, dy:dy + h, dx:dx + w, :] = torch.where(sel[..., None], src[s, sy:sy + h, sx:sx + w, :], dst[d, dy:dy + h, dx:dx + w, :])
    return dst


def measure(a):
    """-> [[format, selected share, dst bytes, ours ms list, u8 ms list, expr ms list], ...]"""
    import torch

    import llcomp_amd as mi

    assert mi.device_count() >= 1 and torch.cuda.is_available(), "needs a GPU"
    c, n, s = 3, a.samples, a.side
    codec = mi.Codec(1, 64, 64, c, device=0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(a.seed)
    blocks = torch.randint(0, 8, (n, (s + 31) // 32, (s + 31) // 32), generator=g, dtype=torch.uint8)
    narrow = blocks.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :s, :s].contiguous().cuda()
    mask = narrow.to(torch.int16).contiguous()  # (ids below 256: the same bits as uint16)
    ids = [1, 3, 4, 6]
    tuples = [(i, (i + 1) % n, 0, 0, 0, 0, s, s, ids) for i in range(n)]
    pieces16, pieces8 = mi.paste_pieces16(tuples), mi.paste_pieces(tuples)
    assert len(pieces16) == n
    share = float(torch.isin(narrow, torch.tensor(ids, dtype=torch.uint8).cuda()).float().mean())
    rows = []
    for dtype, layout in (("float16", "chw"), ("uint8", "hwc")):
        tdt = getattr(torch, dtype)
        bits = torch.uint8 if dtype == "uint8" else torch.int16
        shape = (n, c, s, s) if layout == "chw" else (n, s, s, c)
        if dtype == "uint8":
            src, dst0 = (torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).cuda() for _ in range(2))
        else:
            src, dst0 = (torch.randn(shape, generator=g).to(tdt).cuda() for _ in range(2))

        def ours(dst):
            codec.paste_batch16(src.data_ptr(), mask.data_ptr(), n, s, s, dst.data_ptr(), n, s, s, pieces16, dtype=dtype, layout=layout, stream=st)
            return dst

        def u8(dst):
            codec.paste_batch(src.data_ptr(), narrow.data_ptr(), n, s, s, dst.data_ptr(), n, s, s, pieces8, dtype=dtype, layout=layout, stream=st)
            return dst

        # what is timed is also right: ours against torch's loop and against the 8-bit call, once
        want = expression(dst0.clone(), src, mask, tuples, layout).view(bits)
        assert torch.equal(ours(dst0.clone()).view(bits), want) and torch.equal(u8(dst0.clone()).view(bits), want), (dtype, layout)
        dst = dst0.clone()
        legs = {"ours": lambda: ours(dst), "u8": lambda: u8(dst), "expr": lambda: expression(dst, src, mask, tuples, layout)}
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
        rows.append([f"{dtype} {layout}", share, dst.numel() * dst.element_size()] + [times[who] for who in ("ours", "u8", "expr")])
        del src, dst0, dst
    codec.close()
    return rows


def table(rows):
    def span(v):
        return f"{statistics.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})"

    out = ["  format       selected  dst MB  ours ms: median (min .. max)   u8 ms: median (min .. max)        expr ms: median (min .. max)  ours/u8 expr/ours"]
    for fmt, share, nbytes, ours, u8, expr in rows:
        mo = statistics.median(ours)
        out.append(f"  {fmt:<12} {share:8.2f} {nbytes / 1e6:7.0f} {span(ours)}   {span(u8)}   {span(expr)}   "
                   f"{mo / statistics.median(u8):7.2f} {statistics.median(expr) / mo:9.2f}")
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
    lines = ["Batch copy-paste by 16-bit ids against the 8-bit call on the narrowed maps and torch's where per piece (tools/ubench/paste_batch16.py)",
             f"  {a.samples} samples of 3 x {a.side} x {a.side}, one full-size piece per sample; device events around each leg, {a.warmup} warm-up rounds, then",
             f"  {a.calls} rounds, the legs alternating; ours and u8 include the host's plan and the table's copy"]
    lines += table(measure(a))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
