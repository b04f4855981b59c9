#!/usr/bin/env python3
"""What the batch copy-paste costs in HBM, against two yardsticks on the same pieces in the same run:

    compose  compose_batch(keep=True) of the same rectangles: the unmasked ceiling -- the same tiles, units and shifted copies without
             the mask fetch and the id test, and with every byte written
    expr     torch's where per piece, which is what a user writes today:
               sel = lut[mask[s, sy:sy+h, sx:sx+w]];  dst[d, :, ys, xs] = torch.where(sel, src[s, :, ...], dst[d, :, ys, xs])

    copy_paste  Simple Copy-Paste on 256 samples of 3 x 448 x 448: one full-size piece per sample from the sample behind it, which
                selects half of the 8 ids of an id map of blobs (blocks of 32 x 32 pixels of one id)

on float16 CHW and uint8 HWC.  Every leg is timed with device events around it, after a warm-up, `--calls` times, the legs alternating;
the table has the median, the least and the most of each, and both yardsticks over ours.  Our leg includes the host's plan and the
table's copy; the pieces' ctypes table is built once, ahead.

    python tools/ubench/paste_batch.py [--samples 256] [--side 448] [--calls 20] [--out FILE]

Needs a GPU; there is no fallback."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def expression(dst, src, mask, tuples, layout):
    """torch's loop: dst [n, c, h, w] or [n, h, w, c] in place"""
    import torch

    for d, s, dx, dy, sx, sy, w, h, ids in tuples:
        lut = torch.zeros(256, dtype=torch.bool, device=dst.device)
        lut[torch.tensor(ids, device=dst.device)] = True
        sel = lut[mask[s, sy:sy + h, sx:sx + w].long()]
        if layout == "chw":
            dst[d, :, dy:dy + h, dx:dx + w] = torch.where(sel, src[s, :, sy:sy + h, sx:sx + w], dst[d, :, dy:dy + h, dx:dx + w])
        else:
            dst[d, dy:dy + h, dx:dx + w, :] = torch.where(sel[..., None], src[s, sy:sy + h, sx:sx + w, :], dst[d, dy:dy + h, dx:dx + w, :])
    return dst


def measure(a):
    """-> [[format, selected share, ours ms list, compose ms list, expr ms list], ...]"""
    import torch

    import llcomp_amd as mi

    assert mi.device_count() >= 1 and torch.cuda.is_available(), "needs a GPU"
    c, n, s = 3, a.samples, a.side
    codec = mi.Codec(1, 64, 64, c, device=0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(a.seed)
    blocks = torch.randint(0, 8, (n, (s + 31) // 32, (s + 31) // 32), generator=g, dtype=torch.uint8)
    mask = blocks.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :s, :s].contiguous().cuda()
    ids = [1, 3, 4, 6]
    tuples = [(i, (i + 1) % n, 0, 0, 0, 0, s, s, ids) for i in range(n)]
    pieces = mi.paste_pieces(tuples)
    rects = mi.compose_pieces([t[:8] for t in tuples])
    share = float(torch.isin(mask, torch.tensor(ids, dtype=torch.uint8).cuda()).float().mean())
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
            codec.paste_batch(src.data_ptr(), mask.data_ptr(), n, s, s, dst.data_ptr(), n, s, s, pieces, dtype=dtype, layout=layout, stream=st)
            return dst

        def compose(dst):
            codec.compose_batch(src.data_ptr(), n, s, s, dst.data_ptr(), n, s, s, rects, dtype=dtype, layout=layout, keep=True, stream=st)
            return dst

        # what is timed is also right: ours against torch's loop, once
        assert torch.equal(ours(dst0.clone()).view(bits), expression(dst0.clone(), src, mask, tuples, layout).view(bits)), (dtype, layout)
        dst = dst0.clone()
        legs = {"ours": lambda: ours(dst), "compose": lambda: compose(dst), "expr": lambda: expression(dst, src, mask, tuples, layout)}
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
        rows.append([f"{dtype} {layout}", share, dst.numel() * dst.element_size()] + [times[who] for who in ("ours", "compose", "expr")])
        del src, dst0, dst
    codec.close()
    return rows


def table(rows):
    def span(v):
        return f"{statistics.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})"

    out = ["  format       selected  dst MB  ours ms: median (min .. max)   compose ms: median (min .. max)   expr ms: median (min .. max)  compose/ours expr/ours"]
    for fmt, share, nbytes, ours, compose, expr in rows:
        mo = statistics.median(ours)
        out.append(f"  {fmt:<12} {share:8.2f} {nbytes / 1e6:7.0f} {span(ours)}   {span(compose)}   {span(expr)}   "
                   f"{statistics.median(compose) / mo:10.2f} {statistics.median(expr) / mo:9.2f}")
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
    lines = ["Batch copy-paste against compose_batch(keep) of the same rectangles and torch's where per piece (tools/ubench/paste_batch.py)",
             f"  {a.samples} samples of 3 x {a.side} x {a.side}, one full-size piece per sample; device events around each leg, {a.warmup} warm-up rounds, then",
             f"  {a.calls} rounds, the legs alternating; ours includes the host's plan and the table's copy"]
    lines += table(measure(a))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
