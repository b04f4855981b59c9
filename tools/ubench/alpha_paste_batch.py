#!/usr/bin/env python3
"""What the batch alpha paste costs, in GB/s over the bytes a call has to move -- dst read, src, alpha and dst write -- beside two
yardsticks on the same shapes in the same run:

    paste    paste_batch of this same build with every id selected: the copy-paste's kernel on the same rectangles, which reads the
             mask and src and writes dst, but never reads dst and blends nothing
    copy     a device-to-device copy of as many bytes as the alpha paste's leg moves (read + written)

    opaque / transparent / soft   one full-size rectangle per sample from the sample behind it, under a matte of 255s, of 0s (src is
             not read: the bytes are dst's, read and written back, and the alpha) and a half-soft one (blocks of 32 x 32 pixels:
             a quarter 0, a quarter 255, the rest noise)
    over     Image.alpha_composite on uint8 HWC RGBA, the batch's own alpha channel half-soft

on float16 CHW and uint8 HWC with c = 3 (over: c = 4).  Every leg is timed with device events around it, after a warm-up, `--calls`
times, the legs alternating; the table has the median, the least and the most of each and the rates of the medians.  Our legs include
the host's plan and the table's copy; the pieces' ctypes tables are built once, ahead.  Nothing is asserted about the rates.

    python tools/ubench/alpha_paste_batch.py [--samples 256] [--side 448] [--calls 20] [--out FILE]

Needs a GPU; there is no fallback."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def mattes(n, s, g):
    import torch

    kind = torch.randint(0, 4, (n, (s + 31) // 32, (s + 31) // 32), generator=g).repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :s, :s]
    soft = torch.randint(0, 256, (n, s, s), generator=g, dtype=torch.uint8)
    soft[kind == 0] = 0
    soft[kind == 1] = 255
    return {"opaque": torch.full((n, s, s), 255, dtype=torch.uint8), "transparent": torch.zeros((n, s, s), dtype=torch.uint8), "soft": soft.contiguous()}


def timed(legs, warmup, calls):
    import torch

    times = {who: [] for who in legs}
    for it in range(warmup + calls):
        for who, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[who].append(e0.elapsed_time(e1))
    return times


def measure(a):
    """-> [[format, leg, bytes moved, ms list], ...]"""
    import torch

    import llcomp_amd as mi

    assert mi.device_count() >= 1 and torch.cuda.is_available(), "needs a GPU"
    n, s = a.samples, a.side
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(a.seed)
    rows = []
    tuples = [(i, (i + 1) % n, 0, 0, 0, 0, s, s) for i in range(n)]
    alpha_pieces = mi.alpha_pieces(tuples)
    paste_pieces = mi.paste_pieces([t + (list(range(256)),) for t in tuples])
    m = {k: v.cuda() for k, v in mattes(n, s, g).items()}
    for dtype, layout, c in (("float16", "chw", 3), ("uint8", "hwc", 3)):
        codec = mi.Codec(1, 64, 64, c, device=0)
        shape = (n, c, s, s) if layout == "chw" else (n, s, s, c)
        if dtype == "uint8":
            src, dst = (torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).cuda() for _ in range(2))
        else:
            src, dst = (torch.randn(shape, generator=g).to(torch.float16).cuda() for _ in range(2))
        batch, matte = dst.numel() * dst.element_size(), n * s * s
        moved = {"opaque": 3 * batch + matte, "transparent": 2 * batch + matte, "soft": 3 * batch + matte, "paste": 2 * batch + matte}
        moved["copy"] = moved["soft"]
        half = torch.empty(moved["copy"] // 2, dtype=torch.uint8, device="cuda")
        other = torch.empty_like(half)

        def alpha_leg(which):
            return lambda: codec.alpha_paste_batch(src.data_ptr(), m[which].data_ptr(), 1, 0, n, s, s, dst.data_ptr(), n, s, s, alpha_pieces, dtype=dtype,
                                                   layout=layout, stream=st)

        legs = {k: alpha_leg(k) for k in ("opaque", "transparent", "soft")}
        legs["paste"] = lambda: codec.paste_batch(src.data_ptr(), m["opaque"].data_ptr(), n, s, s, dst.data_ptr(), n, s, s, paste_pieces, dtype=dtype,
                                                  layout=layout, stream=st)
        legs["copy"] = lambda: other.copy_(half)
        times = timed(legs, a.warmup, a.calls)
        rows += [[f"{dtype} {layout} c={c}", who, moved[who], times[who]] for who in legs]
        codec.close()
        del src, dst, half, other
    # OVER: uint8 HWC RGBA, its own alpha
    codec = mi.Codec(1, 64, 64, 4, device=0)
    src, dst = (torch.randint(0, 256, (n, s, s, 4), generator=g, dtype=torch.uint8) for _ in range(2))
    src[..., 3] = mattes(n, s, g)["soft"]
    src, dst = src.cuda(), dst.cuda()
    over_pieces = mi.alpha_pieces([t + (mi.ALPHA_OVER,) for t in tuples])
    batch = dst.numel()
    half = torch.empty(3 * batch // 2, dtype=torch.uint8, device="cuda")
    other = torch.empty_like(half)
    legs = {"over": lambda: codec.alpha_paste_batch(src.data_ptr(), None, 1, 0, n, s, s, dst.data_ptr(), n, s, s, over_pieces, dtype="uint8", layout="hwc", stream=st),
            "own A": lambda: codec.alpha_paste_batch(src.data_ptr(), src.data_ptr(), 4, 3, n, s, s, dst.data_ptr(), n, s, s, alpha_pieces, dtype="uint8", layout="hwc",
                                                     stream=st),
            "copy": lambda: other.copy_(half)}
    times = timed(legs, a.warmup, a.calls)
    rows += [["uint8 hwc c=4", who, 3 * batch, times[who]] for who in legs]
    codec.close()
    return rows


def table(rows):
    out = ["  format            leg          moved MB   ms: median (min .. max)          GB/s   leg/paste"]
    paste = {fmt: nbytes / statistics.median(t) / 1e6 for fmt, who, nbytes, t in rows if who == "paste"}  # GB/s
    for fmt, who, nbytes, t in rows:
        med = statistics.median(t)
        rate = nbytes / med / 1e6
        rel = f"{rate / paste[fmt]:8.2f}" if fmt in paste and who not in ("paste", "copy") else ""
        out.append(f"  {fmt:<17} {who:<12} {nbytes / 1e6:8.0f}   {med:8.3f} ({min(t):.3f} .. {max(t):.3f})   {rate:8.0f}   {rel}")
    out.append("  (leg/paste: the leg's GB/s over paste_batch's GB/s on the same shapes)")
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
    lines = ["Batch alpha paste beside paste_batch with every id selected and a device-to-device copy of the same bytes (tools/ubench/alpha_paste_batch.py)",
             f"  {a.samples} samples of {a.side} x {a.side}, one full-size rectangle per sample; device events around each leg, {a.warmup} warm-up rounds, then",
             f"  {a.calls} rounds, the legs alternating; our legs include the host's plan and the table's copy; moved = dst read + src + alpha + dst write"]
    lines += table(measure(a))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
