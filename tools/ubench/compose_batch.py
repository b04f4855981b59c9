#!/usr/bin/env python3
"""What the batch composition costs on three workloads in HBM, against two yardsticks of torch's on the same pieces in the same run:

    expr   torch's slice-assignment loop for the same pieces, one launch per rectangle, which is what a user writes today:
             out[d, :, dy:dy+h, dx:dx+w] = src[s, :, sy:sy+h, sx:sx+w]      (a FILL piece: = fill[:, None, None])
           behind one broadcast assignment of the fill over the whole dst batch unless the call keeps what no piece covers
    copy   y.copy_(x) of as many bytes as the call WRITES into a buffer that exists: one read and one write per byte, the floor for a
           kernel that moves the same bytes with the same access width

    mosaic        256 canvases of 3 x 448 x 448 from 1024 samples of 224 x 224, four per canvas around a centre drawn as load_mosaic
                  draws it, fill 114: every dst byte is written
    batch_images  256 samples of 224 x 224, one piece each at (0, 0) of a canvas of 256 x 256, fill 0: every dst byte is written
    gridmask      a 4 x 4 grid of 28 x 28 holes on each of 256 samples of 224 x 224, in place (no src, KEEP): the holes are written

on float16 CHW and uint8 HWC.  Every leg is timed with device events around it, after a warm-up, `--calls` times, the legs alternating;
the table has the median, the least and the most of each, the GB/s of the bytes written (twice, where they are read from a src) over
our median, and both yardsticks over ours.  The spread of the copy leg, whose work never changes, is the run-to-run spread to read the
other columns against.  Our leg includes the host's plan and the table's copy; the pieces' ctypes table is built once, ahead.

    python tools/ubench/compose_batch.py [--canvases 256] [--side 224] [--calls 20] [--out FILE]

Needs a GPU; there is no fallback."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def expression(dst, src, tuples, fill, keep, layout):
    """torch's loop: dst [n, c, h, w] or [n, h, w, c] in place"""
    fv = fill.view(-1, 1, 1) if layout == "chw" else fill.view(1, 1, -1)
    if not keep:
        dst[:] = fv
    for d, s, dx, dy, sx, sy, w, h, flags in tuples:
        if layout == "chw":
            dst[d, :, dy:dy + h, dx:dx + w] = fv if flags else src[s, :, sy:sy + h, sx:sx + w]
        else:
            dst[d, dy:dy + h, dx:dx + w, :] = fv if flags else src[s, sy:sy + h, sx:sx + w, :]
    return dst


def workloads(mi, a, rng):
    """-> [(name, n_src, iw, ih, n_dst, ow, oh, pieces, fill, keep, pixels written per channel), ...]"""
    n, s = a.canvases, a.side
    centres = [(int(rng.uniform(s / 2, 3 * s / 2)), int(rng.uniform(s / 2, 3 * s / 2))) for _ in range(n)]
    big = s + 32
    holes = [(i, 0, gx * (s // 4) + s // 16, gy * (s // 4) + s // 16, 0, 0, s // 8, s // 8, mi.COMPOSE_FILL) for i in range(n) for gy in range(4) for gx in range(4)]
    return [("mosaic", 4 * n, s, s, n, 2 * s, 2 * s, mi.mosaic_pieces(centres, s, s, s), 114.0, False, n * 4 * s * s),
            ("batch_images", n, s, s, n, big, big, mi.compose_pieces([(i, i, 0, 0, 0, 0, s, s) for i in range(n)]), 0.0, False, n * big * big),
            ("gridmask", 0, 0, 0, n, s, s, mi.compose_pieces(holes), 0.0, True, n * 16 * (s // 8) ** 2)]


def measure(a):
    """-> [[format, workload, bytes moved, ours ms list, expr ms list, copy ms list], ...]"""
    import random

    import torch

    import llcomp_amd as mi

    assert mi.device_count() >= 1 and torch.cuda.is_available(), "needs a GPU"
    c = 3
    codec = mi.Codec(1, 64, 64, c, device=0)
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(a.seed)
    rows = []
    for dtype, layout in (("float16", "chw"), ("uint8", "hwc")):
        es = 1 if dtype == "uint8" else 2
        tdt = getattr(torch, dtype)
        bits = torch.uint8 if dtype == "uint8" else torch.int16

        def batch(n, w, h):
            shape = (n, c, h, w) if layout == "chw" else (n, h, w, c)
            if dtype == "uint8":
                return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).cuda()
            return torch.randn(shape, generator=g).to(tdt).cuda()

        for name, n_src, iw, ih, n_dst, ow, oh, pieces, fill, keep, px in workloads(mi, a, random.Random(a.seed)):
            src = batch(n_src, iw, ih) if n_src else None
            dst0 = batch(n_dst, ow, oh)
            tuples = [(p.dst, p.src, p.dx, p.dy, p.sx, p.sy, p.w, p.h, p.flags) for p in pieces if p.w and p.h]
            fv = torch.full((c,), fill).to(tdt).cuda()
            written = px * c * es
            x = torch.randint(0, 256, (written,), generator=g, dtype=torch.uint8).cuda()
            y = torch.empty_like(x)

            def ours(dst):
                codec.compose_batch(src.data_ptr() if n_src else None, n_src, iw, ih, dst.data_ptr(), n_dst, ow, oh, pieces, dtype=dtype, layout=layout,
                                    fill=fill, keep=keep, stream=st)
                return dst

            # what is timed is also right: ours against torch's loop, once
            assert torch.equal(ours(dst0.clone()).view(bits), expression(dst0.clone(), src, tuples, fv, keep, layout).view(bits)), (dtype, layout, name)
            dst = dst0.clone()
            legs = {"ours": lambda: ours(dst), "expr": lambda: expression(dst, src, tuples, fv, keep, layout), "copy": lambda: y.copy_(x)}
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
            rows.append([f"{dtype} {layout}", name, written * (2 if n_src else 1), len(tuples)] + [times[who] for who in ("ours", "expr", "copy")])
            del src, dst0, dst, x, y
    codec.close()
    return rows


def table(rows):
    def span(v):
        return f"{statistics.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})"

    out = ["  format       workload      pieces  ours ms: median (min .. max)    GB/s   expr ms: median (min .. max)     copy ms: median (min .. max)  expr/ours copy/ours"]
    for fmt, name, moved, n_pieces, ours, expr, copy in rows:
        mo = statistics.median(ours)
        out.append(f"  {fmt:<12} {name:<13} {n_pieces:6d} {span(ours)} {moved / (mo * 1e-3) / 1e9:7.0f}   {span(expr)}   {span(copy)}   "
                   f"{statistics.median(expr) / mo:7.2f} {statistics.median(copy) / mo:8.2f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--canvases", type=int, default=256)
    ap.add_argument("--side", type=int, default=224)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["Batch composition against torch's slice-assignment loop and a plain copy_ of the bytes written (tools/ubench/compose_batch.py)",
             f"  {a.canvases} canvases, samples of 3 x {a.side} x {a.side}; device events around each leg, {a.warmup} warm-up rounds, then {a.calls} rounds, the legs",
             "  alternating; GB/s of the bytes written (twice where a src is read) over our median; ours includes the host's plan and the table's copy"]
    lines += table(measure(a))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
