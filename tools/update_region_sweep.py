#!/usr/bin/env python3
"""Region update against the only way there was before it (DESIGN.md "Region update"): device-resident batches of 16 frames of 4K RGB8
(photo-like "nat" and g3 noise from the seeded generators of bench.make_frames) on 480x1 planes and 64x64 interleaved tiles; rectangles
of 64x64, 224x224, 512x512 and 1920x1080, each with its origin on the tile grid and offset by half a tile.  Per case the medians over
the repeats of
    update   Codec.update_region (covered slices coded again, spliced in HBM),
    encode   Codec.encode_region alone (no splice),
    baseline Codec.decode of the whole batch + a torch paste + Codec.encode of the whole batch,
in the same process, the three legs in rotating order from repeat to repeat, hipEvents on the stream with a synchronise behind each
leg.  Every update is checked: decode(update) == the modified frames.  "whole_box" says whether the rectangle is exactly its box's
pixels (then nothing is decoded).  --host adds one 8192 x 8192 RGB noise image in 512x1 planes through the host calls: update_region
against decompress_image + paste + compress_image, with the bytes that cross PCIe each way computed from the slice table.

    python tools/update_region_sweep.py [out.jsonl] [--reps N] [--tag TEXT] [--host] [--only SLICING]     # on a GPU box; one JSON line per case
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/update_region_sweep.py --profile-case
        # one case alone for a kernel trace: photo-like, 480x1 planes, 224x224 offset by half a tile, 20 calls of Codec.update_region
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, W, H, C = 16, 3840, 2160, 3
SLICINGS = [(480, 1, True), (64, 64, False)]
SIZES = [(64, 64), (224, 224), (512, 512), (1920, 1080)]
X0, Y0 = 960, 512  # on the grid of both slicings (960 = 2 * 480 = 15 * 64, 512 = 8 * 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tag", default="")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--profile-case", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch

    import bench
    import llcomp_amd as mi

    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            print(line, file=out, flush=True)

    emit({"tool": "update_region_sweep", "tag": a.tag, "frames": FRAMES, "w": W, "h": H, "c": C, "reps": a.reps, "device": torch.cuda.get_device_name(0)})
    st = torch.cuda.current_stream()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        ev0.record(st)
        fn()
        ev1.record(st)
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1)

    if a.profile_case:
        d_img = torch.from_numpy(bench.make_frames("nat", FRAMES, 0, distinct=4)).cuda()
        codec = mi.Codec(FRAMES, W, H, C, 480, 1, True, device=0)
        codec.prepare(encode=True, decode=True, region=True, update=True)
        cap = min(codec.max_payload_bytes, 2 * d_img.numel() + 64 * codec.n_slices + 4096)
        d_pay, d_new = (torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(2))
        d_len, d_new_len = (torch.empty(codec.n_slices, dtype=torch.int32, device="cuda") for _ in range(2))
        d_tot, d_st = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        codec.encode(d_img.data_ptr(), d_pay.data_ptr(), cap, d_len.data_ptr(), d_tot.data_ptr(), d_st.data_ptr(), st.cuda_stream)
        torch.cuda.synchronize()
        total, x, y = int(d_tot.item()), X0 + 240, Y0
        d_rect = torch.randint(0, 256, (FRAMES, 224, 224, C), dtype=torch.uint8, device="cuda")
        for _ in range(20):
            codec.update_region(d_pay.data_ptr(), total, d_len.data_ptr(), x, y, 224, 224, d_rect.data_ptr(), d_new.data_ptr(), cap,
                                d_new_len.data_ptr(), d_tot.data_ptr(), d_st.data_ptr(), st.cuda_stream)
        torch.cuda.synchronize()
        assert int(d_st.item()) == 0
        emit({"profile_case": "nat 480x1p 224x224 offset", "calls": 20, "payload_mb": round(total / 1e6, 1)})
        return
    for content in ("nat", "g3"):
        d_img = torch.from_numpy(bench.make_frames(content, FRAMES, 0, distinct=4)).cuda()
        for tw, th, planar in SLICINGS:
            name = f"{tw}x{th}{'p' if planar else 'i'}"
            if a.only and a.only != name:
                continue
            codec = mi.Codec(FRAMES, W, H, C, tw, th, planar, device=0)
            codec.prepare(encode=True, decode=True, region=True, update=True)
            cap = min(codec.max_payload_bytes, 2 * d_img.numel() + 64 * codec.n_slices + 4096)
            d_pay, d_new = (torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(2))
            d_len, d_new_len = (torch.empty(codec.n_slices, dtype=torch.int32, device="cuda") for _ in range(2))
            d_tot, d_new_tot = (torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(2))
            d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
            codec.encode(d_img.data_ptr(), d_pay.data_ptr(), cap, d_len.data_ptr(), d_tot.data_ptr(), d_st.data_ptr(), st.cuda_stream)
            torch.cuda.synchronize()
            assert int(d_st.item()) == 0
            total = int(d_tot.item())
            d_full = torch.empty_like(d_img)
            for rw, rh in SIZES:
                for offset in (False, True):
                    x, y = X0 + (tw // 2 if offset else 0), Y0 + (th // 2 if offset else 0)
                    (box, n_cov) = mi.region_plan(W, H, C, tw, th, planar, x, y, rw, rh)
                    whole = (x % tw == 0 and y % th == 0 and (rw % tw == 0 or x + rw == W) and (rh % th == 0 or y + rh == H))
                    d_rect = torch.randint(0, 256, (FRAMES, rh, rw, C), dtype=torch.uint8, device="cuda")
                    d_rect[:, : rh // 2] = d_img[:, y:y + rh // 2, x:x + rw] // 2 + 31  # (half noise, half picture-like)
                    want = d_img.clone()
                    want[:, y:y + rh, x:x + rw] = d_rect

                    def update():
                        codec.update_region(d_pay.data_ptr(), total, d_len.data_ptr(), x, y, rw, rh, d_rect.data_ptr(), d_new.data_ptr(), cap,
                                            d_new_len.data_ptr(), d_new_tot.data_ptr(), d_st.data_ptr(), st.cuda_stream)

                    def encode_only():
                        codec.encode_region(d_pay.data_ptr(), total, d_len.data_ptr(), x, y, rw, rh, d_rect.data_ptr(), d_new.data_ptr(), cap,
                                            d_new_len.data_ptr(), d_new_tot.data_ptr(), d_st.data_ptr(), st.cuda_stream)

                    def baseline():
                        codec.decode(d_pay.data_ptr(), total, d_len.data_ptr(), d_full.data_ptr(), d_st.data_ptr(), st.cuda_stream)
                        d_full[:, y:y + rh, x:x + rw] = d_rect
                        codec.encode(d_full.data_ptr(), d_new.data_ptr(), cap, d_new_len.data_ptr(), d_new_tot.data_ptr(), d_st.data_ptr(), st.cuda_stream)

                    legs = [("update", update), ("encode", encode_only), ("baseline", baseline)]
                    for _, fn in legs:  # warm-up, and the check of each leg that writes a full batch
                        fn()
                        torch.cuda.synchronize()
                        assert int(d_st.item()) == 0, (content, name, rw, rh, offset)
                    base_total = int(d_new_tot.item())
                    update()
                    torch.cuda.synchronize()
                    assert int(d_new_tot.item()) == base_total, "update_region and a full encode disagree on the payload size"
                    codec.decode(d_new.data_ptr(), base_total, d_new_len.data_ptr(), d_full.data_ptr(), d_st.data_ptr(), st.cuda_stream)
                    torch.cuda.synchronize()
                    assert int(d_st.item()) == 0 and torch.equal(d_full, want), (content, name, rw, rh, offset)
                    ms = {k: [] for k, _ in legs}
                    for r in range(a.reps):
                        for i in range(3):
                            k, fn = legs[(r + i) % 3]
                            ms[k].append(timed(fn))
                    assert int(d_st.item()) == 0
                    med = {k: float(np.median(v)) for k, v in ms.items()}
                    fam = codec.region_family(x, y, rw, rh)
                    emit({"content": content, "slicing": name, "rect": f"{rw}x{rh}", "x": x, "y": y, "whole_box": whole,
                          "covered_slices_per_frame": n_cov, "slices_per_frame": codec.n_slices // FRAMES,
                          "family": "".join(k[0] for k in ("rows", "lds_table", "snapshot", "bank_cache") if fam[k]) or "-",
                          "update_ms": round(med["update"], 3), "encode_region_ms": round(med["encode"], 3), "baseline_ms": round(med["baseline"], 3),
                          "update_over_baseline": round(med["update"] / med["baseline"], 4), "update_ms_min": round(min(ms["update"]), 3),
                          "baseline_ms_min": round(min(ms["baseline"]), 3), "payload_mb": round(total / 1e6, 1)})
                    del d_rect, want
            codec.close()
            del d_pay, d_new, d_len, d_new_len, d_full
            torch.cuda.empty_cache()
        del d_img
    if a.host:
        side, tw = 8192, 512
        img = np.random.default_rng(7).integers(0, 256, size=(side, side, 3), dtype=np.uint8)
        old = mi.compress_image(img, side, side, 3, format=mi.FORMAT_SLICED, tile_w=tw, tile_h=1, planar=True, device=0)
        n = int.from_bytes(old[20:24], "little")
        lens = np.frombuffer(old, dtype="<u4", count=n, offset=24).astype(np.int64)
        for rw, rh in SIZES:
            for offset in (False, True):
                x, y = 1024 + (tw // 2 if offset else 0), 1024
                patch = np.random.default_rng(rw + offset).integers(0, 256, size=(rh, rw, 3), dtype=np.uint8)
                (tx0, ty0, tx1, ty1), n_cov = mi.region_plan(side, side, 3, tw, 1, True, x, y, rw, rh)
                whole = x % tw == 0 and rw % tw == 0
                ntx = side // tw
                ids = np.array([(ty * ntx + tx) * 3 + ch for ty in range(ty0, ty1) for tx in range(tx0, tx1) for ch in range(3)])
                first, last = int(ids.min()), int(ids.max())
                span = int(lens[first:last + 1].sum())  # the covered span: first covered slice's first byte to the last one's end
                t_upd, t_base = [], []
                got = None
                for r in range(max(3, a.reps // 2)):
                    t0 = time.perf_counter()
                    got = mi.update_region(old, x, y, patch, device=0)
                    t1 = time.perf_counter()
                    px = mi.decompress_image(old, device=0).pixels
                    px[y:y + rh, x:x + rw] = patch
                    ref = mi.compress_image(px, side, side, 3, format=mi.FORMAT_SLICED, tile_w=tw, tile_h=1, planar=True, device=0)
                    t2 = time.perf_counter()
                    t_upd.append(1e3 * (t1 - t0))
                    t_base.append(1e3 * (t2 - t1))
                    assert got == ref, "update_region differs from a full encode of the modified picture"
                new_lens = np.frombuffer(got, dtype="<u4", count=n, offset=24).astype(np.int64)
                up = 24 + 4 * n + rw * rh * 3 + (0 if whole else span)
                down = 16 + ((4 * n_cov + 15) & ~15) + int(new_lens[ids].sum())
                emit({"host": f"{side}x{side} noise, {tw}x1p", "rect": f"{rw}x{rh}", "x": x, "y": y, "whole_box": whole, "covered_slices": n_cov,
                      "update_ms": round(float(np.median(t_upd)), 2), "baseline_ms": round(float(np.median(t_base)), 2),
                      "update_over_baseline": round(float(np.median(t_upd) / np.median(t_base)), 4), "bytes_up": up, "bytes_down": down,
                      "baseline_bytes_up": len(old) + img.size, "baseline_bytes_down": img.size + len(old), "container_mb": round(len(old) / 1e6, 1)})
    if out:
        out.close()


if __name__ == "__main__":
    main()
