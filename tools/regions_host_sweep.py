#!/usr/bin/env python3
"""Crops of HOST containers into HBM (DESIGN.md "Region decode"): Codec.decode_regions_host, which sends only the windows' bytes over
PCIe, against the two ways a data loader had before it -- pack_batch + an upload of the whole batch + Codec.decode_regions, and a loop of
decompress_region (one container per call) whose crops are then uploaded.  Each is timed end to end, from a Python list of bytes
containers to the crops in HBM with a synchronise behind them.  16 frames of 4K RGB8 (nat = photo-like, g3 = noise, the seeded
generators of bench.make_frames), 480x1 planar and 64x64 interleaved slices, 224x224 and 512x512 crops at seeded random offsets; at
64x64 (2160 % 64 != 0) once with every window above the last tile row (one class) and once with half the frames' windows in it (two).

Per case: the median of each variant in ms; the time until decode_regions_host returns (the single-threaded gather into pinned memory);
the bytes each variant sends host to device; and for the streaming pipeline (4 frames per job, depth 4) crops/s of region jobs against
decode jobs plus a NumPy crop of every frame.  Every variant is warmed up first, the three rotate their order from repeat to repeat, and
every output is checked against the crops of the source frames.

    python tools/regions_host_sweep.py [out.jsonl] [--reps N] [--tag TEXT]      # on a GPU box; one JSON line per case
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
CROPS = [224, 512]
STREAM_FPJ, STREAM_DEPTH, STREAM_JOBS = 4, 4, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tag", default="")
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

    emit({"tool": "regions_host_sweep", "tag": a.tag, "frames": FRAMES, "w": W, "h": H, "c": C, "reps": a.reps,
          "device": torch.cuda.get_device_name(0)})
    st = torch.cuda.current_stream()
    rng = np.random.default_rng(224)
    for content in ("nat", "g3"):
        imgs = bench.make_frames(content, FRAMES, 0, distinct=4)
        d_img = torch.from_numpy(imgs).cuda()
        for tw, th, planar in SLICINGS:
            conts = [mi.compress_image(imgs[f], W, H, C, format=mi.FORMAT_SLICED, tile_w=tw, tile_h=th, planar=planar, device=0)
                     for f in range(FRAMES)]
            n = mi.slice_count(W, H, C, tw, th, planar)
            tabs = [np.frombuffer(d, dtype="<u4", count=n, offset=24).astype(np.int64) for d in conts]
            codec = mi.Codec(FRAMES, W, H, C, tw, th, planar, device=0)
            codec.prepare(encode=False, decode=True, region=True, regions=True)
            d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
            xys = []
            for r in CROPS:
                last_row0 = (H - 1) // th * th  # the first pixel row of the last tile row
                kinds = [("random", None)] if H % th == 0 else [("1class", False), ("2class", True)]
                for kind, bottom in kinds:
                    xs = rng.integers(0, W - r + 1, size=FRAMES)
                    if bottom is None:
                        ys = rng.integers(0, H - r + 1, size=FRAMES)
                    else:  # windows clear of the last tile row, and (2 classes) every other frame's crop at the bottom edge
                        ys = rng.integers(0, max(1, last_row0 - 2 * th - r), size=FRAMES)
                        if bottom:
                            ys[1::2] = H - r
                    xy = np.stack([xs, ys], axis=1).astype(np.uint32)
                    xys.append((r, kind, xy))
                    n_classes = mi.regions_plan(W, H, C, tw, th, planar, r, r, xy)[1]
                    want = torch.stack([d_img[f, int(y):int(y) + r, int(x):int(x) + r] for f, (x, y) in enumerate(xy)])
                    d_out = torch.empty((FRAMES, r, r, C), dtype=torch.uint8, device="cuda")
                    gather_s = []

                    def pack_upload():
                        pay, lens = mi.pack_batch(conts)
                        d_pay = torch.from_numpy(pay).cuda()
                        d_len = torch.from_numpy(lens.view(np.int32)).cuda()
                        codec.decode_regions(d_pay.data_ptr(), len(pay), d_len.data_ptr(), xy, r, r, d_out.data_ptr(), d_st.data_ptr(), st.cuda_stream)
                        torch.cuda.synchronize()

                    def host():
                        t0 = time.perf_counter()
                        codec.decode_regions_host(conts, xy, r, r, d_out.data_ptr(), d_st.data_ptr(), st.cuda_stream)
                        gather_s.append(time.perf_counter() - t0)
                        torch.cuda.synchronize()

                    def loop():
                        got = np.stack([mi.decompress_region(conts[f], int(x), int(y), r, r, device=0).pixels for f, (x, y) in enumerate(xy)])
                        d_out.copy_(torch.from_numpy(got).cuda())
                        torch.cuda.synchronize()

                    variants = [("pack_upload", pack_upload), ("host", host), ("loop", loop)]
                    for _, fn in variants:
                        d_out.zero_()
                        fn()
                        fn()
                        assert int(d_st.item()) == 0 and torch.equal(d_out, want), (content, tw, th, r, kind)
                    gather_s.clear()
                    times = {name: [] for name, _ in variants}
                    for rep in range(a.reps):
                        k = rep % len(variants)
                        for name, fn in variants[k:] + variants[:k]:
                            t0 = time.perf_counter()
                            fn()
                            times[name].append(1e3 * (time.perf_counter() - t0))
                    assert int(d_st.item()) == 0 and torch.equal(d_out, want)
                    # bytes host -> device: the whole batch and its tables; the gathered slot; per frame the header, the table and the
                    # covered span (llcomp_mi_decode_region), plus the crops' upload
                    pay_b = sum(int(t.sum()) for t in tabs)
                    g_pay, g_len, _ = mi.regions_gather(conts, xy, r, r)
                    host_b = ((32 * FRAMES + 4 * g_len.size + 7) & ~7) + 8 * g_len.size + g_pay.size
                    planes = C if planar else 1
                    ntx = -(-W // tw)
                    loop_b = FRAMES * r * r * C
                    for f, (x, y) in enumerate(xy):
                        (tx0, ty0, tx1, ty1), _ = mi.region_plan(W, H, C, tw, th, planar, int(x), int(y), r, r)
                        s0, s1 = (ty0 * ntx + tx0) * planes, ((ty1 - 1) * ntx + tx1) * planes
                        loop_b += 24 + 4 * n + int(tabs[f][s0:s1].sum())
                    med = {name: float(np.median(t)) for name, t in times.items()}
                    emit({"content": content, "slicing": f"{tw}x{th}{'p' if planar else 'i'}", "crop": f"{r}x{r}", "offsets": kind,
                          "classes": n_classes, "pack_upload_ms": round(med["pack_upload"], 3), "host_ms": round(med["host"], 3),
                          "loop_ms": round(med["loop"], 3), "host_gather_ms": round(1e3 * float(np.median(gather_s)), 3),
                          "host_over_pack_upload": round(med["host"] / med["pack_upload"], 3), "host_over_loop": round(med["host"] / med["loop"], 3),
                          "h2d_bytes": {"pack_upload": pay_b + 4 * n * FRAMES, "host": host_b, "loop": loop_b},
                          "pack_upload_ms_min": round(min(times["pack_upload"]), 3), "host_ms_min": round(min(times["host"]), 3),
                          "loop_ms_min": round(min(times["loop"]), 3)})
                    del d_out, want
            codec.close()
            torch.cuda.empty_cache()
            # the streaming pipeline: region jobs against decode jobs plus a NumPy crop, STREAM_JOBS jobs of STREAM_FPJ frames kept in flight
            s = mi.Stream(W, H, C, tw, th, planar, depth=STREAM_DEPTH, device=0, frames_per_job=STREAM_FPJ)
            bufs = [np.frombuffer(d, np.uint8) for d in conts]
            for r, kind, xy in xys:
                def run(regions):
                    done, sub, crops = 0, 0, 0
                    while done < STREAM_JOBS:
                        while sub < STREAM_JOBS:
                            f0 = (sub * STREAM_FPJ) % FRAMES
                            part, pxy = bufs[f0:f0 + STREAM_FPJ], xy[f0:f0 + STREAM_FPJ]
                            ok = s.submit_decode_regions(part, pxy, r, r, tag=sub) if regions else s.submit_decode(part, tag=sub)
                            if not ok:
                                break
                            sub += 1
                        job = s.wait()
                        assert job.status == mi.OK
                        f0 = (job.tag * STREAM_FPJ) % FRAMES
                        for j in range(STREAM_FPJ):
                            x, y = (int(v) for v in xy[f0 + j])
                            crop = job.data[j] if regions else np.ascontiguousarray(job.data[j, y:y + r, x:x + r])
                            if done == 0:
                                assert np.array_equal(crop, imgs[f0 + j, y:y + r, x:x + r])
                            crops += 1
                        s.release(job)
                        done += 1
                    return crops

                rates = {True: [], False: []}
                run(True)
                run(False)
                for rep in range(3):
                    for regions in ((True, False) if rep % 2 == 0 else (False, True)):
                        t0 = time.perf_counter()
                        k = run(regions)
                        rates[regions].append(k / (time.perf_counter() - t0))
                emit({"content": content, "slicing": f"{tw}x{th}{'p' if planar else 'i'}", "crop": f"{r}x{r}", "offsets": kind,
                      "stream": {"frames_per_job": STREAM_FPJ, "depth": STREAM_DEPTH, "jobs": STREAM_JOBS},
                      "stream_region_crops_per_s": round(float(np.median(rates[True])), 1),
                      "stream_decode_crop_crops_per_s": round(float(np.median(rates[False])), 1)})
            s.close()
            del conts, bufs
        del d_img
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
