#!/usr/bin/env python3
"""Writes tests/golden/resize_filters_pil.json: what PIL's Image.resize gives for crops of the deterministic images of
llcomp_amd/synth.py under each of its five weighted filters, as FNV-1a-64 of the output bytes.  The resized calls promise these bytes
(include/llcomp_mi.h: llcomp_mi_resize_filter_weights); the golden file lets the tests hold the rule to them where PIL is absent.

    python3 tools/gen_resize_filters_golden.py [--per-filter 12] [--out tests/golden/resize_filters_pil.json]

The reference of a case is Image.fromarray(crop).resize((ow, oh), resample): crop first, then resize (torchvision's resized_crop), not
resize's box= argument, which reads outside the box.  c = 4 is resized band by band: PIL premultiplies alpha when it resizes RGBA."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from llcomp_amd import synth  # noqa: E402

FILTERS = ("bilinear", "box", "hamming", "bicubic", "lanczos")  # (nearest is an integer formula, it needs no recorded bytes)
REACH = {"bilinear": 1, "box": 1, "hamming": 1, "bicubic": 2, "lanczos": 3}


def fnv1a64(data):
    h = 1469598103934665603
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def pil_resize(crop, ow, oh, name):
    from PIL import Image

    resample = getattr(Image.Resampling, name.upper())
    if crop.shape[2] == 1:
        return np.asarray(Image.fromarray(crop[:, :, 0]).resize((ow, oh), resample))[:, :, None]
    if crop.shape[2] == 3:
        return np.asarray(Image.fromarray(crop).resize((ow, oh), resample))
    return np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(crop[:, :, k])).resize((ow, oh), resample))
                     for k in range(crop.shape[2])], axis=2)


def random_case(rng, name, w, h):
    """a rectangle inside w x h with sides 4..min(side, 500) and an output with sides 3..230 inside the filter's downscale limit"""
    while True:
        rw, rh = int(rng.integers(4, min(w, 500) + 1)), int(rng.integers(4, min(h, 500) + 1))
        ow, oh = int(rng.integers(3, 231)), int(rng.integers(3, 231))
        if REACH[name] * rw <= 64 * ow and REACH[name] * rh <= 64 * oh:
            return [int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1)), rw, rh], [ow, oh]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-filter", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "resize_filters_pil.json"))
    args = ap.parse_args()
    import PIL

    rng = np.random.default_rng(20260)
    gens = ("g3", "nat", "g1", "mid", "checker", "g2")
    cases = []
    for name in FILTERS:
        for i in range(args.per_filter):
            gen, c = gens[i % len(gens)], (1, 3, 4)[i % 3]
            w, h = int(rng.integers(40, 521)), int(rng.integers(40, 521))
            rect, out = random_case(rng, name, w, h)
            img = synth.GENERATORS[gen](w, h, c)
            x, y, rw, rh = rect
            got = pil_resize(np.ascontiguousarray(img[y:y + rh, x:x + rw]), out[0], out[1], name)
            cases.append({"gen": gen, "shape": [w, h, c], "rect": rect, "out": out, "filter": name, "fnv": fnv1a64(got.tobytes())})
    with open(args.out, "w") as f:
        f.write('{"pil": "%s", "cases": [\n' % PIL.__version__)
        f.write(",\n".join(json.dumps(c, separators=(",", ":")) for c in cases))
        f.write("\n]}\n")
    print(f"{len(cases)} cases -> {args.out}")


if __name__ == "__main__":
    main()
