#!/usr/bin/env python3
"""Writes tests/golden/photo_area_rule.json: seeded images and what PIL gives for them under ImageFilter.GaussianBlur(radius) and under
torchvision's adjust_hue as its PIL backend computes it (convert("HSV"), a wrapping byte add on H, convert("RGB")) -- so that a machine
without PIL still checks GAUSSIAN_BLUR and ADJUST_HUE of the photometric chains (include/llcomp_mi.h) byte for byte
(tests/test_photo_area_rule.py).  Needs Pillow and numpy; run once, by hand:  python tools/make_photo_area_golden.py

A vector names its image by the seeded generator of tests/photo_spec.py (gen_image: kind, w, h, c, seed), gives the op with its
parameter as a float32 in hex, and the FNV-1a-64 of PIL's output; the vectors under "full" are tiny and carry input and output in full."""
import json
import os
import sys

import numpy as np
from PIL import Image, ImageFilter

import PIL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import photo_spec  # noqa: E402  (the image generators only: the outputs recorded here are PIL's)

RADII = [0.0, 1e-4, 0.1, 0.5, 1.0, 2.0, 11.5, 32.0]
SIZES = [(1, 1), (2, 3), (3, 1), (23, 17), (80, 5)]
FACTORS = [0.0, 0.1, -0.1, 0.5, -0.5, 1 / 255, -1 / 255]


def fnv1a64(data):
    h = 0xCBF29CE484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def pil_op(img, op, p):
    p = float(np.float32(p))
    im = Image.fromarray(img[..., 0] if img.shape[2] == 1 else img)
    if op == "gaussian_blur":
        im = im.filter(ImageFilter.GaussianBlur(p))
    elif op == "adjust_hue":  # torchvision.transforms._functional_pil.adjust_hue
        if im.mode == "RGB":
            h, s, v = im.convert("HSV").split()
            # np_h += np.array(hue_factor * 255).astype("uint8") there: the cast of a negative double to uint8 is the platform's, and
            # on x86-64 and AArch64 builds of numpy it truncates toward zero and wraps -- stated here with integers
            np_h = ((np.array(h, dtype=np.int64) + (int(p * 255.0) & 0xFF)) & 0xFF).astype(np.uint8)
            im = Image.merge("HSV", (Image.fromarray(np_h), s, v)).convert("RGB")
    else:
        raise ValueError(op)
    return np.asarray(im).reshape(img.shape)


def main():
    vectors, seed = [], 500

    def add(kind, w, h, c, op, p):
        nonlocal seed
        seed += 1
        img = photo_spec.gen_image(kind, w, h, c, seed)
        vectors.append(dict(kind=kind, w=w, h=h, c=c, seed=seed, op=op, param=float(np.float32(p)).hex(), fnv=fnv1a64(pil_op(img, op, p).tobytes())))

    for c in (1, 3):
        for i, (w, h) in enumerate(SIZES):
            for j, radius in enumerate(RADII):
                add(("noise", "narrow", "ramp")[(i + j) % 3], w, h, c, "gaussian_blur", radius)
        for j, f in enumerate(FACTORS):
            add("noise", 23, 17, c, "adjust_hue", f)
            add(("narrow", "ramp", "constant")[j % 3], 40, 9, c, "adjust_hue", f)
    full = []
    for c, kind, w, h, op, p in ((3, "noise", 3, 2, "gaussian_blur", 1.0), (1, "noise", 5, 1, "gaussian_blur", 2.0), (3, "noise", 2, 3, "gaussian_blur", 32.0),
                                 (3, "noise", 4, 3, "adjust_hue", 0.1), (3, "narrow", 3, 2, "adjust_hue", -0.5), (1, "noise", 2, 2, "adjust_hue", 0.3)):
        seed += 1
        img = photo_spec.gen_image(kind, w, h, c, seed)
        full.append(dict(w=w, h=h, c=c, op=op, param=float(np.float32(p)).hex(), image=img.reshape(-1).tolist(), out=pil_op(img, op, p).reshape(-1).tolist()))
    doc = dict(about="PIL %s ImageFilter.GaussianBlur and the HSV round trip of adjust_hue on the seeded images of tests/photo_spec.py; written by "
                     "tools/make_photo_area_golden.py" % PIL.__version__, vectors=vectors, full=full)
    path = os.path.join(ROOT, "tests", "golden", "photo_area_rule.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("%d vectors, %d in full -> %s" % (len(vectors), len(full), path))


if __name__ == "__main__":
    main()
