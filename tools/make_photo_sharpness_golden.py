#!/usr/bin/env python3
"""Writes tests/golden/photo_sharpness_rule.json: seeded images and what PIL gives for them under ImageEnhance.Sharpness(image).enhance(a)
and, at a = 0, under image.filter(ImageFilter.SMOOTH) -- so that a machine without PIL still checks ADJUST_SHARPNESS of the photometric
chains (include/llcomp_mi.h) byte for byte (tests/test_photo_sharpness_rule.py).  Needs Pillow and numpy; run once, by hand:
    python tools/make_photo_sharpness_golden.py

A vector names its image by the seeded generator of tests/photo_spec.py (gen_image: kind, w, h, c, seed; kind "checker": its
checker()), gives the factor as a float32 in hex and the FNV-1a-64 of PIL's output; the vectors under "full" are tiny and carry
input and output in full.  The file records the Pillow version that wrote it."""
import json
import os
import sys

import numpy as np
from PIL import Image, ImageEnhance, ImageFilter

import PIL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import photo_spec  # noqa: E402  (the image generators only: the outputs recorded here are PIL's)

FACTORS = [0.0, 1.0, 2.0, 0.5, 1.9, 7.5, 0.3, 256.0]
SIZES = [(1, 1), (2, 3), (3, 2), (3, 3), (4, 3), (23, 17), (80, 5), (5, 80)]


def fnv1a64(data):
    h = 0xCBF29CE484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def pil_sharpness(img, a):
    im = Image.fromarray(img[..., 0] if img.shape[2] == 1 else img)
    return np.asarray(ImageEnhance.Sharpness(im).enhance(float(np.float32(a)))).reshape(img.shape)


def pil_smooth(img):
    im = Image.fromarray(img[..., 0] if img.shape[2] == 1 else img)
    return np.asarray(im.filter(ImageFilter.SMOOTH)).reshape(img.shape)


def main():
    vectors, seed = [], 900
    for c in (1, 3):
        for i, (w, h) in enumerate(SIZES):
            for j, a in enumerate(FACTORS):
                seed += 1
                kind = ("noise", "narrow", "ramp", "checker")[(i + j) % 4]
                img = photo_spec.gen_image(kind, w, h, c, seed)
                out = pil_sharpness(img, a)
                if a == 0.0:
                    assert np.array_equal(out, pil_smooth(img))
                vectors.append(dict(kind=kind, w=w, h=h, c=c, seed=seed, param=float(np.float32(a)).hex(), fnv=fnv1a64(out.tobytes())))
    full = []
    for c, kind, w, h, a in ((3, "noise", 3, 3, 0.0), (1, "noise", 5, 4, 2.0), (3, "checker", 4, 3, 7.5), (1, "checker", 6, 5, 0.5), (3, "noise", 2, 5, 1.9)):
        seed += 1
        img = photo_spec.gen_image(kind, w, h, c, seed)
        full.append(dict(w=w, h=h, c=c, param=float(np.float32(a)).hex(), image=img.reshape(-1).tolist(), out=pil_sharpness(img, a).reshape(-1).tolist()))
    doc = dict(about="PIL %s ImageEnhance.Sharpness on the seeded images of tests/photo_spec.py and the checkers of this tool; written by "
                     "tools/make_photo_sharpness_golden.py" % PIL.__version__, pillow=PIL.__version__, vectors=vectors, full=full)
    path = os.path.join(ROOT, "tests", "golden", "photo_sharpness_rule.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("%d vectors, %d in full -> %s" % (len(vectors), len(full), path))


if __name__ == "__main__":
    main()
