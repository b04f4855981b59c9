#!/usr/bin/env python3
"""Writes tests/golden/photo_rule.json: seeded images, photometric chains and what PIL's ImageEnhance / ImageOps give for them -- so
that a machine without PIL still checks the rule of the photometric chains (include/llcomp_mi.h) byte for byte
(tests/test_photo_rule.py).  Needs Pillow and numpy; run once, by hand:  python tools/make_photo_golden.py

A vector names its image by the seeded generator of tests/photo_spec.py (gen_image: kind, w, h, c, seed), gives the chain with every
parameter as a float32 in hex, and the FNV-1a-64 of PIL's output; the vectors under "full" are tiny and carry input and output in full."""
import json
import os
import sys

import numpy as np
from PIL import Image, ImageEnhance, ImageOps

import PIL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import photo_spec  # noqa: E402  (the image generators only: the outputs recorded here are PIL's)


def fnv1a64(data):
    h = 0xCBF29CE484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def pil_chain(img, chain):
    im = Image.fromarray(img[..., 0] if img.shape[2] == 1 else img)
    for op, p in chain:
        p = float(np.float32(p))
        if op == "brightness":
            im = ImageEnhance.Brightness(im).enhance(p)
        elif op == "contrast":
            im = ImageEnhance.Contrast(im).enhance(p)
        elif op == "color":
            im = ImageEnhance.Color(im).enhance(p)
        elif op == "grayscale":
            im = im.convert("L").convert(im.mode)
        elif op == "invert":
            im = ImageOps.invert(im)
        elif op == "solarize":
            im = ImageOps.solarize(im, int(p))
        elif op == "posterize":
            im = ImageOps.posterize(im, int(p))
        elif op == "autocontrast":
            im = ImageOps.autocontrast(im)
        elif op == "equalize":
            im = ImageOps.equalize(im)
        else:
            raise ValueError(op)
    return np.asarray(im).reshape(img.shape)


def chain_json(chain):
    return [[op, float(np.float32(p)).hex()] for op, p in chain]


FACTORS = [0.0, 1.0, 0.37, 2.75]  # 0, 1, one inside (0, 1), one above 1 that saturates
ALONE = ([(op, a) for op in ("brightness", "contrast", "color") for a in FACTORS] +
         [("grayscale", 0), ("invert", 0), ("solarize", 0), ("solarize", 128), ("solarize", 256), ("posterize", 1), ("posterize", 4),
          ("posterize", 8), ("autocontrast", 0), ("equalize", 0)])
CHAINS = [
    [("contrast", 1.4), ("equalize", 0)],
    [("brightness", 1.3), ("contrast", 0.7), ("color", 1.6), ("equalize", 0)],
    [("color", 0.4), ("contrast", 1.8), ("brightness", 0.8), ("grayscale", 0)],
    [("brightness", 1.2), ("contrast", 1.5), ("color", 0.3), ("equalize", 0), ("solarize", 140), ("posterize", 3), ("autocontrast", 0), ("invert", 0)],
    [("posterize", 2), ("autocontrast", 0), ("contrast", 0.5), ("equalize", 0), ("brightness", 2.0), ("contrast", 3.0), ("autocontrast", 0),
     ("equalize", 0)],
]


def main():
    vectors, seed = [], 100

    def add(kind, w, h, c, chain):
        nonlocal seed
        seed += 1
        img = photo_spec.gen_image(kind, w, h, c, seed)
        vectors.append(dict(kind=kind, w=w, h=h, c=c, seed=seed, chain=chain_json(chain), fnv=fnv1a64(pil_chain(img, chain).tobytes())))

    for c in (1, 3):
        for op in ALONE:  # each op alone, on noise and on a narrow histogram
            add("noise", 23, 17, c, [op])
            add("narrow", 40, 31, c, [op])
        for op in (("autocontrast", 0), ("equalize", 0), ("contrast", 1.5)):
            add("constant", 9, 7, c, [op])   # a constant image: left unchanged
            add("noise", 1, 1, c, [op])      # 1 x 1
            add("noise", 15, 16, c, [op])    # fewer than 255 pixels: equalize's step is 0
            add("ramp", 37, 5, c, [op])
        add("clip", 32, 16, c, [("equalize", 0)])  # 511 pixels of 10 and one of 200: the table entry 256, clipped
        for chain in CHAINS:
            add("noise", 40, 29, c, chain)
            add("narrow", 33, 40, c, chain)
            add("ramp", 29, 3, c, chain)
    full = []
    for c, kind, w, h, chain in ((3, "noise", 3, 2, CHAINS[1]), (1, "noise", 4, 4, CHAINS[3]), (3, "ramp", 5, 1, [("equalize", 0)]),
                                 (1, "noise", 1, 1, [("contrast", 2.75)]), (3, "narrow", 4, 3, [("color", 2.75), ("autocontrast", 0)])):
        seed += 1
        img = photo_spec.gen_image(kind, w, h, c, seed)
        full.append(dict(w=w, h=h, c=c, chain=chain_json(chain), image=img.reshape(-1).tolist(), out=pil_chain(img, chain).reshape(-1).tolist()))
    doc = dict(about="PIL %s ImageEnhance / ImageOps on the seeded images of tests/photo_spec.py; written by tools/make_photo_golden.py" % PIL.__version__,
               vectors=vectors, full=full)
    path = os.path.join(ROOT, "tests", "golden", "photo_rule.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("%d vectors, %d in full -> %s" % (len(vectors), len(full), path))


if __name__ == "__main__":
    main()
