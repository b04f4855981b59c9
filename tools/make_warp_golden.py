#!/usr/bin/env python3
"""Writes tests/golden/warp_rule.json: images, affine matrices and what PIL's Image.transform(AFFINE) gives for them under NEAREST,
BILINEAR and BICUBIC -- so that a machine without PIL still checks the rule of the warped views (include/llcomp_mi.h) bit for bit
(tests/test_warp_rule.py).  Needs Pillow and numpy; run once, by hand:  python tools/make_warp_golden.py

The last vector is chosen so that evaluating the rule with fused multiply-adds changes an output byte.  It is a vertical translate of
a two-row step under BILINEAR, v = a + (b - a) * dy at output pixel (0, 0): the search below walks (a, b, k) and the doubles next to
dy = (a - k) / (a - b), evaluates v with every operation rounded by itself (Python's floats) and with the product and the sum rounded
once (exact rationals), and keeps the first case where truncation gives k one way and k - 1 the other.  Both outputs are recorded;
PIL gives the unfused one."""
import json
import math
import os
from fractions import Fraction

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = {"nearest": Image.NEAREST, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}


def pil_warp(img, m, name, ow, oh, fill):
    if img.ndim == 2 or img.shape[2] in (1, 3):
        a = img[..., 0] if img.ndim == 3 and img.shape[2] == 1 else img
        fc = int(fill[0]) if a.ndim == 2 else tuple(int(v) for v in fill)
        out = np.asarray(Image.fromarray(a).transform((ow, oh), Image.AFFINE, tuple(m), FILTERS[name], fillcolor=fc))
        return out.reshape(oh, ow, -1)
    # any other channel count: band by band, as the library treats every channel
    return np.stack([pil_warp(img[..., ch:ch + 1], m, name, ow, oh, fill[ch:ch + 1])[..., 0] for ch in range(img.shape[2])], axis=-1)


def fma(a, b, c):
    """a * b + c rounded once"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def bilinear_model(img, m, ow, oh, fused):
    """the header's BILINEAR rule on a one-channel image with zero fill, every a * b + c of it fused or not"""
    h, w = img.shape[:2]
    P = img.reshape(h, w).astype(float)
    mad = fma if fused else (lambda a, b, c: a * b + c)
    cl = lambda t, n: min(max(t, 0), n - 1)
    out = np.zeros((oh, ow, 1), np.uint8)
    for y in range(oh):
        for x in range(ow):
            xs, ys = x + 0.5, y + 0.5
            xin, yin = mad(m[0], xs, m[1] * ys) + m[2], mad(m[3], xs, m[4] * ys) + m[5]
            if not (0 <= xin < w and 0 <= yin < h):
                continue
            xin, yin = xin - 0.5, yin - 0.5
            X, Y = math.floor(xin), math.floor(yin)
            dx, dy = xin - X, yin - Y
            row = lambda r: mad(P[r][cl(X + 1, w)] - P[r][cl(X, w)], dx, P[r][cl(X, w)])
            v1 = row(cl(Y, h))
            v2 = row(Y + 1) if 0 <= Y + 1 < h else v1
            out[y, x, 0] = int(mad(v2 - v1, dy, v1))
    return out


def find_contraction_vector():
    for a in range(255, 1, -1):
        for b in range(0, a - 1):
            for k in range(b + 1, a):
                t = (a - k) / (a - b)
                for dy0 in (math.nextafter(t, 0.0), t, math.nextafter(t, 1.0)):
                    if not 0.0 < dy0 < 1.0:
                        continue
                    yin = (0.0 * 0.5 + 1.0 * 0.5) + dy0  # m3 = 0, m4 = 1, m5 = dy0 at output row 0
                    dy = (yin - 0.5) - math.floor(yin - 0.5)
                    if math.floor(yin - 0.5) != 0:
                        continue
                    unfused = int(a + (b - a) * dy)
                    fused = int(float(Fraction(a) + Fraction(b - a) * Fraction(dy)))
                    if unfused != fused:
                        return a, b, dy0, unfused, fused
    raise SystemExit("no contraction-sensitive vector found")


def main():
    rng = np.random.default_rng(20261019)
    vectors = []
    shapes = [(7, 5, 1), (9, 6, 3), (1, 1, 3), (1, 8, 1), (12, 9, 3), (5, 11, 4), (10, 7, 3), (6, 6, 2)]
    for i, (w, h, c) in enumerate(shapes):
        img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        ow, oh = int(rng.integers(1, 11)), int(rng.integers(1, 11))
        ang, sc, sh = rng.uniform(0, 2 * math.pi), rng.uniform(0.5, 2.0), rng.uniform(-0.5, 0.5)
        m = [sc * math.cos(ang), sc * (math.sin(ang) + sh), rng.uniform(-2, w / 2), -sc * math.sin(ang), sc * math.cos(ang), rng.uniform(-2, h / 2)]
        if i == 4:
            m[1] = m[3] = 0.0  # a pure scale: NEAREST's table form
        if i == 6:
            m = [1.0, 0.0, 2.0, 0.0, 1.0, -1.0]  # an integer translate
        fill = [int(v) for v in rng.integers(0, 256, c)]
        vec = dict(w=w, h=h, c=c, ow=ow, oh=oh, m=[float(v).hex() for v in m], fill=fill, image=img.reshape(-1).tolist())
        for name in FILTERS:
            vec[name] = pil_warp(img, m, name, ow, oh, np.array(fill)).reshape(-1).tolist()
        vectors.append(vec)
    a, b, dy0, unfused, fused = find_contraction_vector()
    img = np.array([[a, a, 9, 200], [b, b, 77, 3], [50, 60, 70, 80]], np.uint8).reshape(3, 4, 1)
    m = [1.0, 0.0, 0.0, 0.0, 1.0, dy0]
    out = pil_warp(img, m, "bilinear", 2, 2, np.array([0]))
    out_fused = bilinear_model(img, m, 2, 2, True)
    assert np.array_equal(out, bilinear_model(img, m, 2, 2, False)) and out[0, 0, 0] == unfused and out_fused[0, 0, 0] == fused != unfused
    vectors.append(dict(w=4, h=3, c=1, ow=2, oh=2, m=[float(v).hex() for v in m], fill=[0], image=img.reshape(-1).tolist(),
                        bilinear=out.reshape(-1).tolist(), bilinear_fused=out_fused.reshape(-1).tolist(), contraction_sensitive=True))
    path = os.path.join(ROOT, "tests", "golden", "warp_rule.json")
    with open(path, "w") as f:
        json.dump(dict(pillow=Image.__version__, vectors=vectors), f, separators=(",", ":"))
        f.write("\n")
    print(path, os.path.getsize(path), "bytes; contraction vector", (a, b, dy0.hex(), unfused, fused))


if __name__ == "__main__":
    main()
