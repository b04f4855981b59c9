#!/usr/bin/env python3
"""Writes tests/golden/perspective_rule.json: images, perspective coefficients (as hex floats) and what PIL's
Image.transform(PERSPECTIVE) gives for them under NEAREST, BILINEAR and BICUBIC -- so that a machine without PIL still checks the rule of
the perspective views (include/llcomp_mi.h) bit for bit (tests/test_perspective_rule.py).  Needs Pillow, numpy and g++; run once, by
hand:  python tools/make_perspective_golden.py

Besides random keystones (c = 1 and 3) it holds maps with a strong a6 and a7, a view partly outside and one wholly outside the image,
and two special vectors:
  * `differs_from_affine`: a6 = a7 = 0 under NEAREST, where PIL's PERSPECTIVE (binary64 per pixel) and PIL's AFFINE (16.16 fixed
    point) disagree on the same six numbers; both outputs are recorded.
  * `contraction_sensitive`: found by tools/perspective_contraction_search.cpp (std::fma): a NEAREST view one pixel of which reads
    column k with every operation rounded by itself and column k - 1 once a0 xs + a1 ys or a6 xs + a7 ys is contracted into a fused
    multiply-add.  The image is a ramp along x, so the two give different bytes; PIL gives the unfused one, `nearest_fused` records the
    other (the model below, with exact rationals for the fused sums)."""
import json
import os
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = {"nearest": Image.NEAREST, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}


def pil_transform(img, method, data, name, ow, oh, fill):
    if img.shape[2] in (1, 3):
        a = img[..., 0] if img.shape[2] == 1 else img
        fc = int(fill[0]) if a.ndim == 2 else tuple(int(v) for v in fill)
        return np.asarray(Image.fromarray(a).transform((ow, oh), method, tuple(data), FILTERS[name], fillcolor=fc)).reshape(oh, ow, -1)
    return np.stack([pil_transform(img[..., ch:ch + 1], method, data, name, ow, oh, fill[ch:ch + 1])[..., 0] for ch in range(img.shape[2])], axis=-1)


def coeffs(sp, ep):
    """the eight numbers that send the output's ep to the source's sp (four (x, y) pairs each)"""
    A = np.zeros((8, 8))
    for i in range(4):
        (x, y), (u, v) = ep[i], sp[i]
        A[2 * i] = [x, y, 1, 0, 0, 0, -u * x, -u * y]
        A[2 * i + 1] = [0, 0, 0, x, y, 1, -v * x, -v * y]
    return [float(v) for v in np.linalg.solve(A, np.asarray(sp, float).reshape(8))]


def nearest_model(img, a, ow, oh, fill, fused):
    """the header's NEAREST rule on a one-channel image; fused: the two sums of products rounded once, as a fused multiply-add does"""
    h, w = img.shape[:2]
    mad = (lambda p, q, r: float(Fraction(p) * Fraction(q) + Fraction(r))) if fused else (lambda p, q, r: p * q + r)
    out = np.full((oh, ow, 1), fill, np.uint8)
    for y in range(oh):
        for x in range(ow):
            xs, ys = x + 0.5, y + 0.5
            den = mad(a[6], xs, a[7] * ys) + 1.0
            xin, yin = (mad(a[0], xs, a[1] * ys) + a[2]) / den, (mad(a[3], xs, a[4] * ys) + a[5]) / den
            xi, yi = (-1 if xin < 0 else int(xin)), (-1 if yin < 0 else int(yin))
            if 0 <= xi < w and 0 <= yi < h:
                out[y, x, 0] = img[yi, xi, 0]
    return out


def vector(img, a, ow, oh, fill, **extra):
    h, w, c = img.shape
    vec = dict(w=w, h=h, c=c, ow=ow, oh=oh, a=[float(v).hex() for v in a], fill=[int(v) for v in fill], image=img.reshape(-1).tolist())
    for name in FILTERS:
        vec[name] = pil_transform(img, Image.PERSPECTIVE, a, name, ow, oh, np.array(fill)).reshape(-1).tolist()
    vec.update(extra)
    return vec


def main():
    rng = np.random.default_rng(20261020)
    vectors = []
    # random keystones: the source quadrilateral is the image's corners moved by up to a quarter of a side (partly outside the image)
    for w, h, c, ow, oh in [(9, 7, 1, 6, 5), (12, 9, 3, 10, 8), (7, 11, 3, 5, 9), (16, 13, 1, 12, 10), (10, 10, 4, 7, 7), (1, 1, 3, 3, 2)]:
        img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        sp = np.array([[0, 0], [w, 0], [w, h], [0, h]], float) + rng.uniform(-0.25, 0.25, (4, 2)) * [w, h]
        a = coeffs(sp, [[0, 0], [ow, 0], [ow, oh], [0, oh]])
        vectors.append(vector(img, a, ow, oh, rng.integers(0, 256, c)))
    # a strong a6 and a7: the denominator runs from 1 to about 3.4 across the output
    img = rng.integers(0, 256, (11, 14, 3), dtype=np.uint8)
    vectors.append(vector(img, [2.5, 0.3, 0.2, -0.2, 2.2, 0.4, 0.14, 0.17], 9, 8, [7, 99, 201], strong=True))
    # the denominator falls towards 0.28: the far corner is magnified
    img = rng.integers(0, 256, (13, 10, 1), dtype=np.uint8)
    vectors.append(vector(img, [0.5, 0.05, 1.0, 0.02, 0.45, 2.0, -0.04, -0.05], 8, 8, [31], strong=True))
    # wholly outside: all fill
    img = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    v = vector(img, [1.0, 0.1, 30.0, 0.05, 1.0, -40.0, 0.01, 0.02], 5, 4, [1, 2, 3], wholly_outside=True)
    assert all(v[n] == [1, 2, 3] * 20 for n in FILTERS)
    vectors.append(v)
    # a6 = a7 = 0 under NEAREST: not the affine call's 16.16 path
    for _ in range(10000):
        img = rng.integers(0, 256, (17, 19, 1), dtype=np.uint8)
        ang, sc = rng.uniform(0, 6.28), rng.uniform(0.6, 1.5)
        a = [sc * np.cos(ang), sc * np.sin(ang), rng.uniform(0, 9), -sc * np.sin(ang), sc * np.cos(ang), rng.uniform(0, 9), 0.0, 0.0]
        a = [float(t) for t in a]
        persp = pil_transform(img, Image.PERSPECTIVE, a, "nearest", 16, 16, np.array([0]))
        affine = pil_transform(img, Image.AFFINE, a[:6], "nearest", 16, 16, np.array([0]))
        if not np.array_equal(persp, affine):
            vectors.append(vector(img, a, 16, 16, [0], differs_from_affine=True, affine_nearest=affine.reshape(-1).tolist()))
            break
    else:
        raise SystemExit("no a6 = a7 = 0 vector that differs from the affine path")
    # the contraction-sensitive vector
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "search")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "perspective_contraction_search.cpp")])
        words = subprocess.check_output([exe], text=True).split()
    a = [float.fromhex(t) for t in words[:8]]
    px, py, col, col_fused = (int(t) for t in words[8:])
    img = np.tile((np.arange(12) * 20 + 5).astype(np.uint8), (9, 1)).reshape(9, 12, 1)  # a ramp along x: column k holds 20 k + 5
    v = vector(img, a, 8, 8, [0], contraction_sensitive=True, pixel=[px, py])
    unfused, fused = nearest_model(img, a, 8, 8, 0, False), nearest_model(img, a, 8, 8, 0, True)
    assert v["nearest"] == unfused.reshape(-1).tolist(), "PIL is not the unfused rule"
    assert unfused[py, px, 0] == 20 * col + 5 and fused[py, px, 0] == 20 * col_fused + 5 and col != col_fused
    v["nearest_fused"] = fused.reshape(-1).tolist()
    vectors.append(v)
    path = os.path.join(ROOT, "tests", "golden", "perspective_rule.json")
    with open(path, "w") as f:
        json.dump(dict(pillow=Image.__version__, vectors=vectors), f, separators=(",", ":"))
        f.write("\n")
    print(path, os.path.getsize(path), "bytes;", len(vectors), "vectors; contraction pixel", (px, py), "columns", (col, col_fused))


if __name__ == "__main__":
    main()
