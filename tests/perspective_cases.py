"""What the perspective tests share (test_perspective_rule.py, test_perspective_plan.py, test_gpu_perspective_views.py): PIL's
Image.transform(PERSPECTIVE) on band images, and seeded families of maps."""
import numpy as np

FILTERS = ("nearest", "bilinear", "bicubic")


def pil_perspective(Image, img, a, name, ow, oh, fill):
    """Image.transform on an image of 1 (L), 3 (RGB) or 4 (CMYK) independent bands; any other count band by band, as L images"""
    res = {"nearest": Image.NEAREST, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[name]
    h, w, c = img.shape
    if c not in (1, 3, 4):
        return np.stack([pil_perspective(Image, img[..., ch:ch + 1], a, name, ow, oh, fill[ch:ch + 1])[..., 0] for ch in range(c)], axis=-1)
    im = Image.frombytes({1: "L", 3: "RGB", 4: "CMYK"}[c], (w, h), np.ascontiguousarray(img).tobytes())
    fc = int(fill[0]) if c == 1 else tuple(int(v) for v in fill)
    return np.asarray(im.transform((ow, oh), Image.PERSPECTIVE, tuple(float(t) for t in a), res, fillcolor=fc)).reshape(oh, ow, c)


def keystone(mi, rng, w, h, ow, oh, spread=0.25, shift=0.0):
    """the map that sends the output's corners to the image's corners, each moved by up to `spread` of a side (so part of the output
    falls outside the image) and all of them by `shift` sides"""
    sp = np.array([[0, 0], [w, 0], [w, h], [0, h]], float) + rng.uniform(-spread, spread, (4, 2)) * [w, h] + np.asarray(shift, float) * [w, h]
    return mi.perspective_coeffs(sp, [[0, 0], [ow, 0], [ow, oh], [0, oh]])


def coords(a, ow, oh):
    """the rule's (den, xin, yin) of every output pixel, [oh][ow] each, in binary64 with every operation rounded by itself (numpy)"""
    a = [np.float64(t) for t in a]
    xs, ys = np.meshgrid(np.arange(ow, dtype=np.float64) + 0.5, np.arange(oh, dtype=np.float64) + 0.5)
    den = (a[6] * xs + a[7] * ys) + 1.0
    return den, ((a[0] * xs + a[1] * ys) + a[2]) / den, ((a[3] * xs + a[4] * ys) + a[5]) / den
