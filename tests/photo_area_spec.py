"""The two photometric ops that are not pointwise tables or blends (include/llcomp_mi.h: "Photometric chains", GAUSSIAN_BLUR and
ADJUST_HUE) restated with numpy, independent of the library: PIL's ImageFilter.GaussianBlur -- three box passes along the rows, then
three along the columns, in wrapping 32-bit integers -- and torchvision's adjust_hue on the PIL backend -- PIL's RGB -> HSV, a wrapping
byte add on H, HSV -> RGB.  apply() extends photo_spec.apply, so that a chain mixing the old and the new ops has one spec."""
import numpy as np

import photo_spec

GAUSSIAN_BLUR, ADJUST_HUE = 16, 17
AREA_NAMES = {"gaussian_blur": GAUSSIAN_BLUR, "adjust_hue": ADJUST_HUE}
F = np.float32
M32 = 0xFFFFFFFF


def blur_weights(radius):
    """(fr, r, ww, fw) of ImageFilter.GaussianBlur(radius) with three passes: every operation rounded to binary32 but the square root"""
    radius = F(radius)
    s2 = radius * radius / F(3)
    big_l = F(np.sqrt(np.float64(F(12) * s2 + F(1))))
    lo = np.floor((big_l - F(1)) / F(2))
    a = ((F(2) * lo + F(1)) * (lo * (lo + F(1)) - F(3) * s2)) / (F(6) * (s2 - (lo + F(1)) * (lo + F(1))))
    fr = lo + a
    assert all(isinstance(v, np.float32) for v in (s2, big_l, lo, a, fr))
    r = int(fr)
    ww = int(F(1 << 24) / (fr * F(2) + F(1))) & M32
    fw = (((1 << 24) - (2 * r + 1) * ww) & M32) // 2
    return fr, r, ww, fw


def line_pass(a, r, ww, fw):
    """one box pass along axis 0 of a uint8 array, the line's ends replicated"""
    n = a.shape[0]
    idx = np.clip(np.arange(-r - 1, n + r + 1), 0, n - 1)
    p = a[idx].astype(np.int64)  # p[j] = in[cl(j - r - 1)]
    cs = np.concatenate([np.zeros((1,) + p.shape[1:], np.int64), np.cumsum(p, axis=0)])
    acc = cs[2 * r + 2:2 * r + 2 + n] - cs[1:1 + n]  # in[cl(x - r)] .. in[cl(x + r)]
    far = p[0:n] + p[2 * r + 2:2 * r + 2 + n]
    return ((((acc * ww) & M32) + ((far * fw) & M32) + (1 << 23)) & M32) >> 24


def gaussian_blur(img, radius):
    fr, r, ww, fw = blur_weights(radius)
    out = img
    for _ in range(3):  # along every row: axis 1
        out = np.swapaxes(line_pass(np.swapaxes(out, 0, 1), r, ww, fw).astype(np.uint8), 0, 1)
    for _ in range(3):
        out = line_pass(out, r, ww, fw).astype(np.uint8)
    return np.ascontiguousarray(out)


def clip8(v):
    return np.clip(v, 0, 255)


def rgb2hsv(rgb):
    """PIL's convert("HSV") of [..., 3] uint8"""
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    gray = mx == mn
    cr = np.where(gray, 1, mx - mn).astype(F)
    s = cr / np.where(gray, 1, mx).astype(F)
    rc, gc, bc = ((mx - v).astype(F) / cr for v in (r, g, b))
    assert s.dtype == F and rc.dtype == F
    d = np.float64
    h = np.where(r == mx, bc.astype(d) - gc.astype(d),
                 np.where(g == mx, (2.0 + rc.astype(d)) - bc.astype(d), (4.0 + gc.astype(d)) - rc.astype(d))).astype(F)
    h = np.fmod(h.astype(d) / 6.0 + 1.0, 1.0).astype(F)
    hh = clip8((h.astype(d) * 255.0).astype(np.int64))
    ss = clip8((s.astype(d) * 255.0).astype(np.int64))
    return np.stack([np.where(gray, 0, hh), np.where(gray, 0, ss), mx], axis=-1).astype(np.uint8)


def c_round(x):
    """C's round: halves away from zero"""
    return np.where(x >= 0, np.floor(np.abs(x) + 0.5), -np.floor(np.abs(x) + 0.5))


def hsv2rgb(hsv):
    """PIL's convert("RGB") of [..., 3] uint8 HSV"""
    d = np.float64
    h8, s8, v8 = (hsv[..., i] for i in range(3))
    hh = h8.astype(F).astype(d) * 6.0 / 255.0
    i = np.floor(hh)
    f = (hh - i.astype(F).astype(d)).astype(F)
    fs = (s8.astype(F).astype(d) / 255.0).astype(F)
    v = v8.astype(d)
    fd, fsd = f.astype(d), fs.astype(d)
    p = clip8(c_round(v * (1.0 - fsd))).astype(np.uint8)
    q = clip8(c_round(v * (1.0 - fsd * fd))).astype(np.uint8)
    t = clip8(c_round(v * (1.0 - fsd * (1.0 - fd)))).astype(np.uint8)
    sel = i.astype(np.int64) % 6
    table = [(v8, t, p), (q, v8, p), (p, v8, t), (p, q, v8), (t, p, v8), (v8, p, q)]
    out = np.empty(hsv.shape, np.uint8)
    for ch in range(3):
        out[..., ch] = np.where(s8 == 0, v8, np.choose(sel, [table[k][ch] for k in range(6)]))
    return out


def hue_shift(factor):
    """the byte added to H: (uint8)(int32)((double)(float)factor * 255.0), truncated toward zero"""
    return int(np.float64(F(factor)) * 255.0) & 0xFF


def adjust_hue(img, factor):
    if img.shape[2] == 1:
        return img.copy()
    hsv = rgb2hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int64) + hue_shift(factor)) & 0xFF
    return hsv2rgb(hsv)


def code_of(op):
    if isinstance(op, str):
        return AREA_NAMES.get(op)
    return int(op) if int(op) in (GAUSSIAN_BLUR, ADJUST_HUE) else None


def apply(img, ops):
    """the chain on one image: photo_spec.apply with the two ops above"""
    out = np.ascontiguousarray(img, dtype=np.uint8)
    if out.ndim == 2:
        return apply(out[..., None], ops)[..., 0]
    for o in ops:
        o = (o,) if isinstance(o, (str, int)) else tuple(o)
        code = code_of(o[0])
        if code is None:
            out = photo_spec.apply(out, [o])
            continue
        param = float(np.float32(o[1])) if len(o) > 1 and o[1] is not None else 0.0
        out = gaussian_blur(out, param) if code == GAUSSIAN_BLUR else adjust_hue(out, param)
    return out
