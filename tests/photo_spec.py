"""The rule of the photometric chains (include/llcomp_mi.h: "Photometric chains") restated with numpy, independent of the library: what
llcomp_mi_photo_reference and the GPU's kernels have to give, byte for byte.  An image is [h, w, c] uint8 with c = 1 or 3; a chain a list
of (op, param), op a name of CODES or its code.  The pointwise family is PIL's ImageEnhance / ImageOps.  GAUSSIAN_BLUR is PIL's
ImageFilter.GaussianBlur -- three box passes along the rows, then three along the columns, in wrapping 32-bit integers.  ADJUST_HUE is
torchvision's adjust_hue on the PIL backend -- PIL's RGB -> HSV, a wrapping byte add on H, HSV -> RGB.  ADJUST_SHARPNESS is PIL's
ImageEnhance.Sharpness(view).enhance(a) = Image.blend(view.filter(ImageFilter.SMOOTH), view, a), torchvision's adjust_sharpness on the
PIL backend: SMOOTH in integers -- the outermost rows and columns copied, an interior sample (S + 6) // 13 with S the sum of its 3 x 3
window plus four times the sample -- then the blend; smooth_float() is PIL's own float form, kept beside it to show the two agree."""
import numpy as np

# the one table of names and codes (the enum keeps its gaps)
CODES = dict(brightness=0, contrast=1, color=2, grayscale=3, invert=4, solarize=5, posterize=6, autocontrast=7, equalize=8,
             gaussian_blur=16, adjust_hue=17, adjust_sharpness=19)
NAMES = tuple(CODES)[:9]  # the pointwise family, whose codes are their places
AREA_NAMES = tuple(CODES)[9:11]  # the blur and the hue
F = np.float32
M32 = 0xFFFFFFFF


def name_of(op):
    return op if isinstance(op, str) else {code: name for name, code in CODES.items()}[int(op)]


def luma(img):
    """PIL's L of every pixel, [h, w] int64"""
    if img.shape[2] == 1:
        return img[..., 0].astype(np.int64)
    r, g, b = (img[..., i].astype(np.int64) for i in range(3))
    return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16


def blend(d, v, a):
    """PIL's ImagingBlend in binary32, every operation rounded by itself: d the degenerate image's samples, v the image's"""
    a = np.float32(a)
    d = np.asarray(d, np.int64)
    diff = (np.asarray(v, np.int64) - d).astype(np.float32)
    t = d.astype(np.float32) + a * diff
    assert t.dtype == np.float32
    if 0 <= a <= 1:
        return np.trunc(t).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def autocontrast_lut(h):
    lut = np.arange(256)
    present = np.nonzero(h)[0]
    if present.size == 0 or present[-1] <= present[0]:
        return lut
    lo, hi = int(present[0]), int(present[-1])
    s = 255.0 / (hi - lo)  # (Python floats: binary64)
    o = -lo * s
    return np.array([min(max(int(i * s + o), 0), 255) for i in range(256)])


def equalize_lut(h):
    lut = list(range(256))
    present = [i for i in range(256) if h[i]]
    if len(present) < 2:
        return np.array(lut)
    step = (int(h.sum()) - int(h[present[-1]])) // 255
    if step == 0:
        return np.array(lut)
    acc = step // 2
    for i in range(256):
        lut[i] = min(255, acc // step)
        acc += int(h[i])
    return np.array(lut)


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


def smooth(img):
    """ImageFilter.SMOOTH of [h, w, c] uint8, in integers"""
    h, w = img.shape[:2]
    out = img.copy()
    if h < 3 or w < 3:
        return out
    v = img.astype(np.int64)
    s = sum(v[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) + 4 * v[1:-1, 1:-1]
    out[1:-1, 1:-1] = (s + 6) // 13
    return out


def smooth_float(img):
    """the same as PIL computes it: nine binary32 products of (1 1 1 / 1 5 1 / 1 1 1) / 13 summed onto 0.5 row by row, then truncated"""
    h, w = img.shape[:2]
    out = img.copy()
    if h < 3 or w < 3:
        return out
    F = np.float32
    k = (np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], np.float64) / 13.0).astype(F)  # (PIL divides the kernel by the scale in float)
    v = img.astype(F)
    acc = np.full(v[1:-1, 1:-1].shape, F(0.5), F)
    # PIL flips the kernel's rows (the last kernel row meets the row above); it is symmetric, so only the order of the sum is its
    for j, dy in enumerate((1, 0, -1)):
        for i, dx in enumerate((-1, 0, 1)):
            acc = acc + v[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx] * k[3 * j + i]
    assert acc.dtype == F
    out[1:-1, 1:-1] = np.clip(acc.astype(np.int64), 0, 255)
    return out


def adjust_sharpness(img, factor):
    return blend(smooth(img), img, factor).astype(np.uint8)


def checker(w, h, c, seed):
    """black and white squares of side 1 + seed % 3: the smooth value and the clamps of the blend reach 0 and 255"""
    side = 1 + seed % 3
    y, x = np.mgrid[0:h, 0:w]
    a = ((((x // side) + (y // side) + seed) & 1) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(a[..., None], c, axis=2))


def apply_op(img, op, param=0.0):
    op = name_of(op)
    c = img.shape[2]
    if op == "brightness":
        return blend(np.zeros_like(img), img, param)
    if op == "contrast":
        n = img.shape[0] * img.shape[1]
        m = int(float(int(luma(img).sum())) / float(n) + 0.5)
        return blend(np.full(img.shape, m), img, param)
    if op == "color":
        return img.copy() if c == 1 else blend(np.repeat(luma(img)[..., None], 3, axis=2), img, param)
    if op == "grayscale":
        return img.copy() if c == 1 else np.repeat(luma(img)[..., None], 3, axis=2).astype(np.uint8)
    if op == "invert":
        return (255 - img.astype(np.int64)).astype(np.uint8)
    if op == "solarize":
        t = int(param)
        return np.where(img < t, img, 255 - img.astype(np.int64)).astype(np.uint8)
    if op == "posterize":
        return (img & np.uint8(~((1 << (8 - int(param))) - 1) & 0xFF)).astype(np.uint8)
    if op in ("autocontrast", "equalize"):
        out = np.empty_like(img)
        for ch in range(c):
            h = np.bincount(img[..., ch].reshape(-1), minlength=256)
            lut = autocontrast_lut(h) if op == "autocontrast" else equalize_lut(h)
            out[..., ch] = lut[img[..., ch]]
        return out
    if op == "gaussian_blur":
        return gaussian_blur(img, param)
    if op == "adjust_hue":
        return adjust_hue(img, param)
    if op == "adjust_sharpness":
        return adjust_sharpness(img, param)
    raise ValueError(op)


def apply(img, ops):
    """the chain on one image"""
    out = np.ascontiguousarray(img, dtype=np.uint8)
    if out.ndim == 2:
        return apply(out[..., None], ops)[..., 0]
    for o in ops:
        o = (o,) if isinstance(o, (str, int)) else tuple(o)
        out = apply_op(out, o[0], float(np.float32(o[1])) if len(o) > 1 and o[1] is not None else 0.0)
    return out


# ---- the seeded images the golden vectors name (tools/make_photo*_golden.py) ---------------------------------------------------------
def gen_image(kind, w, h, c, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == "narrow":  # a narrow Gaussian around a seeded level
        return np.clip(np.rint(rng.normal(40 + seed % 170, 5.0, (h, w, c))), 0, 255).astype(np.uint8)
    if kind == "constant":
        return np.full((h, w, c), (37 * seed + 11) % 256, np.uint8) + np.arange(c, dtype=np.uint8) * (seed % 2)
    if kind == "ramp":
        x = (np.arange(w) * 255 // max(w - 1, 1)).astype(np.uint8)
        return np.ascontiguousarray(np.broadcast_to(x[None, :, None], (h, w, c))) ^ np.uint8(seed % 4)
    if kind == "clip":  # equalize's clipped table entry: 511 pixels of value 10 and one of value 200 give lut[200] = 256
        img = np.full((h * w,), 10, np.uint8)
        img[w * h // 2] = 200
        return np.ascontiguousarray(np.repeat(img.reshape(h, w, 1), c, axis=2))
    if kind == "checker":
        return checker(w, h, c, seed)
    raise ValueError(kind)
