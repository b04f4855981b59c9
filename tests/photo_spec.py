"""The rule of the photometric chains (include/llcomp_mi.h: "Photometric chains") restated with numpy, independent of the library: what
llcomp_mi_photo_reference and the GPU's kernels have to give, byte for byte.  An image is [h, w, c] uint8 with c = 1 or 3; a chain a list
of (op, param), op a name of NAMES or its index."""
import numpy as np

NAMES = ("brightness", "contrast", "color", "grayscale", "invert", "solarize", "posterize", "autocontrast", "equalize")
STATS_OPS = ("contrast", "autocontrast", "equalize")


def name_of(op):
    return op if isinstance(op, str) else NAMES[int(op)]


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


# ---- the seeded images the golden vectors name (tools/make_photo_golden.py) ----------------------------------------------------------
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
    raise ValueError(kind)
