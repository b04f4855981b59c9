"""ADJUST_SHARPNESS of the photometric chains (include/llcomp_mi.h: "Photometric chains") restated with numpy, independent of the library:
PIL's ImageEnhance.Sharpness(view).enhance(a) = Image.blend(view.filter(ImageFilter.SMOOTH), view, a), which is torchvision's
adjust_sharpness on the PIL backend.  SMOOTH in integers -- the outermost rows and columns copied, an interior sample
(S + 6) // 13 with S the sum of its 3 x 3 window plus four times the sample -- then photo_spec's blend.  smooth_float() is PIL's own
float form, kept beside it to show the two agree.  apply() extends photo_area_spec.apply, so that a chain mixing every op has one spec."""
import numpy as np

import photo_area_spec
import photo_spec

ADJUST_SHARPNESS = 19
NAME = "adjust_sharpness"


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
    return photo_spec.blend(smooth(img), img, factor).astype(np.uint8)


def checker(w, h, c, seed):
    """black and white squares of side 1 + seed % 3: the smooth value and the clamps of the blend reach 0 and 255"""
    side = 1 + seed % 3
    y, x = np.mgrid[0:h, 0:w]
    a = ((((x // side) + (y // side) + seed) & 1) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(a[..., None], c, axis=2))


def gen_image(kind, w, h, c, seed):
    return checker(w, h, c, seed) if kind == "checker" else photo_spec.gen_image(kind, w, h, c, seed)


def is_sharpness(op):
    return op.lower() == NAME if isinstance(op, str) else int(op) == ADJUST_SHARPNESS


def apply(img, ops):
    """the chain on one image: photo_area_spec.apply with the op above"""
    out = np.ascontiguousarray(img, dtype=np.uint8)
    if out.ndim == 2:
        return apply(out[..., None], ops)[..., 0]
    for o in ops:
        o = (o,) if isinstance(o, (str, int)) else tuple(o)
        if not is_sharpness(o[0]):
            out = photo_area_spec.apply(out, [o])
            continue
        out = adjust_sharpness(out, float(np.float32(o[1])) if len(o) > 1 and o[1] is not None else 0.0)
    return out
