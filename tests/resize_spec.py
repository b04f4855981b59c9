"""The resampling rule of Codec.decode_resized_regions restated in numpy (include/llcomp_mi.h: llcomp_mi_resize_weights), for the tests:
the triangle filter with antialiasing in Q22 integers, horizontal pass first, rounded to u8 in between, then the optional mirror."""
import numpy as np


def ref_weights(in_len, out_len):
    """(lo[out_len], list of float64 weight arrays) of one axis, straight from the rule's text"""
    scale = in_len / out_len
    support = max(scale, 1.0)
    los, ws = [], []
    for i in range(out_len):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_len)
        w = np.array([max(0.0, 1.0 - abs((lo + j - center + 0.5) / support)) for j in range(hi - lo)], np.float64)
        los.append(lo)
        ws.append(w / w.sum())
    return np.array(los, np.int64), ws


def _axis(img, lo, q, axis):
    """one pass along `axis` (0 = rows of an [h, w, c] array, 1 = columns) with Q22 weights q[out, K] from lo[out]"""
    n_in = img.shape[axis]
    idx = np.minimum(lo.astype(np.int64)[:, None] + np.arange(q.shape[1])[None, :], n_in - 1)  # (padded taps have weight 0)
    g = np.take(img.astype(np.int64), idx, axis=axis)  # axis 1: [h, out, K, c]; axis 0: [out, K, w, c]
    if axis == 1:
        acc = (g * q.astype(np.int64)[None, :, :, None]).sum(axis=2)
    else:
        acc = (g * q.astype(np.int64)[:, :, None, None]).sum(axis=1)
    return np.clip((acc + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def resize(mi, img, ow, oh, flip=False):
    """img [h, w, c] u8 -> [oh, ow, c] u8 by the rule, with the library's weights (mi.resize_weights)"""
    h, w = img.shape[:2]
    lx, qx = mi.resize_weights(w, ow)
    ly, qy = mi.resize_weights(h, oh)
    out = _axis(_axis(img, lx, qx, 1), ly, qy, 0)
    return np.ascontiguousarray(out[:, ::-1]) if flip else out


def random_resized_crop(rng, w, h, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3)):
    """torchvision's RandomResizedCrop.get_params, on a numpy generator: (x, y, rw, rh)"""
    area = w * h
    log_ratio = (np.log(ratio[0]), np.log(ratio[1]))
    for _ in range(10):
        target = area * rng.uniform(scale[0], scale[1])
        ar = np.exp(rng.uniform(log_ratio[0], log_ratio[1]))
        rw = int(round(np.sqrt(target * ar)))
        rh = int(round(np.sqrt(target / ar)))
        if 0 < rw <= w and 0 < rh <= h:
            return int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1)), rw, rh
    in_ratio = w / h
    if in_ratio < ratio[0]:
        rw, rh = w, int(round(w / ratio[0]))
    elif in_ratio > ratio[1]:
        rh, rw = h, int(round(h * ratio[1]))
    else:
        rw, rh = w, h
    return (w - rw) // 2, (h - rh) // 2, rw, rh
