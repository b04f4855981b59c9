"""The resampling rule of the resized calls for all six filters (include/llcomp_mi.h: llcomp_mi_resize_filter_weights), restated with
`math` alone and independent of the library: PIL's 8-bit resampler -- the filter's weights in double, normalised, rounded to Q22,
horizontal pass first, rounded and clamped to u8 in between -- and the centre-aligned nearest neighbour in exact integers."""
import math

import numpy as np

BILINEAR, NEAREST, BOX, HAMMING, BICUBIC, LANCZOS = range(6)
NAMES = ("bilinear", "nearest", "box", "hamming", "bicubic", "lanczos")
WEIGHTED = (BILINEAR, BOX, HAMMING, BICUBIC, LANCZOS)
RADIUS = {BILINEAR: 1.0, BOX: 0.5, HAMMING: 1.0, BICUBIC: 2.0, LANCZOS: 3.0}
REACH = {BILINEAR: 1, NEAREST: 1, BOX: 1, HAMMING: 1, BICUBIC: 2, LANCZOS: 3}  # R: R * in <= 64 * out


def _triangle(x):
    return max(0.0, 1.0 - abs(x))


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


KERNEL = {BILINEAR: _triangle, BOX: _box, HAMMING: _hamming, BICUBIC: _bicubic, LANCZOS: _lanczos}


def allowed(filt, in_len, out_len):
    return 0 <= filt < 6 and in_len > 0 and out_len > 0 and REACH[filt] * in_len <= 64 * out_len


def weights(filt, in_len, out_len):
    """(lo int64[out_len], q int64[out_len, K]): every output's first tap and its Q22 weights, zero-padded to the K of the axis -- the
    longest run up to an output's last non-zero weight"""
    if filt == NEAREST:
        lo = np.array([((2 * i + 1) * in_len) // (2 * out_len) for i in range(out_len)], np.int64)
        return lo, np.full((out_len, 1), 1 << 22, np.int64)
    f, scale = KERNEL[filt], in_len / out_len
    fs = max(scale, 1.0)
    support, ss = RADIUS[filt] * fs, 1.0 / fs
    los, runs = [], []
    for i in range(out_len):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_len)
        w = [f((lo + j - center + 0.5) * ss) for j in range(hi - lo)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        q = [int(v * (1 << 22) + 0.5) if v >= 0 else int(v * (1 << 22) - 0.5) for v in w]
        while q and q[-1] == 0:
            q.pop()
        los.append(lo)
        runs.append(q)
    k = max(1, max(len(r) for r in runs))
    out = np.zeros((out_len, k), np.int64)
    for i, r in enumerate(runs):
        out[i, :len(r)] = r
    return np.array(los, np.int64), out


def _axis(img, lo, q, axis):
    """one pass along `axis` (0 = rows of an [h, w, c] array, 1 = columns) with Q22 weights q[out, K] from lo[out]"""
    n_in = img.shape[axis]
    idx = np.minimum(lo[:, None] + np.arange(q.shape[1])[None, :], n_in - 1)  # (padded taps have weight 0)
    g = np.take(img.astype(np.int64), idx, axis=axis)  # axis 1: [h, out, K, c]; axis 0: [out, K, w, c]
    if axis == 1:
        acc = (g * q[None, :, :, None]).sum(axis=2)
    else:
        acc = (g * q[:, :, None, None]).sum(axis=1)
    return np.clip((acc + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def resize(img, ow, oh, filt, flip=False):
    """img [h, w, c] u8 -> [oh, ow, c] u8 by the rule: horizontal pass, u8, vertical pass, then the mirror"""
    h, w = img.shape[:2]
    lx, qx = weights(filt, w, ow)
    ly, qy = weights(filt, h, oh)
    out = _axis(_axis(img, lx, qx, 1), ly, qy, 0)
    return np.ascontiguousarray(out[:, ::-1]) if flip else out


def fnv1a64(data):
    h = 1469598103934665603
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h
