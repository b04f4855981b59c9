"""The folded rule of the padded calls (include/llcomp_mi.h: llcomp_mi_pad, llcomp_mi_pad_axis, llcomp_mi_padded_filter_weights) against
np.pad and the resampling rule restated in tests/resize_filters_spec.py: "pad, then crop, then resample" must equal the folded weights
applied to the source interval alone, plus bias * fill.  Host only: no GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_filters_spec as spec  # noqa: E402

MODES = ("constant", "edge", "reflect", "symmetric")


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


def limit(mode, n):
    return n - 1 if mode == "reflect" else n


def index_map(mode, n, t):
    """m(t) as the header's table states it; None for a padded index of "constant" """
    if 0 <= t < n:
        return t
    if mode == "constant":
        return None
    if mode == "edge":
        return 0 if t < 0 else n - 1
    if mode == "reflect":
        return -t if t < 0 else 2 * (n - 1) - t
    return -t - 1 if t < 0 else 2 * n - 1 - t


def cases(mode, filt, count, seed):
    """seeded (n, x, r, out): pads of 0 and of the mode's limit on either side included, r -> out within the filter's limit"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        n = int(rng.integers(1, 41))
        lim = limit(mode, n)
        kind = len(out) % 6
        p = [0, lim, int(rng.integers(0, lim + 1)), 0, lim, int(rng.integers(0, lim + 1))][kind]
        e = [0, int(rng.integers(0, lim + 1)), lim, lim, lim, int(rng.integers(0, lim + 1))][kind]
        if p:
            x = -p
            hi = n + e if e else int(rng.integers(1, n + 1))  # (the end: past the image by e, or inside it)
        else:
            x = int(rng.integers(0, n))
            hi = n + e if e else int(rng.integers(x + 1, n + 1))
        r = hi - x
        o = int(rng.integers(1, 2 * r + 2))
        if not spec.allowed(filt, r, o):
            o = r
        out.append((n, x, r, o))
    return out


def apply(lo, q, src):
    k = q.shape[1]
    idx = lo[:, None].astype(np.int64) + np.arange(k)[None, :]
    assert idx.max() < len(src) or not q[idx >= len(src)].any()
    return (q.astype(np.int64) * src[np.minimum(idx, len(src) - 1)]).sum(axis=1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("filt", range(6))
def test_folded_weights_equal_pad_then_resample(mi, mode, filt):
    """300 seeded axes per mode and filter: the folded accumulator equals the unfolded one on the np.pad-ed axis, for a random source
    and a random fill; pad_axis is the min and max of m over the rectangle; lo' + K' <= s_len; the bias is 0 outside "constant" """
    rng = np.random.default_rng(1000 * filt + MODES.index(mode))
    for n, x, r, out in cases(mode, filt, 300, 77 + filt):
        s0, s_len = mi.pad_axis(mode, n, x, r)
        ms = [index_map(mode, n, t) for t in range(x, x + r)]
        inside = [m for m in ms if m is not None]
        assert (s0, s_len) == (min(inside), max(inside) - min(inside) + 1), (mode, n, x, r)
        assert set(inside) == set(range(s0, s0 + s_len)), "the source indices are one interval"
        g0, lo, q, bias = mi.padded_weights(filt, mode, n, x, r, out)
        assert g0 == s0 and lo.shape == (out,) and q.shape[0] == out and bias.shape == (out,)
        kp = q.shape[1]
        assert kp >= 1 and (lo.astype(np.int64) + kp <= s_len).all(), (mode, filt, n, x, r, out)
        ulo, uq = spec.weights(filt, r, out)
        assert kp <= uq.shape[1]
        assert mode == "constant" or not bias.any()
        # pad, crop, resample: np.pad with the mode's name (constant: the fill pasted around), the rectangle, the unfolded weights
        img = rng.integers(0, 256, n).astype(np.int64)
        fill = int(rng.integers(0, 256))
        p, e = max(-x, 0), max(x + r - n, 0)
        padded = np.pad(img, (p, e), mode=mode, **({"constant_values": fill} if mode == "constant" else {}))
        crop = padded[x + p:x + p + r]
        want = apply(ulo, uq, crop)
        got = apply(lo, q, img[s0:s0 + s_len]) + bias.astype(np.int64) * fill
        assert np.array_equal(got, want), (mode, filt, n, x, r, out)
        assert (np.abs(q.astype(np.int64)).sum(axis=1) + np.abs(bias.astype(np.int64)) <= np.abs(uq).sum(axis=1)).all()


@pytest.mark.parametrize("mode", MODES)
def test_inside_rectangle_is_the_unpadded_rule(mi, mode):
    """a rectangle inside the image: s0 = x, no bias, and the unpadded lo and q -- every run moved left until lo + K <= r, as the
    kernels' tables have always placed it"""
    rng = np.random.default_rng(5)
    for filt in range(6):
        for _ in range(40):
            n = int(rng.integers(1, 60))
            x = int(rng.integers(0, n))
            r = int(rng.integers(1, n - x + 1))
            out = int(rng.integers(1, 2 * r + 2))
            if not spec.allowed(filt, r, out):
                out = r
            s0, lo, q, bias = mi.padded_weights(filt, mode, n, x, r, out)
            ulo, uq = mi.resize_weights(r, out, filt)
            k = uq.shape[1]
            assert s0 == x and not bias.any() and q.shape == uq.shape
            a = np.minimum(ulo.astype(np.int64), r - k)
            placed = np.zeros_like(uq)
            for i in range(out):
                s = int(ulo[i] - a[i])
                placed[i, s:] = uq[i, :k - s]
                assert not uq[i, k - s:].any()
            assert np.array_equal(lo, a) and np.array_equal(q, placed)
            assert np.array_equal(s0 + lo.astype(np.int64), x + a)


def test_refusals(mi):
    """every refusal of the rule: an unknown mode, a side of 0, no image pixel, a pad above the mode's limit, what the unpadded weights
    refuse (an unknown filter, a downscale above the filter's limit, checked on r -> out)"""
    bad = mi.BAD_ARGS

    def refused(f, *a):
        with pytest.raises(mi.LlcompError) as e:
            f(*a)
        assert e.value.status == bad

    for mode in MODES:
        n = 10
        lim = limit(mode, n)
        assert mi.pad_axis(mode, n, -lim, lim + 1) == (0, 1 if mode in ("constant", "edge") else n)  # (the limit itself)
        assert mi.pad_axis(mode, n, n - 1, lim + 1)[1] >= 1
        refused(mi.pad_axis, mode, n, -lim - 1, lim + 2)      # left pad above the limit
        refused(mi.pad_axis, mode, n, n - 1, lim + 2)         # right pad above the limit
        refused(mi.pad_axis, mode, n, n, 1)                   # starts at the right edge: no image pixel
        refused(mi.pad_axis, mode, n, -3, 3)                  # ends at the left edge
        refused(mi.pad_axis, mode, n, 0, 0)
        refused(mi.pad_axis, mode, 0, 0, 1)
        refused(mi.padded_weights, 0, mode, n, -lim - 1, lim + 2, 4)
        refused(mi.padded_weights, 6, mode, n, -1, 4, 4)      # an unknown filter
        refused(mi.padded_weights, 0, mode, n, -1, 4, 0)
        refused(mi.padded_weights, 5, mode, 100, -50, 200, 9)  # Lanczos: 3 * 200 > 64 * 9, although the source interval is 100
        refused(mi.padded_regions_plan, 10, 10, [(0, 0, 0, 4)], mode)
        refused(mi.padded_regions_plan, 10, 10, [(0, 0, 4, 4), (10, 0, 4, 4)], mode)
        refused(mi.padded_regions_plan, 10, 10, [(0, -lim - 1, 4, lim + 2)], mode)
        assert mi.padded_weights(5, mode, 100, -50, 200, 10)[0] == 0
    refused(mi.pad_axis, 4, 10, 0, 5)
    refused(mi.pad_axis, "wrap", 10, 0, 5)
    refused(mi.padded_weights, 0, 4, 10, 0, 5, 5)
    L = mi._lib.load()
    import ctypes as C

    rects = (C.c_int32 * 4)(-1, -1, 4, 4)
    src = (C.c_uint32 * 4)(9, 9, 9, 9)
    small = mi._lib.Pad(C.sizeof(mi._lib.Pad) - 1, 1, None)
    assert L.llcomp_mi_padded_regions_plan(10, 10, rects, 1, None, src) == bad
    assert L.llcomp_mi_padded_regions_plan(10, 10, rects, 1, C.byref(small), src) == bad
    assert L.llcomp_mi_padded_regions_plan(10, 10, rects, 1, C.byref(mi._lib.Pad(C.sizeof(mi._lib.Pad), 4, None)), src) == bad
    assert list(src) == [9, 9, 9, 9]
    assert C.sizeof(mi._lib.Pad) == 16 and mi._lib.Pad.fill.offset == 8
    assert L.llcomp_mi_abi_version() == 4


def test_padded_regions_plan_is_pad_axis_per_axis(mi):
    rng = np.random.default_rng(11)
    w, h = 37, 23
    for mode in MODES:
        rects = []
        for _ in range(30):
            lw, lh = limit(mode, w), limit(mode, h)
            x, y = int(rng.integers(-lw, w)), int(rng.integers(-lh, h))
            rw = int(rng.integers(max(1, 1 - x), w + lw - x + 1))
            rh = int(rng.integers(max(1, 1 - y), h + lh - y + 1))
            rects.append((x, y, rw, rh))
        src = mi.padded_regions_plan(w, h, rects, mode)
        for (x, y, rw, rh), s in zip(rects, src.tolist()):
            assert (s[0], s[2]) == mi.pad_axis(mode, w, x, rw) and (s[1], s[3]) == mi.pad_axis(mode, h, y, rh)
            assert s[0] + s[2] <= w and s[1] + s[3] <= h
