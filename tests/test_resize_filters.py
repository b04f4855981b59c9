"""The resampling filters of the resized calls, on the CPU: llcomp_mi_resize_filter_weights against the rule restated with `math`
(tests/resize_filters_spec.py), the rule's properties, the rule against PIL bit for bit (where PIL is installed) and against PIL's
recorded bytes (tests/golden/resize_filters_pil.json, where it is not), and nearest neighbour against its integer formula and torch."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import resize_filters_spec as spec
from conftest import GOLDEN


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


GRID = [(1, 1), (1, 300), (2, 1), (3, 3), (17, 5), (5, 17), (64, 1), (100, 100), (1000, 999), (999, 1000), (640, 10), (3840, 224), (4096, 224),
        (224, 3840), (7, 448), (1280, 20)]
LIMIT = {spec.BICUBIC: (32 * 100, 100), spec.LANCZOS: (21 * 224, 224)}


def grid_of(filt):
    g = [(a, b) for a, b in GRID if spec.allowed(filt, a, b)]
    if filt in LIMIT:
        g.append(LIMIT[filt])
    for must in ((1, 1), (1, 300), (17, 5), (5, 17), (1000, 999), (999, 1000), (3840, 224), (4096, 224)):
        assert must in g, (filt, must)
    return g


@pytest.mark.parametrize("filt", range(6), ids=spec.NAMES)
def test_weights_equal_the_restated_rule(mi, filt):
    """lo and every q, exactly; K <= 129; no tap outside the input; the int32 accumulator cannot overflow; only bicubic and Lanczos
    have negative weights"""
    k_max = 0
    for in_len, out_len in grid_of(filt):
        lo, q = mi.resize_weights(in_len, out_len, filt)
        want_lo, want_q = spec.weights(filt, in_len, out_len)
        assert lo.dtype == np.uint32 and q.dtype == np.int32
        assert np.array_equal(lo, want_lo), (in_len, out_len)
        assert q.shape == want_q.shape and np.array_equal(q, want_q), (in_len, out_len, q.shape, want_q.shape)
        k = q.shape[1]
        k_max = max(k_max, k)
        assert 1 <= k <= 129
        taps = np.array([np.flatnonzero(r)[-1] + 1 if r.any() else 0 for r in q])
        assert (lo + taps <= in_len).all(), (in_len, out_len)
        assert int(np.abs(q.astype(np.int64)).sum(axis=1).max()) * 255 + (1 << 21) < 1 << 31, (in_len, out_len)
        assert abs(int(q.astype(np.int64).sum(axis=1).min()) - (1 << 22)) <= k and abs(int(q.astype(np.int64).sum(axis=1).max()) - (1 << 22)) <= k
        if filt not in (spec.BICUBIC, spec.LANCZOS):
            assert (q >= 0).all(), (in_len, out_len)
    assert k_max <= 129
    if filt in (spec.BICUBIC, spec.LANCZOS):
        assert (mi.resize_weights(5, 17, filt)[1] < 0).any() and (mi.resize_weights(3840, 224, filt)[1] < 0).any()


def test_names_and_codes(mi):
    assert (mi.FILTER_BILINEAR, mi.FILTER_NEAREST, mi.FILTER_BOX, mi.FILTER_HAMMING, mi.FILTER_BICUBIC, mi.FILTER_LANCZOS) == tuple(range(6))
    for code, name in enumerate(spec.NAMES):
        a, b = mi.resize_weights(640, 100, code), mi.resize_weights(640, 100, name)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert mi.filter_code(name) == mi.filter_code(name.upper()) == mi.filter_code(code) == code
    for bad in ("cubic", 6, -1, None, 1.0, True):
        with pytest.raises(mi.LlcompError) as e:
            mi.filter_code(bad)
        assert e.value.status == mi.BAD_ARGS


def test_filter_0_is_the_bilinear_export(mi):
    """llcomp_mi_resize_weights stays, and is filter 0: the same K, lo and q"""
    L = mi._lib.load()
    for in_len, out_len in grid_of(0):
        k = L.llcomp_mi_resize_weights(in_len, out_len, None, None)
        assert k == L.llcomp_mi_resize_filter_weights(0, in_len, out_len, None, None) > 0
        lo, q = np.zeros(out_len, np.uint32), np.zeros((out_len, k), np.int32)
        L.llcomp_mi_resize_weights(in_len, out_len, lo.ctypes.data, q.ctypes.data)
        lo2, q2 = mi.resize_weights(in_len, out_len, 0)
        lo3, q3 = mi.resize_weights(in_len, out_len)
        assert np.array_equal(lo, lo2) and np.array_equal(q, q2) and np.array_equal(lo, lo3) and np.array_equal(q, q3)


@pytest.mark.parametrize("filt", range(6), ids=spec.NAMES)
def test_same_size_is_the_identity(mi, filt):
    for n in (1, 2, 3, 64, 999):
        lo, q = mi.resize_weights(n, n, filt)
        dense = np.zeros((n, n + q.shape[1]), np.int64)
        for i in range(n):
            dense[i, lo[i]:lo[i] + q.shape[1]] = q[i]
        assert np.array_equal(dense[:, :n], np.eye(n, dtype=np.int64) << 22), n
    img = np.random.default_rng(filt).integers(0, 256, size=(13, 17, 3), dtype=np.uint8)
    assert np.array_equal(spec.resize(img, 17, 13, filt), img)


def test_refusals(mi):
    L = mi._lib.load()
    for filt in range(6):
        r = spec.REACH[filt]
        for out_len in (1, 3, 224):
            most = 64 * out_len // r
            assert L.llcomp_mi_resize_filter_weights(filt, most, out_len, None, None) > 0, (filt, out_len)
            assert L.llcomp_mi_resize_filter_weights(filt, most + 1, out_len, None, None) == 0, (filt, out_len)
            with pytest.raises(mi.LlcompError) as e:
                mi.resize_weights(most + 1, out_len, filt)
            assert e.value.status == mi.BAD_ARGS
        assert L.llcomp_mi_resize_filter_weights(filt, 0, 5, None, None) == 0 and L.llcomp_mi_resize_filter_weights(filt, 5, 0, None, None) == 0
    for code in (6, 7, 8, 255, 0x10, 0xFFFFFFFF):
        assert L.llcomp_mi_resize_filter_weights(code, 10, 10, None, None) == 0
        with pytest.raises(mi.LlcompError) as e:
            mi.resize_weights(10, 10, code)
        assert e.value.status == mi.BAD_ARGS
    with pytest.raises(mi.LlcompError):
        mi.resize_weights(10, 10, "cubic")


# ---- the rule against PIL ----

def _pil_resize(crop, ow, oh, name):
    from PIL import Image

    resample = getattr(Image.Resampling, name.upper())
    if crop.shape[2] == 3:
        return np.asarray(Image.fromarray(crop).resize((ow, oh), resample))
    # (c = 1, and c = 4 band by band: PIL premultiplies alpha when it resizes RGBA)
    return np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(crop[:, :, k])).resize((ow, oh), resample)) for k in range(crop.shape[2])],
                    axis=2)


def _random_case(rng, filt, w, h):
    while True:
        rw, rh = int(rng.integers(4, min(w, 500) + 1)), int(rng.integers(4, min(h, 500) + 1))
        ow, oh = int(rng.integers(3, 231)), int(rng.integers(3, 231))
        if spec.allowed(filt, rw, ow) and spec.allowed(filt, rh, oh):
            return (int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1)), rw, rh), (ow, oh)


@pytest.mark.parametrize("filt", spec.WEIGHTED, ids=[spec.NAMES[f] for f in spec.WEIGHTED])
def test_rule_equals_pil_bit_for_bit(filt):
    """42 crops per filter of the deterministic images, c = 1, 3 and 4: crop first, then Image.resize -- 0 differing bytes"""
    pytest.importorskip("PIL")
    from llcomp_amd import synth

    rng = np.random.default_rng(1000 + filt)
    gens = ("g3", "nat", "g1", "mid", "checker", "g2")
    differing = 0
    for i in range(42):
        gen, c = gens[i % len(gens)], (1, 3, 4)[(i // 2) % 3]
        w, h = int(rng.integers(40, 521)), int(rng.integers(40, 521))
        (x, y, rw, rh), (ow, oh) = _random_case(rng, filt, w, h)
        crop = np.ascontiguousarray(synth.GENERATORS[gen](w, h, c)[y:y + rh, x:x + rw])
        want = _pil_resize(crop, ow, oh, spec.NAMES[filt])
        got = spec.resize(crop, ow, oh, filt)
        n = int((got != want).sum())
        assert n == 0, (gen, (w, h, c), (x, y, rw, rh), (ow, oh), n)
        differing += n
    assert differing == 0


def test_rule_equals_pils_recorded_bytes(mi):
    """the same without PIL: tools/gen_resize_filters_golden.py recorded the FNV-1a-64 of PIL's output for 12 crops per filter; the rule
    with the LIBRARY's weights reproduces every one"""
    from llcomp_amd import synth

    with open(os.path.join(GOLDEN, "resize_filters_pil.json")) as f:
        golden = json.load(f)
    per_filter = {}
    for case in golden["cases"]:
        filt = spec.NAMES.index(case["filter"])
        w, h, c = case["shape"]
        x, y, rw, rh = case["rect"]
        ow, oh = case["out"]
        crop = np.ascontiguousarray(synth.GENERATORS[case["gen"]](w, h, c)[y:y + rh, x:x + rw])
        got = spec.resize(crop, ow, oh, filt)
        assert spec.fnv1a64(got.tobytes()) == mi.fnv1a64(got.tobytes()) == case["fnv"], case
        lx, qx = mi.resize_weights(rw, ow, filt)
        ly, qy = mi.resize_weights(rh, oh, filt)
        mine = spec._axis(spec._axis(crop, lx.astype(np.int64), qx.astype(np.int64), 1), ly.astype(np.int64), qy.astype(np.int64), 0)
        assert np.array_equal(mine, got), case
        per_filter[filt] = per_filter.get(filt, 0) + 1
    assert sorted(per_filter) == sorted(spec.WEIGHTED) and min(per_filter.values()) >= 10


# ---- nearest ----

def test_nearest_is_the_integer_formula_everywhere(mi):
    rng = np.random.default_rng(3)
    axes = [(1, 1), (1, 300), (17, 5), (5, 17), (1000, 999), (999, 1000), (3840, 224), (640, 10)]
    axes += [(int(rng.integers(1, 3000)), int(rng.integers(1, 3000))) for _ in range(300)]
    for in_len, out_len in axes:
        if not spec.allowed(spec.NEAREST, in_len, out_len):
            continue
        lo, q = mi.resize_weights(in_len, out_len, "nearest")
        assert q.shape == (out_len, 1) and (q == 1 << 22).all()
        assert lo.tolist() == [((2 * i + 1) * in_len) // (2 * out_len) for i in range(out_len)], (in_len, out_len)


def test_nearest_equals_torch_nearest_exact_on_odd_sides(mi):
    """an odd input side has no output position on an exact integer -- where float rounding may pick the other neighbour -- so torch's
    float64 nearest-exact and the integer formula must agree everywhere"""
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F

    rng = np.random.default_rng(4)
    n = 0
    while n < 150:
        in_len, out_len = 2 * int(rng.integers(0, 700)) + 1, int(rng.integers(1, 1500))
        if not spec.allowed(spec.NEAREST, in_len, out_len):
            continue
        n += 1
        src = torch.arange(in_len, dtype=torch.float64).reshape(1, 1, in_len)
        want = F.interpolate(src, size=out_len, mode="nearest-exact").reshape(-1).numpy().astype(np.int64)
        lo, _ = mi.resize_weights(in_len, out_len, mi.FILTER_NEAREST)
        assert np.array_equal(lo, want), (in_len, out_len)


def test_nearest_invents_no_class_id():
    """a label image comes out holding only ids that went in; every other filter invents some on the same image"""
    rng = np.random.default_rng(5)
    ids = np.array([0, 3, 7, 19, 200, 255], np.uint8)
    mask = ids[rng.integers(0, len(ids), size=(9, 12))].repeat(11, axis=0).repeat(7, axis=1)[:, :, None]  # 99 x 84 blocks of class ids
    for ow, oh in ((31, 45), (224, 224), (84, 99), (5, 3)):
        out = spec.resize(mask, ow, oh, spec.NEAREST)
        assert set(np.unique(out)) <= set(ids.tolist())
        ly, lx = spec.weights(spec.NEAREST, 99, oh)[0], spec.weights(spec.NEAREST, 84, ow)[0]
        assert np.array_equal(out, mask[ly][:, lx])
    for filt in spec.WEIGHTED:
        assert not set(np.unique(spec.resize(mask, 31, 45, filt))) <= set(ids.tolist()), spec.NAMES[filt]


def test_python_flags_carry_the_filter(mi):
    """filter= is OR-ed into bits 4-6 of the flags; a bad filter is BAD_ARGS before anything else happens"""
    ft = mi._flags_table
    assert ft(None, 3) is None
    assert list(ft(None, 3, "bicubic")) == [0x40] * 3
    assert list(ft([1, 0, 1], 3, ["nearest", 0, mi.FILTER_LANCZOS])) == [0x11, 0x00, 0x51]
    assert list(ft(np.array([1, 0], np.uint8), 2)) == [1, 0]
    for bad in ("cubic", 6, ["box"], ["box", "box", "boxy"]):
        with pytest.raises(mi.LlcompError) as e:
            ft(None, 3, bad)
        assert e.value.status == mi.BAD_ARGS
    assert C.sizeof(C.c_uint8) == 1 and mi.FLAG_FILTER_SHIFT == 4


def test_weight_tables_need_ten_sides_not_six(mi):
    """what the staging buffer's bound counts per frame and axis: out * (K + 1) int32.  The triangle's K <= 2 * max(in / out, 1) + 3 kept
    that within 6 * max(in, out); a radius of 3 gives K <= 6 * max(in / out, 1) + 3 and 10 * max(in, out).  Lanczos at its limit is past
    the old factor, and no filter is past the new one"""
    worst = 0.0
    for filt in range(6):
        for in_len, out_len in grid_of(filt) + [(21 * 300, 300), (2100, 100), (300, 300), (100, 300)]:
            if not spec.allowed(filt, in_len, out_len):
                continue
            k = mi.resize_weights(in_len, out_len, filt)[1].shape[1]
            ints, side = out_len * (k + 1), max(in_len, out_len)
            assert ints <= 10 * side, (filt, in_len, out_len, k)
            if filt in (spec.BILINEAR, spec.NEAREST, spec.BOX, spec.HAMMING):
                assert ints <= 6 * side, (filt, in_len, out_len, k)
            worst = max(worst, ints / side)
    assert worst > 6.0  # (Lanczos 6300 -> 300: 300 * (126 + 1) = 6.05 sides)
