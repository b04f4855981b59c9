"""The rule of the perspective views (include/llcomp_mi.h "Views under a projective map"; llcomp_mi_perspective_reference, host only):
byte for byte PIL's Image.transform(PERSPECTIVE) under NEAREST, BILINEAR and BICUBIC.  Against PIL itself where it is installed -- 300
seeded keystones -- and against tests/golden/perspective_rule.json (tools/make_perspective_golden.py wrote it from PIL) everywhere.
No GPU."""
import numpy as np
import pytest
from conftest import load_golden
from perspective_cases import FILTERS, coords, keystone, pil_perspective


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


def family(mi, n=300, seed=1207):
    """1, 3 and 4 bands; images and outputs of 3 .. 40 pixels a side; the image's corners moved by up to a quarter of a side"""
    rng = np.random.default_rng(seed)
    for i in range(n):
        c = (1, 3, 4)[i % 3]
        w, h, ow, oh = (int(v) for v in rng.integers(3, 41, 4))
        img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        yield i, img, keystone(mi, rng, w, h, ow, oh), ow, oh, rng.integers(0, 256, c)


def test_equal_to_pil_on_300_keystones(mi):
    Image = pytest.importorskip("PIL.Image")
    inside = []
    for i, img, a, ow, oh, fill in family(mi):
        _, xin, yin = coords(a, ow, oh)
        inside.append(np.mean((xin >= 0) & (xin < img.shape[1]) & (yin >= 0) & (yin < img.shape[0])))
        for name in FILTERS:
            want = pil_perspective(Image, img, a, name, ow, oh, fill)
            got = mi.perspective_reference(img, a, name, ow, oh, fill)
            assert np.array_equal(got, want), (i, name, img.shape, (ow, oh), a)
    assert np.mean(inside) > 0.6  # (the family reads the image, not the fill)


def test_committed_vectors(mi):
    """tests/golden/perspective_rule.json: what PIL gave when tools/make_perspective_golden.py ran.  One vector has a6 = a7 = 0 and
    differs under NEAREST from PIL's AFFINE on the same six numbers (and so from warp_reference); one is the vector a fused
    multiply-add changes: the rule -- and PIL -- give `nearest`, contracting a0 xs + a1 ys or a6 xs + a7 ys gives `nearest_fused`."""
    gold = load_golden("perspective_rule.json")
    assert len(gold["vectors"]) >= 11
    seen = dict(sensitive=0, affine=0, outside=0, strong=0, c1=0, c3=0)
    for i, v in enumerate(gold["vectors"]):
        img = np.array(v["image"], np.uint8).reshape(v["h"], v["w"], v["c"])
        a = [float.fromhex(t) for t in v["a"]]
        shape = (v["oh"], v["ow"], v["c"])
        for name in FILTERS:
            want = np.array(v[name], np.uint8).reshape(shape)
            assert np.array_equal(mi.perspective_reference(img, a, name, v["ow"], v["oh"], v["fill"]), want), (i, name)
        seen["c1"] += v["c"] == 1
        seen["c3"] += v["c"] == 3
        seen["strong"] += bool(v.get("strong"))
        if v.get("wholly_outside"):
            seen["outside"] += 1
            assert mi.perspective_source_rect(v["w"], v["h"], a, "bilinear", v["ow"], v["oh"]) == ((0, 0, 0, 0), True)
        if v.get("differs_from_affine"):
            seen["affine"] += 1
            assert a[6] == 0.0 and a[7] == 0.0
            affine = np.array(v["affine_nearest"], np.uint8).reshape(shape)
            got = mi.perspective_reference(img, a, "nearest", v["ow"], v["oh"], v["fill"])
            assert (got != affine).any() and np.array_equal(mi.warp_reference(img, a[:6], "nearest", v["ow"], v["oh"], v["fill"]), affine)
        if v.get("contraction_sensitive"):
            seen["sensitive"] += 1
            fused = np.array(v["nearest_fused"], np.uint8).reshape(shape)
            got = mi.perspective_reference(img, a, "nearest", v["ow"], v["oh"], v["fill"])
            x, y = v["pixel"]
            assert got[y, x, 0] != fused[y, x, 0] and np.array_equal(got, np.array(v["nearest"], np.uint8).reshape(shape))
    assert seen["sensitive"] == 1 and seen["affine"] == 1 and seen["outside"] >= 1 and seen["strong"] >= 2 and seen["c1"] and seen["c3"]


def test_identity_and_views_wholly_outside(mi):
    rng = np.random.default_rng(8)
    for c in (1, 2, 3, 5):
        img = rng.integers(0, 256, (9, 14, c), dtype=np.uint8)
        fill = np.arange(c) + 40
        for name in FILTERS:
            assert np.array_equal(mi.perspective_reference(img, [1, 0, 0, 0, 1, 0, 0, 0], name), img)  # the identity returns the image
            for a in ([1, 0, 14, 0, 1, 0, 0, 0], [1, 0, 0, 0, 1, -20, 0.01, 0.01], [0.5, 0.5, -100, -0.5, 0.5, 3, 0.02, 0], [1, 0, 3000, 0, 1, 0, 0, 0.1]):
                out = mi.perspective_reference(img, a, name, 6, 5, fill)
                assert out.shape == (5, 6, c) and (out == fill.astype(np.uint8)).all(), (c, name, a)
                assert mi.perspective_source_rect(14, 9, a, name, 6, 5) == ((0, 0, 0, 0), True)
            assert (mi.perspective_reference(img, [1, 0, 14, 0, 1, 0, 0, 0], name, 3, 3) == 0).all()  # no fill: zeros
    assert np.array_equal(mi.perspective_reference(img[..., 0], [1, 0, 0, 0, 1, 0, 0, 0], "bicubic"), img[..., 0])  # [h, w] in, [h, w] out


def test_perspective_coeffs_solves_the_system(mi):
    """the map sends every endpoint to its startpoint; four pairs that are a pure scale give a6 = a7 = 0"""
    rng = np.random.default_rng(11)
    for _ in range(20):
        sp, ep = rng.uniform(0, 100, (4, 2)), np.array([[0, 0], [64, 0], [64, 48], [0, 48]], float) + rng.uniform(-8, 8, (4, 2))
        a = mi.perspective_coeffs(sp, ep)
        for (x, y), (u, v) in zip(ep, sp):
            den = a[6] * x + a[7] * y + 1
            assert abs((a[0] * x + a[1] * y + a[2]) / den - u) < 1e-7 and abs((a[3] * x + a[4] * y + a[5]) / den - v) < 1e-7
    a = mi.perspective_coeffs([[0, 0], [20, 0], [20, 10], [0, 10]], [[0, 0], [10, 0], [10, 5], [0, 5]])
    assert np.allclose(a, [2, 0, 0, 0, 2, 0, 0, 0], atol=1e-12)
    with pytest.raises(mi.LlcompError):
        mi.perspective_coeffs([[0, 0]] * 3, [[0, 0]] * 4)


LIMITS = [
    ("a coefficient that is not finite", [1, 0, 0, 0, 1, float("nan"), 0, 0], "bilinear", 4, 4),
    ("an infinite coefficient", [1, 0, 0, 0, 1, 0, float("inf"), 0], "nearest", 4, 4),
    ("a filter other than the three", [1, 0, 0, 0, 1, 0, 0, 0], "lanczos", 4, 4),
    ("the box filter", [1, 0, 0, 0, 1, 0, 0, 0], "box", 4, 4),
    ("den = 0 at the far corner", [1, 0, 0, 0, 1, 0, -1 / 3.5, 0], "bilinear", 4, 4),
    ("den < 0 at a corner", [1, 0, 0, 0, 1, 0, 0, -0.5], "nearest", 4, 4),
    ("den < 0 at the first pixel", [1, 0, 0, 0, 1, 0, -4, 0], "bicubic", 1, 1),
    ("|xin| at 2^30", [1, 0, 2.0 ** 30, 0, 1, 0, 0, 0], "bilinear", 4, 4),
    ("|yin| beyond 2^30 through a small den", [1, 0, 0, 0, 1, 5, 0, -(1 - 2.0 ** -31) / 3.5], "nearest", 4, 4),
]


@pytest.mark.parametrize("what,a,name,ow,oh", LIMITS, ids=[t[0] for t in LIMITS])
def test_limits_are_bad_args_with_out_untouched(mi, what, a, name, ow, oh):
    import ctypes as C

    L = mi._lib.load()
    img = np.full((6, 7, 2), 3, np.uint8)
    out = np.full((oh, ow, 2), 0xA5, np.uint8)
    rect, empty = (C.c_uint32 * 4)(9, 9, 9, 9), C.c_uint32(7)
    coef = (C.c_double * 8)(*[float(t) for t in a])
    code = mi.filter_code(name)
    assert L.llcomp_mi_perspective_reference(img.ctypes.data, 7, 6, 2, coef, code, None, ow, oh, out.ctypes.data) == mi.BAD_ARGS
    assert (out == 0xA5).all()
    assert L.llcomp_mi_perspective_source_rect(7, 6, coef, code, ow, oh, rect, C.byref(empty)) == mi.BAD_ARGS
    assert list(rect) == [9, 9, 9, 9] and empty.value == 7
    with pytest.raises(mi.LlcompError):
        mi.perspective_reference(img, a, name, ow, oh)


def test_more_bad_args(mi):
    import ctypes as C

    L = mi._lib.load()
    img = np.full((6, 7, 2), 3, np.uint8)
    out = np.full((4, 4, 2), 0xA5, np.uint8)
    ident = (C.c_double * 8)(1, 0, 0, 0, 1, 0, 0, 0)
    for args in ((None, 7, 6, 2, ident, 0, None, 4, 4, out.ctypes.data), (img.ctypes.data, 7, 6, 2, None, 0, None, 4, 4, out.ctypes.data),
                 (img.ctypes.data, 7, 6, 2, ident, 0, None, 4, 4, None), (img.ctypes.data, 0, 6, 2, ident, 0, None, 4, 4, out.ctypes.data),
                 (img.ctypes.data, 7, 6, 0, ident, 0, None, 4, 4, out.ctypes.data), (img.ctypes.data, 7, 6, 2, ident, 0, None, 0, 4, out.ctypes.data),
                 (img.ctypes.data, 7, 6, 2, ident, 0, None, 4, 0, out.ctypes.data)):
        assert L.llcomp_mi_perspective_reference(*args) == mi.BAD_ARGS
    assert (out == 0xA5).all()
    with pytest.raises(mi.LlcompError):
        mi.perspective_reference(img, [1, 0, 0, 0, 1, 0], "nearest")  # six numbers are an affine map
