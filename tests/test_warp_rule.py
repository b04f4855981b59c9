"""The rule of the warped views (include/llcomp_mi.h "Views under an affine map"; llcomp_mi_warp_reference, host only): byte for byte
PIL's Image.transform(AFFINE) under NEAREST, BILINEAR and BICUBIC.  Against PIL itself where it is installed -- 300 seeded cases and the
corner cases -- and against tests/golden/warp_rule.json (tools/make_warp_golden.py wrote it from PIL) everywhere.  No GPU."""
import math

import numpy as np
import pytest
from conftest import load_golden

FILTERS = ("nearest", "bilinear", "bicubic")


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


def pil_warp(Image, img, m, name, ow, oh, fill):
    """Image.transform on an image of 1 (L), 3 (RGB) or 4 (CMYK) independent bands; any other count band by band, as L images"""
    res = {"nearest": Image.NEAREST, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[name]
    h, w, c = img.shape
    if c not in (1, 3, 4):
        return np.stack([pil_warp(Image, img[..., ch:ch + 1], m, name, ow, oh, fill[ch:ch + 1])[..., 0] for ch in range(c)], axis=-1)
    im = Image.frombytes({1: "L", 3: "RGB", 4: "CMYK"}[c], (w, h), np.ascontiguousarray(img).tobytes())
    fc = int(fill[0]) if c == 1 else tuple(int(v) for v in fill)
    return np.asarray(im.transform((ow, oh), Image.AFFINE, tuple(m), res, fillcolor=fc)).reshape(oh, ow, c)


def family(n=300, seed=4242):
    """1, 3 and 4 bands; images and outputs of 1 .. 39 pixels a side; rotations, shears and scales of 0.5 .. 2; every fifth case a pure
    scale, every seventh an integer translate"""
    rng = np.random.default_rng(seed)
    for i in range(n):
        c = (1, 3, 4)[i % 3]
        w, h, ow, oh = (int(v) for v in rng.integers(1, 40, 4))
        img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        ang, sx, sy, sh = rng.uniform(0, 2 * math.pi), rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0), rng.uniform(-0.7, 0.7)
        m = [sx * math.cos(ang), sx * (math.sin(ang) + sh), rng.uniform(-w / 2, w), -sy * math.sin(ang), sy * math.cos(ang), rng.uniform(-h / 2, h)]
        if i % 5 == 0:
            m[0], m[1], m[3], m[4] = sx * (1 if i % 2 else -1), 0.0, 0.0, sy
            if m[0] < 0:
                m[2] = rng.uniform(0, 1.5 * w)
        if i % 7 == 0:
            m = [1.0, 0.0, float(rng.integers(-w, w + 1)), 0.0, 1.0, float(rng.integers(-h, h + 1))]
        yield i, img, m, ow, oh, rng.integers(0, 256, c)


def test_equal_to_pil_on_300_cases(mi):
    Image = pytest.importorskip("PIL.Image")
    for i, img, m, ow, oh, fill in family():
        for name in FILTERS:
            want = pil_warp(Image, img, m, name, ow, oh, fill)
            got = mi.warp_reference(img, m, name, ow, oh, fill)
            assert np.array_equal(got, want), (i, name, img.shape, (ow, oh), m)


def test_corner_cases_against_pil(mi):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    rot = [0.8, 0.6, -1.25, -0.6, 0.8, 2.5]
    for w, h in ((1, 1), (1, 9), (9, 1), (1, 2), (2, 1)):  # 1 x 1 and 1 x N images: every clamp of the taps
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for m in (rot, [0.3, 0.0, 0.1, 0.0, 0.4, -0.2], [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], [0.5, 0.1, -0.5, -0.1, 0.5, 0.5]):
            for name in FILTERS:
                assert np.array_equal(mi.warp_reference(img, m, name, 7, 6, (9, 8, 7)), pil_warp(Image, img, m, name, 7, 6, (9, 8, 7))), (w, h, m, name)
    img = rng.integers(0, 256, (11, 13, 2), dtype=np.uint8)  # two channels: two L images
    for name in FILTERS:
        got = mi.warp_reference(img, rot, name, 10, 12, (200, 100))
        for ch in range(2):
            assert np.array_equal(got[..., ch:ch + 1], pil_warp(Image, img[..., ch:ch + 1], rot, name, 10, 12, (200, 100)[ch:ch + 1]))


def test_identity_and_views_wholly_outside(mi):
    rng = np.random.default_rng(8)
    for c in (1, 2, 3, 5):
        img = rng.integers(0, 256, (9, 14, c), dtype=np.uint8)
        fill = np.arange(c) + 40
        for name in FILTERS:
            assert np.array_equal(mi.warp_reference(img, [1, 0, 0, 0, 1, 0], name), img)  # the identity returns the image
            for m in ([1, 0, 14, 0, 1, 0], [1, 0, 0, 0, 1, -20], [0.5, 0.5, -100, -0.5, 0.5, 3], [1, 0, 3000, 0, 1, 0]):
                out = mi.warp_reference(img, m, name, 6, 5, fill)
                assert out.shape == (5, 6, c) and (out == fill.astype(np.uint8)).all(), (c, name, m)
                assert mi.warp_source_rect(14, 9, m, name, 6, 5) == ((0, 0, 0, 0), True)
            assert (mi.warp_reference(img, [1, 0, 14, 0, 1, 0], name, 3, 3) == 0).all()  # no fill: zeros
    assert np.array_equal(mi.warp_reference(img[..., 0], [1, 0, 0, 0, 1, 0], "bicubic"), img[..., 0])  # [h, w] in, [h, w] out


def test_committed_vectors(mi):
    """tests/golden/warp_rule.json: what PIL gave when tools/make_warp_golden.py ran.  The last vector is the one a fused multiply-add
    changes: the rule -- and PIL -- give `bilinear`, an evaluation with a * b + c rounded once gives `bilinear_fused`."""
    gold = load_golden("warp_rule.json")
    assert len(gold["vectors"]) >= 9
    sensitive = 0
    for i, v in enumerate(gold["vectors"]):
        img = np.array(v["image"], np.uint8).reshape(v["h"], v["w"], v["c"])
        m = [float.fromhex(t) for t in v["m"]]
        for name in FILTERS:
            if name in v:
                want = np.array(v[name], np.uint8).reshape(v["oh"], v["ow"], v["c"])
                assert np.array_equal(mi.warp_reference(img, m, name, v["ow"], v["oh"], v["fill"]), want), (i, name)
        if v.get("contraction_sensitive"):
            sensitive += 1
            fused = np.array(v["bilinear_fused"], np.uint8).reshape(v["oh"], v["ow"], v["c"])
            got = mi.warp_reference(img, m, "bilinear", v["ow"], v["oh"], v["fill"])
            assert (got != fused).any() and np.array_equal(got, np.array(v["bilinear"], np.uint8).reshape(fused.shape))
    assert sensitive == 1


def test_rotate_matrix_is_image_rotate(mi):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(9)
    w, h = 23, 17
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    im = Image.frombytes("RGB", (w, h), img.tobytes())
    res = {"nearest": Image.NEAREST, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}
    cases = [(30, None, None), (-30, None, None), (45, None, None), (1.5, None, None), (123.456, None, None), (200, None, None), (359, None, None),
             (33, (0, 0), None), (75, (5.5, 3.25), None), (10, None, (3, -2)), (271, (20, 2), (-4, 5)), (90, (3, 4), None), (180, None, (1, 1)),
             (-400.25, (11.5, 8.5), (0, 7))]
    for angle, center, translate in cases:
        m = mi.rotate_matrix(w, h, angle, center, translate)
        for name in FILTERS:
            want = np.asarray(im.rotate(angle, res[name], center=center, translate=translate, fillcolor=(5, 6, 7)))
            assert np.array_equal(mi.warp_reference(img, m, name, fill=(5, 6, 7)), want), (angle, center, translate, name)
