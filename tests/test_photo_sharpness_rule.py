"""ADJUST_SHARPNESS of the photometric chains on the host (include/llcomp_mi.h: "Photometric chains"): llcomp_mi_photo_reference --
compiled from the functions the GPU's kernel is compiled from -- against tests/photo_spec.py (the rule restated with numpy, in
integers), against the recorded outputs of PIL in tests/golden/photo_sharpness_rule.json, and against PIL itself where it is installed
(ImageEnhance.Sharpness, and ImageFilter.SMOOTH at a factor of 0); and the limits."""
import ctypes as C

import numpy as np
import pytest

import photo_spec
from conftest import load_golden
from test_photo_area_rule import mixed_chain
from test_photo_rule import fnv1a64

FACTORS = [0.0, 1.0, 2.0, 0.5, 1.9, 7.5]


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


def sharp_chain(rng):
    """a chain of all the other ops (test_photo_area_rule.py's mixed chains) with the sharpness put in once or twice at seeded places"""
    chain = mixed_chain(rng)[:int(rng.integers(0, 8))]
    for _ in range(int(rng.integers(1, 3))):
        if len(chain) == 8:
            break
        chain.insert(int(rng.integers(0, len(chain) + 1)), ("adjust_sharpness", float(rng.choice(FACTORS + [rng.uniform(0, 2)]))))
    return chain


def test_seeded_chains_with_the_op_equal_the_spec(mi):
    rng = np.random.default_rng(1913)
    seen = set()
    for i in range(320):
        c = (1, 3)[i % 2]
        img = photo_spec.gen_image(("noise", "narrow", "constant", "ramp")[i % 4], int(rng.integers(1, 81)), int(rng.integers(1, 81)), c, i)
        chain = sharp_chain(rng)
        seen |= {op for op, _ in chain}
        ref = mi.photo_reference(img, chain)
        assert np.array_equal(ref, photo_spec.apply(img, chain)), (i, chain)
        step = img
        for op in chain:  # op by op is the chain
            step = mi.photo_reference(step, [op])
        assert np.array_equal(step, ref), (i, chain)
    assert "adjust_sharpness" in seen and len(seen) == 12  # (every other op has been its neighbour)


def test_the_float_form_is_the_integer_form():
    """what the header states in one sentence: PIL's nine binary32 products onto 0.5, truncated, are (S + 6) // 13"""
    rng = np.random.default_rng(5)
    for i in range(60):
        c = (1, 3)[i % 2]
        img = photo_spec.gen_image(("noise", "narrow", "checker", "ramp")[i % 4], int(rng.integers(3, 81)), int(rng.integers(3, 81)), c, i)
        assert np.array_equal(photo_spec.smooth_float(img), photo_spec.smooth(img)), i


def test_reference_equals_the_golden_vectors(mi):
    doc = load_golden("photo_sharpness_rule.json")
    assert doc["pillow"] and len(doc["vectors"]) == 2 * 8 * 8 and len(doc["full"]) == 5
    for v in doc["vectors"]:
        img = photo_spec.gen_image(v["kind"], v["w"], v["h"], v["c"], v["seed"])
        chain = [("adjust_sharpness", float.fromhex(v["param"]))]
        ref = mi.photo_reference(img, chain)
        assert fnv1a64(ref.tobytes()) == v["fnv"], v
        assert np.array_equal(ref, photo_spec.apply(img, chain)), v
    for v in doc["full"]:
        img = np.array(v["image"], np.uint8).reshape(v["h"], v["w"], v["c"])
        want = np.array(v["out"], np.uint8).reshape(img.shape)
        chain = [("adjust_sharpness", float.fromhex(v["param"]))]
        assert np.array_equal(mi.photo_reference(img, chain), want) and np.array_equal(photo_spec.apply(img, chain), want)


def test_reference_equals_pil(mi):
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance, ImageFilter

    rng = np.random.default_rng(77)
    sides = [1, 2, 3]
    for i in range(760):
        c = (1, 3)[i % 2]
        w = sides[i % 3] if i < 60 else int(rng.integers(1, 81))
        h = sides[(i // 3) % 3] if i < 30 else int(rng.integers(1, 81))
        img = photo_spec.gen_image(("noise", "narrow", "constant", "ramp", "checker")[i % 5], w, h, c, 7000 + i)
        a = float(np.float32((FACTORS + [rng.uniform(0, 2)])[i % 7]))
        im = Image.fromarray(img[..., 0] if c == 1 else img)
        want = np.asarray(ImageEnhance.Sharpness(im).enhance(a)).reshape(img.shape)
        got = mi.photo_reference(img, [("adjust_sharpness", a)])
        assert np.array_equal(got, want), (i, w, h, c, a)
        if a == 0.0:
            assert np.array_equal(got, np.asarray(im.filter(ImageFilter.SMOOTH)).reshape(img.shape)), (i, w, h, c)
    # black and white: the smooth value and both clamps of the blend reach 0 and 255
    img = photo_spec.checker(31, 17, 3, 2)
    for a in (0.0, 7.5, 256.0):
        got = mi.photo_reference(img, [("adjust_sharpness", a)])
        assert np.array_equal(got, np.asarray(ImageEnhance.Sharpness(Image.fromarray(img)).enhance(a)))
        assert got.min() == 0 and got.max() == 255


def test_limits(mi):
    from llcomp_amd import _lib

    L = _lib.load()
    img = photo_spec.gen_image("noise", 6, 5, 3, 1)
    out = np.full_like(img, 0x5A)

    def rc(ops, src=img, dst=out):
        arr = (_lib.PhotoOp * max(1, len(ops)))(*[_lib.PhotoOp(o, p) for o, p in ops])
        return L.llcomp_mi_photo_reference(src.ctypes.data, src.shape[1], src.shape[0], src.shape[2], arr, len(ops), dst.ctypes.data)

    nan, inf = float("nan"), float("inf")
    for p in (-1e-3, 256.5, nan, inf, -inf):
        assert rc([(mi.PHOTO_INVERT, 0.0), (mi.PHOTO_ADJUST_SHARPNESS, p)]) == mi.BAD_ARGS, p
        assert (out == 0x5A).all()
    assert rc([(mi.PHOTO_ADJUST_SHARPNESS, 0.0), (mi.PHOTO_ADJUST_SHARPNESS, 256.0)]) == 0
    # the Python layer: torchvision's functional name; the enum keeps its gap
    assert mi.PHOTO_ADJUST_SHARPNESS == 19 and mi.photo_chain([("adjust_sharpness", 1.5), (19, 2)]) == [(19, 1.5), (19, 2.0)]
    with pytest.raises(mi.LlcompError) as e:
        mi.photo_reference(img, [("adjust_sharpness", 300.0)])
    assert e.value.status == mi.BAD_ARGS
    # a = 1 is the identity, sides below 3 are the identity, and something happens otherwise
    assert np.array_equal(mi.photo_reference(img, [("adjust_sharpness", 1.0)]), img)
    assert not np.array_equal(mi.photo_reference(img, [("adjust_sharpness", 1.5)]), img)
    for w, h in ((1, 1), (2, 9), (9, 2), (1, 40), (40, 1)):
        for c in (1, 3):
            small = photo_spec.gen_image("noise", w, h, c, 3)
            for a in (0.0, 0.3, 8.0):
                assert np.array_equal(mi.photo_reference(small, [("adjust_sharpness", a)]), small), (w, h, c, a)
    # src == out gives what out of place gives
    chain = [(mi.PHOTO_ADJUST_SHARPNESS, 1.7), (mi.PHOTO_INVERT, 0.0), (mi.PHOTO_ADJUST_SHARPNESS, 0.0)]
    for c in (1, 3):
        src = photo_spec.gen_image("noise", 33, 21, c, 9)
        apart, inplace = np.empty_like(src), src.copy()
        assert rc(chain, src, apart) == 0 and rc(chain, inplace, inplace) == 0
        assert np.array_equal(apart, inplace) and np.array_equal(apart, photo_spec.apply(src, [(o, p) for o, p in chain]))
    assert C.sizeof(_lib.PhotoOp) == 8 and C.sizeof(_lib.PhotoChain) == 68 and C.sizeof(_lib.PhotoGroup) == 16
