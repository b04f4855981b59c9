"""GAUSSIAN_BLUR and ADJUST_HUE of the photometric chains on the host (include/llcomp_mi.h: "Photometric chains"):
llcomp_mi_photo_reference -- compiled from the functions the GPU's kernels are compiled from -- against tests/photo_spec.py (both
rules restated with numpy), against the recorded outputs of PIL in tests/golden/photo_area_rule.json, and against PIL itself where it
is installed; and the limits."""
import ctypes as C

import numpy as np
import pytest

import photo_spec
from conftest import load_golden
from test_photo_rule import fnv1a64, random_chain


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


def mixed_chain(rng):
    """a chain of test_photo_rule.py's ops with one to three of the new ones put in at seeded places, at most eight in all"""
    chain = random_chain(rng)[:int(rng.integers(0, 7))]
    for _ in range(int(rng.integers(1, 4))):
        if len(chain) == 8:
            break
        new = (("gaussian_blur", float(rng.choice([0.0, 1e-4, 0.1, 1.0, 2.0, rng.uniform(0.1, 2.0), rng.uniform(2.0, 32.0), 32.0]))) if rng.integers(0, 2)
               else ("adjust_hue", float(rng.choice([0.0, 0.5, -0.5, 1 / 255, -1 / 255, rng.uniform(-0.5, 0.5)]))))
        chain.insert(int(rng.integers(0, len(chain) + 1)), new)
    return chain


def test_seeded_mixed_chains_equal_the_spec(mi):
    rng = np.random.default_rng(4242)
    seen = set()
    for i in range(300):
        c = (1, 3)[i % 2]
        img = photo_spec.gen_image(("noise", "narrow", "constant", "ramp")[i % 4], int(rng.integers(1, 81)), int(rng.integers(1, 41)), c, i)
        chain = mixed_chain(rng)
        seen |= {op for op, _ in chain}
        ref = mi.photo_reference(img, chain)
        assert np.array_equal(ref, photo_spec.apply(img, chain)), (i, chain)
        step = img
        for op in chain:  # op by op is the chain
            step = mi.photo_reference(step, [op])
        assert np.array_equal(step, ref), (i, chain)
    assert seen == set(photo_spec.NAMES) | set(photo_spec.AREA_NAMES)


def test_reference_equals_the_golden_vectors(mi):
    doc = load_golden("photo_area_rule.json")
    assert len(doc["vectors"]) == 2 * (5 * 8 + 2 * 7) and len(doc["full"]) == 6
    for v in doc["vectors"]:
        img = photo_spec.gen_image(v["kind"], v["w"], v["h"], v["c"], v["seed"])
        chain = [(v["op"], float.fromhex(v["param"]))]
        ref = mi.photo_reference(img, chain)
        assert fnv1a64(ref.tobytes()) == v["fnv"], v
        assert np.array_equal(ref, photo_spec.apply(img, chain)), v
    for v in doc["full"]:
        img = np.array(v["image"], np.uint8).reshape(v["h"], v["w"], v["c"])
        want = np.array(v["out"], np.uint8).reshape(img.shape)
        chain = [(v["op"], float.fromhex(v["param"]))]
        assert np.array_equal(mi.photo_reference(img, chain), want) and np.array_equal(photo_spec.apply(img, chain), want)
    # the box radii the rule's statement quotes
    assert [float(photo_spec.blur_weights(r)[0]) for r in (1.0, 2.0, 12.0)] == [float(np.float32(x)) for x in (0.25000003, 1.375, 11.479167)]
    # the hue's byte: truncation toward zero, then mod 256 (the float32 nearest 1/255 lies above it, so +-1/255 give +-1: 1 and 255)
    assert [photo_spec.hue_shift(f) for f in (0.1, -0.5, 0.5, 1 / 255, -1 / 255, 0.0, -0.001)] == [25, 129, 127, 1, 255, 0, 0]


def test_reference_equals_pil(mi):
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageFilter

    rng = np.random.default_rng(99)
    for i in range(700):
        c = (1, 3)[i % 2]
        img = photo_spec.gen_image(("noise", "narrow", "constant", "ramp")[i % 4], int(rng.integers(1, 81)), int(rng.integers(1, 81)), c, 3000 + i)
        radius = float(np.float32(rng.choice([0.0, 1e-4, rng.uniform(0.1, 2.0), rng.uniform(0.1, 2.0), rng.uniform(12.0, 32.0)])))
        im = Image.fromarray(img[..., 0] if c == 1 else img)
        want = np.asarray(im.filter(ImageFilter.GaussianBlur(radius))).reshape(img.shape)
        assert np.array_equal(mi.photo_reference(img, [("gaussian_blur", radius)]), want), (i, radius)
    # the hue shift on all 2^24 RGB triples as one 4096 x 4096 image: convert("HSV"), the uint8 wrap add, convert("RGB")
    a = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([a >> 16, (a >> 8) & 255, a & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
    hsv = np.array(Image.fromarray(rgb).convert("HSV"))
    for factor in (0.1, -0.5, 1 / 255):
        shifted = hsv.copy()
        shifted[..., 0] += np.uint8(photo_spec.hue_shift(factor))  # (wraps)
        want = np.asarray(Image.frombytes("HSV", (4096, 4096), shifted.tobytes()).convert("RGB"))
        got = mi.photo_reference(rgb, [("adjust_hue", factor)])
        assert np.array_equal(got, want), (factor, int((got != want).any(axis=2).sum()))


def test_limits(mi):
    from llcomp_amd import _lib

    L = _lib.load()
    img = photo_spec.gen_image("noise", 6, 5, 3, 1)
    out = np.full_like(img, 0x5A)

    def rc(ops):
        arr = (_lib.PhotoOp * max(1, len(ops)))(*[_lib.PhotoOp(o, p) for o, p in ops])
        return L.llcomp_mi_photo_reference(img.ctypes.data, 6, 5, 3, arr, len(ops), out.ctypes.data)

    nan, inf = float("nan"), float("inf")
    bad = [(mi.PHOTO_GAUSSIAN_BLUR, -1e-3), (mi.PHOTO_GAUSSIAN_BLUR, 32.5), (mi.PHOTO_GAUSSIAN_BLUR, nan), (mi.PHOTO_GAUSSIAN_BLUR, inf),
           (mi.PHOTO_GAUSSIAN_BLUR, -inf), (mi.PHOTO_ADJUST_HUE, 0.5001), (mi.PHOTO_ADJUST_HUE, -0.5001), (mi.PHOTO_ADJUST_HUE, nan),
           (mi.PHOTO_ADJUST_HUE, inf), (mi.PHOTO_ADJUST_HUE, -inf)] + [(code, 0.0) for code in range(9, 16)] + [(18, 0.0), (0xFFFFFFFF, 0.0)]
    for op in bad:
        assert rc([(mi.PHOTO_INVERT, 0.0), op]) == mi.BAD_ARGS, op
        assert (out == 0x5A).all()
    good = [(mi.PHOTO_GAUSSIAN_BLUR, 0.0), (mi.PHOTO_GAUSSIAN_BLUR, 32.0), (mi.PHOTO_ADJUST_HUE, 0.5), (mi.PHOTO_ADJUST_HUE, -0.5)]
    assert rc(good) == 0
    # the Python layer: torchvision's functional names; "hue" and "sharpness" stay refused
    assert mi.PHOTO_GAUSSIAN_BLUR == 16 and mi.PHOTO_ADJUST_HUE == 17 and mi.PHOTO_EQUALIZE == 8 and len(mi.PHOTO_NAMES) == 9
    assert mi.photo_chain([("gaussian_blur", 1.5), ("adjust_hue", -0.25), (16, 2), (17,)]) == [(16, 1.5), (17, -0.25), (16, 2.0), (17, 0.0)]
    for call in (lambda: mi.photo_chain([("hue", 0.1)]), lambda: mi.photo_reference(img, [("hue", 0.1)]), lambda: mi.photo_chain(["sharpness"]),
                 lambda: mi.photo_chain(["blur"]), lambda: mi.photo_reference(img, [("gaussian_blur", 33.0)]),
                 lambda: mi.photo_reference(img, [("adjust_hue", 0.6)]), lambda: mi.photo_reference(img, [(12, 0.0)])):
        with pytest.raises(mi.LlcompError) as e:
            call()
        assert e.value.status == mi.BAD_ARGS
    # radius 0 and a hue factor of 0 on gray pixels change nothing; one channel is left alone by the hue; the blur takes it
    assert np.array_equal(mi.photo_reference(img, [("gaussian_blur", 0.0)]), img)
    gray = np.repeat(img[..., :1], 3, axis=2)
    assert np.array_equal(mi.photo_reference(gray, [("adjust_hue", 0.3)]), gray)
    one = img[..., 0]
    assert np.array_equal(mi.photo_reference(one, [("adjust_hue", 0.3)]), one)
    assert not np.array_equal(mi.photo_reference(one, [("gaussian_blur", 1.0)]), one)
    assert C.sizeof(_lib.PhotoOp) == 8 and C.sizeof(_lib.PhotoChain) == 68 and C.sizeof(_lib.PhotoGroup) == 16
