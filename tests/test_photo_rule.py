"""The rule of the photometric chains on the host (include/llcomp_mi.h: "Photometric chains"): llcomp_mi_photo_reference -- compiled from
the functions the GPU's kernels are compiled from -- against tests/photo_spec.py (the rule restated with numpy), against the recorded
outputs of PIL in tests/golden/photo_rule.json, and against PIL itself where it is installed; and the limits."""
import ctypes as C

import numpy as np
import pytest

import photo_spec
from conftest import load_golden


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


def fnv1a64(data):
    h = 0xCBF29CE484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def chain_of(v):
    return [(op, float.fromhex(p)) for op, p in v["chain"]]


def test_reference_equals_the_spec_and_the_golden_vectors(mi):
    doc = load_golden("photo_rule.json")
    assert len(doc["vectors"]) == 144 and len(doc["full"]) == 5
    seen_ops, lengths = set(), set()
    for v in doc["vectors"]:
        img = photo_spec.gen_image(v["kind"], v["w"], v["h"], v["c"], v["seed"])
        chain = chain_of(v)
        ref = mi.photo_reference(img, chain)
        assert np.array_equal(ref, photo_spec.apply(img, chain)), v
        assert fnv1a64(ref.tobytes()) == v["fnv"], v
        seen_ops |= {op for op, _ in chain}
        lengths.add(len(chain))
    assert seen_ops == set(photo_spec.NAMES) and {1, 2, 4, 8} <= lengths
    for v in doc["full"]:
        img = np.array(v["image"], np.uint8).reshape(v["h"], v["w"], v["c"])
        want = np.array(v["out"], np.uint8).reshape(img.shape)
        assert np.array_equal(mi.photo_reference(img, chain_of(v)), want) and np.array_equal(photo_spec.apply(img, chain_of(v)), want)


def test_the_named_corner_cases(mi):
    # equalize's table entry of 256 is clipped: 511 pixels of 10 and one of 200
    img = photo_spec.gen_image("clip", 32, 16, 1, 0)
    out = mi.photo_reference(img, ["equalize"])
    assert out.max() == 255 and (out[img == 200] == 255).all() and np.array_equal(out, photo_spec.apply(img, ["equalize"]))
    # a constant image, a 1 x 1 image and fewer than 255 pixels (step == 0): autocontrast and equalize change nothing
    for img in (np.full((9, 7, 3), 77, np.uint8), np.array([[[5, 200, 90]]], np.uint8), photo_spec.gen_image("noise", 15, 16, 3, 4)):
        assert np.array_equal(mi.photo_reference(img, ["equalize"]), img)
    assert np.array_equal(mi.photo_reference(np.full((9, 7, 1), 77, np.uint8), ["autocontrast"]), np.full((9, 7, 1), 77, np.uint8))
    # factors 0 and 1; color and grayscale leave one channel alone; [h, w] images
    img = photo_spec.gen_image("noise", 13, 11, 3, 9)
    assert not mi.photo_reference(img, [("brightness", 0.0)]).any()
    for op in ("brightness", "contrast", "color"):
        assert np.array_equal(mi.photo_reference(img, [(op, 1.0)]), img)
    g = mi.photo_reference(img, ["grayscale"])
    assert (g[..., 0] == g[..., 1]).all() and (g[..., 0] == g[..., 2]).all() and np.array_equal(g[..., 0], photo_spec.luma(img))
    assert np.array_equal(mi.photo_reference(img, [("color", 0.0)]), g)
    one = img[..., 0]
    assert np.array_equal(mi.photo_reference(one, [("color", 0.3), "grayscale"]), one)
    assert np.array_equal(mi.photo_reference(one, ["invert"]), 255 - one)
    assert np.array_equal(mi.photo_reference(img, []), img)
    # the names and codes agree with the spec's
    assert mi.PHOTO_NAMES == photo_spec.NAMES and mi.photo_code("saturation") == mi.PHOTO_COLOR and mi.PHOTO_EQUALIZE == 8


def test_seeded_chains_equal_the_spec(mi):
    rng = np.random.default_rng(2024)
    for i in range(300):
        c = (1, 3)[i % 2]
        img = photo_spec.gen_image(("noise", "narrow", "constant", "ramp")[i % 4], int(rng.integers(1, 41)), int(rng.integers(1, 41)), c, i)
        chain = random_chain(rng)
        assert np.array_equal(mi.photo_reference(img, chain), photo_spec.apply(img, chain)), (i, chain)


def random_chain(rng):
    chain = []
    for _ in range(int(rng.integers(1, 9))):
        op = photo_spec.NAMES[int(rng.integers(0, 9))]
        p = {"solarize": float(rng.integers(0, 257)), "posterize": float(rng.integers(1, 9))}.get(
            op, float(rng.choice([0.0, 1.0, rng.uniform(0, 1), rng.uniform(1, 3)])))
        chain.append((op, p))
    return chain


def test_reference_equals_pil(mi):
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance, ImageOps

    def pil(img, chain):
        im = Image.fromarray(img[..., 0] if img.shape[2] == 1 else img)
        for op, p in chain:
            p = float(np.float32(p))
            im = {"brightness": lambda: ImageEnhance.Brightness(im).enhance(p), "contrast": lambda: ImageEnhance.Contrast(im).enhance(p),
                  "color": lambda: ImageEnhance.Color(im).enhance(p), "grayscale": lambda: im.convert("L").convert(im.mode),
                  "invert": lambda: ImageOps.invert(im), "solarize": lambda: ImageOps.solarize(im, int(p)),
                  "posterize": lambda: ImageOps.posterize(im, int(p)), "autocontrast": lambda: ImageOps.autocontrast(im),
                  "equalize": lambda: ImageOps.equalize(im)}[op]()
        return np.asarray(im).reshape(img.shape)

    rng = np.random.default_rng(77)
    for i in range(400):
        c = (1, 3)[i % 2]
        img = photo_spec.gen_image(("noise", "narrow", "constant", "ramp")[i % 4], int(rng.integers(1, 41)), int(rng.integers(1, 41)), c, 1000 + i)
        chain = random_chain(rng)
        assert np.array_equal(mi.photo_reference(img, chain), pil(img, chain)), (i, chain)
    img = photo_spec.gen_image("clip", 32, 16, 3, 0)
    assert np.array_equal(mi.photo_reference(img, ["equalize"]), pil(img, [("equalize", 0)]))


def test_limits(mi):
    from llcomp_amd import _lib

    L = _lib.load()
    img = photo_spec.gen_image("noise", 6, 5, 3, 1)
    out = np.full_like(img, 0x5A)

    def rc(ops, src=img, w=6, h=5, c=3, n=None, dst=out):
        arr = (_lib.PhotoOp * max(1, len(ops)))(*[_lib.PhotoOp(o, p) for o, p in ops])
        return L.llcomp_mi_photo_reference(src.ctypes.data if src is not None else None, w, h, c, arr if ops or n is None else None,
                                           len(ops) if n is None else n, dst.ctypes.data if dst is not None else None)

    bad = [[(mi.PHOTO_BRIGHTNESS, float("nan"))], [(mi.PHOTO_CONTRAST, float("inf"))], [(mi.PHOTO_COLOR, -0.25)], [(mi.PHOTO_BRIGHTNESS, 256.5)],
           [(mi.PHOTO_CONTRAST, -float("inf"))], [(mi.PHOTO_SOLARIZE, 1.5)], [(mi.PHOTO_SOLARIZE, 257.0)], [(mi.PHOTO_SOLARIZE, -1.0)],
           [(mi.PHOTO_POSTERIZE, 0.0)], [(mi.PHOTO_POSTERIZE, 9.0)], [(mi.PHOTO_POSTERIZE, 2.5)], [(mi.PHOTO_POSTERIZE, float("nan"))],
           [(9, 1.0)], [(0xFFFFFFFF, 0.0)], [(mi.PHOTO_INVERT, 0.0)] * 9]
    for ops in bad:
        assert rc([(mi.PHOTO_INVERT, 0.0)] + ops if len(ops) < 8 else ops) == mi.BAD_ARGS, ops
        assert (out == 0x5A).all()
    for kw in (dict(c=2), dict(c=4), dict(c=0), dict(w=0), dict(h=0), dict(src=None), dict(dst=None), dict(n=1)):
        assert rc([] if "n" in kw else [(mi.PHOTO_INVERT, 0.0)], **kw) == mi.BAD_ARGS, kw
    assert (out == 0x5A).all()
    # the limits' own ends are inside; the parameter of an op that takes none is ignored
    good = [(mi.PHOTO_BRIGHTNESS, 256.0), (mi.PHOTO_CONTRAST, 0.0), (mi.PHOTO_SOLARIZE, 256.0), (mi.PHOTO_SOLARIZE, 0.0), (mi.PHOTO_POSTERIZE, 1.0),
            (mi.PHOTO_POSTERIZE, 8.0), (mi.PHOTO_EQUALIZE, float("nan")), (mi.PHOTO_GRAYSCALE, -3.0)]
    assert rc(good) == 0 and rc([]) == 0
    # the Python layer: names, a chain's length, shapes
    for call in (lambda: mi.photo_chain(["sharpness"]), lambda: mi.photo_chain(["invert"] * 9), lambda: mi.photo_chain([("invert", 1, 2)]),
                 lambda: mi.photo_reference(np.zeros((2, 2, 2, 2), np.uint8), []), lambda: mi.photo_reference(img, [("hue", 0.1)]),
                 lambda: mi.photo_reference(np.zeros((4, 4, 4), np.uint8), ["invert"]), lambda: mi.photo_reference(img, ["invert"] * 9)):
        with pytest.raises(mi.LlcompError) as e:
            call()
        assert e.value.status == mi.BAD_ARGS
    assert mi.photo_chain([("brightness", 1.2), "grayscale", (mi.PHOTO_SOLARIZE, 128), ("invert",)]) == \
        [(0, float(np.float32(1.2))), (3, 0.0), (5, 128.0), (4, 0.0)]
    assert C.sizeof(_lib.PhotoOp) == 8 and C.sizeof(_lib.PhotoChain) == 68 and C.sizeof(_lib.PhotoGroup) == 16
