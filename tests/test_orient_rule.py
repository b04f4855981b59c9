"""The rule of the batch orientation on the host (llcomp_mi_orient_reference; include/llcomp_mi.h: "Batch orientation") against
tests/orient_spec.py -- numpy's flip, rot90 and transposition -- and PIL's Image.transpose, bit for bit; the group's laws; the refusals."""
import ctypes as C

import numpy as np
import pytest

import orient_spec
from orient_spec import bits_of

DTYPES = ("uint8", "float32", "float16", "bfloat16")
# (ow, oh, c): the smallest; the smallest with a partner for every pixel; odd squares with a centre; one row, one column; not square
SHAPES = ((1, 1, 1), (2, 2, 3), (3, 3, 1), (5, 5, 3), (3, 1, 3), (1, 4, 1), (7, 5, 3))


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


@pytest.mark.parametrize("layout", ("chw", "hwc"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_is_the_spec_for_every_code(mi, dtype, layout):
    for si, (ow, oh, c) in enumerate(SHAPES):
        codes = [k for k in range(8) if ow == oh or k not in orient_spec.TRANSPOSING]
        batch = orient_spec.gen_batch(dtype, len(codes), c, oh, ow, layout, seed=si)
        want = bits_of(orient_spec.apply(batch, codes, layout))
        got = mi.orient_reference(batch, codes, layout=layout, dtype=dtype)
        assert got.shape == batch.shape and got.dtype == batch.dtype
        assert np.array_equal(bits_of(got), want), (dtype, layout, ow, oh, c)
        # ... and with out == batch
        twice = batch.copy()
        u8 = (C.c_uint8 * len(codes))(*codes)
        rc = mi._lib.load().llcomp_mi_orient_reference(twice.ctypes.data, len(codes), c, ow, oh, mi._dtype_code(dtype), mi._layout_code(layout), u8,
                                                       twice.ctypes.data)
        assert rc == mi.OK and np.array_equal(bits_of(twice), want), (dtype, layout, ow, oh, c, "in place")


@pytest.mark.parametrize("c", (1, 3))
def test_reference_is_pil_transpose(mi, c):
    from PIL import Image

    for ow, oh in ((5, 5), (7, 5), (1, 4), (2, 2)):
        codes = [k for k in range(1, 8) if ow == oh or k not in orient_spec.TRANSPOSING]
        batch = orient_spec.gen_batch("uint8", len(codes), c, oh, ow, "hwc", seed=ow)
        got = mi.orient_reference(batch, codes, layout="hwc")
        for i, code in enumerate(codes):
            img = Image.fromarray(batch[i, :, :, 0] if c == 1 else batch[i])
            want = np.asarray(img.transpose(Image.Transpose(code - 1))).reshape(oh, ow, c)
            assert np.array_equal(got[i], want), (ow, oh, c, code)


def test_group_laws(mi):
    x = orient_spec.gen_batch("float32", 1, 3, 5, 5, "chw", seed=11)

    def turn(a, *codes):
        for code in codes:
            a = mi.orient_reference(a, [code])
        return bits_of(a)

    for code in (1, 2, 4, 6, 7):
        assert np.array_equal(turn(x, code, code), bits_of(x)), code
        assert not np.array_equal(turn(x, code), bits_of(x)), code
    assert np.array_equal(turn(x, 3, 3, 3, 3), bits_of(x))
    assert np.array_equal(turn(x, 3, 5), bits_of(x)) and np.array_equal(turn(x, 3, 3), turn(x, 4))
    assert np.array_equal(turn(x, 6, 1), turn(x, 5))  # TRANSPOSE then FLIP_LEFT_RIGHT is ROTATE_270 ...
    assert np.array_equal(bits_of(np.flip(np.swapaxes(x[0], 1, 2), 2)), bits_of(np.rot90(x[0], 3, (1, 2))))  # ... as numpy says it is


def test_refusals_leave_out_untouched(mi):
    L = mi._lib.load()
    n, c, ow, oh = 3, 3, 4, 4
    batch = orient_spec.gen_batch("float32", n, c, oh, ow, "chw", seed=2)
    out = np.full(batch.shape, 7.0, np.float32)

    def u8(*v):
        return (C.c_uint8 * len(v))(*v)

    ok = u8(1, 3, 0)
    b, o = batch.ctypes.data, out.ctypes.data
    flat = orient_spec.gen_batch("float32", n, c, 3, 4, "chw", seed=2)  # 4 x 3: not square
    cases = [(None, n, c, ow, oh, 1, 1, ok, o), (b, n, c, ow, oh, 1, 1, None, o), (b, n, c, ow, oh, 1, 1, ok, None), (b, 0, c, ow, oh, 1, 1, ok, o),
             (b, 65536, c, ow, oh, 1, 1, ok, o), (b, n, c, 0, oh, 1, 1, ok, o), (b, n, c, ow, 0, 1, 1, ok, o), (b, n, 0, ow, oh, 1, 1, ok, o),
             (b, n, c, ow, oh, 4, 1, ok, o), (b, n, c, ow, oh, 1, 2, ok, o), (b, n, c, ow, oh, 1, 1, u8(0, 8, 0), o), (b, n, c, ow, oh, 1, 1, u8(0, 0, 255), o)]
    cases += [(flat.ctypes.data, n, c, 4, 3, 1, 1, u8(1, code, 2), o) for code in orient_spec.TRANSPOSING]
    for args in cases:
        assert L.llcomp_mi_orient_reference(*args) == mi.BAD_ARGS, args[1:7]
    assert (out == 7.0).all()
    assert L.llcomp_mi_orient_reference(flat.ctypes.data, n, c, 4, 3, 1, 1, u8(1, 4, 2), o) == mi.OK  # the codes that keep the shape
    assert L.llcomp_mi_orient_reference(b, n, c, ow, oh, 1, 1, ok, o) == mi.OK
    assert np.array_equal(bits_of(out), bits_of(orient_spec.apply(batch, [1, 3, 0], "chw")))
    for bad in ([0, 8, 0], [0, 0], "sideways", [None, "rotate_45", 0]):
        with pytest.raises(mi.LlcompError) as e:
            mi.orient_reference(batch, bad)
        assert e.value.status == mi.BAD_ARGS
    with pytest.raises(mi.LlcompError):
        mi.orient_reference(batch[0], [1])  # not 4-D
    with pytest.raises(mi.LlcompError):
        mi.orient_reference(batch, [1, 1, 1], layout="nchw")


def test_orient_code_names(mi):
    from PIL import Image

    assert mi.orient_code(None) == mi.orient_code("none") == mi.orient_code("NONE") == mi.ORIENT_NONE == 0
    for method in Image.Transpose:  # PIL's names, in any letter case, and its values plus 1
        for name in (method.name, method.name.lower(), method.name.title()):
            assert mi.orient_code(name) == method.value + 1 == getattr(mi, "ORIENT_" + method.name), name
        assert mi.orient_code(method.value + 1) == method.value + 1
    assert mi.ORIENT_NAMES == orient_spec.NAMES and len(Image.Transpose) == 7
    for bad in ("rotate_45", 8, -1, 1.0, True, b"transpose"):
        with pytest.raises(mi.LlcompError) as e:
            mi.orient_code(bad)
        assert e.value.status == mi.BAD_ARGS
    assert mi.orient_tile() == mi._lib.load().llcomp_mi_orient_tile() >= 8
