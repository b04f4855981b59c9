"""The rule of the batch mixing on the host (include/llcomp_mi.h: "Batch mixing"): llcomp_mi_mix_reference -- compiled from the functions
the GPU's kernels are compiled from -- against tests/mix_spec.py, torchvision's and timm's expressions run by torch on the CPU.  Every
comparison is of the elements' bit patterns over the whole batch."""
import ctypes as C
import random

import numpy as np
import pytest

import mix_spec
from mix_batches import Case, bits_of, to_layout

FLOATS = ("float32", "float16", "bfloat16")
LAMS = (0.0, 1.0, 0.5, 0.3712345678901234)


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


def run(mi, batch, case, layout, in_place=False):
    """mix_reference on the torch batch [n, c, h, w] in the layout -> bits; in_place: through the C call with out = batch"""
    a = to_layout(batch, layout)
    name = {v: k for k, v in mix_spec.DTYPES.items()}[batch.dtype]
    n = len(batch)
    if not in_place:
        return bits_of(mi.mix_reference(a, case.samples(mi, n), layout=layout, erase_value=case.erase_value, dtype=name))
    c, h, w = batch.shape[1:]
    a = a.copy()
    ev = None if case.erase_value is None else (C.c_float * c)(*([case.erase_value] * c if isinstance(case.erase_value, (int, float)) else case.erase_value))
    rc = mi._lib.load().llcomp_mi_mix_reference(a.ctypes.data, n, c, w, h, mi._dtype_code(name), 1 if layout == "chw" else 0, case.samples(mi, n), ev,
                                                a.ctypes.data)
    assert rc == 0
    return bits_of(a)


def check(mi, batch, case, layout="chw"):
    want = case.expected(batch, layout)
    for in_place in (False, True):
        got = run(mi, batch, case, layout, in_place)
        assert got.shape == want.shape and np.array_equal(got, want), (case, batch.dtype, layout, in_place, int((got != want).sum()))


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("layout", ("chw", "hwc"))
def test_mixup_is_torchs_bits(mi, dtype, layout):
    """roll, flip (even and odd n) and a seeded permutation, every lam of the issue, c = 1 and 3, inputs with +-0, the largest finite
    value (float16: the blend can overflow to inf), subnormals"""
    rng = random.Random(11)
    for c in (1, 3):
        for n, partner in ((4, "roll"), (4, "flip"), (5, "flip"), (1, "roll"), (7, None)):
            batch = mix_spec.gen_batch(dtype, n, c, 5, 7, seed=100 * n + c)
            if partner is None:
                partner = list(range(n))
                rng.shuffle(partner)
            for lam in LAMS:
                check(mi, batch, Case(partner, lam), layout)
    big = mix_spec.from_bits(np.full((2, 1, 2, 2), 0x7BFF, np.uint16), "float16")  # 65504 everywhere
    out = mi.mix_reference(to_layout(big, "chw"), mi.mix_samples(2, "roll", 0.3712345678901234))
    assert np.array_equal(bits_of(out), Case("roll", 0.3712345678901234).expected(big, "chw"))


@pytest.mark.parametrize("dtype", FLOATS)
def test_per_sample_lam(mi, dtype):
    batch = mix_spec.gen_batch(dtype, 6, 3, 4, 6, seed=7)
    check(mi, batch, Case("roll", [0.25, None, 1.0, 0.0, 0.3712345678901234, 0.9]))
    check(mi, batch, Case([1, 0, 3, 2, 5, 4], [0.5, 0.5, None, 0.1, 0.7, None]), "hwc")


@pytest.mark.parametrize("dtype", FLOATS + ("uint8",))
@pytest.mark.parametrize("layout", ("chw", "hwc"))
def test_cutmix_and_erase(mi, dtype, layout):
    """boxes empty, of one pixel, the whole picture and at every edge; the same for erase, with one value and with one per channel"""
    w, h = 9, 6
    rects = [None, (0, 0, 0, 3), (4, 2, 1, 1), (0, 0, w, h), (0, 0, 3, 2), (w - 2, h - 3, 2, 3), (0, h - 1, w, 1), (w - 1, 0, 1, h)]
    n = len(rects)
    for c in (1, 3):
        batch = mix_spec.gen_batch(dtype, n, c, h, w, seed=31 + c)
        values = (None, 3.0, [1.0, 0.0, 254.0][:c]) if dtype == "uint8" else (None, 0.4914, [0.1, -2.1179039478302, 1e-7][:c])
        for partner in ("roll", "flip"):
            check(mi, batch, Case(partner, boxes=rects), layout)
        check(mi, batch, Case("roll", boxes=(2, 1, 4, 3)), layout)
        for value in values:
            check(mi, batch, Case(None, erase=rects, erase_value=value), layout)
            check(mi, batch, Case("roll", erase=rects[::-1], erase_value=value, boxes=rects), layout)


@pytest.mark.parametrize("dtype", FLOATS)
def test_everything_on_one_sample(mi, dtype):
    """erase, box and blend together: the partner's erase shows through the box and in the blend"""
    batch = mix_spec.gen_batch(dtype, 4, 3, 8, 10, seed=5)
    case = Case("roll", lam=[0.3, None, 0.8, 0.5], boxes=[(1, 1, 5, 4), (0, 0, 10, 8), None, (6, 3, 4, 5)],
                erase=[(3, 2, 4, 4), (0, 0, 2, 2), (5, 5, 5, 3), None], erase_value=[0.5, -1.0, 2.25])
    for layout in ("chw", "hwc"):
        check(mi, batch, case, layout)


def test_refusals_leave_the_output_untouched(mi):
    L = mi._lib.load()
    n, c, w, h = 3, 3, 4, 2
    src = np.arange(n * c * w * h, dtype=np.float32)

    def call(samples, dtype=1, layout=1, ev=None, n_=n, c_=c, w_=w, h_=h, batch=True, out_ok=True, recs=True):
        out = np.full(src.size, 7, np.float32)
        rc = L.llcomp_mi_mix_reference(src.ctypes.data if batch else None, n_, c_, w_, h_, dtype, layout, samples if recs else None,
                                       None if ev is None else (C.c_float * len(ev))(*ev), out.ctypes.data if out_ok else None)
        assert (out == 7).all() or rc == 0
        return rc

    good = mi.mix_samples(n, "roll", 0.5)
    assert call(good) == 0
    for kw in (dict(batch=False), dict(out_ok=False), dict(recs=False), dict(n_=0), dict(c_=0), dict(w_=0), dict(h_=0), dict(dtype=4), dict(layout=2),
               dict(ev=[float("nan"), 0, 0]), dict(ev=[0, float("inf"), 0]), dict(dtype=0), dict(dtype=0, ev=[0.5, 0, 0]),
               dict(dtype=0, ev=[256.0, 0, 0]), dict(dtype=0, ev=[-1.0, 0, 0])):
        s = mi.mix_samples(n, "roll") if kw.get("dtype") == 0 and "ev" in kw else good
        assert call(s, **kw) == mi.BAD_ARGS, kw

    def bad(edit):
        s = mi.mix_samples(n, "roll", 0.5)
        edit(s)
        return call(s)

    def set_(i, field, value):
        def f(s):
            if isinstance(value, tuple):
                getattr(s[i], field)[:] = value
            else:
                setattr(s[i], field, value)
        return f

    for edit in (set_(0, "partner", n), set_(1, "partner", 2), set_(0, "flags", 2), set_(0, "flags", 0x80000001), set_(2, "w_own", float("inf")),
                 set_(2, "w_partner", float("nan")), set_(0, "box", (0, 0, w + 1, 1)), set_(0, "box", (w, 0, 1, 1)), set_(0, "box", (0, 1, 1, h)),
                 set_(1, "erase", (1, 0, w, 1)), set_(1, "erase", (0, h, 1, 1)), set_(1, "erase", (0xFFFFFFFF, 0, 2, 1))):
        assert bad(edit) == mi.BAD_ARGS
    assert bad(set_(0, "box", (w + 5, h + 5, 0, 0))) == 0  # (an empty rectangle is none, wherever it is)
    assert call(mi.mix_samples(n, "roll"), dtype=0, ev=[255.0, 0.0, 7.0]) == 0
    with pytest.raises(mi.LlcompError):
        mi.mix_reference(src.reshape(n, c, h, w), mi.mix_samples(n + 1, "roll"))
    with pytest.raises(mi.LlcompError):
        mi.mix_samples(3, "spin")
