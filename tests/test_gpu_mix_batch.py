"""Batch mixing on the GPU (llcomp_mi_codec_mix_batch; include/llcomp_mi.h: "Batch mixing"): RandomErasing, MixUp and CutMix in place on
a dense batch in HBM, against tests/mix_spec.py -- torchvision's and timm's expressions run by torch on the CPU -- bit for bit over the
whole batch, with guard bytes on both sides of it.  The batches are filled from torch directly; one case runs behind decode_views."""
import random

import numpy as np
import pytest

import mix_spec
from batch_support import DTYPES, ESIZE, NP_NAME, bits_of, guards_intact, mi, put, stream  # noqa: F401
from mix_batches import Case, to_layout

pytestmark = pytest.mark.gpu

LAM = 0.3712345678901234
# (ow, oh, c): the smallest batch element; no whole 16-byte chunk; E * esize no multiple of 16; chunks that straddle rows; whole chunks
# only; the general case
SHAPES = ((1, 1, 1), (3, 1, 3), (5, 3, 3), (7, 5, 1), (8, 2, 1), (33, 9, 3))


@pytest.fixture(scope="module")
def codecs(mi):
    made = {c: mi.Codec(1, 32, 16, c, 32, 16, False, device=0) for c in (1, 3)}
    yield made
    for k in made.values():
        k.close()


def run(mi, codec, batch, case, layout, offset=0, samples=None, expect_error=False):
    """mix_batch on the torch batch [n, c, h, w] in the layout, `offset` elements past a 256-byte boundary -> the batch's bits after
    the call; the bytes around it have to be untouched"""
    import torch

    name = {v: k for k, v in mix_spec.DTYPES.items()}[batch.dtype]
    raw = to_layout(batch, layout)
    n, (c, h, w) = len(batch), batch.shape[1:]
    buf, lo = put(raw, offset * ESIZE[name])
    err = None
    try:
        codec.mix_batch(buf.data_ptr() + lo, n, w, h, case.samples(mi, n) if samples is None else samples, dtype=name, layout=layout,
                        erase_value=case.erase_value, stream=stream())
    except mi.LlcompError as e:
        err = e
    torch.cuda.synchronize()
    assert (err is not None) == expect_error, err
    host = buf.cpu().numpy()
    assert guards_intact(host, lo, raw.nbytes), "a byte outside the batch was written"
    return bits_of(host[lo:lo + raw.nbytes].copy().view(NP_NAME[name]).reshape(raw.shape))


def check(mi, codecs, batch, case, layout, offset=0):
    got = run(mi, codecs[batch.shape[1]], batch, case, layout, offset)
    want = case.expected(batch, layout)
    assert np.array_equal(got, want), (case, batch.dtype, tuple(batch.shape), layout, offset, np.argwhere(got != want)[:4].tolist())


def mixed_case(dtype, w, h):
    """sample 0 blends (uint8: takes a box), sample 1 takes a box only, sample 2 is erased only, sample 3 stays as it is"""
    box = (w // 2, 0, w - w // 2, max(1, h // 2))
    blend = dtype != "uint8"
    return Case([1, 0, 2, 3], lam=[LAM, None, None, None] if blend else None, boxes=[None if blend else (0, h - 1, w, 1), box, None, None],
                erase=[None, None, (0, 0, max(1, w - 1), h), None], erase_value=[3.0, 0.0, 200.0] if dtype == "uint8" else [0.25, -1.5, 1e-6])


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_shape_offset_and_layout(mi, codecs, dtype):
    for si, (w, h, c) in enumerate(SHAPES):
        batch = mix_spec.gen_batch(dtype, 4, c, h, w, seed=si)
        case = mixed_case(dtype, w, h)
        case.erase_value = case.erase_value[:c]
        for layout in ("chw", "hwc"):
            for offset in (0, 1, 3):
                check(mi, codecs, batch, case, layout, offset)


@pytest.mark.parametrize("dtype", DTYPES[1:])
def test_signed_zeros_and_the_largest_finite_value(mi, codecs, dtype):
    """-0 blended with -0 stays -0 (a fused multiply-add with an addend of +0 would make it +0), +0 with -0 is +0, and the largest
    finite value blended with itself may round up to inf: whatever torch gives"""
    neg0, top = {"float32": (0x80000000, 0x7F7FFFFF), "float16": (0x8000, 0x7BFF), "bfloat16": (0x8000, 0x7F7F)}[dtype]
    rows = np.array([[neg0] * 8, [neg0] * 4 + [0] * 4, [top] * 8, [top] * 4 + [top | neg0] * 4, [0] * 8, [neg0, 0] * 4], np.uint64)
    batch = mix_spec.from_bits(rows.reshape(6, 1, 1, 8), dtype)
    for lam in (LAM, 0.5, 0.0, 1.0):
        check(mi, codecs, batch, Case("roll", lam), "chw")
        check(mi, codecs, batch, Case("flip", lam), "hwc", 1)


def test_roll_on_either_side_of_the_segment_length(mi, codecs):
    """one cycle of n samples: whole in one segment up to S, cut and with saved heads above -- blended, with boxes, and with the partner's
    erase rectangle showing through a saved head; in the aligned and in the element-by-element path"""
    S = mi.mix_segment()
    boxes = (1, 0, 3, 1)
    for n in (1, 2, 3, S, S + 1, 2 * S + 1):
        assert mi.mix_plan(mi.mix_samples(n, "roll"))[2] == (0 if n <= S else -(-n // S))
        for (w, h, c), dtype, layout, offset in (((33, 9, 3), "float16", "chw", 0), ((5, 3, 3), "float32", "hwc", 1), ((8, 2, 1), "bfloat16", "chw", 3),
                                                 ((8, 2, 1), "float32", "chw", 0), ((7, 5, 1), "uint8", "hwc", 1)):
            batch = mix_spec.gen_batch(dtype, n, c, h, w, seed=n)
            erase = [(0, 0, 2, 1) if i % 2 == 0 else None for i in range(n)]
            if dtype != "uint8":
                check(mi, codecs, batch, Case("roll", LAM), layout, offset)
                check(mi, codecs, batch, Case("roll", LAM, boxes=boxes, erase=erase, erase_value=0.5), layout, offset)
            check(mi, codecs, batch, Case("roll", boxes=boxes, erase=erase, erase_value=7.0), layout, offset)


@pytest.mark.parametrize("dtype", DTYPES)
def test_flip_and_a_seeded_permutation(mi, codecs, dtype):
    S = mi.mix_segment()
    rng = random.Random(17)
    lam = None if dtype == "uint8" else 0.5
    box = None if lam is not None else (0, 0, 17, 4)
    for n in (5, 2 * S + 5):
        batch = mix_spec.gen_batch(dtype, n, 3, 9, 33, seed=40 + n)
        check(mi, codecs, batch, Case("flip", lam, boxes=box), "chw")  # odd n: the middle sample is its own partner
        perm = list(range(n))
        rng.shuffle(perm)
        check(mi, codecs, batch, Case(perm, lam, boxes=box), "hwc", 1)
        lams = None if dtype == "uint8" else [rng.choice([None, 0.0, 1.0, LAM, rng.random()]) for _ in range(n)]
        boxes = [rng.choice([None, (rng.randrange(30), rng.randrange(8), 3, 1)]) for _ in range(n)]
        check(mi, codecs, batch, Case(perm, lams, boxes=boxes, erase=boxes[::-1], erase_value=1.0), "chw", 3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ("chw", "hwc"))
def test_rectangles_at_the_edges_and_on_chunk_boundaries(mi, codecs, dtype, layout):
    w, h, c = 33, 9, 3
    per = 16 // ESIZE[dtype]
    rects = [(0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, 1, 1), (0, 0, w, 1), (0, h - 1, w, 1), (0, 0, 1, h), (w - 1, 0, 1, h), (per, 1, per, 2),
             (per - 1, 0, 2, h), (2 * per, 3, w - 2 * per, 1), (0, 4, per, 5), None]
    n = len(rects)
    batch = mix_spec.gen_batch(dtype, n, c, h, w, seed=3)
    value = [255.0, 0.0, 17.0] if dtype == "uint8" else [0.485, -0.456, 65504.0]
    lam = None if dtype == "uint8" else LAM
    check(mi, codecs, batch, Case("roll", boxes=rects), layout)
    check(mi, codecs, batch, Case(None, erase=rects, erase_value=value), layout)
    check(mi, codecs, batch, Case("roll", lam, boxes=rects, erase=rects[3:] + rects[:3], erase_value=value), layout, 1)


def test_refusals_leave_the_batch_as_it_is(mi, codecs):
    n, c, w, h = 4, 3, 5, 3
    batch = mix_spec.gen_batch("float32", n, c, h, w, seed=9)
    before = bits_of(to_layout(batch, "chw"))
    edits = [("partner", 0, n), ("partner", 1, 2), ("flags", 0, 2), ("w_own", 2, float("nan")), ("w_partner", 2, float("inf")),
             ("box", 0, (0, 0, w + 1, 1)), ("box", 3, (w, 0, 1, 1)), ("erase", 1, (0, h - 1, 1, 2)), ("erase", 1, (4, 0, 0xFFFFFFFF, 1))]
    for field, i, value in edits:
        s = mi.mix_samples(n, "roll", 0.5)
        if isinstance(value, tuple):
            getattr(s[i], field)[:] = value
        else:
            setattr(s[i], field, value)
        assert np.array_equal(run(mi, codecs[c], batch, Case(), "chw", samples=s, expect_error=True), before), (field, value)
    ok = mi.mix_samples(n, "roll", 0.5)
    for value in ([float("nan"), 0, 0], [0, float("-inf"), 0]):
        assert np.array_equal(run(mi, codecs[c], batch, Case(erase_value=value), "chw", samples=ok, expect_error=True), before)
    u8 = mix_spec.gen_batch("uint8", n, c, h, w, seed=9)
    for samples, value in ((ok, None), (mi.mix_samples(n, "roll"), [0.5, 0, 0]), (mi.mix_samples(n, "roll"), [256.0, 0, 0])):  # BLEND on U8; no u8 values
        assert np.array_equal(run(mi, codecs[c], u8, Case(erase_value=value), "hwc", samples=samples, expect_error=True), bits_of(to_layout(u8, "hwc")))
    k, L = codecs[c], mi._lib.load()
    import torch

    buf = torch.zeros(n * c * w * h + 4, dtype=torch.float32, device="cuda")
    for args in ((None, buf.data_ptr(), n, w, h, 1, 1, ok), (k._h, None, n, w, h, 1, 1, ok), (k._h, buf.data_ptr(), n, w, h, 1, 1, None),
                 (k._h, buf.data_ptr(), 0, w, h, 1, 1, ok), (k._h, buf.data_ptr(), n, 0, h, 1, 1, ok), (k._h, buf.data_ptr(), n, w, 0, 1, 1, ok),
                 (k._h, buf.data_ptr(), n, w, h, 4, 1, ok), (k._h, buf.data_ptr(), n, w, h, 1, 2, ok), (k._h, buf.data_ptr() + 2, n, w, h, 1, 1, ok),
                 (k._h, buf.data_ptr() + 1, n, w, h, 2, 1, ok)):
        assert L.llcomp_mi_codec_mix_batch(*args, None, stream()) == mi.BAD_ARGS, args[2:7]
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any()
    # ... and a call that is fine, on the same buffers
    check(mi, codecs, batch, Case("roll", 0.5), "chw")
    assert codecs[c].allocated_bytes() <= codecs[c].mix_workspace_bytes(2 * mi.mix_segment() + 5, 33, 9, "float32")


def test_behind_decode_views_on_the_same_stream(mi, orc):
    """decode_views into a float16 CHW group, mix_batch behind it on the stream with roll and lam 0.3: the spec applied to what
    decode_views alone writes"""
    import torch

    import photo_gpu

    try:
        c, h, _imgs, _conts, dev, codec = photo_gpu.setup(mi, orc, "100x44_32x16i_c3")
        ow, oh = 24, 16
        groups = [photo_gpu.PG(photo_gpu.views_of(h), ow, oh, dtype="float16", layout="chw")]
        n = len(groups[0].views)
        st, (plain,) = photo_gpu.run(mi, codec, groups, c, dev=dev)
        assert st == 0 and plain.shape == (n, c, oh, ow) and plain.dtype == np.float16
        (out,) = photo_gpu.run(mi, codec, groups, c, dev=dev, read=False)
        codec.mix_batch(out.ptr, n, ow, oh, mi.mix_samples(n, "roll", 0.3), dtype="float16", layout="chw", stream=stream())
        st, got = out.read()
        want = Case("roll", 0.3).expected(torch.from_numpy(plain.copy()), "chw")
        assert st == 0 and np.array_equal(bits_of(got), want)
        assert not np.array_equal(bits_of(got), bits_of(plain))
    finally:
        photo_gpu.close_shared_codecs()
