"""Batch orientation on the GPU (llcomp_mi_codec_orient_batch; include/llcomp_mi.h: "Batch orientation"): flips, quarter turns and
transpositions per sample in place on a dense batch in HBM, against tests/orient_spec.py -- numpy's flip, rot90 and transposition -- bit
for bit over the whole batch, with guard bytes on both sides of it.  The batches are filled from torch directly; one case runs behind
decode_resized_regions.  T = llcomp_mi_orient_tile() sizes the shapes: a sample smaller than a tile, one tile exactly, a tile and a
pixel (the tile that straddles the middle, the diagonal, the centre pixel), two tiles and a pixel."""
import ctypes as C

import numpy as np
import pytest

import orient_spec
from batch_support import DTYPES, ESIZE, bits_of, guards_intact, mi, put, stream  # noqa: F401

pytestmark = pytest.mark.gpu

ALL_CODES = [0, 1, 2, 3, 4, 5, 6, 7, 3]  # every code, and a second ROTATE_90
KEEPING = [0, 1, 2, 4]                   # the codes that keep the shape of a sample that is not square


@pytest.fixture(scope="module")
def codecs(mi):
    made = {c: mi.Codec(1, 32, 16, c, 32, 16, False, device=0) for c in (1, 3, 5)}
    yield made
    for k in made.values():
        k.close()


def run(mi, codec, batch, codes, dtype, layout, offset=0, expect_error=False, **kw):
    """orient_batch on the numpy batch ([n, c, h, w] or [n, h, w, c] by the layout), `offset` elements past a 256-byte boundary -> the
    batch's bits after the call; the bytes around it have to be untouched.  kw replaces arguments of the call (the refusals;
    call_dtype and call_layout replace the call's, the batch keeps its own)."""
    import torch

    n = len(batch)
    (c, h, w) = batch.shape[1:] if layout == "chw" else (batch.shape[3], batch.shape[1], batch.shape[2])
    buf, lo = put(batch, offset * ESIZE[dtype])
    args = dict(d_batch=buf.data_ptr() + lo, n=n, ow=w, oh=h, codes=codes, dtype=dtype, layout=layout, stream=stream())
    args.update({name[5:] if name.startswith("call_") else name: v for name, v in kw.items()})
    err = None
    try:
        codec.orient_batch(**args)
    except mi.LlcompError as e:
        err = e
    torch.cuda.synchronize()
    assert (err is not None) == expect_error, err
    assert err is None or err.status == mi.BAD_ARGS
    host = buf.cpu().numpy()
    assert guards_intact(host, lo, batch.nbytes), "a byte outside the batch was written"
    return bits_of(host[lo:lo + batch.nbytes].copy().view(batch.dtype).reshape(batch.shape))


def check(mi, codecs, dtype, layout, c, w, h, codes, offset=0, seed=0):
    batch = orient_spec.gen_batch(dtype, len(codes), c, h, w, layout, seed)
    got = run(mi, codecs[c], batch, codes, dtype, layout, offset)
    want = bits_of(orient_spec.apply(batch, codes, layout))
    assert np.array_equal(got, want), (dtype, layout, c, w, h, codes, offset, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("c", (1, 3))
@pytest.mark.parametrize("layout", ("chw", "hwc"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_square_sides_around_the_tile_every_code_in_one_call(mi, codecs, dtype, layout, c):
    T = mi.orient_tile()
    for side in (1, 2, 3, T - 1, T, T + 1, 2 * T + 1):
        check(mi, codecs, dtype, layout, c, side, side, ALL_CODES, seed=side)


@pytest.mark.parametrize("c", (1, 3))
@pytest.mark.parametrize("layout", ("chw", "hwc"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_shapes_that_are_not_square(mi, codecs, dtype, layout, c):
    T = mi.orient_tile()
    for w, h in ((3, 1), (1, 3), (5, 3), (2 * T + 3, 7), (7, 2 * T + 3)):
        check(mi, codecs, dtype, layout, c, w, h, KEEPING, seed=w)


@pytest.mark.parametrize("dtype", DTYPES)
def test_batches_at_any_element_address(mi, codecs, dtype):
    """HWC with c = 3 puts 3-, 6- and 12-byte pixels at every alignment: no row starts where a 16-byte access may"""
    T = mi.orient_tile()
    for offset in (1, 3, 5):
        check(mi, codecs, dtype, "hwc", 3, 2 * T + 1, 2 * T + 1, ALL_CODES, offset, seed=offset)
        check(mi, codecs, dtype, "hwc", 3, 5, 3, KEEPING, offset, seed=offset)
        check(mi, codecs, dtype, "chw", 1, 5, 3, KEEPING, offset, seed=offset)


@pytest.mark.parametrize("dtype", ("uint8", "float32"))
def test_pixels_longer_than_a_piece(mi, codecs, dtype):
    """five channels in HWC: a float32 pixel is 20 bytes and moves in two pieces, a workgroup each; a uint8 pixel of 5 bytes moves whole"""
    T = mi.orient_tile()
    for side in (3, T + 1):
        check(mi, codecs, dtype, "hwc", 5, side, side, ALL_CODES, seed=side)
        check(mi, codecs, dtype, "chw", 5, side, side, ALL_CODES, seed=side)
    check(mi, codecs, dtype, "hwc", 5, T + 3, 7, KEEPING, 1)


def test_all_codes_zero_changes_nothing(mi, codecs):
    for dtype, layout in (("float16", "chw"), ("uint8", "hwc")):
        batch = orient_spec.gen_batch(dtype, 4, 3, 9, 9, layout, seed=4)
        assert np.array_equal(run(mi, codecs[3], batch, [0, 0, 0, 0], dtype, layout), bits_of(batch))
        assert np.array_equal(run(mi, codecs[3], batch, None, dtype, layout, 1), bits_of(batch))


def test_refusals_leave_the_batch_as_it_is(mi, codecs):
    import torch

    n, c, w, h = 4, 3, 5, 5
    batch = orient_spec.gen_batch("float32", n, c, h, w, "chw", seed=9)
    before = bits_of(batch)
    k, L = codecs[c], mi._lib.load()
    for kw in (dict(codes=[0, 8, 0, 0]), dict(codes=[0, 0, 0, 255]), dict(codes=[1, 2, 3]), dict(n=0), dict(n=65536), dict(ow=0), dict(oh=0),
               dict(call_dtype=4), dict(call_layout=2), dict(call_layout="nchw"), dict(codes="rotate_45")):
        codes = kw.pop("codes", [1, 2, 3, 4])
        assert np.array_equal(run(mi, k, batch, codes, "float32", "chw", expect_error=True, **kw), before), (codes, kw)
    flat = orient_spec.gen_batch("float32", n, c, 3, 5, "chw", seed=9)
    for code in orient_spec.TRANSPOSING:  # 5 x 3: a transposing code would change the shape
        assert np.array_equal(run(mi, k, flat, [1, 2, code, 4], "float32", "chw", expect_error=True), bits_of(flat)), code
    buf = torch.zeros(n * c * w * h + 4, dtype=torch.float32, device="cuda")
    ok = (C.c_uint8 * n)(1, 2, 3, 4)
    for args in ((None, buf.data_ptr(), n, w, h, 1, 1, ok), (k._h, None, n, w, h, 1, 1, ok), (k._h, buf.data_ptr(), n, w, h, 1, 1, None),
                 (k._h, buf.data_ptr(), 0, w, h, 1, 1, ok), (k._h, buf.data_ptr(), n, 0, h, 1, 1, ok), (k._h, buf.data_ptr(), n, w, 0, 1, 1, ok),
                 (k._h, buf.data_ptr(), n, w, h, 4, 1, ok), (k._h, buf.data_ptr(), n, w, h, 1, 2, ok), (k._h, buf.data_ptr() + 2, n, w, h, 1, 1, ok),
                 (k._h, buf.data_ptr() + 1, n, w, h, 2, 1, ok), (k._h, buf.data_ptr(), n, w, h, 1, 1, (C.c_uint8 * n)(0, 0, 8, 0)),
                 (k._h, buf.data_ptr(), n, w, h + 1, 1, 1, ok)):
        assert L.llcomp_mi_codec_orient_batch(*args, stream()) == mi.BAD_ARGS, args[2:7]
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any()
    # ... and a call that is fine, on the same codec
    check(mi, codecs, "float32", "chw", c, w, h, [1, 2, 3, 4])
    assert k.allocated_bytes() <= k.orient_workspace_bytes(9)
    assert k.orient_workspace_bytes(9) == L.llcomp_mi_codec_workspace_bytes(k._h) + 8 * 9


def test_behind_decode_resized_regions_on_the_same_stream(mi, orc):
    """decode_resized_regions of 4 frames, orient_batch behind it on the stream with codes 2, 3, 0, 7: the spec applied to what the decode
    alone writes -- float16 CHW -- and, for U8 HWC, PIL's crop.resize((ow, oh), BILINEAR).transpose(code - 1)"""
    from PIL import Image

    from test_gpu_regions_host import make_batch
    from test_gpu_resized_output import TOut
    from test_gpu_resized_regions import packed

    frames, w, h, c, ow, oh = 4, 100, 44, 3, 24, 24
    codes = [2, 3, 0, 7]
    rects = [(0, 0, 100, 44), (10, 4, 50, 40), (37, 11, 24, 24), (60, 0, 33, 17)]
    imgs, conts = make_batch(orc, frames, w, h, c, 32, 16, False)
    codec = mi.Codec(frames, w, h, c, 32, 16, False, device=0)
    try:
        d_pay, n_pay, d_len = packed(mi, conts)
        for dtype, layout, kw in (("float16", "chw", dict(scale=True, mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])), ("uint8", "hwc", {})):
            outs = []
            for oriented in (False, True):
                o = TOut(frames, ow, oh, c, dtype, layout)
                codec.decode_resized_regions(d_pay.data_ptr(), n_pay, d_len.data_ptr(), rects, ow, oh, o.ptr, o.st.data_ptr(), stream=stream(),
                                             dtype=dtype, layout=layout, filter="bilinear", **kw)
                if oriented:
                    codec.orient_batch(o.ptr, frames, ow, oh, codes, dtype=dtype, layout=layout, stream=stream())
                st, got = o.read()
                assert st == 0
                outs.append(got)
            plain, got = outs
            assert np.array_equal(bits_of(got), bits_of(orient_spec.apply(plain, codes, layout))), (dtype, layout)
            assert not np.array_equal(bits_of(got), bits_of(plain))
            if dtype == "uint8":
                for f, ((x, y, rw, rh), code) in enumerate(zip(rects, codes)):
                    img = Image.fromarray(np.ascontiguousarray(imgs[f, y:y + rh, x:x + rw])).resize((ow, oh), Image.Resampling.BILINEAR)
                    want = np.asarray(img.transpose(Image.Transpose(code - 1)) if code else img)
                    assert np.array_equal(got[f], want), (f, code)
    finally:
        codec.close()
