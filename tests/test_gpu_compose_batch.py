"""Batch composition on the GPU (llcomp_mi_codec_compose_batch; include/llcomp_mi.h: "Batch composition"): rectangles of a src batch
into a dst batch in HBM, against tests/compose_spec.py -- numpy's slice assignments in list order -- bit for bit over the whole dst
batch, with 256 guard bytes on both sides of dst that have to stay and a src batch that has to be byte-identical after the call.  The
batches are filled from torch directly; one case runs behind decode_resized_regions.  T = compose_tile() and R = compose_tile(pixel
bytes), the kernel's tile, size the shapes."""
import ctypes as C

import numpy as np
import pytest

import compose_spec
from batch_support import DTYPES, ESIZE, bits_of, guards_intact, mi, put, stream  # noqa: F401
from compose_spec import FILL

pytestmark = pytest.mark.gpu



@pytest.fixture(scope="module")
def codecs(mi):
    made = {c: mi.Codec(1, 32, 16, c, 32, 16, False, device=0) for c in (1, 3, 5)}
    yield made
    for k in made.values():
        k.close()


def run(mi, codec, src, dst, pieces, dtype, layout, fill=None, keep=False, src_offset=0, dst_offset=0, expect_error=False, **kw):
    """compose_batch on the numpy batches ([n, c, h, w] or [n, h, w, c] by the layout; src None: no src batch), each `offset` elements
    past a 256-byte boundary -> dst's bits after the call; the guard bytes and the src batch have to be untouched.  kw replaces
    arguments of the call (the refusals; call_dtype and call_layout replace the call's, the batches keep their own)."""
    import torch

    es = ESIZE[dtype]
    (c, oh, ow) = dst.shape[1:] if layout == "chw" else (dst.shape[3], dst.shape[1], dst.shape[2])
    dbuf, dlo = put(dst, dst_offset * es)
    args = dict(d_src=None, n_src=0, iw=0, ih=0, d_dst=dbuf.data_ptr() + dlo, n_dst=len(dst), ow=ow, oh=oh, pieces=pieces, dtype=dtype, layout=layout,
                fill=fill, keep=keep, stream=stream())
    if src is not None:
        sbuf, slo = put(src, src_offset * es)
        (ih, iw) = src.shape[2:] if layout == "chw" else src.shape[1:3]
        args.update(d_src=sbuf.data_ptr() + slo, n_src=len(src), iw=iw, ih=ih)
    args.update({name[5:] if name.startswith("call_") else name: v for name, v in kw.items()})
    err = None
    try:
        codec.compose_batch(**args)
    except mi.LlcompError as e:
        err = e
    torch.cuda.synchronize()
    assert (err is not None) == expect_error, err
    assert err is None or err.status == mi.BAD_ARGS
    host = dbuf.cpu().numpy()
    assert guards_intact(host, dlo, dst.nbytes), "a byte outside the dst batch was written"
    if src is not None:
        shost = sbuf.cpu().numpy()
        assert guards_intact(shost, slo, src.nbytes)
        assert np.array_equal(shost[slo:slo + src.nbytes], np.ascontiguousarray(src).reshape(-1).view(np.uint8)), "the src batch was written"
    return bits_of(host[dlo:dlo + dst.nbytes].copy().view(dst.dtype).reshape(dst.shape))


def check(mi, codecs, dtype, layout, c, src_shape, dst_shape, pieces, fill=None, keep=False, src_offset=0, dst_offset=0, seed=0):
    """src_shape (n_src, iw, ih) or None, dst_shape (n_dst, ow, oh)"""
    src = compose_spec.gen_batch(dtype, src_shape[0], c, src_shape[2], src_shape[1], layout, seed) if src_shape else None
    dst = compose_spec.gen_batch(dtype, dst_shape[0], c, dst_shape[2], dst_shape[1], layout, seed + 1000)
    got = run(mi, codecs[c], src, dst, pieces, dtype, layout, fill, keep, src_offset, dst_offset)
    want = bits_of(compose_spec.apply(src, dst, pieces, layout, dtype, fill, keep))
    assert np.array_equal(got, want), (dtype, layout, c, src_shape, dst_shape, keep, src_offset, dst_offset, np.argwhere(got != want)[:4].tolist())


def fill_of(dtype, c):
    return [float(17 * ch + 3) if dtype == "uint8" else 0.3 * (ch + 1) - 1.0 for ch in range(c)]


def straddling(T, R, ow, oh, n_dst, rng):
    """pieces across every border of the tiles of an ow x oh sample (src: 2 samples of the same shape), and a few drawn ones"""
    out = []
    for bx in range(T, ow, T):  # columns bx - 3 .. bx + 4, every row, read from one column further left
        out.append((int(rng.integers(n_dst)), 0, bx - 3, 0, bx - 4, 0, min(8, ow - bx + 3), oh))
    for by in range(R, oh, R):  # rows by - 2 .. by + 2, every column but the first
        out.append((int(rng.integers(n_dst)), 1, min(1, ow - 1), by - 2, 0, by - 2, ow - min(1, ow - 1), min(5, oh - by + 2)))
    for bx in range(T, ow, T):  # the tiles' corners
        for by in range(R, oh, R):
            out.append((int(rng.integers(n_dst)), 1, bx - 1, by - 1, bx - 1, by - 1, min(2, ow - bx + 1), min(2, oh - by + 1)))
    return out + compose_spec.random_pieces(rng, 2, ow, oh, n_dst, ow, oh, 5)


@pytest.mark.parametrize("layout", ("chw", "hwc"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_sides_around_the_tile(mi, codecs, dtype, layout):
    c = 3
    T, R = mi.compose_tile(), mi.compose_tile(ESIZE[dtype] * (1 if layout == "chw" else c))
    rng = np.random.default_rng(T)
    squares = [(s, s) for s in (1, 2, T - 1, T, T + 1, 2 * T + 1)]
    for ow, oh in squares + [(2 * T + 1, R + 1), (3, 2 * R + 1), (T + 1, R - 1), (T - 1, R), (2 * T, 2 * R)]:
        for keep in (False, True):
            check(mi, codecs, dtype, layout, c, (2, ow, oh), (2, ow, oh), straddling(T, R, ow, oh, 2, rng), fill_of(dtype, c), keep, seed=ow + oh)


@pytest.mark.parametrize("dtype,layout,c", [("uint8", "chw", 1), ("float16", "chw", 1), ("bfloat16", "chw", 1), ("float32", "chw", 1), ("uint8", "hwc", 3),
                                            ("float16", "hwc", 3), ("float32", "hwc", 3)])
def test_all_sixteen_shifts(mi, codecs, dtype, layout, c):
    """sx in 0..15 against dx in 0..15 with widths 1, 15, 16, 17 and 33, each on a dst sample of its own: 1280 samples in one call"""
    widths = (1, 15, 16, 17, 33)
    pieces = []
    for sx in range(16):
        for dx in range(16):
            for k, w in enumerate(widths):
                pieces.append(((sx * 16 + dx) * 5 + k, (sx + dx) % 3, dx, k & 1, sx, 1 + (k & 1), w, 1))
    for keep in (False, True):
        check(mi, codecs, dtype, layout, c, (3, 52, 3), (len(pieces), 50, 2), pieces, fill_of(dtype, c), keep, seed=7)


@pytest.mark.parametrize("dtype", DTYPES)
def test_batches_at_any_element_address(mi, codecs, dtype):
    """both batches at element offsets 0, 1, 3 and 15 past a 256-byte boundary, independently; HWC with c = 3 puts pixels at every alignment"""
    T = mi.compose_tile()
    rng = np.random.default_rng(3)
    for layout, c in (("hwc", 3), ("chw", 1)):
        ow, oh, iw, ih = T + 5, 9, 40, 7
        pieces = [(0, 0, 0, 0, 0, 0, iw, ih), (1, 1, ow - iw, oh - ih, 0, 0, iw, ih), (0, 1, 3, 1, 1, 0, 37, 6)] + compose_spec.random_pieces(rng, 2, iw, ih, 2, ow, oh, 6)
        for so in (0, 1, 3, 15):
            for do in (0, 1, 3, 15):
                check(mi, codecs, dtype, layout, c, (2, iw, ih), (2, ow, oh), pieces, fill_of(dtype, c), bool((so + do) & 1), so, do, seed=so * 16 + do)


def test_overlaps_hidden_empty_fill_pieces_and_samples_without_pieces(mi, codecs):
    for dtype, layout in (("float16", "chw"), ("uint8", "hwc"), ("float32", "hwc")):
        c = 3
        pieces = [(0, 0, 0, 0, 0, 0, 20, 20), (0, 1, 10, 10, 0, 0, 20, 20), (0, 2, 5, 15, 0, 2, 20, 10),  # three overlapping, the later winning
                  (1, 0, 4, 4, 1, 1, 8, 8), (1, 1, 0, 0, 0, 0, 20, 20),                                   # the first hidden entirely
                  (1, 2, 40, 30, 20, 20, 0, 0), (1, 0, 0, 0, 0, 0, 0, 7),                                 # empty ones
                  (3, 0, 1, 1, 0, 0, 17, 9), (3, 0, 5, 3, 0, 0, 9, 4, FILL), (3, 2, 8, 2, 2, 2, 3, 18), (3, 0, 0, 20, 0, 0, 40, 1, FILL)]  # FILL between copies
        for keep in (False, True):  # sample 2 has no piece: the fill without KEEP, untouched with it
            check(mi, codecs, dtype, layout, c, (3, 20, 20), (4, 40, 30), pieces, fill_of(dtype, c), keep, seed=5)
        check(mi, codecs, dtype, layout, c, (3, 20, 20), (4, 40, 30), pieces, None, False, seed=6)  # fill NULL: zeros
        check(mi, codecs, dtype, layout, c, (3, 20, 20), (4, 40, 30), [], fill_of(dtype, c), False, seed=6)  # no piece at all: the fill
        check(mi, codecs, dtype, layout, c, (3, 20, 20), (4, 40, 30), pieces[5:7], fill_of(dtype, c), True, seed=6)  # KEEP, empty pieces only: nothing queued


@pytest.mark.parametrize("c", (1, 3, 5))
@pytest.mark.parametrize("layout", ("chw", "hwc"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_dtype_layout_and_channel_count(mi, codecs, dtype, layout, c):
    """c = 5 in HWC float32 has a pixel of 20 bytes, above a unit"""
    T, R = mi.compose_tile(), mi.compose_tile(ESIZE[dtype] * (1 if layout == "chw" else c))
    rng = np.random.default_rng(c)
    ow, oh, iw, ih = T + 9, R + 3, 61, R + 1
    for keep in (False, True):
        pieces = compose_spec.random_pieces(rng, 3, iw, ih, 3, ow, oh, 12)
        check(mi, codecs, dtype, layout, c, (3, iw, ih), (3, ow, oh), pieces, fill_of(dtype, c), keep, 1, 3, seed=c)


def test_gridmask_in_place_without_a_src(mi, codecs):
    """d_src = NULL with KEEP: a 4 x 4 GridMask on every sample of a batch, in place"""
    for dtype, layout, c in (("float16", "chw", 3), ("uint8", "hwc", 3), ("float32", "hwc", 5)):
        n, ow, oh = 3, 150, 70
        pieces = [(i, 0, 7 + gx * 36, 3 + gy * 17, 0, 0, 19, 9, FILL) for i in range(n) for gy in range(4) for gx in range(4)]
        check(mi, codecs, dtype, layout, c, None, (n, ow, oh), pieces, fill_of(dtype, c), True, dst_offset=1, seed=2)


def test_refusals_queue_nothing_and_leave_dst_untouched(mi, codecs):
    import torch

    c = 3
    src = compose_spec.gen_batch("float32", 2, c, 4, 5, "chw", seed=1)
    dst = compose_spec.gen_batch("float32", 2, c, 6, 8, "chw", seed=2)
    before = bits_of(dst)
    k, L = codecs[c], mi._lib.load()
    ok = [(1, 1, 2, 1, 1, 0, 4, 4), (0, 0, 0, 0, 0, 0, 3, 3, FILL)]
    bad_pieces = [(2, 0, 0, 0, 0, 0, 1, 1), (0, 2, 0, 0, 0, 0, 1, 1), (0, 0, 5, 0, 0, 0, 4, 1), (0, 0, 0, 3, 0, 0, 1, 4), (0, 0, 9, 0, 0, 0, 0, 0),
                  (0, 0, 0, 0, 2, 0, 4, 1), (0, 0, 0, 0, 0, 1, 1, 4), (0, 0, 0, 0, 0, 0, 1, 1, 2), (0, 1, 0, 0, 0, 0, 1, 1, FILL),
                  (0, 0, 0, 0, 1, 0, 1, 1, FILL), (0, 0, 0, 0, 0, 1, 1, 1, FILL)]
    for p in bad_pieces:
        assert np.array_equal(run(mi, k, src, dst, [ok[0], p], "float32", "chw", expect_error=True), before), p
    for kw in (dict(n_dst=0), dict(n_dst=65536), dict(n_src=65536), dict(n_src=0), dict(d_src=None), dict(ow=0), dict(oh=0), dict(iw=0), dict(ih=0),
               dict(call_dtype=4), dict(call_layout=2), dict(call_layout="nchw"), dict(fill=[0.0, float("inf"), 0.0]), dict(fill=[float("nan")] * 3),
               dict(call_dtype="uint8", fill=[1.0, 2.5, 3.0]), dict(call_dtype="uint8", fill=[1.0, 256.0, 3.0])):
        assert np.array_equal(run(mi, k, src, dst, ok, "float32", "chw", expect_error=True, **kw), before), kw
    cap = mi.compose_max_pieces_per_sample()
    assert np.array_equal(run(mi, k, src, dst, [ok[0]] * (cap + 1), "float32", "chw", expect_error=True), before)
    # straight at the C entry: NULLs, flags, reserved bits, alignment, overlapping byte ranges
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    d, s = buf.data_ptr(), buf.data_ptr() + 8192
    recs = mi.compose_pieces(ok)
    reserved = mi.compose_pieces(ok)
    reserved[0].reserved = 1
    f32 = (1, 1)  # dtype, layout
    for args in ((None, s, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2, None, 0), (k._h, s, 2, 5, 4, None, 2, 8, 6, *f32, recs, 2, None, 0),
                 (k._h, None, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2, None, 0), (k._h, s, 2, 5, 4, d, 2, 8, 6, *f32, None, 2, None, 0),
                 (k._h, s, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2, None, 2), (k._h, s, 2, 5, 4, d, 2, 8, 6, *f32, reserved, 2, None, 0),
                 (k._h, s + 2, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2, None, 0), (k._h, s, 2, 5, 4, d + 2, 2, 8, 6, *f32, recs, 2, None, 0),
                 (k._h, s + 1, 2, 5, 4, d, 2, 8, 6, 2, 1, recs, 2, None, 0), (k._h, d + 2 * 3 * 48 * 4 - 4, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2, None, 0),
                 (k._h, d, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2, None, 1), (k._h, d - 2 * 3 * 20 * 4 + 4, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2, None, 0),
                 (k._h, s, 2, 5, 4, d, 2, 8, 6, *f32, recs, (1 << 20) + 1, None, 0)):
        assert L.llcomp_mi_codec_compose_batch(*args, stream()) == mi.BAD_ARGS, args[1:11]
    # batches that touch without overlapping are fine
    assert L.llcomp_mi_codec_compose_batch(k._h, d + 2 * 3 * 48 * 4, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2, None, 0, stream()) == mi.OK
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any()  # (zeros into zeros, and the zero fill)
    # ... and a call that is fine, on the same codec
    check(mi, codecs, "float32", "chw", c, (2, 5, 4), (2, 8, 6), ok)
    # the bound on a codec's memory, on a codec that has seen these calls only
    fresh = mi.Codec(1, 32, 16, c, 32, 16, False, device=0)
    try:
        check(mi, {c: fresh}, "float32", "chw", c, (2, 5, 4), (2, 8, 6), ok)
        check(mi, {c: fresh}, "float32", "chw", c, (2, 5, 4), (3, 8, 6), ok + ok)
        assert fresh.allocated_bytes() <= fresh.compose_workspace_bytes(3, 4)
        assert fresh.compose_workspace_bytes(9, 70) == L.llcomp_mi_codec_workspace_bytes(fresh._h) + 12 * 9 + 32 * 70 + 4 * c
    finally:
        fresh.close()
    assert L.llcomp_mi_codec_compose_workspace_bytes(None, 9, 70) == 0


def test_per_sample_cap(mi, codecs):
    """llcomp_mi_compose_max_pieces_per_sample() pieces on one dst sample pass, painter's order among all of them; one more is refused"""
    cap = mi.compose_max_pieces_per_sample()
    rng = np.random.default_rng(1)
    pieces = [(1, int(rng.integers(2)), int(rng.integers(0, 140)), int(rng.integers(0, 60)), int(rng.integers(0, 10)), int(rng.integers(0, 10)), 10, 10,
               0) for _ in range(cap)]
    more = pieces + [(0, 0, 0, 0, 0, 0, 0, 5, 0), (0, 1, 2, 2, 0, 0, 5, 5, 0)]  # an empty piece and another sample's do not count
    check(mi, codecs, "float16", "chw", 1, (2, 20, 20), (2, 150, 70), more, [1.5], False, seed=1)
    src = compose_spec.gen_batch("float16", 2, 1, 20, 20, "chw", seed=1)
    dst = compose_spec.gen_batch("float16", 2, 1, 70, 150, "chw", seed=2)
    assert np.array_equal(run(mi, codecs[1], src, dst, pieces + [(1, 0, 0, 0, 0, 0, 1, 1)], "float16", "chw", expect_error=True), bits_of(dst))


def test_mosaic_behind_decode_resized_regions_on_the_same_stream(mi, orc):
    """decode_resized_regions of 8 frames, compose_batch behind it on the stream: mosaic_pieces over the eight decoded views into two
    canvases with fill 114, against the spec applied to what the decode alone writes -- float16 CHW and uint8 HWC -- and, for uint8 HWC,
    against load_mosaic's expressions on PIL's resized crops"""
    import torch
    from PIL import Image

    from test_gpu_regions_host import make_batch
    from test_gpu_resized_output import TOut
    from test_gpu_resized_regions import packed

    frames, w, h, c, ow, oh, s = 8, 100, 44, 3, 24, 20, 24
    centres = [(17, 29), (24, 11)]
    rects = [(0, 0, 100, 44), (10, 4, 50, 40), (37, 11, 24, 24), (60, 0, 33, 17)] * 2
    imgs, conts = make_batch(orc, frames, w, h, c, 32, 16, False)
    codec = mi.Codec(frames, w, h, c, 32, 16, False, device=0)
    pieces = mi.mosaic_pieces(centres, ow, oh, s)
    tuples = [(p.dst, p.src, p.dx, p.dy, p.sx, p.sy, p.w, p.h, p.flags) for p in pieces]
    try:
        d_pay, n_pay, d_len = packed(mi, conts)
        for dtype, layout, kw in (("float16", "chw", dict(scale=True, mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])), ("uint8", "hwc", {})):
            o = TOut(frames, ow, oh, c, dtype, layout)
            canvas = TOut(2, 2 * s, 2 * s, c, dtype, layout)
            codec.decode_resized_regions(d_pay.data_ptr(), n_pay, d_len.data_ptr(), rects, ow, oh, o.ptr, o.st.data_ptr(), stream=stream(),
                                         dtype=dtype, layout=layout, filter="bilinear", **kw)
            codec.compose_batch(o.ptr, frames, ow, oh, canvas.ptr, 2, 2 * s, 2 * s, pieces, dtype=dtype, layout=layout, fill=114, stream=stream())
            st, decoded = o.read()
            assert st == 0
            _, got = canvas.read()
            want = compose_spec.apply(decoded, np.zeros_like(got), tuples, layout, dtype, 114)
            assert np.array_equal(bits_of(got), bits_of(want)), (dtype, layout)
            if dtype == "uint8":
                crops = [np.asarray(Image.fromarray(np.ascontiguousarray(imgs[f, y:y + rh, x:x + rw])).resize((ow, oh), Image.Resampling.BILINEAR))
                         for f, (x, y, rw, rh) in enumerate(rects)]
                for i, (xc, yc) in enumerate(centres):
                    assert np.array_equal(got[i], compose_spec.mosaic(crops[4 * i:4 * i + 4], xc, yc, s)), i
        torch.cuda.synchronize()
    finally:
        codec.close()
