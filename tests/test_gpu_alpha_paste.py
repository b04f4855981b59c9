"""Batch alpha paste on the GPU (llcomp_mi_codec_alpha_paste_batch; include/llcomp_mi.h: "Batch alpha paste") against
tests/alpha_paste_spec.py -- the numpy statement of both rules, piece by piece in list order -- bit for bit over the whole dst batch,
with 256 guard bytes on both sides of dst that have to stay and a src and an alpha batch that have to be byte-identical after the call.
One case runs behind decode_resized_regions, one against PIL itself.  T = compose_tile() and R = compose_tile(pixel bytes), the
kernel's tile, size the shapes."""
import numpy as np
import pytest

import alpha_paste_spec as spec
from alpha_paste_spec import ALPHA_OVER, ALPHA_VALUE, ALPHA_VALUE_PIXEL
from batch_support import DTYPES, ESIZE, bits_of, gen_batch, guards_intact, mi, put, stream  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codecs(mi):
    made = {c: mi.Codec(1, 32, 16, c, 32, 16, False, device=0) for c in (1, 3, 4)}
    yield made
    for k in made.values():
        k.close()


def run(mi, codec, src, alpha, dst, pieces, dtype, layout, alpha_byte=0, src_offset=0, dst_offset=0, alpha_offset=0, own_alpha=False, expect_error=False,
        queues=True, **kw):
    """alpha_paste_batch on the numpy batches, src and dst `offset` elements and the alpha `offset` bytes past a 256-byte boundary -> dst
    after the call, as dst's type; the guard bytes, the src batch and the alpha batch have to be untouched.  own_alpha: the src batch is
    its own alpha.  kw replaces arguments of the call (the refusals)."""
    import torch

    (oh, ow) = dst.shape[2:] if layout == "chw" else dst.shape[1:3]
    es = ESIZE[dtype]
    dbuf, dlo = put(dst, dst_offset * es)
    sbuf, slo = put(src, src_offset * es) if src is not None else (None, 0)
    abuf, alo = (sbuf, slo) if own_alpha else put(alpha, alpha_offset) if alpha is not None else (None, 0)
    ref = src if src is not None else alpha
    n_src = len(ref)
    (ih, iw) = (ref.shape[2:] if layout == "chw" else ref.shape[1:3]) if src is not None else alpha.shape[1:3]
    apx = (src if own_alpha else alpha).nbytes // (n_src * ih * iw) if (alpha is not None or own_alpha) else 1
    args = dict(d_src=None if sbuf is None else sbuf.data_ptr() + slo, d_alpha=None if abuf is None else abuf.data_ptr() + alo, alpha_px_bytes=apx,
                alpha_byte=alpha_byte, n_src=n_src, iw=iw, ih=ih, d_dst=dbuf.data_ptr() + dlo, n_dst=len(dst), ow=ow, oh=oh, pieces=pieces, dtype=dtype,
                layout=layout, stream=stream())
    args.update(kw)
    err = None
    before = codec.allocated_bytes()
    try:
        codec.alpha_paste_batch(**args)
    except mi.LlcompError as e:
        err = e
    torch.cuda.synchronize()
    assert (err is not None) == expect_error, err
    assert err is None or err.status == mi.BAD_ARGS
    if not queues:
        assert codec.allocated_bytes() == before, "a call that queues nothing allocated"
    host = dbuf.cpu().numpy()
    assert guards_intact(host, dlo, dst.nbytes), "a byte outside the dst batch was written"
    for buf, lo, arr in ((sbuf, slo, src), (None if own_alpha else abuf, alo, alpha)):
        if buf is not None:
            h = buf.cpu().numpy()
            assert guards_intact(h, lo, arr.nbytes) and np.array_equal(h[lo:lo + arr.nbytes], arr.reshape(-1).view(np.uint8)), "src or alpha was written"
    got = host[dlo:dlo + dst.nbytes].copy().view(dst.dtype).reshape(dst.shape)
    if expect_error or not queues:
        assert np.array_equal(bits_of(got), bits_of(dst)), "a call that queues nothing wrote"
    return got


def same(a, b):
    return np.array_equal(bits_of(a), bits_of(b))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ("chw", "hwc"))
def test_soft_pieces_across_every_tile_border(mi, codecs, dtype, layout):
    c = 3
    T, R = mi.compose_tile(), mi.compose_tile((1 if layout == "chw" else c) * ESIZE[dtype])
    n, ow, oh, iw, ih = 2, T + 5, R + 3, T + 9, R + 4
    rng = np.random.default_rng(ESIZE[dtype] * 7 + len(layout))
    src, dst = gen_batch(dtype, n, c, ih, iw, layout, 1), gen_batch(dtype, n, c, oh, ow, layout, 2)
    matte = spec.gen_matte(rng, n, ih, iw)
    opaque = np.full_like(matte, 255)
    top = (1 << (8 * ESIZE[dtype])) - 1
    pieces = [(0, 1, T - 9, R - 2, 0, 0, 14, 5),                              # soft, across both borders
              (0, 0, T - 4, R - 1, 3, 1, 9, 4),                               # soft over soft
              (1, 0, 0, R - 1, 3, 0, ow, 2),                                  # a band across the vertical border
              (1, 1, T - 1, 0, 1, 1, 2, oh),                                  # a band across the horizontal border
              (1, 0, 5, 3, 0, 0, 40, R - 2, ALPHA_VALUE, 0x3C5A & top),       # VALUE
              (0, 1, 0, 0, 2, 2, T + 5, R + 2)]                               # soft over everything before it on sample 0
    if dtype == "uint8" and layout == "hwc":
        pieces.append((1, 1, T - 6, R - 2, 7, 0, 11, 5, ALPHA_VALUE | ALPHA_VALUE_PIXEL, 0x0311C8))
    want = spec.apply(src, matte, dst, pieces, dtype, layout)
    got = run(mi, codecs[c], src, matte, dst, pieces, dtype, layout, src_offset=3, dst_offset=5, alpha_offset=7)
    assert same(got, want) and not same(want, dst)
    assert same(want, mi.alpha_paste_reference(src, matte, dst, pieces, layout, dtype))
    # overlaps of three: an opaque piece over a soft one, and a soft one over an opaque one (the matte's sample 1 made opaque)
    both = matte.copy()
    both[1] = opaque[1]
    three = [(0, 0, T - 20, 1, 0, 0, 25, R), (0, 1, T - 10, 2, 5, 1, 15, R - 1), (0, 0, T - 5, 0, 9, 2, 10, R + 2),
             (1, 1, T - 20, 1, 0, 0, 25, R), (1, 0, T - 10, 2, 5, 1, 15, R - 1), (1, 1, T - 5, 0, 9, 2, 10, R + 2)]
    want = spec.apply(src, both, dst, three, dtype, layout)
    got = run(mi, codecs[c], src, both, dst, three, dtype, layout, src_offset=1, dst_offset=2, alpha_offset=15)
    assert same(got, want) and not same(want, dst)


@pytest.mark.parametrize("dtype,layout", [("uint8", "hwc"), ("float16", "chw")])
def test_every_pair_of_element_offsets(mi, codecs, dtype, layout):
    """dst and src at element offsets 0..15 in all pairs, the alpha at byte offsets 0, 1, 7 and 15, on a 40 x 5 shape"""
    c = 3
    rng = np.random.default_rng(40)
    src, dst = gen_batch(dtype, 1, c, 5, 40, layout, 1), gen_batch(dtype, 1, c, 5, 40, layout, 2)
    matte = spec.gen_matte(rng, 1, 5, 40)
    pieces = [(0, 0, 1, 0, 0, 1, 37, 4), (0, 0, 9, 1, 3, 0, 30, 3), (0, 0, 0, 2, 5, 2, 33, 2, ALPHA_VALUE, 0x5A)]
    want = spec.apply(src, matte, dst, pieces, dtype, layout)
    assert not same(want, dst)
    for so in range(16):
        for do in range(16):
            got = run(mi, codecs[c], src, matte, dst, pieces, dtype, layout, src_offset=so, dst_offset=do, alpha_offset=(0, 1, 7, 15)[(so + do) % 4])
            assert same(got, want), (so, do)


@pytest.mark.parametrize("apx,ab", [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (4, 0), (4, 1), (4, 2), (4, 3)])
def test_wider_alpha_pixels_with_every_alpha_byte(mi, codecs, apx, ab):
    T = mi.compose_tile()
    rng = np.random.default_rng(apx * 4 + ab)
    for dtype, layout, c in (("uint8", "chw", 3), ("float32", "hwc", 3), ("bfloat16", "chw", 1), ("uint8", "hwc", 4)):
        n, iw, ih, ow, oh = 2, T + 11, 6, T + 3, 7
        src, dst = gen_batch(dtype, n, c, ih, iw, layout, 1), gen_batch(dtype, n, c, oh, ow, layout, 2)
        alpha = spec.gen_matte(rng, n, ih, iw, apx, ab)
        pieces = spec.gen_pieces(rng, 6, n, iw, ih, n, ow, oh, dtype, layout, c) + [(0, 1, T - 7, 1, T - 2, 0, 10, 5)]
        want = spec.apply(src, alpha, dst, pieces, dtype, layout, ab)
        got = run(mi, codecs[c], src, alpha, dst, pieces, dtype, layout, alpha_byte=ab, src_offset=1, dst_offset=3, alpha_offset=(1, 7, 13, 15)[ab])
        assert same(got, want) and not same(want, dst), (dtype, layout)


def test_the_rgba_batch_as_its_own_alpha(mi, codecs):
    T = mi.compose_tile()
    rng = np.random.default_rng(44)
    n, iw, ih, ow, oh = 2, T + 6, 9, T + 9, 8
    src, dst = gen_batch("uint8", n, 4, ih, iw, "hwc", 1), gen_batch("uint8", n, 4, oh, ow, "hwc", 2)
    src[..., 3] = spec.gen_matte(rng, n, ih, iw)
    pieces = [(0, 1, 2, 0, 0, 1, T + 4, 8), (1, 0, T - 3, 2, 1, 0, 9, 6), (0, 0, T - 8, 1, T - 10, 3, 16, 5)]
    want = spec.apply(src, src, dst, pieces, "uint8", "hwc", 3)
    for so in (0, 1, 6):
        got = run(mi, codecs[4], src, None, dst, pieces, "uint8", "hwc", alpha_byte=3, src_offset=so, dst_offset=5, own_alpha=True)
        assert same(got, want) and not same(want, dst)


def test_over_across_tile_borders_at_4_byte_offsets(mi, codecs):
    T, R = mi.compose_tile(), mi.compose_tile(4)
    rng = np.random.default_rng(45)
    n, iw, ih, ow, oh = 2, T + 8, R + 5, T + 5, R + 3
    src, dst = gen_batch("uint8", n, 4, ih, iw, "hwc", 1), gen_batch("uint8", n, 4, oh, ow, "hwc", 2)
    src[..., 3] = spec.gen_matte(rng, n, ih, iw)
    dst[..., 3] = spec.gen_matte(rng, n, oh, ow)
    matte = spec.gen_matte(rng, n, ih, iw)
    pieces = [(0, 1, T - 9, R - 2, 0, 0, 14, 5, ALPHA_OVER), (0, 0, T - 4, R - 1, 3, 1, 9, 4, ALPHA_OVER), (1, 0, 0, R - 1, 3, 0, ow, 2, ALPHA_OVER),
              (1, 1, T - 1, 0, 1, 1, 2, oh, ALPHA_OVER), (0, 1, T - 6, 0, 2, 2, 10, R + 3), (0, 0, 1, 1, 0, 0, T + 2, R, ALPHA_OVER),
              (1, 1, 3, 2, 0, 0, 50, 20, ALPHA_VALUE | ALPHA_VALUE_PIXEL, 0x80C81103)]
    want = spec.apply(src, matte, dst, pieces, "uint8", "hwc")
    for so, do in ((0, 0), (4, 8), (12, 4), (8, 12)):
        got = run(mi, codecs[4], src, matte, dst, pieces, "uint8", "hwc", src_offset=so, dst_offset=do, alpha_offset=so + 1)
        assert same(got, want) and not same(want, dst), (so, do)
    only_over = [p for p in pieces if len(p) > 8 and p[8] == ALPHA_OVER]
    got = run(mi, codecs[4], src, None, dst, only_over, "uint8", "hwc", src_offset=4, dst_offset=4)  # no alpha batch at all
    assert same(got, spec.apply(src, None, dst, only_over, "uint8", "hwc"))
    run(mi, codecs[4], src, matte, dst, pieces, "uint8", "hwc", src_offset=2, expect_error=True)  # OVER off 4 bytes
    run(mi, codecs[4], src, matte, dst, pieces, "uint8", "hwc", dst_offset=1, expect_error=True)


def test_the_cap_of_256_pieces_on_one_sample(mi, codecs):
    rng = np.random.default_rng(256)
    n, iw, ih, ow, oh, c = 2, 90, 9, 97, 9, 3
    src, dst = gen_batch("float16", n, c, ih, iw, "chw", 1), gen_batch("float16", n, c, oh, ow, "chw", 2)
    matte = spec.gen_matte(rng, n, ih, iw)
    pieces = []
    for _ in range(256):
        w, h = int(rng.integers(1, 30)), int(rng.integers(1, 5))
        pieces.append((1, int(rng.integers(2)), int(rng.integers(0, ow - w + 1)), int(rng.integers(0, oh - h + 1)), int(rng.integers(0, iw - w + 1)),
                       int(rng.integers(0, ih - h + 1)), w, h))
    got = run(mi, codecs[c], src, matte, dst, pieces, "float16", "chw", dst_offset=1, alpha_offset=13)
    assert same(got, spec.apply(src, matte, dst, pieces, "float16", "chw"))
    assert codecs[c].allocated_bytes() <= codecs[c].alpha_paste_workspace_bytes(2, 256)
    run(mi, codecs[c], src, matte, dst, pieces + [pieces[0]], "float16", "chw", expect_error=True)  # 257 on one sample
    run(mi, codecs[c], src, matte, dst, pieces + [(1, 0, 0, 0, 0, 0, 0, 3)], "float16", "chw")       # ... an empty one does not count


def test_a_call_without_a_piece_that_has_w_and_h_queues_nothing(mi):
    fresh = mi.Codec(1, 32, 16, 3, 32, 16, False, device=0)
    try:
        src, dst = gen_batch("uint8", 1, 3, 4, 6, "hwc", 1), gen_batch("uint8", 1, 3, 4, 6, "hwc", 2)
        matte = np.full((1, 4, 6), 200, np.uint8)
        run(mi, fresh, src, matte, dst, [], "uint8", "hwc", queues=False)
        run(mi, fresh, src, matte, dst, [(0, 0, 1, 1, 0, 0, 0, 2), (0, 0, 0, 0, 0, 0, 3, 0)], "uint8", "hwc", queues=False)
        base = fresh.allocated_bytes()
        got = run(mi, fresh, src, matte, dst, [(0, 0, 1, 1, 0, 0, 4, 2)], "uint8", "hwc")  # the table buffer comes with the first call that needs it
        assert same(got, spec.apply(src, matte, dst, [(0, 0, 1, 1, 0, 0, 4, 2)], "uint8", "hwc"))
        assert base < fresh.allocated_bytes() <= fresh.alpha_paste_workspace_bytes(1, 1)
        L = mi._lib.load()
        assert fresh.alpha_paste_workspace_bytes(9, 70) == L.llcomp_mi_codec_workspace_bytes(fresh._h) + 12 * 9 + 36 * 70
        assert L.llcomp_mi_codec_alpha_paste_workspace_bytes(None, 9, 70) == 0
    finally:
        fresh.close()


def test_refusals_leave_dst_untouched(mi, codecs):
    rng = np.random.default_rng(1)
    src, dst = gen_batch("uint8", 1, 4, 4, 6, "hwc", 1), gen_batch("uint8", 1, 4, 4, 6, "hwc", 2)
    matte = spec.gen_matte(rng, 1, 4, 6)
    ok = [(0, 0, 0, 0, 0, 0, 3, 2)]
    vp = ALPHA_VALUE | ALPHA_VALUE_PIXEL
    for kw in (dict(alpha_px_bytes=0), dict(alpha_px_bytes=5), dict(alpha_byte=1), dict(d_alpha=None), dict(d_src=None), dict(d_dst=None), dict(n_src=0),
               dict(pieces=[ok[0] + (8,)]), dict(pieces=[ok[0] + (ALPHA_OVER | ALPHA_VALUE,)]), dict(pieces=[ok[0] + (ALPHA_VALUE_PIXEL,)]),
               dict(pieces=[ok[0] + (ALPHA_VALUE, 0x100)]), dict(pieces=[ok[0] + (0, 1)]), dict(pieces=[(0, 0, 0, 0, 0, 0, 7, 2)]),
               dict(pieces=[(1, 0, 0, 0, 0, 0, 3, 2)]), dict(pieces=[(0, 1, 0, 0, 0, 0, 3, 2)]), dict(pieces=[(0, 0, 0, 3, 0, 0, 3, 2)]),
               dict(layout="chw", pieces=[ok[0] + (ALPHA_OVER,)]), dict(layout="chw", pieces=[ok[0] + (vp, 1)])):
        kw = dict(kw)
        run(mi, codecs[4], src, matte, dst, kw.pop("pieces", ok), "uint8", kw.pop("layout", "hwc"), expect_error=True, **kw)
    src3, dst3 = gen_batch("uint8", 1, 3, 4, 6, "hwc", 1), gen_batch("uint8", 1, 3, 4, 6, "hwc", 2)
    run(mi, codecs[3], src3, matte, dst3, [ok[0] + (ALPHA_OVER,)], "uint8", "hwc", expect_error=True)      # OVER on c == 3
    run(mi, codecs[3], src3, matte, dst3, [ok[0] + (vp, 0x01000000)], "uint8", "hwc", expect_error=True)   # a value byte at c
    # dst overlapping src or alpha
    import torch

    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p, L, recs = buf.data_ptr(), mi._lib.load(), mi.alpha_pieces(ok)
    k = codecs[4]
    for s, a, d in ((p + 16, p + 2048, p), (p + 2048, p + 95, p), (p, p + 2048, p + 95)):
        assert L.llcomp_mi_codec_alpha_paste_batch(k._h, s, a, 1, 0, 1, 6, 4, d, 1, 6, 4, 0, 0, recs, 1, stream()) == mi.BAD_ARGS
    assert L.llcomp_mi_codec_alpha_paste_batch(None, p + 1024, p + 2048, 1, 0, 1, 6, 4, p, 1, 6, 4, 0, 0, recs, 1, stream()) == mi.BAD_ARGS
    assert L.llcomp_mi_codec_alpha_paste_batch(k._h, p + 96, p + 192, 1, 0, 1, 6, 4, p, 1, 6, 4, 0, 0, recs, 1, stream()) == mi.OK  # touching is fine
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any()  # (an alpha of zeros keeps everything)
    # ... and a call that is fine, on the same codec
    assert same(run(mi, codecs[4], src, matte, dst, ok, "uint8", "hwc"), spec.apply(src, matte, dst, ok, "uint8", "hwc"))


def test_alpha_paste_behind_decode_resized_regions_on_the_same_stream(mi, orc):
    """decode_resized_regions of 3 RGBA frames twice (the sprites, which are their own alpha, and the canvases from other rectangles) and
    alpha_paste_batch behind them on the stream, PASTE and OVER pieces: against the spec applied to what the decodes alone write"""
    import torch

    from test_gpu_regions_host import make_batch
    from test_gpu_resized_output import TOut
    from test_gpu_resized_regions import packed

    frames, w, h, c, ow, oh = 3, 100, 44, 4, 40, 24
    rects, dst_rects = [(0, 0, 100, 44), (10, 4, 50, 40), (37, 11, 24, 24)], [(5, 2, 80, 40), (0, 0, 100, 44), (20, 10, 40, 30)]
    imgs, conts = make_batch(orc, frames, w, h, c, 32, 16, False)
    codec = mi.Codec(frames, w, h, c, 32, 16, False, device=0)
    pieces = [(0, 1, 0, 0, 0, 0, ow, oh), (1, 0, 3, 2, 5, 1, 30, 20, ALPHA_OVER), (2, 1, 10, 4, 0, 0, 30, 20), (0, 2, 7, 7, 7, 7, 20, 10, ALPHA_OVER),
              (1, 2, 0, 0, 0, 0, 25, 24, ALPHA_VALUE | ALPHA_VALUE_PIXEL, 0xFF0080FF)]
    try:
        d_pay, n_pay, d_len = packed(mi, conts)
        src, dst, dst_alone = (TOut(frames, ow, oh, c, "uint8", "hwc", offset=4), TOut(frames, ow, oh, c, "uint8", "hwc", offset=8),
                               TOut(frames, ow, oh, c, "uint8", "hwc", offset=8))
        for o, r in ((src, rects), (dst, dst_rects), (dst_alone, dst_rects)):
            codec.decode_resized_regions(d_pay.data_ptr(), n_pay, d_len.data_ptr(), r, ow, oh, o.ptr, o.st.data_ptr(), stream=stream(), dtype="uint8",
                                         layout="hwc", filter="bilinear")
        codec.alpha_paste_batch(src.ptr, src.ptr, 4, 3, frames, ow, oh, dst.ptr, frames, ow, oh, pieces, dtype="uint8", layout="hwc", stream=stream())
        (st_s, s_host), (st_d, got), (st_a, before) = src.read(), dst.read(), dst_alone.read()
        torch.cuda.synchronize()
        assert (st_s, st_d, st_a) == (0, 0, 0)
        assert len(np.unique(s_host[..., 3])) > 8  # a soft alpha channel
        want = spec.apply(s_host, s_host, before, pieces, "uint8", "hwc", 3)
        assert same(got, want) and not same(got, before)
    finally:
        codec.close()


def test_against_pil_itself(mi, codecs):
    Image = pytest.importorskip("PIL.Image")
    T = mi.compose_tile()
    rng = np.random.default_rng(12)
    n, iw, ih, ow, oh = 2, 60, 30, T + 60, 40
    src, dst = rng.integers(0, 256, (n, ih, iw, 4), dtype=np.uint8), rng.integers(0, 256, (1, oh, ow, 4), dtype=np.uint8)
    src[..., 3] = spec.gen_matte(rng, n, ih, iw)
    dst[..., 3] |= 1  # (onto a pixel whose alpha is 0 PIL's paste of a COLOUR replaces the colour channels whatever the mask is: its own case)
    bg = Image.fromarray(dst[0], "RGBA")
    sprites = [Image.fromarray(s, "RGBA") for s in src]
    bg.paste(sprites[0], (T - 30, 5), sprites[0])                                                   # paste under its own A
    region = (T - 10, 8, T - 10 + iw, 8 + ih)
    bg.paste(Image.alpha_composite(bg.crop(region), sprites[1]), region[:2])                         # alpha_composite of a region
    bg.paste((10, 200, 30, 255), (3, 2, 3 + iw, 2 + ih), Image.fromarray(src[0, :, :, 3], "L"))     # a colour through a matte
    pieces = [(0, 0, T - 30, 5, 0, 0, iw, ih), (0, 1, T - 10, 8, 0, 0, iw, ih, ALPHA_OVER),
              (0, 0, 3, 2, 0, 0, iw, ih, ALPHA_VALUE | ALPHA_VALUE_PIXEL, 10 | 200 << 8 | 30 << 16 | 255 << 24)]
    got = run(mi, codecs[4], src, None, dst, pieces, "uint8", "hwc", alpha_byte=3, dst_offset=4, own_alpha=True)
    assert np.array_equal(got[0], np.asarray(bg))
