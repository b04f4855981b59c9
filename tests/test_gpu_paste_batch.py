"""Batch copy-paste on the GPU (llcomp_mi_codec_paste_batch; include/llcomp_mi.h: "Batch copy-paste"): the pieces of a src batch that an
id map selects into a dst batch in HBM, against tests/paste_spec.py -- numpy's where per piece in list order -- bit for bit over the
whole dst batch, with 256 guard bytes on both sides of dst that have to stay and a src and a mask batch that have to be byte-identical
after the call.  One case runs behind decode_resized_regions.  T = compose_tile() and R = compose_tile(pixel bytes), the kernel's tile,
size the shapes."""
import numpy as np
import pytest

import paste_spec
from batch_support import DTYPES, ESIZE, bits_of, guards_intact, mi, put, stream  # noqa: F401

pytestmark = pytest.mark.gpu
ALL = list(range(256))


@pytest.fixture(scope="module")
def codecs(mi):
    made = {c: mi.Codec(1, 32, 16, c, 32, 16, False, device=0) for c in (1, 3)}
    yield made
    for k in made.values():
        k.close()


def run(mi, codec, src, mask, dst, pieces, dtype, layout, src_offset=0, dst_offset=0, mask_offset=0, expect_error=False, **kw):
    """paste_batch on the numpy batches, src and dst `offset` elements and the mask `offset` bytes past a 256-byte boundary -> dst's
    bits after the call; the guard bytes, the src batch and the mask batch have to be untouched.  mask None: the src batch is its own
    mask (U8, c = 1).  kw replaces arguments of the call (the refusals)."""
    import torch

    es = ESIZE[dtype]
    (c, oh, ow) = dst.shape[1:] if layout == "chw" else (dst.shape[3], dst.shape[1], dst.shape[2])
    (ih, iw) = src.shape[2:] if layout == "chw" else src.shape[1:3]
    dbuf, dlo = put(dst, dst_offset * es)
    sbuf, slo = put(src, src_offset * es)
    mbuf, mlo = put(mask, mask_offset) if mask is not None else (sbuf, slo)
    args = dict(d_src=sbuf.data_ptr() + slo, d_mask=mbuf.data_ptr() + mlo, n_src=len(src), iw=iw, ih=ih, d_dst=dbuf.data_ptr() + dlo, n_dst=len(dst),
                ow=ow, oh=oh, pieces=pieces, dtype=dtype, layout=layout, stream=stream())
    args.update({name[5:] if name.startswith("call_") else name: v for name, v in kw.items()})
    err = None
    try:
        codec.paste_batch(**args)
    except mi.LlcompError as e:
        err = e
    torch.cuda.synchronize()
    assert (err is not None) == expect_error, err
    assert err is None or err.status == mi.BAD_ARGS
    host = dbuf.cpu().numpy()
    assert guards_intact(host, dlo, dst.nbytes), "a byte outside the dst batch was written"
    for buf, lo, batch, what in ((sbuf, slo, src, "src"), (mbuf, mlo, mask if mask is not None else src, "mask")):
        h = buf.cpu().numpy()
        assert guards_intact(h, lo, batch.nbytes)
        assert np.array_equal(h[lo:lo + batch.nbytes], np.ascontiguousarray(batch).reshape(-1).view(np.uint8)), f"the {what} batch was written"
    return bits_of(host[dlo:dlo + dst.nbytes].copy().view(dst.dtype).reshape(dst.shape))


def check(mi, codecs, dtype, layout, c, src_shape, dst_shape, pieces, src_offset=0, dst_offset=0, mask_offset=0, seed=0, own_mask=False):
    """src_shape (n_src, iw, ih), dst_shape (n_dst, ow, oh)"""
    rng = np.random.default_rng(seed)
    if own_mask:
        src = paste_spec.gen_mask(rng, src_shape[0], src_shape[2], src_shape[1])[:, None]
        mask = src[:, 0]
    else:
        src = paste_spec.gen_batch(dtype, src_shape[0], c, src_shape[2], src_shape[1], layout, seed)
        mask = paste_spec.gen_mask(rng, src_shape[0], src_shape[2], src_shape[1])
    dst = paste_spec.gen_batch(dtype, dst_shape[0], c, dst_shape[2], dst_shape[1], layout, seed + 1000)
    got = run(mi, codecs[c], src, None if own_mask else mask, dst, pieces, dtype, layout, src_offset, dst_offset, mask_offset)
    want = bits_of(paste_spec.apply(src, mask, dst, pieces, layout, dtype))
    assert np.array_equal(got, want), (dtype, layout, c, src_shape, dst_shape, src_offset, dst_offset, mask_offset, np.argwhere(got != want)[:4].tolist())


def half(rng):
    return sorted(int(m) for m in rng.choice(8, 4, replace=False))


@pytest.mark.parametrize("layout", ("chw", "hwc"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_pieces_across_every_tile_border(mi, codecs, dtype, layout):
    c = 3
    T, R = mi.compose_tile(), mi.compose_tile(ESIZE[dtype] * (1 if layout == "chw" else c))
    rng = np.random.default_rng(T + R)
    ow, oh, iw, ih = T + 5, R + 3, T + 9, R + 2
    pieces = [(0, 0, 0, 0, 3, 0, ow, ih, half(rng)),             # a whole sample's objects, under everything else
              (0, 1, T - 3, 0, T - 4, 0, 8, ih, half(rng)),      # columns T - 3 .. T + 4, read from one column further left
              (1, 1, 1, R - 2, 0, R - 2, ow - 1, 4, half(rng)),  # rows R - 2 .. R + 1, every column but the first
              (1, 0, T - 1, R - 1, T - 1, R - 1, 2, 2, ALL),     # the tiles' corner
              (0, 1, T - 2, R - 1, 5, 1, 7, 3, half(rng), 3.0)]  # a VALUE piece over it
    pieces += paste_spec.random_pieces(rng, 2, iw, ih, 2, ow, oh, 6, dtype)
    check(mi, codecs, dtype, layout, c, (2, iw, ih), (2, ow, oh), pieces, 1, 3, 5, seed=T)


@pytest.mark.parametrize("dtype,layout,c", [("uint8", "hwc", 3), ("float16", "chw", 3)])
def test_batches_at_any_element_address_and_masks_at_any_byte(mi, codecs, dtype, layout, c):
    """dst and src at element offsets 0..15, all pairs, with the mask at byte offsets 0, 1, 7 and 15: every dst offset and every src
    offset meets each of the four"""
    rng = np.random.default_rng(3)
    ow, oh, iw, ih = 40, 5, 37, 4
    pieces = [(0, 0, 0, 0, 0, 0, iw, ih, half(rng)), (1, 1, ow - iw, oh - ih, 0, 0, iw, ih, half(rng)), (0, 1, 3, 1, 1, 0, 33, 3, half(rng)),
              (1, 0, 2, 0, 5, 1, 17, 2, half(rng), 9.0)]
    for do in range(16):
        for so in range(16):
            check(mi, codecs, dtype, layout, c, (2, iw, ih), (2, ow, oh), pieces, so, do, (0, 1, 7, 15)[(do + so // 4) % 4], seed=so * 16 + do)


def test_value_pieces_up_to_the_cap_on_one_sample(mi, codecs):
    """a 64 x 48 U8 c = 1 map that is its own mask, with 255 VALUE pieces on one sample (one below the cap) and with the cap's 256;
    257 are refused"""
    cap = mi.paste_max_pieces_per_sample()
    assert cap == 256
    rng = np.random.default_rng(1)

    def piece(i):
        w, h = int(rng.integers(1, 20)), int(rng.integers(1, 20))
        return (1, int(rng.integers(2)), int(rng.integers(0, 64 - w + 1)), int(rng.integers(0, 48 - h + 1)), int(rng.integers(0, 64 - w + 1)),
                int(rng.integers(0, 48 - h + 1)), w, h, half(rng), float(i % 256))

    pieces = [piece(i) for i in range(cap + 1)]
    others = [(0, 0, 0, 0, 0, 0, 0, 5, ALL), (0, 1, 2, 2, 0, 0, 5, 5, [1, 2])]  # an empty piece and another sample's do not count
    check(mi, codecs, "uint8", "chw", 1, (2, 64, 48), (2, 64, 48), pieces[:cap - 1] + others, seed=1, own_mask=True)
    check(mi, codecs, "uint8", "chw", 1, (2, 64, 48), (2, 64, 48), pieces[:cap] + others, seed=2, own_mask=True)
    src = paste_spec.gen_mask(rng, 2, 48, 64)[:, None]
    dst = paste_spec.gen_batch("uint8", 2, 1, 48, 64, "chw", seed=3)
    assert np.array_equal(run(mi, codecs[1], src, None, dst, pieces, "uint8", "chw", expect_error=True), bits_of(dst))


def test_the_id_maps_as_their_own_source(mi, codecs):
    """d_src and d_mask the same buffer: a class map pasted by class, at every alignment of the buffer"""
    T = mi.compose_tile()
    pieces = [(0, 1, 0, 0, 2, 1, T + 1, 30, [2, 3]), (1, 0, 4, 3, 0, 0, T - 3, 25, [1]), (1, 1, 7, 7, 7, 7, 50, 20, "nonzero")]
    for off in (0, 1, 7, 15):
        check(mi, codecs, "uint8", "chw", 1, (2, T + 3, 31), (2, T + 1, 33), pieces, off, (off * 5) % 16, seed=off, own_mask=True)


@pytest.mark.parametrize("dtype,layout", [("float16", "chw"), ("uint8", "hwc"), ("float32", "hwc")])
def test_all_bits_is_compose_batch_under_keep(mi, codecs, dtype, layout):
    import torch

    import compose_spec

    c = 3
    T, R = mi.compose_tile(), mi.compose_tile(ESIZE[dtype] * (1 if layout == "chw" else c))
    rng = np.random.default_rng(2)
    iw, ih, ow, oh = 61, R + 1, T + 9, R + 3
    rects = [p[:8] for p in compose_spec.random_pieces(rng, 3, iw, ih, 3, ow, oh, 14) if not p[8]]
    src = paste_spec.gen_batch(dtype, 3, c, ih, iw, layout, 1)
    dst = paste_spec.gen_batch(dtype, 3, c, oh, ow, layout, 2)
    mask = rng.integers(0, 256, size=(3, ih, iw), dtype=np.uint8)
    got = run(mi, codecs[c], src, mask, dst, [r + (ALL,) for r in rects], dtype, layout, 1, 2, 3)
    sbuf, slo = put(src, 0)
    cbuf, clo = put(dst, 0)  # a copy of dst for the composition
    codecs[c].compose_batch(sbuf.data_ptr() + slo, 3, iw, ih, cbuf.data_ptr() + clo, 3, ow, oh, rects, dtype=dtype, layout=layout, keep=True, stream=stream())
    torch.cuda.synchronize()
    composed = cbuf.cpu().numpy()[clo:clo + dst.nbytes].copy().view(dst.dtype).reshape(dst.shape)
    assert np.array_equal(got, bits_of(composed))


def test_refusals_queue_nothing_and_leave_dst_untouched(mi, codecs):
    import torch

    c = 3
    src = paste_spec.gen_batch("float32", 2, c, 4, 5, "chw", seed=1)
    dst = paste_spec.gen_batch("float32", 2, c, 6, 8, "chw", seed=2)
    mask = paste_spec.gen_mask(np.random.default_rng(1), 2, 4, 5)
    before = bits_of(dst)
    k, L = codecs[c], mi._lib.load()
    A = [1, 2, 3]
    ok = [(1, 1, 2, 1, 1, 0, 4, 4, A), (0, 0, 0, 0, 0, 0, 3, 3, "nonzero", 2.5)]
    bad_pieces = [(2, 0, 0, 0, 0, 0, 1, 1, A), (0, 2, 0, 0, 0, 0, 1, 1, A), (0, 0, 5, 0, 0, 0, 4, 1, A), (0, 0, 0, 3, 0, 0, 1, 4, A), (0, 0, 9, 0, 0, 0, 0, 0, A),
                  (0, 0, 0, 0, 2, 0, 4, 1, A), (0, 0, 0, 0, 0, 1, 1, 4, A), (0, 0, 0, 0, 0, 0, 1, 1, A, float("inf")), (0, 0, 0, 0, 0, 0, 1, 1, A, float("nan"))]
    for p in bad_pieces:
        assert np.array_equal(run(mi, k, src, mask, dst, [ok[0], p], "float32", "chw", expect_error=True), before), p
    for flags, value in ((2, 0.0), (0, 1.0)):  # a flag bit above bit 0; a value without VALUE
        recs = mi.paste_pieces(ok)
        recs[0].flags, recs[0].value = flags, value
        assert np.array_equal(run(mi, k, src, mask, dst, recs, "float32", "chw", expect_error=True), before), (flags, value)
    for kw in (dict(n_dst=0), dict(n_dst=65536), dict(n_src=65536), dict(n_src=0), dict(d_src=None), dict(d_mask=None), dict(ow=0), dict(oh=0), dict(iw=0),
               dict(ih=0), dict(call_dtype=4), dict(call_layout=2), dict(call_layout="nchw"),
               dict(call_dtype="uint8", call_pieces=[(0, 0, 0, 0, 0, 0, 1, 1, A, 2.5)]), dict(call_dtype="uint8", call_pieces=[(0, 0, 0, 0, 0, 0, 1, 1, A, 256.0)])):
        assert np.array_equal(run(mi, k, src, mask, dst, ok, "float32", "chw", expect_error=True, **kw), before), kw
    cap = mi.paste_max_pieces_per_sample()
    assert np.array_equal(run(mi, k, src, mask, dst, [ok[0]] * (cap + 1), "float32", "chw", expect_error=True), before)
    # straight at the C entry: NULLs, alignment, dst overlapping src or mask
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    d, s, m = buf.data_ptr(), buf.data_ptr() + 8192, buf.data_ptr() + 12288
    recs = mi.paste_pieces(ok)
    f32 = (1, 1)  # dtype, layout
    dst_bytes, src_bytes, mask_bytes = 2 * 3 * 48 * 4, 2 * 3 * 20 * 4, 2 * 20
    for args in ((None, s, m, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2), (k._h, s, m, 2, 5, 4, None, 2, 8, 6, *f32, recs, 2),
                 (k._h, None, m, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2), (k._h, s, None, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2),
                 (k._h, s, m, 2, 5, 4, d, 2, 8, 6, *f32, None, 2), (k._h, s + 2, m, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2),
                 (k._h, s, m, 2, 5, 4, d + 2, 2, 8, 6, *f32, recs, 2), (k._h, s + 1, m, 2, 5, 4, d, 2, 8, 6, 2, 1, recs, 2),
                 (k._h, d + dst_bytes - 4, m, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2), (k._h, d - src_bytes + 4, m, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2),
                 (k._h, s, d + dst_bytes - 1, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2), (k._h, s, d - mask_bytes + 1, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2),
                 (k._h, d, m, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2), (k._h, s, m, 2, 5, 4, d, 2, 8, 6, *f32, recs, (1 << 20) + 1)):
        assert L.llcomp_mi_codec_paste_batch(*args, stream()) == mi.BAD_ARGS, args[1:11]
    # batches that touch without overlapping are fine, and so is a mask inside src
    assert L.llcomp_mi_codec_paste_batch(k._h, d + dst_bytes, d + dst_bytes + src_bytes, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2, stream()) == mi.OK
    assert L.llcomp_mi_codec_paste_batch(k._h, s, s + 3, 2, 5, 4, d, 2, 8, 6, *f32, recs, 2, stream()) == mi.OK
    assert L.llcomp_mi_codec_paste_batch(k._h, None, None, 0, 0, 0, d, 2, 8, 6, *f32, None, 0, stream()) == mi.OK  # no piece: nothing queued
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any()  # (a mask of zeros: the first piece selects nothing, the second wants no zero)
    # ... and a call that is fine, on the same codec
    check(mi, codecs, "float32", "chw", c, (2, 5, 4), (2, 8, 6), ok)
    # the bound on a codec's memory, on a codec that has seen these calls only
    fresh = mi.Codec(1, 32, 16, c, 32, 16, False, device=0)
    try:
        check(mi, {c: fresh}, "float32", "chw", c, (2, 5, 4), (2, 8, 6), ok)
        check(mi, {c: fresh}, "float32", "chw", c, (2, 5, 4), (3, 8, 6), ok + ok)
        assert fresh.allocated_bytes() <= fresh.paste_workspace_bytes(3, 4)
        assert fresh.paste_workspace_bytes(9, 70) == L.llcomp_mi_codec_workspace_bytes(fresh._h) + 12 * 9 + 68 * 70
    finally:
        fresh.close()
    assert L.llcomp_mi_codec_paste_workspace_bytes(None, 9, 70) == 0


def test_copy_paste_behind_decode_resized_regions_on_the_same_stream(mi, orc):
    """decode_resized_regions of 4 picture frames twice (the src batch, and the dst batch from other rectangles) and of their 4 id maps
    with the nearest filter (the mask batch), paste_batch behind them on the stream: against the spec applied to what the decodes alone
    write -- float16 CHW and uint8 HWC"""
    import torch

    from test_gpu_regions_host import make_batch
    from test_gpu_resized_output import TOut
    from test_gpu_resized_regions import packed

    frames, w, h, c, ow, oh = 4, 100, 44, 3, 40, 24
    rects = [(0, 0, 100, 44), (10, 4, 50, 40), (37, 11, 24, 24), (60, 0, 33, 17)]
    dst_rects = [(5, 2, 80, 40), (0, 0, 100, 44), (20, 10, 40, 30), (50, 4, 48, 36)]
    imgs, conts = make_batch(orc, frames, w, h, c, 32, 16, False)
    yy, xx = np.mgrid[0:h, 0:w]
    id_maps = [np.ascontiguousarray((((yy + 3 * f) // 9 + (xx + 5 * f) // 13) % 6).astype(np.uint8)[..., None]) for f in range(frames)]
    map_conts = [orc.compress_sliced(m, 32, 16, False) for m in id_maps]
    codec, map_codec = mi.Codec(frames, w, h, c, 32, 16, False, device=0), mi.Codec(frames, w, h, 1, 32, 16, False, device=0)
    pieces = [(0, 1, 0, 0, 0, 0, ow, oh, [1, 2]), (1, 0, 3, 2, 5, 1, 30, 20, [3]), (2, 3, 0, 0, 0, 0, ow, oh, "nonzero"), (3, 2, 10, 4, 0, 0, 30, 20, [0, 5]),
              (0, 2, 7, 7, 7, 7, 20, 10, [4], 0.5)]
    try:
        d_pay, n_pay, d_len = packed(mi, conts)
        m_pay, nm_pay, m_len = packed(mi, map_conts)
        for dtype, layout, kw in (("float16", "chw", dict(scale=True, mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])), ("uint8", "hwc", {})):
            tuples = [p if dtype != "uint8" or len(p) == 9 else p[:9] + (77.0,) for p in pieces]
            src, dst, dst_alone, maps = (TOut(frames, ow, oh, c, dtype, layout), TOut(frames, ow, oh, c, dtype, layout),
                                         TOut(frames, ow, oh, c, dtype, layout), TOut(frames, ow, oh, 1, "uint8", "hwc", offset=7))
            for o, r in ((src, rects), (dst, dst_rects), (dst_alone, dst_rects)):
                codec.decode_resized_regions(d_pay.data_ptr(), n_pay, d_len.data_ptr(), r, ow, oh, o.ptr, o.st.data_ptr(), stream=stream(), dtype=dtype,
                                             layout=layout, filter="bilinear", **kw)
            map_codec.decode_resized_regions(m_pay.data_ptr(), nm_pay, m_len.data_ptr(), rects, ow, oh, maps.ptr, maps.st.data_ptr(), stream=stream(),
                                             dtype="uint8", layout="hwc", filter="nearest")
            codec.paste_batch(src.ptr, maps.ptr, frames, ow, oh, dst.ptr, frames, ow, oh, tuples, dtype=dtype, layout=layout, stream=stream())
            (st_s, s_host), (st_d, got), (st_a, before), (st_m, m_host) = src.read(), dst.read(), dst_alone.read(), maps.read()
            assert (st_s, st_d, st_a, st_m) == (0, 0, 0, 0)
            assert set(np.unique(m_host)) <= set(range(6)) and len(np.unique(m_host)) > 2
            want = paste_spec.apply(s_host, m_host[..., 0], before, tuples, layout, dtype)
            assert np.array_equal(bits_of(got), bits_of(want)), (dtype, layout)
            assert not np.array_equal(bits_of(got), bits_of(before))
        torch.cuda.synchronize()
    finally:
        codec.close()
        map_codec.close()
