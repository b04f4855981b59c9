"""Batch copy-paste by 16-bit ids on the GPU (llcomp_mi_codec_paste_batch16; include/llcomp_mi.h: "Batch copy-paste by 16-bit ids"): the
pieces of a src batch that a 16-bit id map selects into a dst batch in HBM, against tests/paste16_spec.py -- numpy's where per piece in
list order -- bit for bit over the whole dst batch, with 256 guard bytes on both sides of dst that have to stay and a src and a mask
batch that have to be byte-identical after the call.  T = compose_tile() and R = compose_tile(pixel bytes), the kernel's tile, size the
shapes."""
import numpy as np
import pytest

import paste16_spec
from batch_support import DTYPES, ESIZE, bits_of, guards_intact, mi, put, stream  # noqa: F401
from paste16_spec import HIGH_BYTE, Window
from test_paste16_rule import as_array, window_cases, window_piece

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codecs(mi):
    made = {c: mi.Codec(1, 32, 16, c, 32, 16, False, device=0) for c in (1, 2, 3)}
    yield made
    for k in made.values():
        k.close()


def run(mi, codec, src, mask, dst, pieces, dtype, layout, src_offset=0, dst_offset=0, mask_offset=0, expect_error=False, **kw):
    """paste_batch16 on the numpy batches, src and dst `offset` elements and the mask `offset` bytes past a 256-byte boundary -> dst's
    bits after the call; the guard bytes, the src batch and the mask batch have to be untouched.  mask None: the src batch is its own
    mask.  kw replaces arguments of the call (the refusals)."""
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
        codec.paste_batch16(**args)
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


def check(mi, codecs, dtype, layout, c, src_shape, dst_shape, pieces, src_offset=0, dst_offset=0, mask_offset=0, seed=0, pool=HIGH_BYTE, recs=None):
    """src_shape (n_src, iw, ih), dst_shape (n_dst, ow, oh); recs: the pieces as the C structs where the spec's are Windows"""
    rng = np.random.default_rng(seed)
    src = paste16_spec.gen_batch(dtype, src_shape[0], c, src_shape[2], src_shape[1], layout, seed)
    mask = paste16_spec.gen_mask(rng, src_shape[0], src_shape[2], src_shape[1], pool)
    dst = paste16_spec.gen_batch(dtype, dst_shape[0], c, dst_shape[2], dst_shape[1], layout, seed + 1000)
    got = run(mi, codecs[c], src, mask, dst, pieces if recs is None else recs, dtype, layout, src_offset, dst_offset, mask_offset)
    want = bits_of(paste16_spec.apply(src, mask, dst, pieces, layout))
    assert np.array_equal(got, want), (dtype, layout, c, src_shape, dst_shape, src_offset, dst_offset, mask_offset, np.argwhere(got != want)[:4].tolist())
    assert not pieces or not np.array_equal(got, bits_of(dst))


def half(rng, pool=HIGH_BYTE):
    return sorted(int(m) for m in rng.choice(pool, len(pool) // 2, replace=False))


@pytest.mark.parametrize("layout", ("chw", "hwc"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_pieces_across_every_tile_border(mi, codecs, dtype, layout):
    c = 3
    T, R = mi.compose_tile(), mi.compose_tile(ESIZE[dtype] * (1 if layout == "chw" else c))
    rng = np.random.default_rng(T + R)
    ow, oh, iw, ih = T + 7, R + 3, T + 10, R + 2
    pieces = [(0, 0, 0, 0, 3, 0, ow, ih, half(rng)),             # a whole sample's objects, under everything else
              (0, 1, T - 3, 0, T - 4, 0, 8, ih, half(rng)),      # columns T - 3 .. T + 4, read from one column further left
              (1, 1, 1, R - 2, 0, R - 2, ow - 1, 4, half(rng)),  # rows R - 2 .. R + 1, every column but the first
              (1, 0, T - 1, R - 1, T - 1, R - 1, 2, 2, HIGH_BYTE),  # the tiles' corner
              (0, 1, T - 2, R - 1, 5, 1, 7, 3, half(rng), 3)]    # a VALUE piece over it
    pieces += paste16_spec.random_pieces(rng, 2, iw, ih, 2, ow, oh, 6, ESIZE[dtype])
    check(mi, codecs, dtype, layout, c, (2, iw, ih), (2, ow, oh), pieces, 1, 3, 6, seed=T)
    for n, ow2, oh2 in ((3, T - 1, R - 1), (2, T, R)):  # the tile's own width and height, and one less
        pieces = paste16_spec.random_pieces(rng, 2, iw, ih, n, ow2, oh2, 8, ESIZE[dtype]) + [(0, 1, 0, 0, 1, 1, ow2, oh2, half(rng))]
        check(mi, codecs, dtype, layout, c, (2, iw, ih), (n, ow2, oh2), pieces, 2, 1, 14, seed=ow2)


@pytest.mark.parametrize("mo", range(0, 16, 2))
@pytest.mark.parametrize("dtype,layout,c", [("uint8", "chw", 3), ("uint8", "hwc", 3), ("float16", "chw", 3), ("float32", "hwc", 3)])
def test_masks_at_every_even_byte_against_dst_offsets(mi, codecs, dtype, layout, c, mo):
    """the mask at byte offsets 0, 2, .. 14 against dst at element offsets 0..15: every pair, src's offset drawn"""
    rng = np.random.default_rng(3)
    ow, oh, iw, ih = 40, 5, 37, 4
    pieces = [(0, 0, 0, 0, 0, 0, iw, ih, half(rng)), (1, 1, ow - iw, oh - ih, 0, 0, iw, ih, half(rng)), (0, 1, 3, 1, 1, 0, 33, 3, half(rng)),
              (1, 0, 2, 0, 5, 1, 17, 2, half(rng), 9)]
    for do in range(16):
        check(mi, codecs, dtype, layout, c, (2, iw, ih), (2, ow, oh), pieces, (do * 3 + mo) % 16, do, mo, seed=mo * 16 + do)


@pytest.mark.parametrize("dtype,layout,c", [("float16", "chw", 3), ("uint8", "hwc", 3), ("uint8", "chw", 1)])
def test_the_borders_of_a_window(mi, codecs, dtype, layout, c):
    rng = np.random.default_rng(c + len(dtype))
    T = mi.compose_tile()
    for pool, windows in window_cases(rng):
        rects = [(i % 2, (i + 1) % 2, i, 1, 2 * i, 0, T - 10, 8) for i in range(len(windows))]
        value = [None, (1 << (8 * ESIZE[dtype])) - 2, None]
        spec = [r + (Window(b, lut), v) for r, (b, lut), v in zip(rects, windows, value)]
        recs = as_array(mi, [window_piece(mi, r, b, lut, v) for r, (b, lut), v in zip(rects, windows, value)])
        check(mi, codecs, dtype, layout, c, (2, T + 3, 9), (2, T + 1, 11), spec, 1, 2, 4, seed=len(pool), pool=pool, recs=recs)


def test_a_set_of_600_ids_and_the_cap_on_one_sample(mi, codecs):
    rng = np.random.default_rng(600)
    ids = sorted(int(v) for v in rng.choice(3000, 600, replace=False) + 200)
    pool = [int(v) for v in rng.integers(0, 3400, size=400)]
    pieces = [(0, 1, 2, 1, 0, 3, 40, 20, ids), (0, 0, 0, 0, 0, 0, 5, 5, [pool[0]], 0x1234), (1, 1, 3, 3, 1, 1, 30, 10, "nonzero")]
    check(mi, codecs, "float16", "chw", 3, (2, 45, 25), (2, 44, 22), pieces, 1, 1, 2, seed=6, pool=pool)  # ("nonzero": the cap's 256 windows)
    src = paste16_spec.gen_batch("float16", 2, 3, 25, 45, "chw", seed=3)
    dst = paste16_spec.gen_batch("float16", 2, 3, 22, 44, "chw", seed=4)
    mask = paste16_spec.gen_mask(rng, 2, 25, 45, pool)
    too_many = [(1, 1, 3, 3, 1, 1, 30, 10, "nonzero"), (1, 0, 0, 0, 0, 0, 5, 5, [7])]  # 257 pieces on one sample
    assert np.array_equal(run(mi, codecs[3], src, mask, dst, too_many, "float16", "chw", expect_error=True), bits_of(dst))


def test_the_id_maps_as_their_own_source(mi, codecs):
    """d_src and d_mask the same buffer: instance maps pasted by id as a 2-byte dtype with c == 1 and as U8 HWC with c == 2, and VALUE
    pieces that renumber, at every alignment of the buffer"""
    T = mi.compose_tile()
    rng = np.random.default_rng(9)
    pool = (0, 300, 301, 0x2C01, 65535)
    pieces = [(0, 1, 0, 0, 2, 1, T + 1, 30, [300, 0x2C01]), (1, 0, 4, 3, 0, 0, T - 3, 25, [301]), (1, 1, 7, 7, 7, 7, 50, 20, [65535, 300], 40000)]
    for off in (0, 2, 6, 14):
        maps = paste16_spec.gen_mask(rng, 2, 31, T + 3, pool)
        dst = paste16_spec.gen_mask(rng, 2, 33, T + 1, (0, 5, 0x0105))
        want = paste16_spec.apply(maps[:, None], maps, dst[:, None], pieces, "chw")[:, 0]
        got = run(mi, codecs[1], maps[:, None], None, dst[:, None], pieces, "bfloat16", "chw", off // 2, (off * 5) % 16 // 2)
        assert np.array_equal(got[:, 0], want) and not np.array_equal(want, dst)
        as_bytes, dst_bytes = maps.view(np.uint8).reshape(2, 31, T + 3, 2), dst.view(np.uint8).reshape(2, 33, T + 1, 2)
        got = run(mi, codecs[2], as_bytes, None, dst_bytes, pieces[:2], "uint8", "hwc", off, (off * 5) % 16)
        want = paste16_spec.apply(maps[:, None], maps, dst[:, None], pieces[:2], "chw")[:, 0]
        assert np.array_equal(got.reshape(2, 33, 2 * (T + 1)).view(np.uint16), want)


def test_refusals_queue_nothing_and_leave_dst_untouched(mi, codecs):
    import torch

    c = 3
    src = paste16_spec.gen_batch("float16", 2, c, 4, 5, "chw", seed=1)
    dst = paste16_spec.gen_batch("float16", 2, c, 6, 8, "chw", seed=2)
    mask = paste16_spec.gen_mask(np.random.default_rng(1), 2, 4, 5)
    before = bits_of(dst)
    k, L = codecs[c], mi._lib.load()
    A = [1, 0x0101, 0xFF01]
    ok = [(1, 1, 2, 1, 1, 0, 4, 4, A), (0, 0, 0, 0, 0, 0, 3, 3, [2, 0x0102, 0], 0x4100)]
    bad_pieces = [(2, 0, 0, 0, 0, 0, 1, 1, A), (0, 2, 0, 0, 0, 0, 1, 1, A), (0, 0, 5, 0, 0, 0, 4, 1, A), (0, 0, 0, 3, 0, 0, 1, 4, A), (0, 0, 9, 0, 0, 0, 0, 0, A),
                  (0, 0, 0, 0, 2, 0, 4, 1, A), (0, 0, 0, 0, 0, 1, 1, 4, A), (0, 0, 0, 0, 0, 0, 1, 1, A, 0x10000)]
    for p in bad_pieces:
        assert np.array_equal(run(mi, k, src, mask, dst, [ok[0], p], "float16", "chw", expect_error=True), before), p
    for flags, value, base in ((2, 0, 1), (0, 1, 1), (0, 0, 65536), (1, 0x10000, 1)):  # a flag above bit 0; value_bits without VALUE; the base; the bits
        recs = mi.paste_pieces16(ok)
        recs[0].flags, recs[0].value_bits, recs[0].id_base = flags, value, base
        assert np.array_equal(run(mi, k, src, mask, dst, recs, "float16", "chw", expect_error=True), before), (flags, value, base)
    for kw in (dict(n_dst=0), dict(n_dst=65536), dict(n_src=65536), dict(n_src=0), dict(d_src=None), dict(d_mask=None), dict(ow=0), dict(oh=0), dict(iw=0),
               dict(ih=0), dict(call_dtype=4), dict(call_layout=2), dict(call_layout="nchw"),
               dict(call_dtype="uint8", call_pieces=[(0, 0, 0, 0, 0, 0, 1, 1, A, 0x100)])):
        assert np.array_equal(run(mi, k, src, mask, dst, ok, "float16", "chw", expect_error=True, **kw), before), kw
    assert np.array_equal(run(mi, k, src, mask, dst, ok, "float16", "chw", mask_offset=1, expect_error=True), before)  # a mask at an odd address
    # straight at the C entry: NULLs, alignment, dst overlapping src or mask
    buf = torch.zeros(8192, dtype=torch.float16, device="cuda")
    d, s, m = buf.data_ptr(), buf.data_ptr() + 8192, buf.data_ptr() + 12288
    recs = mi.paste_pieces16(ok)
    f16 = (2, 1)  # dtype, layout
    dst_bytes, src_bytes, mask_bytes = 2 * 3 * 48 * 2, 2 * 3 * 20 * 2, 2 * 20 * 2
    for args in ((None, s, m, 2, 5, 4, d, 2, 8, 6, *f16, recs, 2), (k._h, s, m, 2, 5, 4, None, 2, 8, 6, *f16, recs, 2),
                 (k._h, None, m, 2, 5, 4, d, 2, 8, 6, *f16, recs, 2), (k._h, s, None, 2, 5, 4, d, 2, 8, 6, *f16, recs, 2),
                 (k._h, s, m, 2, 5, 4, d, 2, 8, 6, *f16, None, 2), (k._h, s + 1, m, 2, 5, 4, d, 2, 8, 6, *f16, recs, 2),
                 (k._h, s, m, 2, 5, 4, d + 1, 2, 8, 6, *f16, recs, 2), (k._h, s, m + 1, 2, 5, 4, d, 2, 8, 6, *f16, recs, 2),
                 (k._h, d + dst_bytes - 2, m, 2, 5, 4, d, 2, 8, 6, *f16, recs, 2), (k._h, d - src_bytes + 2, m, 2, 5, 4, d, 2, 8, 6, *f16, recs, 2),
                 (k._h, s, d + dst_bytes - 2, 2, 5, 4, d, 2, 8, 6, *f16, recs, 2), (k._h, s, d - mask_bytes + 2, 2, 5, 4, d, 2, 8, 6, *f16, recs, 2),
                 (k._h, d, m, 2, 5, 4, d, 2, 8, 6, *f16, recs, 2), (k._h, s, m, 2, 5, 4, d, 2, 8, 6, *f16, recs, (1 << 20) + 1)):
        assert L.llcomp_mi_codec_paste_batch16(*args, stream()) == mi.BAD_ARGS, args[1:11]
    # batches that touch without overlapping are fine, and so is a mask inside src
    assert L.llcomp_mi_codec_paste_batch16(k._h, d + dst_bytes, d + dst_bytes + src_bytes, 2, 5, 4, d, 2, 8, 6, *f16, recs, len(recs), stream()) == mi.OK
    assert L.llcomp_mi_codec_paste_batch16(k._h, s, s + 4, 2, 5, 4, d, 2, 8, 6, *f16, recs, len(recs), stream()) == mi.OK
    assert L.llcomp_mi_codec_paste_batch16(k._h, None, None, 0, 0, 0, d, 2, 8, 6, *f16, None, 0, stream()) == mi.OK  # no piece: nothing queued
    torch.cuda.synchronize()
    host = buf.cpu().numpy().view(np.uint16)
    assert host[8:19].tolist() == [0x4100] * 3 + [0] * 5 + [0x4100] * 3 and not host[24:48].any() and not host[48 * 3:].any()  # (a mask of zeros: only the VALUE piece's id 0)
    # ... and a call that is fine, on the same codec
    check(mi, codecs, "float16", "chw", c, (2, 5, 4), (2, 8, 6), ok)
    # the bound on a codec's memory, on a codec that has seen these calls only
    fresh = mi.Codec(1, 32, 16, c, 32, 16, False, device=0)
    try:
        check(mi, {c: fresh}, "float16", "chw", c, (2, 5, 4), (2, 8, 6), ok)
        check(mi, {c: fresh}, "float16", "chw", c, (2, 5, 4), (3, 8, 6), ok + ok)
        assert fresh.allocated_bytes() <= fresh.paste16_workspace_bytes(3, len(mi.paste_pieces16(ok + ok)))
        assert fresh.paste16_workspace_bytes(9, 70) == L.llcomp_mi_codec_workspace_bytes(fresh._h) + 12 * 9 + 72 * 70
    finally:
        fresh.close()
    assert L.llcomp_mi_codec_paste16_workspace_bytes(None, 9, 70) == 0
