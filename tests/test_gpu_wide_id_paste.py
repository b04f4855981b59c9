"""The batch copy-paste by ids of 3 and 4 bytes on the GPU (llcomp_mi_codec_paste_batch32; include/llcomp_mi.h: "Wide id maps") against
the numpy spec of tests/test_wide_id_paste_rule.py, bit for bit, with 256 guard bytes around every dst batch and the maps byte-identical
after every call; and the whole chain on panoptic maps on one stream.  T = compose_tile(), the composition's tile, sizes the shapes."""
import numpy as np
import pytest

from batch_support import DTYPES, ESIZE, gen_batch, guards_intact, mi, put, stream  # noqa: F401
from test_label_boxes import as_table
from test_label_targets import index_spec
from test_wide_id_maps_rule import TOP, WIDTHS, blobs, boxes_spec, ids_of, wide_maps
from test_wide_id_paste_rule import POOL, apply32, gen_ids, random_pieces32, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codecs(mi):
    made = {c: mi.Codec(1, 32, 16, c, 32, 16, False, device=0) for c in (1, 3, 4)}
    yield made
    for k in made.values():
        k.close()


def pasted(mi, codec, src, ids, mb, dst, pieces, dtype, layout, moff=0, doff=0, own_source=False, expect_error=False, **kw):
    """paste_batch32 on the numpy batches, the maps `moff` bytes and dst `doff` bytes past a 256-byte boundary -> dst after the call"""
    import torch

    (oh, ow) = dst.shape[2:] if layout == "chw" else dst.shape[1:3]
    (ih, iw) = ids.shape[1:]
    maps = wide_maps(ids, mb)
    dbuf, dlo = put(dst, doff)
    mbuf, mlo = put(maps, moff)
    sbuf, slo = (mbuf, mlo) if own_source else put(src, 0)
    args = dict(d_src=sbuf.data_ptr() + slo, d_mask=mbuf.data_ptr() + mlo, map_bytes=mb, n_src=len(ids), iw=iw, ih=ih, d_dst=dbuf.data_ptr() + dlo, n_dst=len(dst),
                ow=ow, oh=oh, pieces=pieces, dtype=dtype, layout=layout, stream=stream())
    args.update(kw)
    err = None
    try:
        codec.paste_batch32(**args)
    except mi.LlcompError as e:
        err = e
    torch.cuda.synchronize()
    assert (err is not None) == expect_error, err
    assert err is None or err.status == mi.BAD_ARGS
    host = dbuf.cpu().numpy()
    assert guards_intact(host, dlo, dst.nbytes), "a byte outside the dst batch was written"
    mhost = mbuf.cpu().numpy()
    assert guards_intact(mhost, mlo, maps.nbytes) and np.array_equal(mhost[mlo:mlo + maps.nbytes], maps.reshape(-1).view(np.uint8)), "the maps were written"
    got = host[dlo:dlo + dst.nbytes].copy()
    if expect_error:
        assert np.array_equal(got, dst.reshape(-1).view(np.uint8)), "a refused call wrote"
    return got


@pytest.mark.parametrize("mb", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ("chw", "hwc"))
def test_every_dtype_layout_and_channel_count(mi, codecs, mb, dtype, layout):
    T = mi.compose_tile()
    rng = np.random.default_rng(mb * 10 + ESIZE[dtype])
    for c in (1, 3, 4):
        n, iw, ih, ow, oh = 2, T + 10, 9, T + 7, 9
        src, dst = gen_batch(dtype, n, c, ih, iw, layout, 1), gen_batch(dtype, n, c, oh, ow, layout, 2)
        ids = gen_ids(rng, mb, n, ih, iw)
        pieces = random_pieces32(rng, mb, n, iw, ih, n, ow, oh, 10, ESIZE[dtype], c if dtype == "uint8" and layout == "hwc" else 0)
        pieces.append((0, 1, T - 3, 0, T - 4, 0, 8, ih, [POOL[mb][0], POOL[mb][1], TOP[mb]]))  # across the tiles' border
        want = apply32(src, ids, dst, pieces, layout)
        got = pasted(mi, codecs[c], src, ids, mb, dst, pieces, dtype, layout, moff=(7 if mb == 3 else 4), doff=3 * ESIZE[dtype])
        assert same_bits(got, want) and not same_bits(want, dst), c
        assert same_bits(want, mi.paste32_reference(src, wide_maps(ids, mb), dst, pieces, layout, dtype))


@pytest.mark.parametrize("mb", WIDTHS)
def test_all_16_mask_shifts(mi, codecs, mb):
    """the maps at every byte offset of a unit (4-byte maps: every multiple of 4) against every sx 0..15: one to four or five mask units"""
    rng = np.random.default_rng(mb)
    n, iw, ih, ow, oh, c = 1, 80, 4, 64, 4, 3
    src, dst = gen_batch("uint8", n, c, ih, iw, "chw", 1), gen_batch("uint8", n, c, oh, ow, "chw", 2)
    ids = gen_ids(rng, mb, n, ih, iw)
    for shift in range(16):
        moff = shift if mb == 3 else shift % 4 * 4
        pieces = [(0, 0, (shift * 7) % 16, 0, shift, 0, 47, 2, [POOL[mb][0], POOL[mb][2], TOP[mb]]), (0, 0, 1, 1, (shift * 3) % 16, 2, 33, 2, [POOL[mb][1]], 0x5A)]
        got = pasted(mi, codecs[c], src, ids, mb, dst, pieces, "uint8", "chw", moff=moff, doff=shift)
        assert same_bits(got, apply32(src, ids, dst, pieces, "chw")), shift


@pytest.mark.parametrize("mb", WIDTHS)
def test_256_pieces_on_one_sample(mi, codecs, mb):
    rng = np.random.default_rng(256 + mb)
    n, iw, ih, ow, oh, c = 2, 90, 9, 97, 9, 3
    src, dst = gen_batch("float16", n, c, ih, iw, "chw", 1), gen_batch("float16", n, c, oh, ow, "chw", 2)
    ids = gen_ids(rng, mb, n, ih, iw)
    pieces = []
    for i in range(256):
        w, h = int(rng.integers(1, 30)), int(rng.integers(1, 5))
        pieces.append((1, int(rng.integers(2)), int(rng.integers(0, ow - w + 1)), int(rng.integers(0, oh - h + 1)), int(rng.integers(0, iw - w + 1)),
                       int(rng.integers(0, ih - h + 1)), w, h, [POOL[mb][i % 8]]))
    got = pasted(mi, codecs[c], src, ids, mb, dst, pieces, "float16", "chw", moff=(13 if mb == 3 else 12), doff=2)
    assert same_bits(got, apply32(src, ids, dst, pieces, "chw"))
    assert codecs[c].allocated_bytes() <= codecs[c].paste32_workspace_bytes(2, 256)
    pasted(mi, codecs[c], src, ids, mb, dst, pieces + [pieces[0]], "float16", "chw", expect_error=True)  # 257 on one sample


def test_maps_that_are_their_own_source(mi, codecs):
    rng = np.random.default_rng(78)
    for mb, dtype, layout, c in ((3, "uint8", "hwc", 3), (4, "uint8", "hwc", 4), (4, "float32", "chw", 1)):
        ids, dst_ids = gen_ids(rng, mb, 2, 7, 45), gen_ids(rng, mb, 2, 7, 45)
        as_batch = (lambda a: wide_maps(a, 3)) if mb == 3 else (lambda a: wide_maps(a, 4).view(np.uint8).reshape(2, 7, 45, 4)) if c == 4 else \
            (lambda a: wide_maps(a, 4).view(np.float32).reshape(2, 1, 7, 45))
        pieces = [(0, 1, 2, 1, 0, 0, 40, 6, [POOL[mb][1], POOL[mb][6]]), (1, 0, 0, 0, 3, 1, 33, 5, [POOL[mb][0], POOL[mb][2]])]
        got = pasted(mi, codecs[c], None, ids, mb, as_batch(dst_ids), pieces, dtype, layout, moff=(5 if mb == 3 else 8), doff=4, own_source=True)
        own = as_batch(ids)
        want = mi.paste32_reference(own, own, as_batch(dst_ids), pieces, layout, dtype)
        assert same_bits(got, want) and not same_bits(want, as_batch(dst_ids))


def test_refusals_queue_nothing(mi, codecs):
    rng = np.random.default_rng(1)
    src, dst = gen_batch("uint8", 1, 3, 4, 6, "hwc", 1), gen_batch("uint8", 1, 3, 4, 6, "hwc", 2)
    ids = gen_ids(rng, 3, 1, 4, 6)
    ok = [(0, 0, 0, 0, 0, 0, 3, 2, [1])]
    for kw in (dict(map_bytes=2), dict(map_bytes=5), dict(d_mask=None), dict(d_src=None), dict(d_dst=None), dict(n_src=0),
               dict(pieces=[(0, 0, 0, 0, 0, 0, 7, 2, [1])]), dict(pieces=[(1, 0, 0, 0, 0, 0, 3, 2, [1])]), dict(pieces=[(0, 0, 0, 0, 0, 0, 3, 2, [1], 0x04030201, True)]),
               dict(pieces=[(0, 0, 0, 0, 0, 0, 3, 2, [1], 0x100)]), dict(layout="chw", pieces=[(0, 0, 0, 0, 0, 0, 3, 2, [1], 1, True)])):
        kw = dict(kw)
        pasted(mi, codecs[3], src, ids, 3, dst, kw.pop("pieces", ok), "uint8", kw.pop("layout", "hwc"), expect_error=True, **kw)
    for mbad in (2, 5):
        pasted(mi, codecs[3], src, ids, 3, dst, mi.paste_pieces32(ok, 3), "uint8", "hwc", expect_error=True, map_bytes=mbad)
    for off in (1, 2, 3, 6):  # a 4-byte mask at an address that is no multiple of 4
        pasted(mi, codecs[3], src, ids, 4, dst, ok, "uint8", "hwc", moff=off, expect_error=True)
    assert same_bits(pasted(mi, codecs[3], src, ids, 3, dst, ok, "uint8", "hwc", moff=1), apply32(src, ids, dst, ok, "hwc"))


def test_decode_paste_renumber_boxes_and_targets_on_one_stream(mi, orc):
    """the chain on panoptic maps, on one stream with no synchronisation between the steps: RGB-id maps (ids above 65535) encoded as
    three-channel sliced containers decode as nearest views in U8 HWC at odd addresses; paste_batch32 on the images by segment id;
    paste_batch32 with VALUE_PIXEL pieces on the dst maps, which gives the pasted segments new 3-byte ids; label_boxes32 with the lists
    the caller then knows; label_targets32 INDEX from a segment -> category table.  Every step equals its spec."""
    import torch

    from test_gpu_resized_output import TOut
    from test_gpu_resized_regions import packed

    B, S, T = mi.label_boxes_rows(), mi.label_targets_segment(), mi.compose_tile()
    n, w, h, c = 2, T + 7, B + 9, 3
    assert w * h > S
    rng = np.random.default_rng(2410)
    segments = (0x012345, 0x012346, 0x022345, 0xFF2345, 0x0100FF, 0xFFFFFF)
    ids = blobs(rng, 2 * n, h, w, (0,) + segments)  # frames 0..n-1: the src maps; n..2n-1: the dst maps
    maps = wide_maps(ids, 3)
    conts = [orc.compress_sliced(np.ascontiguousarray(m), 32, 16, False) for m in maps]
    src, dst = gen_batch("float16", n, c, h, w, "chw", 1), gen_batch("float16", n, c, h, w, "chw", 2)
    new_id = {m: 0x800000 + 0x010101 * j for j, m in enumerate(segments)}  # what the pasted segments are called in the dst maps
    rect = (3, 2, 0, 1, w - 3, h - 2)
    by_id = [(d, (d + 1) % n) + rect + ([m for j, m in enumerate(segments) if (j + d) % 2],) for d in range(n)]
    renumber = [(d, (d + 1) % n) + rect + ([m], new_id[m] + d, True) for d in range(n) for j, m in enumerate(segments) if (j + d) % 2]
    lists = [sorted([0, segments[0], segments[3]] + [new_id[m] + d for m in segments]) for d in range(n)]
    category = {new_id[m] + d: 10 + j % 3 for d in range(n) for j, m in enumerate(segments)}
    values = [[category.get(m, 80) for m in l] for l in lists]
    map_codec, img_codec = mi.Codec(2 * n, w, h, 3, 32, 16, False, device=0), mi.Codec(1, 32, 16, c, 32, 16, False, device=0)
    try:
        d_pay, n_pay, d_len = packed(mi, conts)
        src_maps, dst_maps = TOut(n, w, h, 3, "uint8", "hwc", offset=7), TOut(n, w, h, 3, "uint8", "hwc", offset=13)
        sbuf, slo = put(src, 2)
        dbuf, dlo = put(dst, 4)
        total = sum(len(l) for l in lists)
        bbuf, blo = put(np.full(total * 20, 0xA5, np.uint8), 0)
        tbuf, tlo = put(np.full(n * h * w * 8, 0xA5, np.uint8), 8)
        groups = [mi.ViewGroup([(f, 0, 0, w, h) for f in range(n)], w, h, src_maps.ptr, dtype="uint8", layout="hwc", filter="nearest"),
                  mi.ViewGroup([(n + f, 0, 0, w, h) for f in range(n)], w, h, dst_maps.ptr, dtype="uint8", layout="hwc", filter="nearest")]
        map_codec.decode_views(d_pay.data_ptr(), n_pay, d_len.data_ptr(), groups, src_maps.st.data_ptr(), stream())
        img_codec.paste_batch32(sbuf.data_ptr() + slo, src_maps.ptr, 3, n, w, h, dbuf.data_ptr() + dlo, n, w, h, by_id, dtype="float16", layout="chw", stream=stream())
        img_codec.paste_batch32(src_maps.ptr, src_maps.ptr, 3, n, w, h, dst_maps.ptr, n, w, h, renumber, dtype="uint8", layout="hwc", stream=stream())
        img_codec.label_boxes32(dst_maps.ptr, 3, n, w, h, lists, bbuf.data_ptr() + blo, stream=stream())
        img_codec.label_targets32(dst_maps.ptr, 3, n, w, h, lists, values, tbuf.data_ptr() + tlo, dtype="int64", default=255, stream=stream())
        torch.cuda.synchronize()
        (st, s_host), (_, d_host) = src_maps.read(), dst_maps.read()
        assert st == 0 and np.array_equal(s_host, maps[:n])  # the decoded maps are the 3-byte id maps that were encoded
        got_img = dbuf.cpu().numpy()
        assert guards_intact(got_img, dlo, dst.nbytes)
        want_img = apply32(src, ids[:n], dst, by_id, "chw")
        assert same_bits(got_img[dlo:dlo + dst.nbytes], want_img) and not same_bits(want_img, dst)
        want_maps = apply32(maps[:n], ids[:n], maps[n:], renumber, "hwc")
        assert np.array_equal(d_host, want_maps)
        want_ids = ids_of(want_maps)
        assert want_ids.max() > 65535 and np.isin(want_ids, list(category)).any()  # the pasted segments are there, under their new ids
        bhost = bbuf.cpu().numpy()
        assert guards_intact(bhost, blo, total * 20)
        got = as_table(bhost[blo:blo + total * 20].copy().view(mi.LABEL_BOX_DTYPE))
        assert np.array_equal(got, boxes_spec(want_ids, lists))
        pasted_rows = [i for i, m in enumerate(sum(lists, [])) if m >= 0x800000]
        assert got[pasted_rows, 0].sum() > 0
        thost = tbuf.cpu().numpy()
        assert guards_intact(thost, tlo, n * h * w * 8)
        assert np.array_equal(thost[tlo:tlo + n * h * w * 8].copy().view(np.int64).reshape(n, h, w), index_spec(want_ids, lists, values, 255, np.int64))
    finally:
        map_codec.close()
        img_codec.close()
