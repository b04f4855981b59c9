"""Label boxes of listed ids on the GPU (llcomp_mi_codec_label_boxes16; include/llcomp_mi.h: "Label boxes of listed ids"): the pixel
count and the bounding box of every id listed for a sample of a batch of 16-bit id maps in HBM, against numpy -- np.argwhere per listed
id (tests/test_label_boxes16.py) -- record for record, with 256 guard bytes on both sides of the records that have to stay and maps
that have to be byte-identical after the call.  B = label_boxes_rows(), the rows of a workgroup's band, sizes the shapes."""
import numpy as np
import pytest

from batch_support import guards_intact, mi, put, stream  # noqa: F401
from test_label_boxes import as_table
from test_label_boxes16 import HIGH_BYTE, blobs16, label_boxes16_spec, lists_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec(mi):
    k = mi.Codec(1, 32, 16, 3, 32, 16, False, device=0)  # (the codec gives the device: the maps have one channel whatever its c)
    yield k
    k.close()


def run(mi, codec, maps, ids, offset=0, expect_error=False, **kw):
    """label_boxes16 on the numpy maps [n, oh, ow] uint16, `offset` bytes past a 256-byte boundary -> the [total, 5] table of the
    records; the records stand between guard bytes over a pattern of 0xA5, so a record that is not written shows"""
    import torch

    n, oh, ow = maps.shape
    total = sum(len(l) for l in ids)
    mbuf, mlo = put(maps, offset)
    boxes = np.full(total * 20, 0xA5, np.uint8)
    bbuf, blo = put(boxes, 0)
    args = dict(d_maps=mbuf.data_ptr() + mlo, n=n, ow=ow, oh=oh, ids=ids, d_boxes=bbuf.data_ptr() + blo, stream=stream())
    args.update(kw)
    err = None
    try:
        codec.label_boxes16(**args)
    except mi.LlcompError as e:
        err = e
    torch.cuda.synchronize()
    assert (err is not None) == expect_error, err
    assert err is None or err.status == mi.BAD_ARGS
    host = bbuf.cpu().numpy()
    assert guards_intact(host, blo, boxes.nbytes), "a byte outside the records was written"
    mhost = mbuf.cpu().numpy()
    assert guards_intact(mhost, mlo, maps.nbytes) and np.array_equal(mhost[mlo:mlo + maps.nbytes], maps.reshape(-1).view(np.uint8)), "the maps were written"
    got = host[blo:blo + boxes.nbytes].copy()
    if expect_error:
        assert (got == 0xA5).all(), "a refused call wrote records"
        return None
    return as_table(got.view(mi.LABEL_BOX_DTYPE))


@pytest.mark.parametrize("ow", (1, 7, 8, 9, 17, 33))
def test_widths_around_a_unit_by_heights_around_a_band(mi, codec, ow):
    B = mi.label_boxes_rows()
    rng = np.random.default_rng(B + 16 + ow)
    for oh in (1, B - 1, B, B + 1, 2 * B + 3):
        for off in (0, 2, 14):
            pool = HIGH_BYTE if off else (3, 700, 0x8000, 65535, 0)
            maps = blobs16(rng, 2, oh, ow, pool) if off != 2 else np.asarray(pool, np.uint16)[rng.integers(0, len(pool), size=(2, oh, ow))]
            ids = lists_for(rng, maps, pool)
            assert np.array_equal(run(mi, codec, maps, ids, off), label_boxes16_spec(maps, ids)), (ow, oh, off)


@pytest.mark.parametrize("count", [1, 257, 1025, 4096])
def test_a_list_for_each_capacity(mi, codec, count):
    B = mi.label_boxes_rows()
    rng = np.random.default_rng(count)
    listed = np.sort(rng.choice(65536, size=count, replace=False))
    others = np.setdiff1d(np.arange(65536), listed)[:50]
    pool = np.concatenate([listed[:: max(2, count // 300)], others])  # (listed ids with and without a pixel, pixels that are not listed)
    maps = pool[rng.integers(0, len(pool), size=(3, 2 * B + 5, 41))].astype(np.uint16)
    maps[:, 3:B + 3, 2:30] = listed[0]
    ids = [listed.tolist(), [], listed[: count // 2 + 1].tolist()]  # (the sample in the middle gets no workgroup)
    got = run(mi, codec, maps, ids, 6)
    assert np.array_equal(got, label_boxes16_spec(maps, ids))
    assert np.array_equal(got, as_table(mi.label_boxes16_reference(maps, ids)))
    assert codec.allocated_bytes() <= codec.label_boxes16_workspace_bytes(3, 2 * 4096)


def test_one_id_and_empty_lists(mi, codec):
    B = mi.label_boxes_rows()
    one = np.full((1, 2 * B + 1, 70), 0x1234, np.uint16)  # every lane at the same LDS address
    ids = [[0x0034, 0x1200, 0x1234, 0x3412]]
    got = run(mi, codec, one, ids, 4)
    assert np.array_equal(got, label_boxes16_spec(one, ids)) and got[2, 0] == 70 * (2 * B + 1) and got[:, 0].sum() == got[2, 0]
    assert len(run(mi, codec, one, [[]])) == 0  # a call without a listed id queues nothing


def test_refusals_queue_nothing(mi, codec):
    import torch

    maps = np.zeros((2, 4, 5), np.uint16)
    ids = [[0, 3, 9], [1, 2]]
    for kw in (dict(d_maps=None), dict(d_boxes=None), dict(n=1), dict(ow=0), dict(oh=0), dict(ids=[[0, 3, 3], [1, 2]]), dict(ids=[[3, 0, 9], [1, 2]]),
               dict(ids=[list(range(4097)), []]), dict(ids=[[1], [70000]])):
        run(mi, codec, maps, kw.pop("ids", ids), expect_error=True, **kw)
    run(mi, codec, maps, ids, offset=1, expect_error=True)  # maps at an odd address
    L = mi._lib.load()
    buf = torch.zeros(16384, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    flat, first = np.array([0, 3, 9, 1, 2], np.uint16), np.array([0, 3, 5], np.uint32)
    i, f = flat.ctypes.data, first.ctypes.data
    bad_first = np.array([0, 4, 3], np.uint32)
    for args in ((None, p, 2, 5, 4, i, f, p + 4096), (codec._h, p, 2, 5, 4, i, f, p + 4098), (codec._h, p, 2, 5, 4, i, f, p + 76), (codec._h, p, 2, 5, 4, None, f, p + 4096),
                 (codec._h, p, 2, 5, 4, i, None, p + 4096), (codec._h, p, 2, 5, 4, i, bad_first.ctypes.data, p + 4096),
                 (codec._h, p + 4096 + 99, 2, 5, 4, i, f, p + 4096), (codec._h, p + 4096 + 98, 2, 5, 4, i, f, p + 4096),
                 (codec._h, p + 4096 - 78, 2, 5, 4, i, f, p + 4096)):
        assert L.llcomp_mi_codec_label_boxes16(*args, stream()) == mi.BAD_ARGS, args[1:]
    assert L.llcomp_mi_codec_label_boxes16(codec._h, p + 4096 - 80, 2, 5, 4, i, f, p + 4096, stream()) == mi.OK  # touching is fine
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert not host[:4096].any() and not host[4096 + 100:].any()
    recs = host[4096:4096 + 100].view(mi.LABEL_BOX_DTYPE)
    assert tuple(recs[0]) == (20, 0, 0, 5, 4) and tuple(recs[1]) == (0, 5, 4, 0, 0) and tuple(recs[4]) == (0, 5, 4, 0, 0)


def test_decode_paste16_renumber_and_boxes_on_one_stream(mi, orc):
    """the chain on 16-bit instance maps, on one stream with no synchronisation between the steps: u16 maps encoded as two-channel
    sliced containers (low byte in channel 0) decode as nearest-filter views in U8 HWC -- the maps that were encoded; paste_batch16 on
    the images by instance id; paste_batch16 with VALUE pieces through a c == 1 codec and a 2-byte dtype, which gives the pasted
    instances ids above 255 in the dst maps; label_boxes16 on the dst maps with the lists the caller then knows.  Equal to the specs of
    all three steps."""
    import torch

    import paste16_spec
    from test_gpu_resized_output import TOut
    from test_gpu_resized_regions import packed

    B, T = mi.label_boxes_rows(), mi.compose_tile()
    n, w, h, c = 2, T + 7, B + 9, 3
    rng = np.random.default_rng(1216)
    classes = (24000, 24001, 26000, 26001, 26002, 33000)  # class * 1000 + k
    maps = blobs16(rng, 2 * n, h, w, (0,) + classes)  # frames 0..n-1: the src maps; n..2n-1: the dst maps
    conts = [orc.compress_sliced(np.ascontiguousarray(m.view(np.uint8).reshape(h, w, 2)), 32, 16, False) for m in maps]
    src = paste16_spec.gen_batch("float16", n, c, h, w, "chw", seed=1)
    dst = paste16_spec.gen_batch("float16", n, c, h, w, "chw", seed=2)
    new_id = {m: 40000 + 10 * j for j, m in enumerate(classes)}  # what the pasted instances are called in the dst maps
    rect = (3, 2, 0, 1, w - 3, h - 2)
    by_id = [(d, (d + 1) % n) + rect + ([m for m in classes if (m + d) % 2],) for d in range(n)]
    renumber = [(d, (d + 1) % n) + rect + ([m], new_id[m] + d) for d in range(n) for m in classes if (m + d) % 2]
    lists = [sorted([0, 24000, 26001] + [new_id[m] + d for m in classes]) for d in range(n)]
    map_codec, img_codec, id_codec = (mi.Codec(2 * n, w, h, 2, 32, 16, False, device=0), mi.Codec(1, 32, 16, c, 32, 16, False, device=0),
                                      mi.Codec(1, 32, 16, 1, 32, 16, False, device=0))
    try:
        d_pay, n_pay, d_len = packed(mi, conts)
        src_maps, dst_maps = TOut(n, w, h, 2, "uint8", "hwc", offset=6), TOut(n, w, h, 2, "uint8", "hwc", offset=10)
        sbuf, slo = put(src, 2)
        dbuf, dlo = put(dst, 4)
        total = sum(len(l) for l in lists)
        boxes = np.full(total * 20, 0xA5, np.uint8)
        bbuf, blo = put(boxes, 0)
        groups = [mi.ViewGroup([(f, 0, 0, w, h) for f in range(n)], w, h, src_maps.ptr, dtype="uint8", layout="hwc", filter="nearest"),
                  mi.ViewGroup([(n + f, 0, 0, w, h) for f in range(n)], w, h, dst_maps.ptr, dtype="uint8", layout="hwc", filter="nearest")]
        map_codec.decode_views(d_pay.data_ptr(), n_pay, d_len.data_ptr(), groups, src_maps.st.data_ptr(), stream())
        img_codec.paste_batch16(sbuf.data_ptr() + slo, src_maps.ptr, n, w, h, dbuf.data_ptr() + dlo, n, w, h, by_id, dtype="float16", layout="chw", stream=stream())
        id_codec.paste_batch16(src_maps.ptr, src_maps.ptr, n, w, h, dst_maps.ptr, n, w, h, renumber, dtype="bfloat16", layout="chw", stream=stream())
        id_codec.label_boxes16(dst_maps.ptr, n, w, h, lists, bbuf.data_ptr() + blo, stream=stream())
        torch.cuda.synchronize()
        (st, s_host), (_, d_host) = src_maps.read(), dst_maps.read()
        assert st == 0
        s_host = np.ascontiguousarray(s_host).reshape(n, h, 2 * w).view(np.uint16)
        assert np.array_equal(s_host, maps[:n])  # the decoded maps are the u16 maps that were encoded
        got_img = dbuf.cpu().numpy()
        assert guards_intact(got_img, dlo, dst.nbytes)
        want_img = paste16_spec.apply(src, maps[:n], dst, by_id, "chw")
        assert np.array_equal(got_img[dlo:dlo + dst.nbytes].view(np.uint16), paste16_spec.bits_of(want_img).reshape(-1))
        assert not np.array_equal(paste16_spec.bits_of(want_img), paste16_spec.bits_of(dst))
        want_maps = paste16_spec.apply(maps[:n, None], maps[:n], maps[n:, None], renumber, "chw")[:, 0]
        assert np.array_equal(np.ascontiguousarray(d_host).reshape(n, h, 2 * w).view(np.uint16), want_maps)
        bhost = bbuf.cpu().numpy()
        assert guards_intact(bhost, blo, boxes.nbytes)
        got = as_table(bhost[blo:blo + boxes.nbytes].copy().view(mi.LABEL_BOX_DTYPE))
        assert np.array_equal(got, label_boxes16_spec(want_maps, lists))
        pasted = [i for i, m in enumerate(sum(lists, [])) if m >= 40000]
        assert got[pasted, 0].sum() > 0 and want_maps.max() > 255  # (the pasted instances are there, under ids above 255)
    finally:
        map_codec.close()
        img_codec.close()
        id_codec.close()
