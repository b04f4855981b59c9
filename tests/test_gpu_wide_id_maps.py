"""The calls on id maps of 3 and 4 bytes per pixel on the GPU (llcomp_mi_codec_label_boxes32, llcomp_mi_codec_label_targets32;
include/llcomp_mi.h: "Wide id maps") against the numpy specs of tests/test_wide_id_maps_rule.py and against the host references, exactly.
Every output stands over a pattern of 0xA5 between 256 guard bytes on both sides, and the maps have to be byte-identical after every
call.  B = label_boxes_rows(), the rows of a band, and S = label_targets_segment(), the pixels of a segment, size the shapes."""
import numpy as np
import pytest

from batch_support import ESIZE, guards_intact, mi, put, stream  # noqa: F401
from test_label_boxes import as_table
from test_label_targets import index_spec, planes_spec
from test_wide_id_maps_rule import BOX_OFFSETS, TOP, WIDTHS, blobs, boxes_spec, draw, ids_of, wide_maps

pytestmark = pytest.mark.gpu

INDEX_ESIZE = {"uint8": 1, "int32": 4, "int64": 8}


@pytest.fixture(scope="module")
def codec(mi):
    k = mi.Codec(1, 32, 16, 3, 32, 16, False, device=0)  # (the codec gives the device: the maps have one channel whatever its c)
    yield k
    k.close()


def call_on(mi, maps, out_bytes, moff, ooff, expect_error, call):
    """call(d_maps, d_out) on the host maps of either width, `moff` bytes past a 256-byte boundary, and an output of out_bytes of 0xA5,
    `ooff` bytes past one -> the output's bytes, or None for a call that was refused and wrote nothing"""
    import torch

    mbuf, mlo = put(maps, moff)
    out = np.full(out_bytes, 0xA5, np.uint8)
    obuf, olo = put(out, ooff)
    err = None
    try:
        call(mbuf.data_ptr() + mlo, obuf.data_ptr() + olo)
    except mi.LlcompError as e:
        err = e
    torch.cuda.synchronize()
    assert (err is not None) == expect_error, err
    assert err is None or err.status == mi.BAD_ARGS
    host = obuf.cpu().numpy()
    assert guards_intact(host, olo, out.nbytes), "a byte outside the output was written"
    mhost = mbuf.cpu().numpy()
    assert guards_intact(mhost, mlo, maps.nbytes) and np.array_equal(mhost[mlo:mlo + maps.nbytes], maps.reshape(-1).view(np.uint8)), "the maps were written"
    got = host[olo:olo + out.nbytes].copy()
    if expect_error:
        assert (got == 0xA5).all(), "a refused call wrote"
        return None
    return got


def boxes(mi, codec, ids, mb, lists, moff=0, expect_error=False, **kw):
    """label_boxes32 on the ids [n, oh, ow] as maps of mb bytes per pixel -> the [total, 5] table of the records"""
    n, oh, ow = ids.shape
    args = dict(map_bytes=mb, n=n, ow=ow, oh=oh, ids=lists, stream=stream())
    args.update(kw)
    total = sum(len(l) for l in lists)
    got = call_on(mi, wide_maps(ids, mb), total * 20, moff, 0, expect_error,
                  lambda m, o: codec.label_boxes32(**{"d_maps": m, "d_boxes": o, **args}))
    return None if got is None else as_table(got.view(mi.LABEL_BOX_DTYPE))


def targets(mi, codec, ids, mb, lists, values, moff=0, ooff=0, expect_error=False, **kw):
    """label_targets32 on the ids [n, oh, ow] as maps of mb bytes per pixel -> the output's bytes"""
    n, oh, ow = ids.shape
    index = kw.get("kind", "index") == "index"
    es = INDEX_ESIZE[kw.get("dtype") or "int64"] if index else ESIZE[kw.get("dtype") or "uint8"]
    elements = n * oh * ow if index else sum(kw["planes"]) * oh * ow
    args = dict(map_bytes=mb, n=n, ow=ow, oh=oh, ids=lists, values=values, stream=stream())
    args.update(kw)
    return call_on(mi, wide_maps(ids, mb), elements * es, moff, ooff, expect_error,
                   lambda m, o: codec.label_targets32(**{"d_maps": m, "d_out": o, **args}))


def target_spec(ids, lists, values, kind="index", dtype=None, default=0, planes=None, on=1, off=0):
    if kind == "index":
        return index_spec(ids, lists, values, default, dtype or "int64").reshape(-1).view(np.uint8)
    return planes_spec(ids, lists, values, default, planes, on, off, dtype or "uint8").reshape(-1).view(np.uint8)


@pytest.mark.parametrize("mb", WIDTHS)
@pytest.mark.parametrize("ow", (1, 5, 6, 7, 11, 16, 17, 33))
def test_boxes_widths_around_a_unit_by_heights_around_a_band(mi, codec, mb, ow):
    B = mi.label_boxes_rows()
    rng = np.random.default_rng(32 * mb + ow)
    for oh in (1, B - 1, B, B + 1, 2 * B + 3):
        for off in BOX_OFFSETS[mb]:
            ids, lists = draw(rng, mb, 3, oh, ow, noise=off in (2, 4))
            assert np.array_equal(boxes(mi, codec, ids, mb, lists, off), boxes_spec(ids, lists)), (ow, oh, off)


@pytest.mark.parametrize("mb", WIDTHS)
@pytest.mark.parametrize("count", [1, 257, 1025, 4096])
def test_boxes_a_list_for_each_capacity(mi, codec, mb, count):
    B = mi.label_boxes_rows()
    rng = np.random.default_rng(count + mb)
    listed = np.concatenate([np.unique(rng.integers(0, TOP[mb], size=count + 64))[:count - 1], [TOP[mb]]])  # (the top id listed last, and present)
    others = rng.integers(0, TOP[mb] + 1, size=50)
    pool = np.concatenate([listed[:: max(2, count // 300)], listed[-1:], others])
    ids = pool[rng.integers(0, len(pool), size=(3, 2 * B + 5, 41))].astype(np.int64)
    ids[:, 3:B + 3, 2:30] = listed[0]
    lists = [listed.tolist(), [], listed[: count // 2 + 1].tolist()]  # (the sample in the middle gets no workgroup)
    got = boxes(mi, codec, ids, mb, lists, BOX_OFFSETS[mb][-1])
    assert np.array_equal(got, boxes_spec(ids, lists))
    assert np.array_equal(got, as_table(mi.label_boxes32_reference(wide_maps(ids, mb), lists)))
    assert got[len(listed) - 1, 0] == (ids[0] == TOP[mb]).sum() > 0  # the top id is counted
    assert codec.allocated_bytes() <= codec.label_boxes32_workspace_bytes(3, 2 * 4096)


@pytest.mark.parametrize("mb", WIDTHS)
def test_boxes_one_id_in_every_pixel_the_top_id_and_empty_lists(mi, codec, mb):
    B = mi.label_boxes_rows()
    for m in (0x123456, TOP[mb]):
        one = np.full((1, 2 * B + 1, 70), m, np.int64)  # every lane at the same LDS address
        lists = [sorted({0x000056, 0x120000, 0x123456, 0x563412, m})]
        got = boxes(mi, codec, one, mb, lists, BOX_OFFSETS[mb][1])
        j = lists[0].index(m)
        assert np.array_equal(got, boxes_spec(one, lists)) and got[j, 0] == 70 * (2 * B + 1) and got[:, 0].sum() == got[j, 0]
        got = boxes(mi, codec, one, mb, [[1, 2]])  # present and not listed: counted nowhere
        assert got[:, 0].sum() == 0
    assert len(boxes(mi, codec, one, mb, [[]])) == 0  # a call without a listed id queues nothing


CASES = [dict(dtype="uint8", default=255), dict(dtype="int32", default=-1), dict(dtype="int64", default=-100),
         dict(kind="planes", dtype="uint8", default=0, planes=[3, 0, 2], on=255, off=7),
         dict(kind="planes", dtype="float16", default=1, planes=[3, 0, 2], on=0.9, off=0.05),
         dict(kind="planes", dtype="bfloat16", default=-1, planes=[3, 0, 2]),
         dict(kind="planes", dtype="float32", default=2, planes=[3, 0, 2], on=0.9, off=0.05)]


@pytest.mark.parametrize("mb", WIDTHS)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_targets_pixel_counts_around_a_segment(mi, codec, mb, case):
    """three samples, the middle one with an empty list and no planes; the boxes' map offsets; the output at none, one element and 16
    bytes less one element; values that several ids share; an "ignore" default"""
    kw = CASES[case]
    S = mi.label_targets_segment()
    rng = np.random.default_rng(100 * mb + case)
    index = "kind" not in kw
    es = INDEX_ESIZE[kw["dtype"]] if index else ESIZE[kw["dtype"]]
    for oh, ow in ((7, 585), (64, 64), (17, 241), (7, 1171)):
        assert oh * ow in (S - 1, S, S + 1, 2 * S + 5)
        ids, lists = draw(rng, mb, 3, oh, ow)
        hi = 256 if kw["dtype"] == "uint8" and index else 4
        values = [rng.integers(0 if hi == 256 else -1, hi, size=len(l)).tolist() for l in lists]
        want = target_spec(ids, lists, values, **kw)
        assert np.array_equal(want, mi.label_targets32_reference(wide_maps(ids, mb), lists, values, **kw).reshape(-1).view(np.uint8))
        for k, moff in enumerate(BOX_OFFSETS[mb]):
            ooff = (0, es, 16 - es)[k % 3]
            assert np.array_equal(targets(mi, codec, ids, mb, lists, values, moff, ooff, **kw), want), (oh, ow, moff, ooff)


@pytest.mark.parametrize("mb", WIDTHS)
@pytest.mark.parametrize("count", [1, 257, 1025, 4096])
def test_targets_a_list_for_each_capacity(mi, codec, mb, count):
    S = mi.label_targets_segment()
    rng = np.random.default_rng(count + 7 * mb)
    listed = np.concatenate([np.unique(rng.integers(0, TOP[mb], size=count + 64))[:count - 1], [TOP[mb]]])
    others = rng.integers(0, TOP[mb] + 1, size=50)
    pool = np.concatenate([listed[:: max(2, count // 300)], listed[-1:], others])
    ids = pool[rng.integers(0, len(pool), size=(3, 5, S // 5 + 13))].astype(np.int64)
    lists = [listed.tolist(), [], listed[: count // 2 + 1].tolist()]
    values = [(np.arange(len(l)) % 11 - 1).tolist() for l in lists]
    got = targets(mi, codec, ids, mb, lists, values, BOX_OFFSETS[mb][1], 8, default=-100)
    assert np.array_equal(got, target_spec(ids, lists, values, default=-100))
    kw = dict(kind="planes", dtype="float16", default=-1, planes=[10, 3, 0])
    assert np.array_equal(targets(mi, codec, ids, mb, lists, values, BOX_OFFSETS[mb][-1], 2, **kw), target_spec(ids, lists, values, **kw))
    assert codec.allocated_bytes() <= max(codec.label_targets32_workspace_bytes(3, 2 * 4096), codec.label_boxes32_workspace_bytes(3, 2 * 4096))


def test_the_same_content_through_the_widths_1_2_3_and_4(mi, codec):
    """ids below 256 through label_boxes, label_boxes16 and label_boxes32, label_targets and label_targets32: the same bytes"""
    import torch

    B = mi.label_boxes_rows()
    ow, oh = 37, B + 1
    rng = np.random.default_rng(B)
    narrow = rng.integers(0, 12, size=(2, oh, ow), dtype=np.uint8)
    narrow[0, 5:20, 3:30] = 200
    narrow[1, B - 1:, :] = 255
    everything = [list(range(256))] * 2
    lists, values = [[0, 3, 7, 200], [1, 2, 255]], [[1, 1, 2, 0], [0, 2, 2]]

    def old(call, m, out_bytes, offset, *args, **kw):
        mbuf, mlo = put(m, offset)
        obuf, olo = put(np.full(out_bytes, 0xA5, np.uint8), 0)
        getattr(codec, call)(mbuf.data_ptr() + mlo, 2, ow, oh, *args, obuf.data_ptr() + olo, stream=stream(), **kw)
        torch.cuda.synchronize()
        host = obuf.cpu().numpy()
        assert guards_intact(host, olo, out_bytes)
        return host[olo:olo + out_bytes].copy()

    by_bytes = as_table(old("label_boxes", narrow, 2 * 256 * 20, 5).view(mi.LABEL_BOX_DTYPE))
    by_words = as_table(old("label_boxes16", narrow.astype(np.uint16), 2 * 256 * 20, 6, everything).view(mi.LABEL_BOX_DTYPE))
    index = old("label_targets", narrow, 2 * ow * oh * 8, 3, lists, values, default=-5)
    assert np.array_equal(by_bytes, by_words)
    for mb in WIDTHS:
        assert np.array_equal(boxes(mi, codec, narrow, mb, everything, 16 - mb), by_bytes), mb
        assert np.array_equal(targets(mi, codec, narrow, mb, lists, values, 16 - mb, 8, default=-5), index), mb


def test_refusals_queue_nothing_and_write_nothing(mi, codec):
    import torch

    ids = np.zeros((2, 4, 5), np.int64)
    lists = [[0, 3, 9], [1, 2]]
    for mb in WIDTHS:
        for kw in (dict(d_maps=None), dict(d_boxes=None), dict(n=1), dict(ow=0), dict(oh=0), dict(ids=[[0, 3, 3], [1, 2]]), dict(ids=[[3, 0, 9], [1, 2]]),
                   dict(ids=[list(range(4097)), []]), dict(map_bytes=1), dict(map_bytes=2), dict(map_bytes=5), dict(map_bytes=0)):
            boxes(mi, codec, ids, mb, kw.pop("ids", lists), expect_error=True, **kw)
        for kw in (dict(d_maps=None), dict(d_out=None), dict(ow=0), dict(ids=[[0, 3, 3], [1, 2]]), dict(dtype="uint8", default=256), dict(kind="planes", planes=[1, 5000])):
            targets(mi, codec, ids, mb, kw.pop("ids", lists), [[0, 1, 2], [3, 4]], expect_error=True, **kw)
    boxes(mi, codec, ids, 3, [[1], [1 << 24]], expect_error=True)  # an id above 0xFFFFFF in a 3-byte map
    targets(mi, codec, ids, 3, [[1], [1 << 24]], [[0], [0]], expect_error=True)
    for off in (1, 2, 3, 6):  # a 4-byte map at an address that is no multiple of 4
        boxes(mi, codec, ids, 4, lists, off, expect_error=True)
        targets(mi, codec, ids, 4, lists, [[0, 1, 2], [3, 4]], off, expect_error=True)
    L = mi._lib.load()
    buf = torch.zeros(16384, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    flat, first = np.array([0, 3, 9, 1, 2], np.uint32), np.array([0, 3, 5], np.uint32)
    i, f = flat.ctypes.data, first.ctypes.data
    for args in ((None, p, 4, 2, 5, 4, i, f, p + 4096), (codec._h, p, 4, 2, 5, 4, i, f, p + 4098), (codec._h, p, 4, 2, 5, 4, i, f, p + 156), (codec._h, p, 4, 2, 5, 4, None, f, p + 4096),
                 (codec._h, p, 4, 2, 5, 4, i, None, p + 4096), (codec._h, p + 4096 + 96, 3, 2, 5, 4, i, f, p + 4096), (codec._h, p + 4096 - 119, 3, 2, 5, 4, i, f, p + 4096)):
        assert L.llcomp_mi_codec_label_boxes32(*args, stream()) == mi.BAD_ARGS, args[1:]
    assert L.llcomp_mi_codec_label_boxes32(codec._h, p + 4096 - 120, 3, 2, 5, 4, i, f, p + 4096, stream()) == mi.OK  # touching is fine
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert not host[:4096].any() and not host[4096 + 100:].any()
    recs = host[4096:4096 + 100].view(mi.LABEL_BOX_DTYPE)
    assert tuple(recs[0]) == (20, 0, 0, 5, 4) and tuple(recs[1]) == (0, 5, 4, 0, 0) and tuple(recs[4]) == (0, 5, 4, 0, 0)


def test_decode_rgb_id_maps_boxes_and_targets_on_one_stream(mi, orc):
    """the chain on panoptic maps, on one stream with no synchronisation between the steps: random RGB-id maps (id = R + 256 G +
    65536 B, ids above 65535) encoded as three-channel sliced containers decode as nearest-filter views in U8 HWC at an odd address --
    the 3-byte id maps that were encoded; label_boxes32 on them with the segment ids the caller knows; label_targets32 INDEX from a
    segment -> category table.  Every step equals its spec.  (The copy-paste steps of a Copy-Paste on such maps are not built.)"""
    import torch

    from test_gpu_resized_output import TOut
    from test_gpu_resized_regions import packed

    B, S = mi.label_boxes_rows(), mi.label_targets_segment()
    n, w, h = 2, 107, B + 9
    assert w * h > S  # (more than one segment, more than one band)
    rng = np.random.default_rng(2409)
    segments = (0x012345, 0x012346, 0x022345, 0xFF2345, 0x0100FF, 0xFFFFFF)  # ids that share low bytes
    ids = blobs(rng, n, h, w, (0,) + segments)
    maps = wide_maps(ids, 3)
    conts = [orc.compress_sliced(np.ascontiguousarray(m), 32, 16, False) for m in maps]
    lists = [sorted(segments), sorted(segments[:4] + (0x000001,))]
    category = {m: 10 + j % 3 for j, m in enumerate(segments)}  # several segments share a category
    values = [[category.get(m, 80) for m in l] for l in lists]
    map_codec, any_codec = mi.Codec(n, w, h, 3, 32, 16, False, device=0), mi.Codec(1, 32, 16, 3, 32, 16, False, device=0)
    try:
        d_pay, n_pay, d_len = packed(mi, conts)
        d_maps = TOut(n, w, h, 3, "uint8", "hwc", offset=7)
        total = sum(len(l) for l in lists)
        bbuf, blo = put(np.full(total * 20, 0xA5, np.uint8), 0)
        tbuf, tlo = put(np.full(n * h * w * 8, 0xA5, np.uint8), 8)
        groups = [mi.ViewGroup([(f, 0, 0, w, h) for f in range(n)], w, h, d_maps.ptr, dtype="uint8", layout="hwc", filter="nearest")]
        map_codec.decode_views(d_pay.data_ptr(), n_pay, d_len.data_ptr(), groups, d_maps.st.data_ptr(), stream())
        any_codec.label_boxes32(d_maps.ptr, 3, n, w, h, lists, bbuf.data_ptr() + blo, stream=stream())
        any_codec.label_targets32(d_maps.ptr, 3, n, w, h, lists, values, tbuf.data_ptr() + tlo, dtype="int64", default=255, stream=stream())
        torch.cuda.synchronize()
        st, m_host = d_maps.read()
        assert st == 0 and np.array_equal(m_host, maps) and np.array_equal(ids_of(m_host), ids) and ids.max() > 65535
        bhost = bbuf.cpu().numpy()
        assert guards_intact(bhost, blo, total * 20)
        got = as_table(bhost[blo:blo + total * 20].copy().view(mi.LABEL_BOX_DTYPE))
        assert np.array_equal(got, boxes_spec(ids, lists)) and got[:, 0].sum() > 0
        thost = tbuf.cpu().numpy()
        assert guards_intact(thost, tlo, n * h * w * 8)
        assert np.array_equal(thost[tlo:tlo + n * h * w * 8].copy().view(np.int64).reshape(n, h, w), index_spec(ids, lists, values, 255, np.int64))
    finally:
        map_codec.close()
        any_codec.close()
