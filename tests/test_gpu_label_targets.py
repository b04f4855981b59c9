"""Label targets on the GPU (llcomp_mi_codec_label_targets; include/llcomp_mi.h: "Label targets"): the class-index tensor, the one-hot
planes and the instance masks of a batch of id maps in HBM, against the numpy spec of tests/test_label_targets.py and against
llcomp_mi_label_targets_reference, byte for byte.  The output stands over a pattern of 0xA5 between 256 guard bytes on both sides, so
an element that is not written shows and so does a byte written outside; the maps have to be byte-identical after the call.
S = label_targets_segment(), the pixels of a workgroup's segment, sizes the shapes."""
import ctypes as C

import numpy as np
import pytest

from batch_support import ESIZE, guards_intact, mi, put, stream  # noqa: F401
from test_label_boxes import as_table
from test_label_boxes16 import blobs16
from test_label_targets import draw, index_spec, planes_spec, shapes, value_spec

pytestmark = pytest.mark.gpu

CHUNK = 32  # planes of a workgroup (label_targets_rule.hpp: kTargetPlaneChunk)
INDEX_ESIZE = {"uint8": 1, "int32": 4, "int64": 8}


@pytest.fixture(scope="module")
def codec(mi):
    k = mi.Codec(1, 32, 16, 3, 32, 16, False, device=0)  # (the codec gives the device: the maps have one channel whatever its c)
    yield k
    k.close()


def counts_of(planes, n):
    return [planes] * n if isinstance(planes, int) else list(planes)


def spec(maps, ids, values, kind="index", dtype=None, default=0, planes=None, on=1, off=0):
    """the numpy spec of a call, flat, as the bytes of the output"""
    if kind == "index":
        return index_spec(maps, ids, values, default, dtype or "int64").reshape(-1).view(np.uint8)
    return planes_spec(maps, ids, values, default, counts_of(planes, len(maps)), on, off, dtype or "uint8").reshape(-1).view(np.uint8)


def run(mi, codec, maps, ids, values, moff=0, ooff=0, expect_error=False, call=None, **kw):
    """label_targets on the numpy maps [n, oh, ow], `moff` bytes past a 256-byte boundary, into an output `ooff` bytes past one -> the
    output's bytes; call: other arguments of the call itself"""
    import torch

    n, oh, ow = maps.shape
    es = INDEX_ESIZE[kw.get("dtype") or "int64"] if kw.get("kind", "index") == "index" else ESIZE[kw.get("dtype") or "uint8"]
    elements = n * oh * ow if kw.get("kind", "index") == "index" else sum(counts_of(kw["planes"], n)) * oh * ow
    mbuf, mlo = put(maps, moff)
    out = np.full(elements * es, 0xA5, np.uint8)
    obuf, olo = put(out, ooff)
    args = dict(d_maps=mbuf.data_ptr() + mlo, n=n, ow=ow, oh=oh, ids=ids, values=values, d_out=obuf.data_ptr() + olo, map_dtype=str(maps.dtype), stream=stream())
    args.update(kw)
    args.update(call or {})
    err = None
    try:
        codec.label_targets(**args)
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


CASES = [(np.uint8, dict(dtype="uint8", default=255)), (np.uint8, dict(dtype="int32", default=-100)), (np.uint8, dict(dtype="int64", default=-100)),
         (np.uint8, dict(kind="planes", dtype="uint8", default=-1, planes=[3, 0, 2])),
         (np.uint8, dict(kind="planes", dtype="float16", default=1, planes=[3, 0, 2], on=0.9, off=0.05)),
         (np.uint8, dict(kind="planes", dtype="float32", default=0, planes=[3, 0, 2])),
         (np.uint16, dict(dtype="uint8", default=0)), (np.uint16, dict(dtype="int32", default=-1)), (np.uint16, dict(dtype="int64", default=-100)),
         (np.uint16, dict(kind="planes", dtype="uint8", default=0, planes=[3, 0, 2], on=255, off=7)),
         (np.uint16, dict(kind="planes", dtype="bfloat16", default=-1, planes=[3, 0, 2])),
         (np.uint16, dict(kind="planes", dtype="float32", default=2, planes=[3, 0, 2], on=0.9, off=0.05))]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_pixel_counts_around_a_segment_at_every_offset(mi, codec, case):
    """three samples, the middle one with an empty list and no planes; every map offset of a 16-byte unit; the output at none, one
    element and 16 bytes less one element"""
    map_dtype, kw = CASES[case]
    rng = np.random.default_rng(100 + case)
    es = INDEX_ESIZE[kw["dtype"]] if "kind" not in kw else ESIZE[kw["dtype"]]
    for oh, ow in shapes(mi.label_targets_segment()):
        maps, ids = draw(rng, map_dtype, 3, oh, ow)
        hi = 256 if kw["dtype"] == "uint8" and "kind" not in kw else 5
        values = [rng.integers(0 if hi == 256 else -1, hi, size=len(l)).tolist() for l in ids]
        want = spec(maps, ids, values, **kw)
        assert np.array_equal(want, mi.label_targets_reference(maps, ids, values, **kw).reshape(-1).view(np.uint8))
        for moff in range(0, 16, maps.itemsize):
            for ooff in (0, es, 16 - es):
                assert np.array_equal(run(mi, codec, maps, ids, values, moff, ooff, **kw), want), (oh, ow, moff, ooff)


@pytest.mark.parametrize("count", [1, 256, 257, 1024, 1025, 4096])
def test_a_list_for_each_capacity(mi, codec, count):
    S = mi.label_targets_segment()
    rng = np.random.default_rng(count)
    listed = np.sort(rng.choice(65536, size=count, replace=False))
    others = np.setdiff1d(np.arange(65536), listed)[:50]
    pool = np.concatenate([listed[:: max(2, count // 300)], others])  # (listed ids with and without a pixel, pixels that are not listed)
    maps = pool[rng.integers(0, len(pool), size=(3, 5, S // 5 + 13))].astype(np.uint16)
    ids = [listed.tolist(), [], listed[: count // 2 + 1].tolist()]
    values = [(np.arange(len(l)) % 11 - 1).tolist() for l in ids]
    for kw in (dict(default=-100), dict(kind="planes", dtype="float16", default=-1, planes=[10, 0, 3])):
        got = run(mi, codec, maps, ids, values, 6, 16 - (8 if "kind" not in kw else 2), **kw)
        assert np.array_equal(got, spec(maps, ids, values, **kw))
        assert np.array_equal(got, mi.label_targets_reference(maps, ids, values, **kw).reshape(-1).view(np.uint8))
    assert codec.allocated_bytes() <= codec.label_targets_workspace_bytes(3, 2 * 4096)
    if count <= 256:  # 1-byte maps hold up to all 256 ids
        narrow = rng.integers(0, 256, size=(2, 3, S // 3 + 5), dtype=np.uint8)
        nids = [np.sort(rng.choice(256, size=count, replace=False)).tolist(), list(range(0, 256, 3))]
        nvalues = [(np.arange(len(l)) % 7).tolist() for l in nids]
        assert np.array_equal(run(mi, codec, narrow, nids, nvalues, 3, 1, dtype="uint8", default=9), spec(narrow, nids, nvalues, dtype="uint8", default=9))


@pytest.mark.parametrize("planes", [1, CHUNK, CHUNK + 1, 4096])
def test_plane_counts_around_a_chunk(mi, codec, planes):
    S = mi.label_targets_segment()
    assert mi.label_targets_max_planes() == 4096
    rng = np.random.default_rng(planes)
    oh, ow = (3, 13) if planes == 4096 else (7, S // 7 + 9)  # (the most planes at P <= S)
    maps = rng.integers(0, 60, size=(3, oh, ow)).astype(np.uint8)
    ids = [list(range(0, 50)), list(range(0, 50)), []]
    values = [rng.integers(-1, planes + 2, size=50).tolist() for _ in range(2)] + [[]]
    counts = [planes, 0, max(planes - 1, 2)]  # (a sample with a list and no planes, one with planes and no list)
    for dtype, ooff in (("uint8", 1), ("bfloat16", 14), ("float32", 4)):
        kw = dict(kind="planes", dtype=dtype, default=planes // 2, planes=counts)
        got = run(mi, codec, maps, ids, values, 5, ooff, **kw)
        assert np.array_equal(got, spec(maps, ids, values, **kw))
    assert run(mi, codec, maps, ids, values, kind="planes", planes=[0, 0, 0]).size == 0  # a call without a plane queues nothing


def test_refusals_queue_nothing(mi, codec):
    import torch

    maps = np.zeros((2, 4, 5), np.uint16)
    ids, values = [[0, 3, 9], [1, 2]], [[0, 1, 2], [3, 4]]
    for kw in (dict(call=dict(d_maps=None)), dict(call=dict(d_out=None)), dict(call=dict(ow=0)), dict(call=dict(oh=0)), dict(call=dict(ids=[[0, 3, 3], [1, 2]])),
               dict(call=dict(ids=[[3, 0, 9], [1, 2]])), dict(call=dict(ids=[list(range(4097)), []], values=[[0] * 4097, []])), dict(moff=1), dict(ooff=4),
               dict(call=dict(map_dtype="uint8", ids=[[0, 3, 300], [1, 2]])), dict(dtype="uint8", call=dict(values=[[0, 1, 256], [3, 4]])),
               dict(dtype="uint8", default=-1), dict(kind="planes", planes=[2, 4097]), dict(kind="planes", dtype="float16", planes=2, ooff=1)):
        run(mi, codec, maps, ids, values, expect_error=True, **kw)
    L = mi._lib.load()
    T = mi._lib.LabelTargets
    buf = torch.zeros(16384, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    flat, vals, first, pf = np.array([0, 3, 9, 1, 2], np.uint16), np.array([0, 1, 2, 3, 4], np.int32), np.array([0, 3, 5], np.uint32), np.array([0, 1, 2], np.uint32)

    def targets(**kw):
        f = dict(struct_size=C.sizeof(T), map_bytes=2, kind=mi.TARGET_INDEX, dtype=mi.TARGET_I32, default_value=7, on_bits=1, off_bits=0, ids=flat.ctypes.data,
                 values=vals.ctypes.data, first=first.ctypes.data, plane_first=pf.ctypes.data)
        f.update(kw)
        return C.byref(T(**f))

    bad_first = np.array([0, 4, 3], np.uint32)
    h, out = codec._h, p + 4096  # the maps are 80 bytes, the index tensor 160
    for args in ((None, p, 2, 5, 4, targets(), out), (h, None, 2, 5, 4, targets(), out), (h, p, 2, 5, 4, None, out), (h, p, 2, 5, 4, targets(), None),
                 (h, p + 1, 2, 5, 4, targets(), out), (h, p, 2, 5, 4, targets(), out + 2), (h, p, 2, 5, 4, targets(struct_size=60), out),
                 (h, p, 2, 5, 4, targets(map_bytes=3), out), (h, p, 2, 5, 4, targets(kind=2), out), (h, p, 2, 5, 4, targets(dtype=3), out),
                 (h, p, 2, 5, 4, targets(ids=None), out), (h, p, 2, 5, 4, targets(values=None), out), (h, p, 2, 5, 4, targets(first=None), out),
                 (h, p, 2, 5, 4, targets(first=bad_first.ctypes.data), out), (h, p, 2, 5, 4, targets(kind=mi.TARGET_PLANES, dtype=mi.DTYPE_F32, plane_first=None), out),
                 (h, p, 2, 5, 4, targets(kind=mi.TARGET_PLANES, dtype=mi.DTYPE_F16, on_bits=0x10000), out),
                 (h, out + 156, 2, 5, 4, targets(), out), (h, out + 4, 2, 5, 4, targets(), out), (h, out - 76, 2, 5, 4, targets(), out)):  # overlapping
        assert L.llcomp_mi_codec_label_targets(*args, stream()) == mi.BAD_ARGS, args[1:5]
    torch.cuda.synchronize()
    assert not buf.cpu().numpy().any()
    assert L.llcomp_mi_codec_label_targets(h, out - 80, 2, 5, 4, targets(), out, stream()) == mi.OK  # touching is fine
    assert L.llcomp_mi_codec_label_targets(h, out + 160, 2, 5, 4, targets(), out, stream()) == mi.OK
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert not host[:4096].any() and not host[4096 + 160:].any()
    got = host[4096:4096 + 160].view(np.int32).reshape(2, 20)
    assert (got[0] == 0).all() and (got[1] == 7).all()  # id 0 is listed for sample 0 with value 0, and not for sample 1


def test_decode_paste16_renumber_and_targets_on_one_stream(mi, orc):
    """the chain of test_gpu_label_boxes16.py on one stream with no synchronisation between the steps: u16 maps encoded as two-channel
    sliced containers decode as nearest-filter views in U8 HWC; paste_batch16 with VALUE pieces renumbers the pasted instances in the dst
    maps; label_targets on the dst maps, INDEX I64 (instance to class) and PLANES U8 (one mask per listed instance), and label_boxes16
    with the same lists.  Equal to the specs; the masks' pixel counts and boxes are what label_boxes16 returns."""
    import torch

    import paste16_spec
    from test_gpu_resized_output import TOut
    from test_gpu_resized_regions import packed

    B, T = mi.label_boxes_rows(), mi.compose_tile()
    n, w, h = 2, T + 7, B + 9
    rng = np.random.default_rng(1217)
    classes = (24000, 24001, 26000, 26001, 26002, 33000)  # class * 1000 + k
    maps = blobs16(rng, 2 * n, h, w, (0,) + classes)  # frames 0..n-1: the src maps; n..2n-1: the dst maps
    conts = [orc.compress_sliced(np.ascontiguousarray(m.view(np.uint8).reshape(h, w, 2)), 32, 16, False) for m in maps]
    new_id = {m: 40000 + 10 * j for j, m in enumerate(classes)}  # what the pasted instances are called in the dst maps
    class_of = {new_id[m] + d: m // 1000 for m in classes for d in range(n)}
    rect = (3, 2, 0, 1, w - 3, h - 2)
    renumber = [(d, (d + 1) % n) + rect + ([m], new_id[m] + d) for d in range(n) for m in classes if (m + d) % 2]
    lists = [sorted([24000, 26001] + [new_id[m] + d for m in classes]) for d in range(n)]
    to_class = [[class_of.get(m, m // 1000) for m in l] for l in lists]
    to_mask = [list(range(len(l))) for l in lists]
    counts = [len(l) for l in lists]
    total = sum(counts)
    map_codec, id_codec = mi.Codec(2 * n, w, h, 2, 32, 16, False, device=0), mi.Codec(1, 32, 16, 1, 32, 16, False, device=0)
    try:
        d_pay, n_pay, d_len = packed(mi, conts)
        src_maps, dst_maps = TOut(n, w, h, 2, "uint8", "hwc", offset=6), TOut(n, w, h, 2, "uint8", "hwc", offset=10)
        ibuf, ilo = put(np.full(n * h * w * 8, 0xA5, np.uint8), 8)
        pbuf, plo = put(np.full(total * h * w, 0xA5, np.uint8), 3)
        bbuf, blo = put(np.full(total * 20, 0xA5, np.uint8), 0)
        groups = [mi.ViewGroup([(f, 0, 0, w, h) for f in range(n)], w, h, src_maps.ptr, dtype="uint8", layout="hwc", filter="nearest"),
                  mi.ViewGroup([(n + f, 0, 0, w, h) for f in range(n)], w, h, dst_maps.ptr, dtype="uint8", layout="hwc", filter="nearest")]
        map_codec.decode_views(d_pay.data_ptr(), n_pay, d_len.data_ptr(), groups, src_maps.st.data_ptr(), stream())
        id_codec.paste_batch16(src_maps.ptr, src_maps.ptr, n, w, h, dst_maps.ptr, n, w, h, renumber, dtype="bfloat16", layout="chw", stream=stream())
        id_codec.label_targets(dst_maps.ptr, n, w, h, lists, to_class, ibuf.data_ptr() + ilo, map_dtype="uint16", dtype="int64", default=-100, stream=stream())
        id_codec.label_targets(dst_maps.ptr, n, w, h, lists, to_mask, pbuf.data_ptr() + plo, map_dtype="uint16", kind="planes", default=-1, planes=counts, stream=stream())
        id_codec.label_boxes16(dst_maps.ptr, n, w, h, lists, bbuf.data_ptr() + blo, stream=stream())
        torch.cuda.synchronize()
        (st, _), (_, d_host) = src_maps.read(), dst_maps.read()
        assert st == 0
        want_maps = paste16_spec.apply(maps[:n, None], maps[:n], maps[n:, None], renumber, "chw")[:, 0]
        assert np.array_equal(np.ascontiguousarray(d_host).reshape(n, h, 2 * w).view(np.uint16), want_maps) and want_maps.max() > 255
        ihost, phost, bhost = ibuf.cpu().numpy(), pbuf.cpu().numpy(), bbuf.cpu().numpy()
        assert guards_intact(ihost, ilo, n * h * w * 8) and guards_intact(phost, plo, total * h * w) and guards_intact(bhost, blo, total * 20)
        index = ihost[ilo:ilo + n * h * w * 8].copy().view(np.int64).reshape(n, h, w)
        assert np.array_equal(index, value_spec(want_maps, lists, to_class, -100))
        assert (index == -100).any() and (index == 24).any() and (index == 33).any()
        masks = phost[plo:plo + total * h * w].reshape(total, h, w)
        assert np.array_equal(masks, planes_spec(want_maps, lists, to_mask, -1, counts, 1, 0, "uint8"))
        boxes = as_table(bhost[blo:blo + total * 20].copy().view(mi.LABEL_BOX_DTYPE))
        assert boxes[:, 0].sum() > 0
        for j in range(total):  # a mask's pixels and box are the record of label_boxes16 for the same listed id
            at = np.argwhere(masks[j])
            rec = (len(at), at[:, 1].min(), at[:, 0].min(), at[:, 1].max() + 1, at[:, 0].max() + 1) if len(at) else (0, w, h, 0, 0)
            assert tuple(boxes[j]) == rec, j
    finally:
        map_codec.close()
        id_codec.close()
