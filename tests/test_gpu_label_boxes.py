"""Label boxes on the GPU (llcomp_mi_codec_label_boxes; include/llcomp_mi.h: "Label boxes"): the pixel count and the bounding box of
each of the 256 ids of every id map of a batch in HBM, against numpy -- np.argwhere per id (tests/test_label_boxes.py) -- record for
record, with 256 guard bytes on both sides of the records that have to stay and maps that have to be byte-identical after the call.
B = label_boxes_rows(), the rows of a workgroup's band, sizes the shapes."""
import numpy as np
import pytest

import paste_spec
from batch_support import guards_intact, mi, put, stream  # noqa: F401
from test_label_boxes import as_table, blobs, label_boxes_spec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec(mi):
    k = mi.Codec(1, 32, 16, 3, 32, 16, False, device=0)  # (the codec gives the device: the maps have one channel whatever its c)
    yield k
    k.close()


def run(mi, codec, maps, offset=0, expect_error=False, **kw):
    """label_boxes on the numpy maps [n, oh, ow], `offset` bytes past a 256-byte boundary -> the [n, 256, 5] table of the records; the
    records stand between guard bytes over a pattern of 0xA5, so a record that is not written shows"""
    import torch

    n, oh, ow = maps.shape
    mbuf, mlo = put(maps, offset)
    boxes = np.full(n * 256 * 20, 0xA5, np.uint8)
    bbuf, blo = put(boxes, 0)
    args = dict(d_maps=mbuf.data_ptr() + mlo, n=n, ow=ow, oh=oh, d_boxes=bbuf.data_ptr() + blo, stream=stream())
    args.update(kw)
    err = None
    try:
        codec.label_boxes(**args)
    except mi.LlcompError as e:
        err = e
    torch.cuda.synchronize()
    assert (err is not None) == expect_error, err
    assert err is None or err.status == mi.BAD_ARGS
    host = bbuf.cpu().numpy()
    assert guards_intact(host, blo, boxes.nbytes), "a byte outside the records was written"
    mhost = mbuf.cpu().numpy()
    assert guards_intact(mhost, mlo, maps.nbytes) and np.array_equal(mhost[mlo:mlo + maps.nbytes], maps.reshape(-1)), "the maps were written"
    got = host[blo:blo + boxes.nbytes].copy()
    if expect_error:
        assert (got == 0xA5).all(), "a refused call wrote records"
        return None
    return as_table(got.view(mi.LABEL_BOX_DTYPE).reshape(n, 256))


def test_widths_around_a_unit_by_heights_around_a_band(mi, codec):
    B = mi.label_boxes_rows()
    rng = np.random.default_rng(B)
    for ow in (1, 15, 16, 17, 33):
        for oh in (1, B - 1, B, B + 1, 2 * B + 3):
            for off in (0, 1, 15):
                maps = blobs(rng, 2, oh, ow, 6) if off else rng.integers(0, 5, size=(2, oh, ow), dtype=np.uint8)
                assert np.array_equal(run(mi, codec, maps, off), label_boxes_spec(maps)), (ow, oh, off)


def test_one_id_all_ids_and_an_all_zero_sample(mi, codec):
    B = mi.label_boxes_rows()
    one = np.full((1, 2 * B + 1, 70), 9, np.uint8)  # every lane at the same LDS address
    assert np.array_equal(run(mi, codec, one, 3), label_boxes_spec(one))
    every = (np.arange(3 * B * 50, dtype=np.uint32) * 37 % 256).astype(np.uint8).reshape(1, 3 * B, 50)  # all 256 ids
    assert len(np.unique(every)) == 256
    assert np.array_equal(run(mi, codec, every, 5), label_boxes_spec(every))
    rng = np.random.default_rng(4)
    three = blobs(rng, 3, B + 7, 45, 9)
    three[1] = 0
    got = run(mi, codec, three, 9)
    assert np.array_equal(got, label_boxes_spec(three))
    assert tuple(got[1, 0]) == (45 * (B + 7), 0, 0, 45, B + 7) and tuple(got[1, 1]) == (0, 45, B + 7, 0, 0)
    assert np.array_equal(got, as_table(mi.label_boxes_reference(three)))


def test_refusals_queue_nothing(mi, codec):
    import torch

    maps = np.zeros((2, 4, 5), np.uint8)
    for kw in (dict(d_maps=None), dict(d_boxes=None), dict(n=0), dict(n=65536), dict(ow=0), dict(oh=0), dict(ow=65536, oh=65536, n=1)):
        run(mi, codec, maps, expect_error=True, **kw)
    L = mi._lib.load()
    buf = torch.zeros(16384, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    for args in ((None, p, 2, 5, 4, p + 4096), (codec._h, p, 2, 5, 4, p + 4098), (codec._h, p, 2, 5, 4, p + 36), (codec._h, p + 4096 + 10239, 2, 5, 4, p + 4096),
                 (codec._h, p + 4096 - 39, 2, 5, 4, p + 4096)):
        assert L.llcomp_mi_codec_label_boxes(*args, stream()) == mi.BAD_ARGS, args[1:]
    assert L.llcomp_mi_codec_label_boxes(codec._h, p + 4096 - 40, 2, 5, 4, p + 4096, stream()) == mi.OK  # touching is fine
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert not host[:4096].any() and not host[4096 + 10240:].any()
    assert tuple(host[4096:4096 + 10240].view(mi.LABEL_BOX_DTYPE)[256]) == (20, 0, 0, 5, 4)


def test_paste_value_pieces_then_boxes_on_one_stream(mi):
    """the second call of a Copy-Paste and the boxes behind it: VALUE pieces give the pasted instances new ids in the dst maps, then
    label_boxes, with no synchronisation between; equal to the spec of both"""
    import torch

    B, T = mi.label_boxes_rows(), mi.compose_tile()
    n, oh, ow = 3, B + 9, T + 7
    rng = np.random.default_rng(12)
    src = blobs(rng, n, oh, ow, 5)
    dst = blobs(rng, n, oh, ow, 4)
    pieces = [(d, (d + 1) % n, 3, 2, 0, 1, ow - 3, oh - 2, [m], 100 + 10 * d + m) for d in range(n) for m in range(1, 5)]
    k = mi.Codec(1, 32, 16, 1, 32, 16, False, device=0)
    try:
        sbuf, slo = put(src, 5)
        dbuf, dlo = put(dst, 11)
        boxes = np.full(n * 256 * 20, 0xA5, np.uint8)
        bbuf, blo = put(boxes, 0)
        k.paste_batch(sbuf.data_ptr() + slo, sbuf.data_ptr() + slo, n, ow, oh, dbuf.data_ptr() + dlo, n, ow, oh, pieces, dtype="uint8", layout="chw",
                      stream=stream())
        k.label_boxes(dbuf.data_ptr() + dlo, n, ow, oh, bbuf.data_ptr() + blo, stream=stream())
        torch.cuda.synchronize()
        want_maps = paste_spec.apply(src[:, None], src, dst[:, None], pieces, "chw", "uint8")[:, 0]
        dhost, bhost = dbuf.cpu().numpy(), bbuf.cpu().numpy()
        assert guards_intact(dhost, dlo, dst.nbytes) and guards_intact(bhost, blo, boxes.nbytes)
        assert np.array_equal(dhost[dlo:dlo + dst.nbytes].reshape(dst.shape), want_maps)
        got = as_table(bhost[blo:blo + boxes.nbytes].copy().view(mi.LABEL_BOX_DTYPE).reshape(n, 256))
        assert np.array_equal(got, label_boxes_spec(want_maps))
        assert got[0, 101:105, 0].sum() > 0  # (the pasted instances are there)
    finally:
        k.close()
