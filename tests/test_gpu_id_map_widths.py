"""The calls on id maps take maps of 1 or 2 bytes per pixel through ONE rule, templated on the width (DESIGN.md "Id maps: what the
two widths share").  What that rests on: the same content through both widths gives the same bytes.  The smallest shapes with a tile
corner, a band border, and units shared between rows and samples: T = compose_tile() and R = compose_tile(pixel bytes), the paste
kernel's tile; B = label_boxes_rows() = 32, the rows of a label-box workgroup's band."""
import numpy as np
import pytest

import paste_spec
from batch_support import ESIZE, bits_of, guards_intact, mi, put, stream  # noqa: F401
from test_label_boxes import as_table
from test_paste16_rule import as_array, window_piece

pytestmark = pytest.mark.gpu
ALL = list(range(256))


@pytest.fixture(scope="module")
def codec(mi):
    k = mi.Codec(1, 32, 16, 3, 32, 16, False, device=0)
    yield k
    k.close()


def half(rng):
    return sorted(int(m) for m in rng.choice(8, 4, replace=False))


def pasted(mi, codec, call, src, mask, dst, pieces, dtype, layout):
    """paste_batch or paste_batch16 on the numpy batches, the mask 6 bytes and dst 3 elements past a 256-byte boundary -> dst's bytes
    after the call; the guard bytes around dst have to be intact"""
    import torch

    (oh, ow) = dst.shape[2:] if layout == "chw" else dst.shape[1:3]
    dbuf, dlo = put(dst, 3 * ESIZE[dtype])
    sbuf, slo = put(src, 0)
    mbuf, mlo = put(mask, 6)
    getattr(codec, call)(sbuf.data_ptr() + slo, mbuf.data_ptr() + mlo, len(src), mask.shape[2], mask.shape[1], dbuf.data_ptr() + dlo, len(dst), ow, oh,
                         pieces, dtype=dtype, layout=layout, stream=stream())
    torch.cuda.synchronize()
    host = dbuf.cpu().numpy()
    assert guards_intact(host, dlo, dst.nbytes), f"{call} wrote a byte outside the dst batch"
    return host[dlo:dlo + dst.nbytes].copy()


@pytest.mark.parametrize("dtype,layout", [("uint8", "hwc"), ("float16", "chw")])
def test_paste_by_bytes_and_by_the_same_ids_widened(mi, codec, dtype, layout):
    """the five border pieces of test_gpu_paste_batch.py::test_pieces_across_every_tile_border on a uint8 mask through paste_batch and
    on the same mask as uint16 through paste_batch16 with windows at id_base 0: byte-identical dst batches"""
    c = 3
    T, R = mi.compose_tile(), mi.compose_tile(ESIZE[dtype] * (1 if layout == "chw" else c))
    rng = np.random.default_rng(T + R)
    ow, oh, iw, ih = T + 7, R + 3, T + 10, R + 2
    pieces = [(0, 0, 0, 0, 3, 0, ow, ih, half(rng)),             # a whole sample's objects, under everything else
              (0, 1, T - 3, 0, T - 4, 0, 8, ih, half(rng)),      # columns T - 3 .. T + 4, read from one column further left
              (1, 1, 1, R - 2, 0, R - 2, ow - 1, 4, half(rng)),  # rows R - 2 .. R + 1, every column but the first
              (1, 0, T - 1, R - 1, T - 1, R - 1, 2, 2, ALL),     # the tiles' corner
              (0, 1, T - 2, R - 1, 5, 1, 7, 3, half(rng), 3.0)]  # a VALUE piece over it
    value_bits = 3 if dtype == "uint8" else int(np.float16(3.0).view(np.uint16))
    windows = []
    for p in pieces:
        lut = np.zeros(256, bool)
        lut[list(p[8])] = True
        windows.append(window_piece(mi, p[:8], 0, lut, value_bits if len(p) > 9 else None))
    src = paste_spec.gen_batch(dtype, 2, c, ih, iw, layout, 1)
    dst = paste_spec.gen_batch(dtype, 2, c, oh, ow, layout, 2)
    mask = paste_spec.gen_mask(rng, 2, ih, iw)
    by_bytes = pasted(mi, codec, "paste_batch", src, mask, dst, pieces, dtype, layout)
    by_words = pasted(mi, codec, "paste_batch16", src, mask.astype(np.uint16), dst, as_array(mi, windows), dtype, layout)
    assert np.array_equal(by_bytes, by_words), np.flatnonzero(by_bytes != by_words)[:8].tolist()
    want = np.ascontiguousarray(paste_spec.apply(src, mask, dst, pieces, layout, dtype)).reshape(-1).view(np.uint8)
    assert np.array_equal(by_bytes, want) and not np.array_equal(want, dst.reshape(-1).view(np.uint8))


def test_boxes_of_byte_maps_and_of_the_same_maps_widened(mi, codec):
    """2 maps of 37 x 33 -- one row past a band, a width that is no multiple of 16 -- as bytes through label_boxes and widened through
    label_boxes16 with the list 0..255 for both samples: the same 2 x 256 records"""
    import torch

    B = mi.label_boxes_rows()
    ow, oh = 37, B + 1
    rng = np.random.default_rng(B)
    maps = rng.integers(0, 12, size=(2, oh, ow), dtype=np.uint8)
    maps[0, 5:20, 3:30] = 200   # a run across many units
    maps[1, B - 1:, :] = 255    # the band's border, and the last id
    maps[rng.integers(0, 2, size=maps.shape, dtype=np.uint8) == 1] //= 4  # (longer runs)

    def boxes(call, m, offset, *lists):
        mbuf, mlo = put(m, offset)
        bbuf, blo = put(np.full(2 * 256 * 20, 0xA5, np.uint8), 0)
        getattr(codec, call)(mbuf.data_ptr() + mlo, 2, ow, oh, *lists, bbuf.data_ptr() + blo, stream=stream())
        torch.cuda.synchronize()
        host = bbuf.cpu().numpy()
        assert guards_intact(host, blo, 2 * 256 * 20), f"{call} wrote a byte outside the records"
        return as_table(host[blo:blo + 2 * 256 * 20].copy().view(mi.LABEL_BOX_DTYPE))

    by_bytes = boxes("label_boxes", maps, 5)
    by_words = boxes("label_boxes16", maps.astype(np.uint16), 6, [ALL, ALL])
    assert np.array_equal(by_bytes, by_words), np.argwhere(by_bytes != by_words)[:4].tolist()
    assert np.array_equal(by_bytes, as_table(mi.label_boxes_reference(maps)).reshape(-1, 5))
    assert int(by_bytes[:, 0].sum()) == 2 * ow * oh
