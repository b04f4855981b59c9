"""The rule of the label boxes on the host (llcomp_mi_label_boxes_reference; include/llcomp_mi.h: "Label boxes") against numpy --
np.argwhere per id -- record for record; the refusals.  label_boxes_spec is what the GPU tests compare with too."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


def label_boxes_spec(maps):
    """maps [n, oh, ow] uint8 -> [n, 256, 5] of (count, x0, y0, x1, y1) by np.argwhere per id; without a pixel (0, ow, oh, 0, 0)"""
    n, oh, ow = maps.shape
    out = np.zeros((n, 256, 5), np.int64)
    out[:] = (0, ow, oh, 0, 0)
    for i in range(n):
        for m in np.unique(maps[i]):  # (the other ids have no pixel)
            at = np.argwhere(maps[i] == m)
            out[i, m] = (len(at), at[:, 1].min(), at[:, 0].min(), at[:, 1].max() + 1, at[:, 0].max() + 1)
    return out


def as_table(recs):
    return np.stack([recs[name].astype(np.int64) for name in ("count", "x0", "y0", "x1", "y1")], axis=-1)


def blobs(rng, n, oh, ow, ids):
    """photo-like maps: rectangles of drawn ids over a background of 0"""
    maps = np.zeros((n, oh, ow), np.uint8)
    for i in range(n):
        for _ in range(2 * ids):
            w, h = int(rng.integers(1, ow + 1)), int(rng.integers(1, oh + 1))
            x, y = int(rng.integers(0, ow - w + 1)), int(rng.integers(0, oh - h + 1))
            maps[i, y:y + h, x:x + w] = rng.integers(0, ids)
    return maps


def test_reference_is_numpy(mi):
    B = mi.label_boxes_rows()
    rng = np.random.default_rng(1)
    for n, oh, ow, ids in ((2, 20, 30, 8), (3, B + 1, 17, 256), (1, 2 * B + 3, 33, 5), (2, 1, 40, 4), (2, 40, 1, 4), (1, 1, 1, 2), (2, B - 1, 15, 3),
                           (1, B, 16, 7)):
        for maps in (rng.integers(0, ids, size=(n, oh, ow), dtype=np.uint8), blobs(rng, n, oh, ow, ids)):
            for off in (0, 1, 15):  # the maps at any byte address
                raw = np.zeros(maps.size + 32, np.uint8)
                base = (-raw.ctypes.data) % 16 + off
                raw[base:base + maps.size] = maps.reshape(-1)
                got = mi.label_boxes_reference(raw[base:base + maps.size].reshape(maps.shape))
                assert got.shape == (n, 256) and got.dtype == mi.LABEL_BOX_DTYPE and mi.LABEL_BOX_DTYPE.itemsize == 20
                assert np.array_equal(as_table(got), label_boxes_spec(maps)), (n, oh, ow, ids, off)


def test_one_id_single_pixels_and_empty_ids(mi):
    maps = np.full((2, 37, 29), 9, np.uint8)  # a map of one id
    maps[1, 5, 7], maps[1, 36, 28], maps[1, 0, 0] = 200, 201, 255  # ids present in one pixel only, at the corners too
    got = mi.label_boxes_reference(maps)
    assert tuple(got[0, 9]) == (37 * 29, 0, 0, 29, 37) and tuple(got[1, 9]) == (37 * 29 - 3, 0, 0, 29, 37)
    assert tuple(got[1, 200]) == (1, 7, 5, 8, 6) and tuple(got[1, 201]) == (1, 28, 36, 29, 37) and tuple(got[1, 255]) == (1, 0, 0, 1, 1)
    for m in (0, 8, 10, 254):
        assert tuple(got[0, m]) == (0, 29, 37, 0, 0)  # the identities of min and max
    assert np.array_equal(as_table(got), label_boxes_spec(maps))
    # records of two maps merge by add, min and max: the halves of a map against the whole
    rng = np.random.default_rng(2)
    whole = blobs(rng, 1, 40, 50, 6)
    top, bottom = as_table(mi.label_boxes_reference(whole[:, :13]))[0], as_table(mi.label_boxes_reference(whole[:, 13:]))[0]
    bottom[:, 2] += 13
    bottom[:, 4] += np.where(bottom[:, 0] > 0, 13, 0)
    top[:, 2] = np.where(top[:, 0] > 0, top[:, 2], 40)
    merged = np.stack([top[:, 0] + bottom[:, 0], np.minimum(top[:, 1], bottom[:, 1]), np.minimum(top[:, 2], bottom[:, 2]),
                       np.maximum(top[:, 3], bottom[:, 3]), np.maximum(top[:, 4], bottom[:, 4])], axis=-1)
    assert np.array_equal(merged, as_table(mi.label_boxes_reference(whole))[0])


def test_refusals(mi):
    L = mi._lib.load()
    maps = np.zeros((2, 4, 5), np.uint8)
    out = np.full((2, 256), 7, mi.LABEL_BOX_DTYPE)
    before = out.copy()
    for args in ((None, 2, 5, 4, out.ctypes.data), (maps.ctypes.data, 2, 5, 4, None), (maps.ctypes.data, 0, 5, 4, out.ctypes.data),
                 (maps.ctypes.data, 65536, 5, 4, out.ctypes.data), (maps.ctypes.data, 2, 0, 4, out.ctypes.data), (maps.ctypes.data, 2, 5, 0, out.ctypes.data),
                 (maps.ctypes.data, 1, 65536, 65536, out.ctypes.data), (maps.ctypes.data, 1, 1 << 31, 2, out.ctypes.data),
                 (maps.ctypes.data, 65535, 0xFFFFFFFF, 0xFFFFFFFF, out.ctypes.data)):
        assert L.llcomp_mi_label_boxes_reference(*args) == mi.BAD_ARGS, args[1:4]
    assert np.array_equal(out, before)
    assert L.llcomp_mi_label_boxes_reference(maps.ctypes.data, 2, 5, 4, out.ctypes.data) == mi.OK
    assert tuple(out[1, 0]) == (20, 0, 0, 5, 4) and tuple(out[1, 1]) == (0, 5, 4, 0, 0)
    for bad in (np.zeros((2, 4), np.uint8), np.zeros((2, 4, 5), np.uint16), np.zeros((0, 4, 5), np.uint8)):
        with pytest.raises(mi.LlcompError):
            mi.label_boxes_reference(bad)
    assert mi.label_boxes_rows() >= 1 and C.sizeof(mi._lib.LabelBox) == 20
