"""The rule of the label boxes of listed ids on the host (llcomp_mi_label_boxes16_reference; include/llcomp_mi.h: "Label boxes of listed
ids") against numpy -- np.argwhere per listed id -- record for record; the refusals.  label_boxes16_spec is what the GPU tests compare
with too."""
import ctypes as C

import numpy as np
import pytest

from test_label_boxes import as_table


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


def label_boxes16_spec(maps, ids):
    """maps [n, oh, ow] uint16, ids: n sequences -> [total, 5] of (count, x0, y0, x1, y1) by np.argwhere per listed id, in the lists'
    order; without a pixel (0, ow, oh, 0, 0)"""
    n, oh, ow = maps.shape
    out = []
    for i in range(n):
        for m in ids[i]:
            at = np.argwhere(maps[i] == m)
            out.append((len(at), at[:, 1].min(), at[:, 0].min(), at[:, 1].max() + 1, at[:, 0].max() + 1) if len(at) else (0, ow, oh, 0, 0))
    return np.array(out, np.int64).reshape(-1, 5)


def blobs16(rng, n, oh, ow, pool):
    """photo-like maps: rectangles of ids drawn from `pool` over a background of pool[0]"""
    pool = np.asarray(pool, np.uint16)
    maps = np.full((n, oh, ow), pool[0], np.uint16)
    for i in range(n):
        for _ in range(2 * min(len(pool), 12)):
            w, h = int(rng.integers(1, ow + 1)), int(rng.integers(1, oh + 1))
            x, y = int(rng.integers(0, ow - w + 1)), int(rng.integers(0, oh - h + 1))
            maps[i, y:y + h, x:x + w] = pool[rng.integers(0, len(pool))]
    return maps


def at_offset(maps, off):
    """a copy of the maps `off` bytes (even) past a 16-byte boundary"""
    raw = np.zeros(maps.nbytes + 48, np.uint8)
    base = (-raw.ctypes.data) % 16 + off
    raw[base:base + maps.nbytes] = maps.reshape(-1).view(np.uint8)
    return raw[base:base + maps.nbytes].view(np.uint16).reshape(maps.shape)


HIGH_BYTE = (0x0001, 0x0101, 0x0201, 0xFF01, 0x0100, 0x0000)  # ids that share low bytes


def lists_for(rng, maps, pool):
    """per sample: some ids of the pool that the map has, some it has not, some of neither; sorted"""
    out = []
    for i in range(len(maps)):
        pick = {int(m) for m in pool if rng.integers(0, 3)} | {int(v) for v in rng.integers(0, 65536, size=3)}
        out.append(sorted(pick))
    return out


def test_reference_is_numpy(mi):
    B = mi.label_boxes_rows()
    rng = np.random.default_rng(16)
    for ow in (1, 7, 8, 9, 17, 33):
        for oh in (1, B - 1, B, B + 1, 2 * B + 3):
            for off in (0, 2, 14):
                pool = HIGH_BYTE if off else (3, 700, 0x8000, 65535, 0)
                maps = blobs16(rng, 2, oh, ow, pool) if off != 2 else np.asarray(pool, np.uint16)[rng.integers(0, len(pool), size=(2, oh, ow))]
                ids = lists_for(rng, maps, pool)
                got = mi.label_boxes16_reference(at_offset(maps, off), ids)
                assert got.dtype == mi.LABEL_BOX_DTYPE and got.shape == (len(ids[0]) + len(ids[1]),)
                assert np.array_equal(as_table(got), label_boxes16_spec(maps, ids)), (ow, oh, off)


@pytest.mark.parametrize("count", [1, 256, 257, 1024, 1025, 4096])
def test_list_lengths_around_the_capacities(mi, count):
    assert mi.label_boxes16_max_ids() == 4096
    B = mi.label_boxes_rows()
    rng = np.random.default_rng(count)
    listed = np.sort(rng.choice(65536, size=count, replace=False))
    others = np.setdiff1d(np.arange(65536), listed)[:50]
    pool = np.concatenate([listed[:: max(2, count // 300)], others])  # (listed ids with and without a pixel, pixels that are not listed)
    maps = pool[rng.integers(0, len(pool), size=(2, B + 5, 41))].astype(np.uint16)
    ids = [listed.tolist(), listed[: count // 2 + 1].tolist()]
    got = as_table(mi.label_boxes16_reference(maps, ids))
    want = label_boxes16_spec(maps, ids)
    assert np.array_equal(got, want)
    assert (want[:, 0] == 0).any() or count == 1
    assert want[:, 0].sum() < 2 * maps[0].size  # (some pixels are counted nowhere)


def test_one_id_high_bytes_and_an_empty_list(mi):
    B = mi.label_boxes_rows()
    one = np.full((1, 2 * B + 1, 70), 0x1234, np.uint16)  # a map of one id
    got = mi.label_boxes16_reference(one, [[0x0034, 0x1200, 0x1234, 0x3412]])
    assert [tuple(r) for r in got] == [(0, 70, 2 * B + 1, 0, 0)] * 2 + [(70 * (2 * B + 1), 0, 0, 70, 2 * B + 1), (0, 70, 2 * B + 1, 0, 0)]
    rng = np.random.default_rng(3)
    high = blobs16(rng, 3, B + 7, 45, HIGH_BYTE)  # ids that differ only in the high byte: a test of the low byte alone fails
    high[:, 0, :6] = HIGH_BYTE
    ids = [[0x0001, 0x0101, 0xFF01], [], [0x0101, 0x0201]]  # a sample with an empty list among three
    got = as_table(mi.label_boxes16_reference(high, ids))
    assert got.shape == (5, 5) and np.array_equal(got, label_boxes16_spec(high, ids))
    assert got[0, 0] < ((high[0] & 0xFF) == 1).sum()  # (what a test of the low byte alone would count)
    assert mi.label_boxes16_reference(high, [[], [], []]).shape == (0,)


def test_listing_every_byte_id_is_the_8_bit_call(mi):
    rng = np.random.default_rng(8)
    narrow = rng.integers(0, 256, size=(2, 37, 29), dtype=np.uint8)
    narrow[1, 5:30, 3:20] = 7
    got = as_table(mi.label_boxes16_reference(narrow.astype(np.uint16), [range(256), range(256)]))
    assert np.array_equal(got.reshape(2, 256, 5), as_table(mi.label_boxes_reference(narrow)))


def test_refusals(mi):
    L = mi._lib.load()
    maps = np.zeros((2, 4, 5), np.uint16)
    ids = np.array([0, 3, 9, 1, 2], np.uint16)
    first = np.array([0, 3, 5], np.uint32)
    out = np.full(5, 7, mi.LABEL_BOX_DTYPE)
    before = out.copy()
    m, i, f, o = maps.ctypes.data, ids.ctypes.data, first.ctypes.data, out.ctypes.data

    def u32(*v):
        return np.array(v, np.uint32)

    def u16(*v):
        return np.array(v, np.uint16)

    long_ids = np.arange(4097, dtype=np.uint16)
    many = np.arange(65536, dtype=np.uint16)[:4096]
    keep = [u32(1, 3, 5), u32(0, 4, 3), u32(0, 4097, 4097), u16(0, 3, 3, 1, 2), u16(0, 3, 2, 1, 2), u16(0, 3, 9, 2, 1), long_ids, many,
            u32(*range(0, 4096 * 258, 4096))]
    for args in ((None, 2, 5, 4, i, f, o), (m, 2, 5, 4, None, f, o), (m, 2, 5, 4, i, None, o), (m, 2, 5, 4, i, f, None), (m, 0, 5, 4, i, f, o),
                 (m, 65536, 5, 4, i, f, o), (m, 2, 0, 4, i, f, o), (m, 2, 5, 0, i, f, o), (m, 1, 65536, 65536, i, f, o),
                 (m + 1, 2, 5, 4, i, f, o),                                   # maps not aligned to 2 bytes
                 (m, 2, 5, 4, i, keep[0].ctypes.data, o),                     # first[0] != 0
                 (m, 2, 5, 4, i, keep[1].ctypes.data, o),                     # a first that decreases
                 (m, 2, 5, 4, long_ids.ctypes.data, keep[2].ctypes.data, o),  # a list that is too long
                 (m, 2, 5, 4, keep[3].ctypes.data, f, o),                     # equal neighbours
                 (m, 2, 5, 4, keep[4].ctypes.data, f, o),                     # descending in the first list
                 (m, 2, 5, 4, keep[5].ctypes.data, f, o),                     # descending in the second
                 (m, 257, 1, 1, many.ctypes.data, keep[8].ctypes.data, o)):   # more than 2^20 ids in all
        assert L.llcomp_mi_label_boxes16_reference(*args) == mi.BAD_ARGS, args[1:4]
    assert np.array_equal(out, before)
    assert L.llcomp_mi_label_boxes16_reference(m, 2, 5, 4, i, f, o) == mi.OK
    assert tuple(out[0]) == (20, 0, 0, 5, 4) and tuple(out[1]) == (0, 5, 4, 0, 0) and tuple(out[3]) == (0, 5, 4, 0, 0)
    ok = mi.label_boxes16_reference(np.zeros((1, 2, 2), np.uint16), [range(4096)])  # the longest list is fine
    assert ok.shape == (4096,) and tuple(ok[0]) == (4, 0, 0, 2, 2)
    for bad, lists in ((np.zeros((2, 4), np.uint16), [[1], [1]]), (np.zeros((2, 4, 5), np.uint8), [[1], [1]]), (np.zeros((0, 4, 5), np.uint16), []),
                       (maps, [[1]]), (maps, [[1], [70000]]), (maps, [[1], [-1]]), (maps, [[2, 1], []]), (maps, [range(4097), []])):
        with pytest.raises(mi.LlcompError):
            mi.label_boxes16_reference(bad, lists)
    with pytest.raises(mi.LlcompError):
        mi.label_boxes_reference(maps)  # the 8-bit call goes on refusing a uint16 array
    assert C.sizeof(mi._lib.LabelBox) == 20
