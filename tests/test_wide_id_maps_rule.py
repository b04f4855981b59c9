"""The rules of the calls on id maps of 3 and 4 bytes per pixel on the host (llcomp_mi_label_boxes32_reference,
llcomp_mi_label_targets32_reference; include/llcomp_mi.h: "Wide id maps") against numpy specs written here: the ids built from the
maps' bytes, np.argwhere per listed id for the boxes, np.searchsorted for the value of a pixel; the refusals; and the same content
through the widths 1, 2, 3 and 4.  Every comparison is exact.  wide_maps, ids_of, at_offset, boxes_spec and draw are what the GPU
tests use too."""
import ctypes as C

import numpy as np
import pytest

from test_label_boxes import as_table
from test_label_boxes16 import blobs16
from test_label_targets import INDEX_DTYPES, PLANE_DTYPES, index_spec, planes_spec


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


WIDTHS = (3, 4)
TOP = {3: 0xFFFFFF, 4: 0xFFFFFFFF}
# ids that differ only in byte 2 or byte 3 while bytes 0-1 agree, and the ends of the range
HIGH_BYTES = {3: (0x000001, 0x010001, 0xFF0001, 0x000000, 0xFFFFFF), 4: (0x000001, 0x010001, 0xFF0001, 0x01000001, 0x00000000, 0xFFFFFFFF, 0x00FFFFFF)}
BOX_OFFSETS = {3: (0, 1, 2, 13, 14, 15), 4: (0, 4, 12)}


def wide_maps(ids, mb):
    """ids [n, oh, ow] of integers -> the host maps the library takes: [n, oh, ow, 3] uint8, little-endian, or [n, oh, ow] uint32"""
    ids = np.asarray(ids, np.int64)
    if mb == 4:
        return ids.astype(np.uint32)
    return np.stack([(ids >> (8 * b)) & 0xFF for b in range(3)], axis=-1).astype(np.uint8)


def ids_of(maps):
    """the ids of host maps of either width as int64 [n, oh, ow], built from the bytes"""
    b = np.ascontiguousarray(maps).view(np.uint8).reshape(maps.shape[:3] + (-1,)).astype(np.int64)
    return sum(b[..., k] << (8 * k) for k in range(b.shape[-1]))


def at_offset(maps, off):
    """a copy of the maps `off` bytes past a 16-byte boundary"""
    raw = np.zeros(maps.nbytes + 48, np.uint8)
    base = (-raw.ctypes.data) % 16 + off
    raw[base:base + maps.nbytes] = maps.reshape(-1).view(np.uint8)
    return raw[base:base + maps.nbytes].view(maps.dtype).reshape(maps.shape)


def boxes_spec(ids, lists):
    """ids [n, oh, ow] int64, lists: n sequences -> [total, 5] of (count, x0, y0, x1, y1) by np.argwhere per listed id"""
    n, oh, ow = ids.shape
    out = []
    for i in range(n):
        for m in lists[i]:
            at = np.argwhere(ids[i] == m)
            out.append((len(at), at[:, 1].min(), at[:, 0].min(), at[:, 1].max() + 1, at[:, 0].max() + 1) if len(at) else (0, ow, oh, 0, 0))
    return np.array(out, np.int64).reshape(-1, 5)


def blobs(rng, n, oh, ow, pool):
    """rectangles of ids drawn from `pool` over a background of pool[0], int64"""
    pool = np.asarray(pool, np.int64)
    return pool[blobs16(rng, n, oh, ow, range(len(pool))).astype(np.int64)]


def draw(rng, mb, n, oh, ow, noise=False):
    """ids [n, oh, ow] of HIGH_BYTES in blobs (or pixel by pixel), and per sample a sorted list of some ids the map has, some it has
    not; the sample in the middle of three lists nothing"""
    pool = HIGH_BYTES[mb]
    ids = np.asarray(pool, np.int64)[rng.integers(0, len(pool), size=(n, oh, ow))] if noise else blobs(rng, n, oh, ow, pool)
    lists = [sorted({int(m) for m in pool if rng.integers(0, 3)} | {int(x) for x in rng.integers(0, TOP[mb] + 1, size=2)}) for _ in range(n)]
    if n == 3:
        lists[1] = []
    return ids, lists


@pytest.mark.parametrize("mb", WIDTHS)
def test_boxes_reference_is_numpy(mi, mb):
    B = mi.label_boxes_rows()
    rng = np.random.default_rng(32 + mb)
    for ow in (1, 5, 6, 7, 11, 16, 17, 33):
        for oh in (1, B - 1, B, B + 1, 2 * B + 3):
            for off in BOX_OFFSETS[mb]:
                ids, lists = draw(rng, mb, 3, oh, ow, noise=off in (2, 4))
                maps = at_offset(wide_maps(ids, mb), off)
                assert np.array_equal(ids_of(maps), ids)
                got = mi.label_boxes32_reference(maps, lists)
                assert got.dtype == mi.LABEL_BOX_DTYPE and got.shape == (sum(len(l) for l in lists),)
                assert np.array_equal(as_table(got), boxes_spec(ids, lists)), (ow, oh, off)


@pytest.mark.parametrize("mb", WIDTHS)
def test_ids_that_differ_in_the_high_bytes_only_and_the_ends_of_the_range(mi, mb):
    B = mi.label_boxes_rows()
    pool = HIGH_BYTES[mb]
    rng = np.random.default_rng(mb)
    ids = blobs(rng, 2, B + 7, 45, pool)
    ids[:, 0, :len(pool)] = pool  # every id is present
    lists = [sorted(pool), sorted(pool)[1:]]
    got = as_table(mi.label_boxes32_reference(at_offset(wide_maps(ids, mb), 5 if mb == 3 else 4), lists))
    assert np.array_equal(got, boxes_spec(ids, lists)) and (got[:, 0] > 0).all()
    assert got[:len(pool), 0].sum() == ids[0].size  # every pixel of sample 0 is counted once
    low = (ids[0] & 0xFFFF) == 1
    assert got[sorted(pool).index(1), 0] < low.sum()  # (what a test of the two low bytes alone would count)
    one = np.full((1, 2 * B + 1, 70), TOP[mb], np.int64)  # a map of the top id alone: the id a finder might take for "none"
    got = mi.label_boxes32_reference(wide_maps(one, mb), [[0, TOP[mb] - 1, TOP[mb]]])
    assert [tuple(r) for r in got] == [(0, 70, 2 * B + 1, 0, 0)] * 2 + [(70 * (2 * B + 1), 0, 0, 70, 2 * B + 1)]
    got = mi.label_boxes32_reference(wide_maps(one, mb), [[0, TOP[mb] - 1]])  # ... and present but not listed
    assert [tuple(r) for r in got] == [(0, 70, 2 * B + 1, 0, 0)] * 2
    assert mi.label_boxes32_reference(wide_maps(one, mb), [[]]).shape == (0,)


@pytest.mark.parametrize("mb", WIDTHS)
@pytest.mark.parametrize("count", [1, 256, 257, 1024, 1025, 4096])
def test_list_lengths_around_the_capacities(mi, mb, count):
    B = mi.label_boxes_rows()
    rng = np.random.default_rng(count + mb)
    listed = np.concatenate([np.unique(rng.integers(0, TOP[mb], size=count + 64))[:count - 1], [TOP[mb]]])  # (ascending, the top id last)
    assert len(listed) == count
    others = rng.integers(0, TOP[mb] + 1, size=50)
    pool = np.concatenate([listed[:: max(2, count // 300)], listed[-1:], others])
    ids = pool[rng.integers(0, len(pool), size=(2, B + 5, 41))].astype(np.int64)
    lists = [listed.tolist(), listed[: count // 2 + 1].tolist()]
    maps = wide_maps(ids, mb)
    assert np.array_equal(as_table(mi.label_boxes32_reference(maps, lists)), boxes_spec(ids, lists))
    values = [rng.integers(-2, 9, size=len(l)).tolist() for l in lists]  # (values that several ids share)
    assert np.array_equal(mi.label_targets32_reference(maps, lists, values, default=-100), index_spec(ids, lists, values, -100, np.int64))


@pytest.mark.parametrize("mb", WIDTHS)
def test_targets_reference_is_numpy(mi, mb):
    S = mi.label_targets_segment()
    rng = np.random.default_rng(64 + mb)
    for k, (oh, ow) in enumerate(((1, 1), (7, 585), (64, 64), (17, 241), (7, 1171))):  # 1, S - 1, S, S + 1 and 2 * S + 5 pixels
        assert oh * ow in (1, S - 1, S, S + 1, 2 * S + 5)
        ids, lists = draw(rng, mb, 3, oh, ow)
        maps = at_offset(wide_maps(ids, mb), BOX_OFFSETS[mb][k % len(BOX_OFFSETS[mb])])
        values = [rng.integers(-1, 4, size=len(l)).tolist() for l in lists]
        for dtype in INDEX_DTYPES:
            dflt, vals = (255, [[v & 0xFF for v in l] for l in values]) if dtype == "uint8" else (-100, values)  # an "ignore" default
            got = mi.label_targets32_reference(maps, lists, vals, dtype=dtype, default=dflt)
            assert got.dtype == np.dtype(dtype) and np.array_equal(got, index_spec(ids, lists, vals, dflt, dtype)), (oh, ow, dtype)
        for dtype in PLANE_DTYPES:
            on, off = (200, 7) if dtype == "uint8" else (0.9, 0.05)
            got = mi.label_targets32_reference(maps, lists, values, kind="planes", dtype=dtype, default=-1, planes=[3, 0, 2], on=on, off=off)
            want = planes_spec(ids, lists, values, -1, [3, 0, 2], on, off, dtype)
            assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), (oh, ow, dtype)


def test_the_same_content_through_the_widths_1_2_3_and_4(mi):
    """ids below 256: the same records and the same targets through label_boxes, label_boxes16 and label_boxes32 of both widths, and
    through label_targets of map_bytes 1 and 2 and label_targets32 of 3 and 4"""
    B = mi.label_boxes_rows()
    rng = np.random.default_rng(1234)
    narrow = rng.integers(0, 12, size=(2, B + 1, 37), dtype=np.uint8)
    narrow[0, 5:20, 3:30] = 200
    narrow[1, B - 1:, :] = 255
    everything = [range(256), range(256)]
    by_bytes = as_table(mi.label_boxes_reference(narrow)).reshape(-1, 5)
    assert np.array_equal(as_table(mi.label_boxes16_reference(narrow.astype(np.uint16), everything)), by_bytes)
    lists = [[0, 3, 7, 200], [1, 2, 255]]
    values = [[1, 1, 2, 0], [0, 2, 2]]
    index = mi.label_targets_reference(narrow, lists, values, default=-5)
    planes = mi.label_targets_reference(narrow, lists, values, kind="planes", dtype="float16", default=-1, planes=3)
    assert np.array_equal(mi.label_targets_reference(narrow.astype(np.uint16), lists, values, default=-5), index)
    for mb in WIDTHS:
        wide = at_offset(wide_maps(narrow, mb), 16 - mb)
        assert np.array_equal(as_table(mi.label_boxes32_reference(wide, everything)), by_bytes), mb
        assert np.array_equal(mi.label_targets32_reference(wide, lists, values, default=-5), index), mb
        assert np.array_equal(mi.label_targets32_reference(wide, lists, values, kind="planes", dtype="float16", default=-1, planes=3), planes), mb


def test_refusals(mi):
    L = mi._lib.load()
    raw = np.zeros(2 * 4 * 5 * 4 + 16, np.uint8)
    base = (-raw.ctypes.data) % 16
    m = raw.ctypes.data + base
    ids = np.array([0, 3, 0x01000001, 1, 2], np.uint32)
    ids3 = np.array([0, 3, 0xFFFFFF, 1, 0xFFFFFF], np.uint32)
    first = np.array([0, 3, 5], np.uint32)
    out = np.full(5, 7, mi.LABEL_BOX_DTYPE)
    before = out.copy()
    i, i3, f, o = ids.ctypes.data, ids3.ctypes.data, first.ctypes.data, out.ctypes.data

    def u32(*v):
        return np.array(v, np.uint32)

    long_ids = np.arange(4097, dtype=np.uint32)
    keep = [u32(1, 3, 5), u32(0, 4, 3), u32(0, 4097, 4097), u32(0, 3, 3, 1, 2), u32(0, 3, 2, 1, 2), u32(0, 3, 9, 2, 1)]
    for args in ((None, 4, 2, 5, 4, i, f, o), (m, 4, 2, 5, 4, None, f, o), (m, 4, 2, 5, 4, i, None, o), (m, 4, 2, 5, 4, i, f, None), (m, 4, 0, 5, 4, i, f, o),
                 (m, 4, 65536, 5, 4, i, f, o), (m, 4, 2, 0, 4, i, f, o), (m, 4, 2, 5, 0, i, f, o), (m, 4, 1, 65536, 65536, i, f, o),
                 (m, 0, 2, 5, 4, i3, f, o), (m, 1, 2, 5, 4, i3, f, o), (m, 2, 2, 5, 4, i3, f, o), (m, 5, 2, 5, 4, i3, f, o),  # a map_bytes that is not 3 or 4
                 (m + 1, 4, 2, 5, 4, i, f, o), (m + 2, 4, 2, 5, 4, i, f, o), (m + 6, 4, 2, 5, 4, i, f, o),                    # 4-byte maps not aligned to 4
                 (m, 3, 2, 5, 4, i, f, o),                                       # an id above 0xFFFFFF in a 3-byte map
                 (m, 4, 2, 5, 4, i, keep[0].ctypes.data, o),                     # first[0] != 0
                 (m, 4, 2, 5, 4, i, keep[1].ctypes.data, o),                     # a first that decreases
                 (m, 4, 2, 5, 4, long_ids.ctypes.data, keep[2].ctypes.data, o),  # a list that is too long
                 (m, 4, 2, 5, 4, keep[3].ctypes.data, f, o),                     # equal neighbours
                 (m, 4, 2, 5, 4, keep[4].ctypes.data, f, o),                     # descending in the first list
                 (m, 3, 2, 5, 4, keep[5].ctypes.data, f, o)):                    # descending in the second
        assert L.llcomp_mi_label_boxes32_reference(*args) == mi.BAD_ARGS, args[1:5]
    assert np.array_equal(out, before)
    assert L.llcomp_mi_label_boxes32_reference(m, 4, 2, 5, 4, i, f, o) == mi.OK
    assert tuple(out[0]) == (20, 0, 0, 5, 4) and tuple(out[1]) == (0, 5, 4, 0, 0) and tuple(out[3]) == (0, 5, 4, 0, 0)
    for off in (1, 2, 3):  # a 3-byte map lies anywhere
        assert L.llcomp_mi_label_boxes32_reference(m + off, 3, 2, 5, 4, i3, f, o) == mi.OK and tuple(out[0]) == (20, 0, 0, 5, 4)
    ok = mi.label_boxes32_reference(np.zeros((1, 2, 2), np.uint32), [range(4096)])  # the longest list is fine
    assert ok.shape == (4096,) and tuple(ok[0]) == (4, 0, 0, 2, 2)
    maps3, maps4 = np.zeros((2, 4, 5, 3), np.uint8), np.zeros((2, 4, 5), np.uint32)
    for bad, lists in ((np.zeros((2, 4, 5), np.uint8), [[1], [1]]), (np.zeros((2, 4, 5), np.uint16), [[1], [1]]), (np.zeros((2, 4, 5, 4), np.uint8), [[1], [1]]),
                       (maps4, [[1]]), (maps4, [[1], [1 << 32]]), (maps3, [[1], [1 << 24]]), (maps4, [[1], [-1]]), (maps4, [[2, 1], []]), (maps3, [range(4097), []])):
        with pytest.raises(mi.LlcompError):
            mi.label_boxes32_reference(bad, lists)
        with pytest.raises(mi.LlcompError):
            mi.label_targets32_reference(bad, lists, [[0] * len(list(l)) for l in lists])
    for old in (mi.label_boxes16_reference, lambda a, l: mi.label_targets_reference(a, l, [[0], [0]])):  # the old calls go on refusing wide maps
        for wide in (maps3, maps4):
            with pytest.raises(mi.LlcompError):
                old(wide, [[1], [1]])
    # llcomp_mi_label_targets.map_bytes of 3 or 4 stays BAD_ARGS; the new struct refuses 1 and 2
    values = np.zeros(5, np.int32)
    tout = np.full(2 * 20 * 8, 0x5A, np.uint8)
    for struct, call, good in ((mi._lib.LabelTargets, L.llcomp_mi_label_targets_reference, (1, 2)), (mi._lib.LabelTargets32, L.llcomp_mi_label_targets32_reference, (3, 4))):
        for mb in (0, 1, 2, 3, 4, 5):
            lst = np.array([0, 3, 9, 1, 2], np.uint16 if struct is mi._lib.LabelTargets else np.uint32)
            t = struct(C.sizeof(struct), mb, mi.TARGET_INDEX, mi.TARGET_I64, -1, 0, 0, lst.ctypes.data, values.ctypes.data, first.ctypes.data, None)
            rc = call(m, 2, 5, 4, C.byref(t), tout.ctypes.data)
            assert rc == (mi.OK if mb in good else mi.BAD_ARGS), (struct.__name__, mb)
            if mb not in good:
                assert (tout == 0x5A).all()
            tout[:] = 0x5A
    assert C.sizeof(mi._lib.LabelTargets32) == 64 and mi._lib.LabelTargets32.ids.offset == 32
