"""The rule of the batch copy-paste by 16-bit ids on the host (llcomp_mi_paste16_reference; include/llcomp_mi.h: "Batch copy-paste by
16-bit ids") against tests/paste16_spec.py -- numpy's where per piece in list order -- bit for bit: ids that differ in the high byte
only, the borders of a window, a window that passes 65535, a set of 600 ids split into windows, the 8-bit call on narrowed maps, maps
that are their own source, the plan, the refusals."""
import ctypes as C

import numpy as np
import pytest

import paste16_spec
import paste_spec
from paste16_spec import Window, bits_of

DTYPES = ("uint8", "float32", "float16", "bfloat16")
ESIZE = {"uint8": 1, "float32": 4, "float16": 2, "bfloat16": 2}


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


def window_piece(mi, rect, base, lut, value_bits=None):
    """one llcomp_mi_paste_piece16 as the C struct has it, for the spec's Window(base, lut)"""
    p = mi.PastePiece16()
    for name, v in zip(("dst", "src", "dx", "dy", "sx", "sy", "w", "h"), rect):
        setattr(p, name, int(v))
    p.id_base = int(base)
    for j in np.flatnonzero(np.asarray(lut, bool)):
        p.ids[int(j) >> 5] |= 1 << (int(j) & 31)
    if value_bits is not None:
        p.flags, p.value_bits = mi.PASTE_VALUE, int(value_bits)
    return p


def as_array(mi, pieces):
    arr = (mi.PastePiece16 * len(pieces))()
    for i, p in enumerate(pieces):
        arr[i] = p
    return arr


def window_cases(rng):
    """(mask pool, [(base, lut)]) for the borders of a window: ids at id_base - 1, id_base, id_base + 255 and id_base + 256 with the
    first and the last bit set, and id_base 65400 with all bits set (bits above 65535 select nothing and are not refused)"""
    edge = np.zeros(256, bool)
    edge[[0, 255]] = True
    drawn = rng.integers(0, 2, size=256).astype(bool)
    return [((999, 1000, 1255, 1256, 1100), [(1000, edge), (1000, drawn), (1000, ~edge)]),
            ((65399, 65400, 65535, 0, 119, 120, 65500), [(65400, np.ones(256, bool)), (65535, np.ones(256, bool)), (65400, drawn)]),
            ((0, 255, 256, 65535), [(0, edge), (1, edge), (0, np.ones(256, bool))])]


@pytest.mark.parametrize("c", (1, 3))
@pytest.mark.parametrize("layout", ("chw", "hwc"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_is_the_spec(mi, dtype, layout, c):
    rng = np.random.default_rng(c * 100 + len(dtype) + len(layout))
    any_value = False
    for rnd in range(10):
        n_src, n_dst = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        iw, ih, ow, oh = (int(rng.integers(1, 40)) for _ in range(4))
        pieces = paste16_spec.random_pieces(rng, n_src, iw, ih, n_dst, ow, oh, int(rng.integers(0, 10)), ESIZE[dtype])
        any_value |= any(len(p) > 9 for p in pieces)
        src = paste16_spec.gen_batch(dtype, n_src, c, ih, iw, layout, seed=rnd)
        mask = paste16_spec.gen_mask(rng, n_src, ih, iw)  # ids that share low bytes: a test of the low byte alone fails here
        dst = paste16_spec.gen_batch(dtype, n_dst, c, oh, ow, layout, seed=100 + rnd)
        want = bits_of(paste16_spec.apply(src, mask, dst, pieces, layout))
        got = mi.paste16_reference(src, mask, dst, pieces, layout=layout, dtype=dtype)
        assert got.shape == dst.shape and got.dtype == dst.dtype
        assert np.array_equal(bits_of(got), want), (dtype, layout, c, rnd, pieces)
        # ... and with out == dst_in
        twice = dst.copy()
        recs = mi.paste_pieces16(pieces)
        rc = mi._lib.load().llcomp_mi_paste16_reference(src.ctypes.data, mask.ctypes.data, n_src, iw, ih, twice.ctypes.data, n_dst, ow, oh, c,
                                                        mi._dtype_code(dtype), mi._layout_code(layout), recs, len(recs), twice.ctypes.data)
        assert rc == mi.OK and np.array_equal(bits_of(twice), want), (dtype, layout, c, rnd, "in place")
    assert any_value
    one = paste16_spec.gen_mask(rng, 1, 30, 30)
    assert 0 < paste16_spec.select(one, [0x0101]).sum() < ((one & 0xFF) == 1).sum()  # (the maps tell the low byte's test from the rule)


@pytest.mark.parametrize("dtype,layout,c", [("float16", "chw", 3), ("uint8", "hwc", 3), ("float32", "hwc", 2), ("uint8", "chw", 1)])
def test_the_borders_of_a_window(mi, dtype, layout, c):
    rng = np.random.default_rng(c + len(dtype))
    for pool, windows in window_cases(rng):
        src = paste16_spec.gen_batch(dtype, 2, c, 9, 37, layout, seed=1)
        dst = paste16_spec.gen_batch(dtype, 2, c, 11, 40, layout, seed=2)
        mask = paste16_spec.gen_mask(rng, 2, 9, 37, pool)
        rects = [(i % 2, (i + 1) % 2, i, 1, 2 * i, 0, 30, 8) for i in range(len(windows))]
        value = [None, (1 << (8 * ESIZE[dtype])) - 2, None]
        spec = [r + (Window(b, lut), v) for r, (b, lut), v in zip(rects, windows, value)]
        recs = as_array(mi, [window_piece(mi, r, b, lut, v) for r, (b, lut), v in zip(rects, windows, value)])
        want = paste16_spec.apply(src, mask, dst, spec, layout)
        got = mi.paste16_reference(src, mask, dst, recs, layout=layout, dtype=dtype)
        assert np.array_equal(bits_of(got), bits_of(want)), (pool, [b for b, _ in windows])
        assert not np.array_equal(bits_of(got), bits_of(dst))
    # the ids next to a window, one by one
    edge = np.zeros(256, bool)
    edge[[0, 255]] = True
    m = np.array([999, 1000, 1255, 1256, 1000 + 65536 - 65536, 488], np.uint16)
    assert paste16_spec.select(m, Window(1000, edge)).tolist() == [False, True, True, False, True, False]
    assert paste16_spec.select(np.array([65399, 65400, 65535, 0, 119], np.uint16), Window(65400, np.ones(256, bool))).tolist() == [False, True, True, False, False]


def test_a_set_of_600_ids_is_split_into_windows(mi):
    rng = np.random.default_rng(600)
    ids = sorted(int(v) for v in rng.choice(3000, 600, replace=False) + 200)
    recs = mi.paste_pieces16([(0, 1, 2, 1, 0, 3, 40, 20, ids), (1, 0, 0, 0, 0, 0, 5, 5, [7], 0x1234)])
    n = len(recs) - 1
    assert 600 / 256 <= n <= 12 and recs[n].flags == mi.PASTE_VALUE and recs[n].value_bits == 0x1234 and recs[n].id_base == 7 and recs[n].ids[0] == 1
    seen = []
    for i in range(n):  # one piece per window, in order, over the same rectangle; a window begins at its lowest id
        p = recs[i]
        assert (p.dst, p.src, p.dx, p.dy, p.sx, p.sy, p.w, p.h, p.flags, p.value_bits) == (0, 1, 2, 1, 0, 3, 40, 20, 0, 0) and p.ids[0] & 1
        seen += [p.id_base + j for j in range(256) if (p.ids[j >> 5] >> (j & 31)) & 1]
    assert seen == ids
    src = paste16_spec.gen_batch("float16", 2, 3, 25, 45, "chw", seed=3)
    dst = paste16_spec.gen_batch("float16", 2, 3, 22, 44, "chw", seed=4)
    mask = rng.integers(0, 3400, size=(2, 25, 45)).astype(np.uint16)
    pieces = [(0, 1, 2, 1, 0, 3, 40, 20, ids), (1, 0, 0, 0, 0, 0, 5, 5, [7], 0x1234)]
    got = mi.paste16_reference(src, mask, dst, pieces, dtype="float16")
    assert np.array_equal(bits_of(got), bits_of(paste16_spec.apply(src, mask, dst, pieces, "chw")))  # (the spec takes the set as a whole)
    nz = mi.paste_pieces16([(0, 0, 0, 0, 0, 0, 1, 1, "nonzero")])
    assert len(nz) == 256 == mi.paste_max_pieces_per_sample() and nz[0].id_base == 1 and nz[255].id_base == 65281
    got = mi.paste16_reference(src, mask, dst, [(0, 1, 0, 0, 0, 0, 44, 22, "nonzero")], dtype="float16")
    assert np.array_equal(bits_of(got), bits_of(paste16_spec.apply(src, mask, dst, [(0, 1, 0, 0, 0, 0, 44, 22, "nonzero")], "chw")))
    assert len(mi.paste_pieces16([(0, 0, 0, 0, 0, 0, 1, 1, [])])) == 1


@pytest.mark.parametrize("dtype,layout,c", [("uint8", "chw", 3), ("float32", "hwc", 3), ("bfloat16", "chw", 1)])
def test_ids_below_256_are_the_8_bit_call(mi, dtype, layout, c):
    rng = np.random.default_rng(8 + c)
    src = paste_spec.gen_batch(dtype, 3, c, 17, 21, layout, seed=1)
    dst = paste_spec.gen_batch(dtype, 2, c, 23, 30, layout, seed=2)
    narrow = paste_spec.gen_mask(rng, 3, 17, 21)
    pieces = [p[:9] for p in paste_spec.random_pieces(rng, 3, 21, 17, 2, 30, 23, 10, dtype)]
    recs = as_array(mi, [window_piece(mi, p[:8], 0, paste_spec.lut_of(p[8])) for p in pieces])
    got = mi.paste16_reference(src, narrow.astype(np.uint16), dst, recs, layout=layout, dtype=dtype)
    assert np.array_equal(bits_of(got), bits_of(mi.paste_reference(src, narrow, dst, pieces, layout=layout, dtype=dtype)))


def test_maps_that_are_their_own_source(mi):
    rng = np.random.default_rng(6)
    maps = paste16_spec.gen_mask(rng, 2, 20, 30, (0, 300, 301, 0x2C01, 65535))
    dst = paste16_spec.gen_mask(rng, 2, 20, 30, (0, 5, 0x0105))
    # a 2-byte dtype with c == 1: the instances of map s land in dst map s under new ids (VALUE pieces), the background stays out
    new_id = {300: 1000, 301: 1001, 0x2C01: 40000, 65535: 2}
    pieces = [(s, s, 4, 2, 1, 3, 22, 15, [m], v) for s in range(2) for m, v in new_id.items()]
    for dtype in ("float16", "bfloat16"):
        as_dtype = (maps.view(np.float16) if dtype == "float16" else maps)[:, None]  # [n, 1, h, w]: src and mask at once
        got = mi.paste16_reference(as_dtype, as_dtype, (dst.view(np.float16) if dtype == "float16" else dst)[:, None], pieces, dtype=dtype)
        want = dst.copy()
        for s in range(2):
            win = maps[s, 3:18, 1:23]
            for m, v in new_id.items():
                want[s, 2:17, 4:26][win == m] = v
        assert np.array_equal(bits_of(got)[:, 0], want)
        assert np.array_equal(want, paste16_spec.apply(maps[:, None], maps, dst[:, None], pieces, "chw")[:, 0])
    # ... and the instance map itself, pasted by id: no VALUE
    own = maps[:, None]
    got = mi.paste16_reference(own, own, dst[:, None], [(0, 1, 0, 0, 0, 0, 30, 20, [301, 0x2C01])], dtype="bfloat16")
    assert np.array_equal(got[0, 0], np.where((maps[1] == 301) | (maps[1] == 0x2C01), maps[1], dst[0])) and np.array_equal(got[1, 0], dst[1])
    # U8 HWC with c == 2: the two bytes of an id are the two channels
    as_bytes, dst_bytes = maps.view(np.uint8).reshape(2, 20, 30, 2), dst.view(np.uint8).reshape(2, 20, 30, 2)
    got = mi.paste16_reference(as_bytes, as_bytes, dst_bytes, [(0, 1, 3, 0, 0, 0, 27, 20, [301, 0x2C01, 65535])], layout="hwc", dtype="uint8")
    want = paste16_spec.apply(maps[:, None], maps, dst[:, None], [(0, 1, 3, 0, 0, 0, 27, 20, [301, 0x2C01, 65535])], "chw")[:, 0]
    assert np.array_equal(got.reshape(2, 20, 60).view(np.uint16), want) and not np.array_equal(want, dst)


def test_plan_is_a_stable_sort_by_dst_without_the_ignored_pieces(mi):
    rng = np.random.default_rng(5)
    for rnd in range(10):
        n_dst = int(rng.integers(1, 9))
        pieces = paste16_spec.random_pieces(rng, 2, 9, 9, n_dst, 300, 70, int(rng.integers(0, 30)), 1)
        pieces = [p[:8] + ([],) + p[9:] if i % 5 == 4 else p for i, p in enumerate(pieces)]  # some select nothing
        recs = mi.paste_pieces16(pieces)
        live = [i for i in range(len(recs)) if recs[i].w and recs[i].h and any(recs[i].ids)]
        for dtype, layout, c, pixel_bytes in (("uint8", "chw", 3, 1), ("float32", "hwc", 3, 12)):
            use = recs
            if dtype != "uint8":
                use = mi.paste_pieces16([p[:9] for p in pieces])
            samples, first, order, wgs = mi.paste16_plan(2, 9, 9, n_dst, 300, 70, c, use, dtype=dtype, layout=layout)
            assert order.tolist() == sorted(live, key=lambda i: recs[i].dst)  # (Python's sort is stable)
            want_samples = sorted({recs[i].dst for i in live})
            assert samples.tolist() == want_samples
            assert first.tolist() == [sum(recs[i].dst < d for i in live) for d in want_samples] + [len(live)]
            T, R = mi.compose_tile(), mi.compose_tile(pixel_bytes)
            assert wgs == len(want_samples) * (c if layout == "chw" else 1) * -(-300 // T) * -(-70 // R)
    # a window that lies above 65535 altogether selects nothing: checked and ignored
    above = as_array(mi, [window_piece(mi, (0, 0, 0, 0, 0, 0, 2, 2), 65535, [False] + [True] * 255)])
    assert mi.paste16_plan(1, 4, 4, 1, 4, 4, 1, above)[3] == 0


def test_refusals_leave_out_untouched(mi):
    L = mi._lib.load()
    n_src, n_dst, c, iw, ih, ow, oh = 2, 2, 3, 5, 4, 8, 6
    src = paste16_spec.gen_batch("float16", n_src, c, ih, iw, "chw", seed=2)
    dst = paste16_spec.gen_batch("float16", n_dst, c, oh, ow, "chw", seed=3)
    mask = paste16_spec.gen_mask(np.random.default_rng(1), n_src, ih, iw)
    out = np.full(dst.shape, 7.0, np.float16)
    ok = [(1, 1, 2, 1, 1, 0, 4, 4, [1, 0x0101, 0xFF01]), (0, 0, 0, 0, 0, 0, 3, 3, [2, 0x0102], 0x4100)]

    def call(pieces=ok, src_p=src.ctypes.data, mask_p=mask.ctypes.data, n_src=n_src, iw=iw, ih=ih, dst_p=dst.ctypes.data, n_dst=n_dst, ow=ow, oh=oh,
             c=c, dtype=2, layout=1, out_p=out.ctypes.data, n_pieces=None, recs=0):
        recs = mi.paste_pieces16(pieces) if recs == 0 else recs
        return L.llcomp_mi_paste16_reference(src_p, mask_p, n_src, iw, ih, dst_p, n_dst, ow, oh, c, dtype, layout, recs,
                                             (len(recs) if recs is not None else 1) if n_pieces is None else n_pieces, out_p)

    assert mi._dtype_code("float16") == 2 and mi._layout_code("chw") == 1
    A = [1]
    bad_pieces = [(2, 0, 0, 0, 0, 0, 1, 1, A), (0, 2, 0, 0, 0, 0, 1, 1, A), (0, 0, 5, 0, 0, 0, 4, 1, A), (0, 0, 0, 3, 0, 0, 1, 4, A),
                  (0, 0, 9, 0, 0, 0, 0, 0, A), (0, 0, 0, 0, 2, 0, 4, 1, A), (0, 0, 0, 0, 0, 1, 1, 4, A), (0, 0, 0, 0, 0, 0, 6, 1, A),
                  (0, 0, 0, 0, 6, 0, 0, 0, A), (0, 0, 0xFFFFFFFF, 0, 0, 0, 2, 1, A), (0, 0, 0, 0, 0, 0, 1, 1, A, 0x10000), (0, 2, 0, 0, 0, 0, 0, 0, [])]
    for p in bad_pieces:
        assert call([ok[0], p]) == mi.BAD_ARGS, p
    for flags, value, base in ((2, 0, 1), (3, 1, 1), (0, 1, 1), (0x80000000, 0, 1), (0, 0, 65536), (0, 0, 0xFFFFFFFF), (1, 0x10000, 1), (1, 0x80000000, 1)):
        recs = mi.paste_pieces16(ok)  # flag bits above bit 0; value_bits without VALUE or above the element; an id_base above 65535
        recs[0].flags, recs[0].value_bits, recs[0].id_base = flags, value, base
        assert call(recs=recs) == mi.BAD_ARGS, (flags, value, base)
    assert call([(0, 0, 0, 0, 0, 0, 1, 1, A, 0x100)], dtype=0) == mi.BAD_ARGS
    assert mi.paste16_plan(2, 5, 4, 2, 8, 6, 3, [(0, 0, 0, 0, 0, 0, 1, 1, A, 0xFFFFFFFF)], dtype="float32")[3] > 0  # (all 32 bits are an F32's)
    out[:] = 7.0
    for kw in (dict(src_p=None), dict(mask_p=None), dict(dst_p=None), dict(out_p=None), dict(recs=None), dict(n_dst=0), dict(n_dst=65536),
               dict(n_src=65536), dict(n_src=0), dict(ow=0), dict(oh=0), dict(c=0), dict(iw=0), dict(ih=0), dict(dtype=4), dict(layout=2),
               dict(n_pieces=(1 << 20) + 1), dict(src_p=src.ctypes.data + 1), dict(out_p=out.ctypes.data + 1),
               dict(mask_p=mask.ctypes.data + 1),                                       # a mask not aligned to 2 bytes
               dict(src_p=out.ctypes.data + 4, n_src=1), dict(mask_p=out.ctypes.data + out.nbytes - 2), dict(mask_p=out.ctypes.data - 2 * 2 * 20 + 2),
               dict(ow=1 << 31, oh=1, pieces=[]), dict(layout=0, ow=1 << 30, c=3, oh=1, pieces=[]), dict(iw=1 << 31, ih=1, pieces=[]),
               dict(n_src=0, iw=0, ih=0, src_p=None, mask_p=None)):
        assert call(**kw) == mi.BAD_ARGS, kw
    cap = mi.paste_max_pieces_per_sample()
    assert call([ok[0][:8] + (A,)] * (cap + 1)) == mi.BAD_ARGS
    assert call([ok[0][:8] + (A,)] * cap + [(1, 0, 1, 1, 0, 0, 1, 1, [])]) == mi.BAD_ARGS  # a piece without an id bit counts: it has w and h
    assert (out == 7.0).all()
    assert call([ok[0][:8] + (A,)] * cap + [(1, 0, 8, 6, 0, 0, 0, 0, A)] + [(0, 0, 0, 0, 0, 0, 1, 1, A)]) == mi.OK  # empty ones do not count
    assert call() == mi.OK
    assert np.array_equal(bits_of(out), bits_of(paste16_spec.apply(src, mask, dst, ok, "chw")))
    assert call(pieces=[], n_src=0, iw=0, ih=0, src_p=None, mask_p=None) == mi.OK  # no piece: no src batch needed, out = dst_in
    assert np.array_equal(bits_of(out), bits_of(dst))
    for bad in ([(0, 0, 0)], [(0, 0, 0, 0, 0, 0, -1, 1, A)], [(0, 0, 0, 0, 0, 0, 1, 1, [65536])], [(0, 0, 0, 0, 0, 0, 1, 1, [-1])],
                [(0, 0, 0, 0, 0, 0, 1, 1, "all")], [(0, 0, 0, 0, 0, 0, 1, 1, A, -1)]):
        with pytest.raises(mi.LlcompError) as e:
            mi.paste_pieces16(bad)
        assert e.value.status == mi.BAD_ARGS
    with pytest.raises(mi.LlcompError):
        mi.paste_pieces([(0, 0, 0, 0, 0, 0, 1, 1, [256])])  # the 8-bit helper goes on refusing ids above 255
    with pytest.raises(mi.LlcompError):
        mi.paste16_reference(src, mask.astype(np.uint8), dst, ok)  # a mask of bytes
    with pytest.raises(mi.LlcompError):
        mi.paste16_reference(src, mask[:1], dst, ok)  # a mask of another shape
    with pytest.raises(mi.LlcompError):
        mi.paste16_plan(2, 5, 4, 2, 8, 6, 3, [(2, 0, 0, 0, 0, 0, 1, 1, A)])
    assert C.sizeof(mi.PastePiece16) == 76 and mi.PastePiece16.ids.offset == 44 and mi.PastePiece16.id_base.offset == 40
