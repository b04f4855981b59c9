"""The rule of the batch copy-paste by ids of 3 and 4 bytes on the host (llcomp_mi_paste32_reference, llcomp_mi_paste32_plan;
include/llcomp_mi.h: "Wide id maps") against a numpy spec written here -- the ids built from the maps' bytes, every piece in list order
pasted by a boolean mask, out = np.where(sel, piece, out) -- bit for bit; windows whose id_base + 255 passes the top id; VALUE_PIXEL for
c = 1..4; the maps as their own source; the refusals; and the same content through the widths 1, 2, 3 and 4.  apply32, gen_ids and
random_pieces32 are what the GPU tests use too."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

import paste16_spec
from batch_support import BITS, DTYPES, ESIZE, gen_batch
from test_wide_id_maps_rule import TOP, WIDTHS, at_offset, ids_of, wide_maps


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


Window = namedtuple("Window", "base lut")  # one piece as the C struct has it: lut 256 bools, bit j for id base + j
POOL = {3: (0x000001, 0x010001, 0xFF0001, 0x000002, 0x010002, 0x000000, 0xFFFFFF, 0x00FF00),
        4: (0x000001, 0x010001, 0xFF0001, 0x01000001, 0x000002, 0x000000, 0xFFFFFFFF, 0x00FFFFFF)}


def select(m, ids):
    """the pixels of the int64 id array m that the ids select: a set of ids by membership, a Window by the struct's rule without wrap"""
    if isinstance(ids, Window):
        d = m - int(ids.base)
        return (d >= 0) & (d < 256) & np.asarray(ids.lut, bool)[np.clip(d, 0, 255)]
    return np.isin(m, np.asarray(list(ids), np.int64))


def apply32(src, ids, dst, pieces, layout):
    """src and dst batches, ids [n_src, ih, iw] int64; a piece (dst, src, dx, dy, sx, sy, w, h, ids[, value_bits[, pixel]]) -> the pasted dst"""
    out = np.ascontiguousarray(dst).copy()
    ob, sb = out.view(BITS[out.itemsize]), np.ascontiguousarray(src).view(BITS[out.itemsize])
    for p in pieces:
        d, s, dx, dy, sx, sy, w, h = (int(v) for v in p[:8])
        sel = select(ids[s, sy:sy + h, sx:sx + w], p[8])
        value = None
        if len(p) > 9 and p[9] is not None:
            value = BITS[out.itemsize](int(p[9]) & ((1 << (8 * out.itemsize)) - 1))
            if len(p) > 10 and p[10]:  # VALUE_PIXEL: channel ch takes byte ch
                assert layout == "hwc" and out.itemsize == 1
                value = np.array([(int(p[9]) >> (8 * ch)) & 0xFF for ch in range(out.shape[3])], np.uint8)
        if layout == "chw":
            piece = value if value is not None else sb[s, :, sy:sy + h, sx:sx + w]
            ob[d][:, dy:dy + h, dx:dx + w] = np.where(sel, piece, ob[d][:, dy:dy + h, dx:dx + w])
        else:
            piece = value if value is not None else sb[s, sy:sy + h, sx:sx + w, :]
            ob[d][dy:dy + h, dx:dx + w, :] = np.where(sel[..., None], piece, ob[d][dy:dy + h, dx:dx + w, :])
    return out


def gen_ids(rng, mb, n, ih, iw):
    return np.asarray(POOL[mb], np.int64)[rng.integers(0, len(POOL[mb]), size=(n, ih, iw))]


def random_pieces32(rng, mb, n_src, iw, ih, n_dst, ow, oh, n, esize, pixel_c=0):
    """n drawn pieces: they overlap and hide each other, some are empty, some VALUE (VALUE_PIXEL where pixel_c channels allow it)"""
    out = []
    for _ in range(n):
        mw, mh = min(iw, ow), min(ih, oh)
        w = 0 if rng.integers(8) == 0 else int(rng.integers(1, mw + 1))
        h = 0 if rng.integers(8) == 0 else int(rng.integers(1, mh + 1))
        chosen = sorted(int(m) for m in rng.choice(POOL[mb], len(POOL[mb]) // 2, replace=False))
        p = (int(rng.integers(n_dst)), int(rng.integers(n_src)), int(rng.integers(0, ow - w + 1)), int(rng.integers(0, oh - h + 1)),
             int(rng.integers(0, iw - w + 1)), int(rng.integers(0, ih - h + 1)), w, h, chosen)
        kind = rng.integers(4)
        if kind == 0:
            p += (int(rng.integers(0, 1 << (8 * esize), dtype=np.uint64)),)
        elif kind == 1 and pixel_c:
            p += (int(rng.integers(0, 1 << (8 * pixel_c), dtype=np.uint64)), True)
        out.append(p)
    return out


def window_array(mi, recs):
    """records whose ids are Windows -> the ctypes array of PastePiece32, one piece each"""
    arr = (mi.PastePiece32 * len(recs))()
    for i, r in enumerate(recs):
        p = arr[i]
        p.dst, p.src, p.dx, p.dy, p.sx, p.sy, p.w, p.h = (int(v) for v in r[:8])
        p.id_base = int(r[8].base)
        for j in np.flatnonzero(r[8].lut):
            p.ids[int(j) >> 5] |= 1 << (int(j) & 31)
        if len(r) > 9 and r[9] is not None:
            p.flags, p.value_bits = mi.PASTE_VALUE | (mi.PASTE_VALUE_PIXEL if len(r) > 10 and r[10] else 0), int(r[9])
    return arr


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8))


@pytest.mark.parametrize("mb", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ("chw", "hwc"))
def test_reference_is_the_spec(mi, mb, dtype, layout):
    rng = np.random.default_rng(mb * 100 + ESIZE[dtype])
    for c in (1, 3, 4):
        for off in (0, 5 if mb == 3 else 4, 15 if mb == 3 else 12):
            n_src, n_dst, iw, ih, ow, oh = 2, 2, 37, 6, 41, 5
            src, dst = gen_batch(dtype, n_src, c, ih, iw, layout, 1), gen_batch(dtype, n_dst, c, oh, ow, layout, 2)
            ids = gen_ids(rng, mb, n_src, ih, iw)
            pixel_c = c if dtype == "uint8" and layout == "hwc" else 0
            pieces = random_pieces32(rng, mb, n_src, iw, ih, n_dst, ow, oh, 9, ESIZE[dtype], pixel_c)
            maps = at_offset(wide_maps(ids, mb), off)
            assert np.array_equal(ids_of(maps), ids)
            got = mi.paste32_reference(src, maps, dst, pieces, layout, dtype)
            assert same_bits(got, apply32(src, ids, dst, pieces, layout)), (c, off)


@pytest.mark.parametrize("mb", WIDTHS)
@pytest.mark.parametrize("c", (1, 2, 3, 4))
def test_value_pixel_writes_a_byte_per_channel(mi, mb, c):
    rng = np.random.default_rng(c)
    ids = gen_ids(rng, mb, 1, 5, 19)
    src, dst = gen_batch("uint8", 1, c, 5, 19, "hwc", 3), gen_batch("uint8", 1, c, 5, 19, "hwc", 4)
    value = 0x04030201 & ((1 << (8 * c)) - 1)
    pieces = [(0, 0, 1, 0, 0, 0, 18, 5, [POOL[mb][0], POOL[mb][1], TOP[mb]], value, True), (0, 0, 0, 1, 0, 1, 19, 3, [POOL[mb][2]], 0x7)]
    got = mi.paste32_reference(src, wide_maps(ids, mb), dst, pieces, "hwc")
    assert same_bits(got, apply32(src, ids, dst, pieces, "hwc"))
    sel = np.isin(ids[0, :, :18], [POOL[mb][0], POOL[mb][1], TOP[mb]]) & ~np.pad(ids[0, 1:4, 1:] == POOL[mb][2], ((1, 1), (0, 0)))
    assert sel.any() and (got[0, :, 1:][sel] == np.arange(1, c + 1)).all()
    if c < 4:
        with pytest.raises(mi.LlcompError):  # a byte at or above c
            mi.paste32_reference(src, wide_maps(ids, mb), dst, [pieces[0][:9] + (1 << (8 * c), True)], "hwc")


@pytest.mark.parametrize("mb", WIDTHS)
def test_windows_that_pass_the_top_id(mi, mb):
    """id_base + 255 above the top id: those bits select nothing -- for 4 bytes not the low ids either, which 32-bit arithmetic would
    wrap into the window -- and a piece with no other bit set is ignored by the plan"""
    rng = np.random.default_rng(mb)
    top = TOP[mb]
    ids = np.asarray([0, 1, 5, top, top - 1, top - 200, 0x0100], np.int64)[rng.integers(0, 7, size=(1, 6, 23))]
    src, dst = gen_batch("float16", 1, 3, 6, 23, "chw", 5), gen_batch("float16", 1, 3, 6, 23, "chw", 6)
    all_bits = np.ones(256, bool)
    low = np.zeros(256, bool)
    low[:10] = True
    high = ~low
    recs = [(0, 0, 0, 0, 0, 0, 23, 6, Window(top - 9, all_bits)),       # selects top - 9 .. top and nothing else
            (0, 0, 0, 0, 0, 0, 23, 3, Window(top - 9, high), 0x3C00),   # no id below 2^(8 mb): ignored
            (0, 0, 2, 1, 1, 0, 20, 5, Window(top - 200, low))]
    arr = window_array(mi, recs)
    got = mi.paste32_reference(src, wide_maps(ids, mb), dst, arr, "chw")
    want = apply32(src, ids, dst, recs, "chw")
    assert same_bits(got, want) and not same_bits(want, dst)
    assert same_bits(want, apply32(src, ids, dst, [recs[0], recs[2]], "chw"))  # the second piece gave nothing
    samples, first, order, _ = mi.paste32_plan(mb, 1, 23, 6, 1, 23, 6, 3, arr, "float16", "chw")
    assert samples.tolist() == [0] and order.tolist() == [0, 2]


def test_maps_that_are_their_own_source(mi):
    rng = np.random.default_rng(77)
    for mb, dtype, layout, c in ((3, "uint8", "hwc", 3), (4, "uint8", "hwc", 4), (4, "float32", "chw", 1)):
        ids = gen_ids(rng, mb, 2, 7, 29)
        dst_ids = gen_ids(rng, mb, 2, 7, 29)
        as_batch = (lambda a: wide_maps(a, 3)) if mb == 3 else (lambda a: wide_maps(a, 4).view(np.uint8).reshape(2, 7, 29, 4)) if c == 4 else \
            (lambda a: wide_maps(a, 4).view(np.float32).reshape(2, 1, 7, 29))
        src, dst = as_batch(ids), as_batch(dst_ids)
        pieces = [(0, 1, 2, 1, 0, 0, 25, 6, [POOL[mb][1], POOL[mb][6]]), (1, 0, 0, 0, 3, 1, 20, 5, [POOL[mb][0], POOL[mb][2]])]
        got = mi.paste32_reference(src, src, dst, pieces, layout, dtype)
        want_ids = dst_ids.copy()
        for d, s, dx, dy, sx, sy, w, h, sel in pieces:
            region = ids[s, sy:sy + h, sx:sx + w]
            want_ids[d, dy:dy + h, dx:dx + w] = np.where(np.isin(region, sel), region, want_ids[d, dy:dy + h, dx:dx + w])
        assert same_bits(got, as_batch(want_ids)) and not np.array_equal(want_ids, dst_ids)


@pytest.mark.parametrize("dtype,layout", [("uint8", "hwc"), ("float16", "chw")])
def test_the_same_content_through_the_widths_1_2_3_and_4(mi, dtype, layout):
    """ids below 256: paste_reference on bytes, paste16_reference on the same ids widened, paste32_reference on both wide widths"""
    rng = np.random.default_rng(9)
    c, n, ih, iw, oh, ow = 3, 2, 6, 37, 5, 41
    src, dst = gen_batch(dtype, n, c, ih, iw, layout, 1), gen_batch(dtype, n, c, oh, ow, layout, 2)
    mask = rng.integers(0, 8, size=(n, ih, iw), dtype=np.uint8)
    recs = [(0, 1, 0, 0, 3, 0, 30, 5, [1, 2, 5]), (1, 0, 4, 1, 0, 2, 33, 4, [0, 7]), (0, 0, 10, 2, 5, 1, 9, 3, [3])]
    by_bytes = mi.paste_reference(src, mask, dst, recs, layout, dtype)
    assert same_bits(by_bytes, mi.paste16_reference(src, mask.astype(np.uint16), dst, recs, layout, dtype))
    for mb in WIDTHS:
        assert same_bits(by_bytes, mi.paste32_reference(src, at_offset(wide_maps(mask, mb), 16 - mb), dst, recs, layout, dtype)), mb
    assert same_bits(by_bytes, paste16_spec.apply(src, mask.astype(np.uint16), dst, recs, layout))


def test_pieces_plan_and_refusals(mi):
    recs = mi.paste_pieces32([(0, 0, 0, 0, 0, 0, 2, 2, [5, 6, 0x010005, 0xFFFFFF])], 3)
    assert len(recs) == 3 and [p.id_base for p in recs] == [5, 0x010005, 0xFFFFFF] and recs[0].ids[0] == 3 and recs[2].ids[0] == 1
    assert C.sizeof(mi.PastePiece32) == 76 and mi.PASTE_VALUE_PIXEL == 2
    for bad in (dict(records=[(0, 0, 0, 0, 0, 0, 2, 2, "nonzero")], map_bytes=3), dict(records=[(0, 0, 0, 0, 0, 0, 2, 2, [1 << 24])], map_bytes=3),
                dict(records=[(0, 0, 0, 0, 0, 0, 2, 2, [1 << 32])], map_bytes=4), dict(records=[(0, 0, 0, 0, 0, 0, 2, 2, [1])], map_bytes=2),
                dict(records=[(0, 0, 0, 0, 0, 0, 2, 2, [1], None, True)], map_bytes=3)):
        with pytest.raises(mi.LlcompError):
            mi.paste_pieces32(**bad)
    src, dst = gen_batch("uint8", 1, 3, 4, 6, "hwc", 1), gen_batch("uint8", 1, 3, 4, 6, "hwc", 2)
    maps3, maps4 = np.zeros((1, 4, 6, 3), np.uint8), np.zeros((1, 4, 6), np.uint32)
    ok = [(0, 0, 0, 0, 0, 0, 3, 2, [0])]
    assert not same_bits(mi.paste32_reference(src, maps3, dst, ok, "hwc"), dst) and not same_bits(mi.paste32_reference(src, maps4, dst, ok, "hwc"), dst)
    L = mi._lib.load()
    out = np.full(dst.nbytes, 0x5A, np.uint8)
    one = mi.paste_pieces32(ok, 3)

    def call(mb, mask_p, piece=None, c=3, dtype=mi.DTYPE_U8, layout=mi.LAYOUT_HWC):
        return L.llcomp_mi_paste32_reference(src.ctypes.data, mask_p, mb, 1, 6, 4, dst.ctypes.data, 1, 6, 4, c, dtype, layout, piece or one, 1, out.ctypes.data)

    raw = np.zeros(6 * 4 * 4 + 32, np.uint8)
    m = raw.ctypes.data + (-raw.ctypes.data) % 16
    assert call(3, m) == mi.OK and call(3, m + 1) == mi.OK and call(4, m) == mi.OK
    out[:] = 0x5A
    for mb in (0, 1, 2, 5):
        assert call(mb, m) == mi.BAD_ARGS
    for off in (1, 2, 3, 6):
        assert call(4, m + off) == mi.BAD_ARGS
    vp = mi.PASTE_VALUE | mi.PASTE_VALUE_PIXEL

    def piece(**kw):
        arr = mi.paste_pieces32(ok, 3)
        for k, v in kw.items():
            setattr(arr[0], k, v)
        return arr

    for p, kw in ((piece(id_base=1 << 24), {}), (piece(flags=4), {}), (piece(flags=mi.PASTE_VALUE_PIXEL), {}), (piece(value_bits=1), {}),
                  (piece(flags=vp, value_bits=0x04030201), {}), (piece(flags=vp, value_bits=1), dict(layout=mi.LAYOUT_CHW)),
                  (piece(flags=vp, value_bits=1), dict(c=5)), (piece(flags=mi.PASTE_VALUE, value_bits=0x100), {}), (piece(dst=1), {}), (piece(w=7), {})):
        assert call(3, m, p, **kw) == mi.BAD_ARGS
    assert (out == 0x5A).all()
    assert call(3, m, piece(flags=vp, value_bits=0x030201)) == mi.OK and call(4, m, piece(id_base=0xFFFFFFFF)) == mi.OK
    # the 8- and 16-bit calls go on refusing flag bits above bit 0
    p16 = mi.paste_pieces16(ok)
    p16[0].flags, p16[0].value_bits = vp, 1
    mask16 = np.zeros((1, 4, 6), np.uint16)
    assert L.llcomp_mi_paste16_reference(src.ctypes.data, mask16.ctypes.data, 1, 6, 4, dst.ctypes.data, 1, 6, 4, 3, mi.DTYPE_U8, mi.LAYOUT_HWC, p16, 1, out.ctypes.data) == mi.BAD_ARGS
    p8 = mi.paste_pieces(ok)
    p8[0].flags = vp
    assert L.llcomp_mi_paste_reference(src.ctypes.data, mask16.ctypes.data, 1, 6, 4, dst.ctypes.data, 1, 6, 4, 3, mi.DTYPE_U8, mi.LAYOUT_HWC, p8, 1, out.ctypes.data) == mi.BAD_ARGS
