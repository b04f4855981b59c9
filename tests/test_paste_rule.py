"""The rule of the batch copy-paste on the host (llcomp_mi_paste_reference; include/llcomp_mi.h: "Batch copy-paste") against
tests/paste_spec.py -- numpy's where per piece in list order -- bit for bit; all 256 bits against the composition under KEEP; a binary
mask against torch.where; VALUE pieces renumbering a map that is its own mask; the plan's CSR against a Python sort; the refusals."""
import ctypes as C

import numpy as np
import pytest

import paste_spec
from paste_spec import bits_of

DTYPES = ("uint8", "float32", "float16", "bfloat16")
ALL = list(range(256))


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


@pytest.mark.parametrize("c", (1, 3, 5))
@pytest.mark.parametrize("layout", ("chw", "hwc"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_is_the_spec(mi, dtype, layout, c):
    rng = np.random.default_rng(c * 100 + len(dtype) + len(layout))
    for rnd in range(12):
        n_src, n_dst = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        iw, ih, ow, oh = (int(rng.integers(1, 24)) for _ in range(4))
        pieces = paste_spec.random_pieces(rng, n_src, iw, ih, n_dst, ow, oh, int(rng.integers(0, 10)), dtype)
        src = paste_spec.gen_batch(dtype, n_src, c, ih, iw, layout, seed=rnd)
        mask = paste_spec.gen_mask(rng, n_src, ih, iw)
        dst = paste_spec.gen_batch(dtype, n_dst, c, oh, ow, layout, seed=100 + rnd)
        stats = []
        want = bits_of(paste_spec.apply(src, mask, dst, pieces, layout, dtype, stats))
        covered, selected = stats[0]
        if covered >= 1000:  # (the generator: uniform bytes over 8 ids against sets of 4 select half)
            assert 0.2 * covered <= selected <= 0.8 * covered, (covered, selected)
        got = mi.paste_reference(src, mask, dst, pieces, layout=layout, dtype=dtype)
        assert got.shape == dst.shape and got.dtype == dst.dtype
        assert np.array_equal(bits_of(got), want), (dtype, layout, c, rnd, pieces)
        # ... and with out == dst_in
        twice = dst.copy()
        recs = mi.paste_pieces(pieces)
        rc = mi._lib.load().llcomp_mi_paste_reference(src.ctypes.data, mask.ctypes.data, n_src, iw, ih, twice.ctypes.data, n_dst, ow, oh, c,
                                                      mi._dtype_code(dtype), mi._layout_code(layout), recs, len(recs), twice.ctypes.data)
        assert rc == mi.OK and np.array_equal(bits_of(twice), want), (dtype, layout, c, rnd, "in place")


def test_the_generator_selects_about_half():
    """the spec's own statistics on one large drawn call, so that the bound above is known to bite"""
    rng = np.random.default_rng(11)
    src = paste_spec.gen_batch("uint8", 2, 1, 60, 60, "chw", seed=1)
    mask = paste_spec.gen_mask(rng, 2, 60, 60)
    stats = []
    paste_spec.apply(src, mask, src.copy(), paste_spec.random_pieces(rng, 2, 60, 60, 2, 60, 60, 20, "uint8"), "chw", "uint8", stats)
    covered, selected = stats[0]
    assert covered >= 1000 and 0.2 * covered <= selected <= 0.8 * covered


@pytest.mark.parametrize("dtype,layout,c", [("float16", "chw", 3), ("uint8", "hwc", 3), ("float32", "hwc", 5), ("bfloat16", "chw", 1)])
def test_all_bits_is_the_composition_under_keep(mi, dtype, layout, c):
    import compose_spec

    rng = np.random.default_rng(c)
    src = paste_spec.gen_batch(dtype, 3, c, 17, 21, layout, seed=1)
    dst = paste_spec.gen_batch(dtype, 2, c, 23, 30, layout, seed=2)
    mask = rng.integers(0, 256, size=(3, 17, 21), dtype=np.uint8)
    rects = [p[:8] for p in compose_spec.random_pieces(rng, 3, 21, 17, 2, 30, 23, 10) if not p[8]]
    got = mi.paste_reference(src, mask, dst, [r + (ALL,) for r in rects], layout=layout, dtype=dtype)
    want = mi.compose_reference(src, dst, rects, layout=layout, keep=True, dtype=dtype)
    assert np.array_equal(bits_of(got), bits_of(want))
    # the empty set: dst unchanged
    same = mi.paste_reference(src, mask, dst, [r + ([],) for r in rects], layout=layout, dtype=dtype)
    assert np.array_equal(bits_of(same), bits_of(dst))


@pytest.mark.parametrize("dtype", ("float32", "uint8", "float16"))
def test_a_nonzero_piece_is_torch_where(mi, dtype):
    import torch

    rng = np.random.default_rng(4)
    n, c, h, w = 2, 3, 19, 33
    t = {"float32": torch.float32, "uint8": torch.uint8, "float16": torch.float16}[dtype]
    image = (torch.from_numpy(rng.integers(0, 256, size=(n, c, h, w)).astype(np.float32)) / (1 if dtype == "uint8" else 255)).to(t)
    paste = (torch.from_numpy(rng.integers(0, 256, size=(n, c, h, w)).astype(np.float32)) / (1 if dtype == "uint8" else 255)).to(t)
    mask = paste_spec.gen_mask(rng, n, h, w, ids=3)
    want = torch.where(torch.from_numpy(mask)[:, None] != 0, paste, image)
    got = mi.paste_reference(paste.numpy(), mask, image.numpy(), [(i, i, 0, 0, 0, 0, w, h, "nonzero") for i in range(n)])
    assert np.array_equal(bits_of(got), bits_of(want.numpy()))


def test_value_pieces_renumber_the_instances_of_a_map_that_is_its_own_mask(mi):
    rng = np.random.default_rng(6)
    maps = paste_spec.gen_mask(rng, 2, 20, 30, ids=5)[:, None]  # [n, 1, h, w]: c = 1 uint8, src and mask at once
    dst = paste_spec.gen_mask(rng, 2, 20, 30, ids=3)[:, None]
    # the instances 1..4 of map s land in dst map s as 11..14, inside a window; instance 0 is the background and stays out
    pieces = [(s, s, 4, 2, 1, 3, 22, 15, [m], 10 + m) for s in range(2) for m in range(1, 5)]
    got = mi.paste_reference(maps, maps, dst, pieces, dtype="uint8")
    want = dst.copy()
    for s in range(2):
        win = maps[s, 0, 3:18, 1:23]
        want[s, 0, 2:17, 4:26] = np.where(win != 0, win + 10, want[s, 0, 2:17, 4:26])
    assert np.array_equal(got, want)
    assert np.array_equal(got, paste_spec.apply(maps, maps[:, 0], dst, pieces, "chw", "uint8"))
    # ... and the class map itself, pasted: no VALUE
    got = mi.paste_reference(maps, maps, dst, [(0, 1, 0, 0, 0, 0, 30, 20, [2, 3])], dtype="uint8")
    assert np.array_equal(got[0, 0], np.where((maps[1, 0] == 2) | (maps[1, 0] == 3), maps[1, 0], dst[0, 0])) and np.array_equal(got[1], dst[1])


def test_plan_is_a_stable_sort_by_dst_without_the_ignored_pieces(mi):
    rng = np.random.default_rng(5)
    for rnd in range(20):
        n_dst = int(rng.integers(1, 9))
        pieces = paste_spec.random_pieces(rng, 2, 9, 9, n_dst, 300, 70, int(rng.integers(0, 30)), "uint8")
        pieces = [p[:8] + ([],) + p[9:] if i % 5 == 4 else p for i, p in enumerate(pieces)]  # some select nothing
        for dtype, layout, c, pixel_bytes in (("uint8", "chw", 3, 1), ("float32", "hwc", 3, 12)):
            pcs = [p[:9] for p in pieces] if dtype != "uint8" else pieces
            samples, first, order, wgs = mi.paste_plan(2, 9, 9, n_dst, 300, 70, c, pcs, dtype=dtype, layout=layout)
            live = [i for i, p in enumerate(pieces) if p[6] and p[7] and len(p[8])]
            assert order.tolist() == sorted(live, key=lambda i: pieces[i][0])  # (Python's sort is stable)
            want_samples = sorted({pieces[i][0] for i in live})
            assert samples.tolist() == want_samples
            assert first.tolist() == [sum(pieces[i][0] < d for i in live) for d in want_samples] + [len(live)]
            T, R = mi.compose_tile(), mi.compose_tile(pixel_bytes)
            assert wgs == len(want_samples) * (c if layout == "chw" else 1) * -(-300 // T) * -(-70 // R)


def test_refusals_leave_out_untouched(mi):
    L = mi._lib.load()
    n_src, n_dst, c, iw, ih, ow, oh = 2, 2, 3, 5, 4, 8, 6
    src = paste_spec.gen_batch("float32", n_src, c, ih, iw, "chw", seed=2)
    dst = paste_spec.gen_batch("float32", n_dst, c, oh, ow, "chw", seed=3)
    mask = paste_spec.gen_mask(np.random.default_rng(1), n_src, ih, iw)
    out = np.full(dst.shape, 7.0, np.float32)
    ok = [(1, 1, 2, 1, 1, 0, 4, 4, [1, 2, 3, 4]), (0, 0, 0, 0, 0, 0, 3, 3, "nonzero", 2.5)]

    def call(pieces=ok, src_p=src.ctypes.data, mask_p=mask.ctypes.data, n_src=n_src, iw=iw, ih=ih, dst_p=dst.ctypes.data, n_dst=n_dst, ow=ow, oh=oh,
             c=c, dtype=1, layout=1, out_p=out.ctypes.data, n_pieces=None, recs=0):
        recs = mi.paste_pieces(pieces) if recs == 0 else recs
        return L.llcomp_mi_paste_reference(src_p, mask_p, n_src, iw, ih, dst_p, n_dst, ow, oh, c, dtype, layout, recs,
                                           len(pieces) if n_pieces is None else n_pieces, out_p)

    A = [1]
    bad_pieces = [(2, 0, 0, 0, 0, 0, 1, 1, A), (0, 2, 0, 0, 0, 0, 1, 1, A), (0, 0, 5, 0, 0, 0, 4, 1, A), (0, 0, 0, 3, 0, 0, 1, 4, A),
                  (0, 0, 9, 0, 0, 0, 0, 0, A), (0, 0, 0, 0, 2, 0, 4, 1, A), (0, 0, 0, 0, 0, 1, 1, 4, A), (0, 0, 0, 0, 0, 0, 6, 1, A),
                  (0, 0, 0, 0, 6, 0, 0, 0, A), (0, 0, 0xFFFFFFFF, 0, 0, 0, 2, 1, A), (0, 0, 0, 0, 0, 0, 1, 1, A, float("inf")),
                  (0, 0, 0, 0, 0, 0, 1, 1, A, float("nan")), (0, 0, 0, 0, 0, 0, 1, 1, [], float("inf")), (0, 2, 0, 0, 0, 0, 0, 0, [])]
    for p in bad_pieces:
        assert call([ok[0], p]) == mi.BAD_ARGS, p
    for flags, value in ((2, 0.0), (3, 1.0), (0, 1.0), (0, float("nan")), (0x80000000, 0.0)):  # flag bits above bit 0; a value without VALUE
        recs = mi.paste_pieces(ok)
        recs[0].flags, recs[0].value = flags, value
        assert call(recs=recs) == mi.BAD_ARGS, (flags, value)
    for kw in (dict(src_p=None), dict(mask_p=None), dict(dst_p=None), dict(out_p=None), dict(recs=None), dict(n_dst=0), dict(n_dst=65536),
               dict(n_src=65536), dict(n_src=0), dict(ow=0), dict(oh=0), dict(c=0), dict(iw=0), dict(ih=0), dict(dtype=4), dict(layout=2),
               dict(n_pieces=(1 << 20) + 1), dict(src_p=src.ctypes.data + 2), dict(out_p=out.ctypes.data + 1),
               dict(src_p=out.ctypes.data + 4, n_src=1), dict(mask_p=out.ctypes.data + out.nbytes - 1), dict(mask_p=out.ctypes.data - 2 * 20 + 1),
               dict(ow=1 << 31, oh=1, pieces=[]), dict(layout=0, ow=1 << 30, c=3, oh=1, pieces=[]), dict(iw=1 << 31, ih=1, pieces=[]),
               dict(n_src=0, iw=0, ih=0, src_p=None, mask_p=None)):
        assert call(**kw) == mi.BAD_ARGS, kw
    for dtype, value in ((0, 2.5), (0, 256.0), (0, -1.0)):  # U8 takes integers 0..255
        assert call([(0, 0, 0, 0, 0, 0, 1, 1, A, value)], dtype=dtype) == mi.BAD_ARGS, value
    cap = mi.paste_max_pieces_per_sample()
    assert cap == 256
    assert call([ok[0]] * (cap + 1)) == mi.BAD_ARGS
    assert call([ok[0]] * cap + [(1, 0, 1, 1, 0, 0, 1, 1, [])]) == mi.BAD_ARGS  # a piece without an id bit counts: it has w and h
    assert (out == 7.0).all()
    assert call([ok[0]] * cap + [(1, 0, 8, 6, 0, 0, 0, 0, A)] + [(0, 0, 0, 0, 0, 0, 1, 1, A)]) == mi.OK  # empty ones do not count, nor another sample's
    assert call() == mi.OK
    assert np.array_equal(bits_of(out), bits_of(paste_spec.apply(src, mask, dst, ok, "chw", "float32")))
    assert call(pieces=[], n_src=0, iw=0, ih=0, src_p=None, mask_p=None) == mi.OK  # no piece: no src batch needed, out = dst_in
    assert np.array_equal(bits_of(out), bits_of(dst))
    for bad in ([(0, 0, 0)], [(0, 0, 0, 0, 0, 0, -1, 1, A)], [(0, 0, 0, 0, 0, 0, 1, 1, [256])], [(0, 0, 0, 0, 0, 0, 1, 1, "all")]):
        with pytest.raises(mi.LlcompError) as e:
            mi.paste_pieces(bad)
        assert e.value.status == mi.BAD_ARGS
    with pytest.raises(mi.LlcompError):
        mi.paste_reference(src, mask, dst[0], ok)  # not 4-D
    with pytest.raises(mi.LlcompError):
        mi.paste_reference(np.zeros(src.shape, np.float16), mask, dst, ok)  # two dtypes
    with pytest.raises(mi.LlcompError):
        mi.paste_reference(src, mask[:1], dst, ok)  # a mask of another shape
    with pytest.raises(mi.LlcompError):
        mi.paste_plan(2, 5, 4, 2, 8, 6, 3, [(2, 0, 0, 0, 0, 0, 1, 1, A)])
    recs = mi.paste_pieces([(1, 0, 2, 3, 4, 5, 6, 7, [0, 31, 32, 255], 1.5), (0, 1, 2, 3, 4, 5, 6, 7, "nonzero")])
    assert (recs[0].dst, recs[0].w, recs[0].h, recs[0].flags, recs[0].value, list(recs[0].ids)) == (1, 6, 7, 1, 1.5, [0x80000001, 1, 0, 0, 0, 0, 0, 1 << 31])
    assert (recs[1].flags, recs[1].value, list(recs[1].ids)) == (0, 0.0, [0xFFFFFFFE] + [0xFFFFFFFF] * 7)
    assert C.sizeof(recs) == 144 and mi.PASTE_VALUE == 1
