"""The rule of the batch composition on the host (llcomp_mi_compose_reference; include/llcomp_mi.h: "Batch composition") against
tests/compose_spec.py -- numpy's slice assignments in list order -- bit for bit; the plan's CSR against a Python sort; grid_pieces and
mosaic_pieces against make_grid's and load_mosaic's expressions; the refusals."""
import ctypes as C

import numpy as np
import pytest

import compose_spec
from compose_spec import FILL, bits_of

DTYPES = ("uint8", "float32", "float16", "bfloat16")


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


def fill_for(dtype, c, rng):
    return [float(rng.integers(0, 256)) if dtype == "uint8" else float(rng.integers(-4000, 4000)) / 7.0 for _ in range(c)]


@pytest.mark.parametrize("c", (1, 3, 5))
@pytest.mark.parametrize("layout", ("chw", "hwc"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_is_the_spec(mi, dtype, layout, c):
    rng = np.random.default_rng(c * 100 + len(dtype) + len(layout))
    for rnd in range(12):
        n_src, n_dst = int(rng.integers(0, 4)) if rnd else 0, int(rng.integers(1, 4))
        iw, ih, ow, oh = (int(rng.integers(1, 20)) for _ in range(4))
        keep = bool(rnd % 2)
        pieces = compose_spec.random_pieces(rng, n_src, iw, ih, n_dst, ow, oh, int(rng.integers(0, 10)))
        src = compose_spec.gen_batch(dtype, n_src, c, ih, iw, layout, seed=rnd) if n_src else None
        dst = compose_spec.gen_batch(dtype, n_dst, c, oh, ow, layout, seed=100 + rnd)
        fill = None if rnd % 3 == 0 else fill_for(dtype, c, rng)
        want = bits_of(compose_spec.apply(src, dst, pieces, layout, dtype, fill, keep))
        got = mi.compose_reference(src, dst, pieces, layout=layout, fill=fill, keep=keep, dtype=dtype)
        assert got.shape == dst.shape and got.dtype == dst.dtype
        assert np.array_equal(bits_of(got), want), (dtype, layout, c, rnd, pieces)
        # ... and with out == dst_in
        twice = dst.copy()
        recs = mi.compose_pieces(pieces)
        fv = (C.c_float * c)(*fill) if fill else None
        rc = mi._lib.load().llcomp_mi_compose_reference(src.ctypes.data if n_src else None, n_src, iw, ih, twice.ctypes.data, n_dst, ow, oh, c,
                                                        mi._dtype_code(dtype), mi._layout_code(layout), recs, len(recs), fv, int(keep), twice.ctypes.data)
        assert rc == mi.OK and np.array_equal(bits_of(twice), want), (dtype, layout, c, rnd, "in place")


def test_painters_order_hidden_and_empty_pieces(mi):
    src = compose_spec.gen_batch("float32", 3, 1, 4, 4, "chw", seed=1)
    dst = compose_spec.gen_batch("float32", 2, 1, 6, 6, "chw", seed=2)
    pieces = [(0, 0, 0, 0, 0, 0, 4, 4), (0, 1, 1, 1, 0, 0, 4, 4), (0, 2, 2, 2, 0, 0, 4, 4),  # three overlapping, the later winning
              (1, 0, 1, 1, 1, 1, 2, 2), (1, 1, 0, 0, 0, 0, 4, 4),                            # the first hidden entirely
              (1, 2, 6, 6, 4, 4, 0, 0), (1, 0, 0, 0, 0, 0, 0, 3, FILL)]                      # empty ones, at the far corner too
    got = mi.compose_reference(src, dst, pieces, fill=[2.5])
    assert np.array_equal(bits_of(got), bits_of(compose_spec.apply(src, dst, pieces, "chw", "float32", [2.5])))
    assert bits_of(got)[0, 0, 0, 0] == bits_of(src)[0, 0, 0, 0] and bits_of(got)[0, 0, 1, 1] == bits_of(src)[1, 0, 0, 0]
    assert bits_of(got)[0, 0, 2, 2] == bits_of(src)[2, 0, 0, 0] and got[0, 0, 0, 5] == 2.5
    assert np.array_equal(bits_of(got)[1, 0, :4, :4], bits_of(src)[1, 0])
    same = mi.compose_reference(src, dst, [], keep=True)
    assert np.array_equal(bits_of(same), bits_of(dst))


def test_plan_is_a_stable_sort_by_dst(mi):
    rng = np.random.default_rng(5)
    for rnd in range(20):
        n_dst = int(rng.integers(1, 9))
        pieces = compose_spec.random_pieces(rng, 2, 9, 9, n_dst, 300, 70, int(rng.integers(0, 30)))
        for keep in (False, True):
            for dtype, layout, c, pixel_bytes in (("uint8", "chw", 3, 1), ("float32", "hwc", 3, 12)):
                samples, first, order, wgs = mi.compose_plan(2, 9, 9, n_dst, 300, 70, c, pieces, dtype=dtype, layout=layout, keep=keep)
                live = [i for i, p in enumerate(pieces) if p[6] and p[7]]
                by_dst = sorted(live, key=lambda i: pieces[i][0])  # (Python's sort is stable)
                assert order.tolist() == by_dst
                want_samples = sorted({pieces[i][0] for i in live}) if keep else list(range(n_dst))
                assert samples.tolist() == want_samples
                assert first.tolist() == [sum(pieces[i][0] < d for i in live) for d in want_samples] + [len(live)]
                T, R = mi.compose_tile(), mi.compose_tile(pixel_bytes)
                assert wgs == len(want_samples) * (c if layout == "chw" else 1) * -(-300 // T) * -(-70 // R)
    assert mi.compose_tile() == 128 and [mi.compose_tile(g) for g in (1, 2, 3, 4, 6, 12, 20)] == [64, 64, 32, 32, 16, 8, 4]


def test_grid_pieces_are_make_grid(mi):
    for n, iw, ih, nrow, padding in ((1, 5, 4, 8, 2), (5, 4, 3, 2, 1), (8, 3, 3, 8, 2), (9, 3, 2, 4, 0), (7, 2, 5, 3, 3)):
        batch = compose_spec.gen_batch("float32", n, 3, ih, iw, "chw", seed=n)
        pieces, ow, oh = mi.grid_pieces(n, iw, ih, nrow=nrow, padding=padding)
        want = compose_spec.make_grid(batch, nrow, padding, 0.5)
        assert want.shape == (3, oh, ow)
        got = mi.compose_reference(batch, np.zeros((1, 3, oh, ow), np.float32), pieces, fill=0.5)
        assert np.array_equal(bits_of(got[0]), bits_of(want)), (n, iw, ih, nrow, padding)


def test_mosaic_pieces_are_load_mosaic(mi):
    rng = np.random.default_rng(8)
    s, iw, ih = 16, 16, 12
    centres = [(8, 8), (24, 24), (16, 16), (0, 0), (32, 32), (5, 30)] + [(int(rng.integers(8, 25)), int(rng.integers(8, 25))) for _ in range(6)]
    src = compose_spec.gen_batch("uint8", 4 * len(centres), 3, ih, iw, "hwc", seed=3)
    pieces = mi.mosaic_pieces(centres, iw, ih, s)
    got = mi.compose_reference(src, np.zeros((len(centres), 2 * s, 2 * s, 3), np.uint8), pieces, layout="hwc", fill=114)
    for i, (xc, yc) in enumerate(centres):
        assert np.array_equal(got[i], compose_spec.mosaic([src[4 * i + k] for k in range(4)], xc, yc, s)), (xc, yc)


def test_refusals_leave_out_untouched(mi):
    L = mi._lib.load()
    n_src, n_dst, c, iw, ih, ow, oh = 2, 2, 3, 5, 4, 8, 6
    src = compose_spec.gen_batch("float32", n_src, c, ih, iw, "chw", seed=2)
    dst = compose_spec.gen_batch("float32", n_dst, c, oh, ow, "chw", seed=3)
    out = np.full(dst.shape, 7.0, np.float32)
    ok = [(1, 1, 2, 1, 1, 0, 4, 4), (0, 0, 0, 0, 0, 0, 3, 3, FILL)]

    def call(pieces=ok, src_p=src.ctypes.data, n_src=n_src, iw=iw, ih=ih, dst_p=dst.ctypes.data, n_dst=n_dst, ow=ow, oh=oh, c=c, dtype=1, layout=1,
             fill=None, flags=0, out_p=out.ctypes.data, n_pieces=None, recs=0):
        recs = mi.compose_pieces(pieces) if recs == 0 else recs
        fv = (C.c_float * len(fill))(*fill) if fill is not None else None
        return L.llcomp_mi_compose_reference(src_p, n_src, iw, ih, dst_p, n_dst, ow, oh, c, dtype, layout, recs, len(pieces) if n_pieces is None else n_pieces,
                                             fv, flags, out_p)

    bad_pieces = [(2, 0, 0, 0, 0, 0, 1, 1), (0, 2, 0, 0, 0, 0, 1, 1), (0, 0, 5, 0, 0, 0, 4, 1), (0, 0, 0, 3, 0, 0, 1, 4), (0, 0, 9, 0, 0, 0, 0, 0),
                  (0, 0, 0, 0, 2, 0, 4, 1), (0, 0, 0, 0, 0, 1, 1, 4), (0, 0, 0, 0, 0, 0, 6, 1), (0, 0, 0, 0, 0, 0, 1, 1, 2), (0, 0, 0, 0, 0, 0, 1, 1, 3),
                  (0, 1, 0, 0, 0, 0, 1, 1, FILL), (0, 0, 0, 0, 1, 0, 1, 1, FILL), (0, 0, 0, 0, 0, 1, 1, 1, FILL), (0, 0, 0xFFFFFFFF, 0, 0, 0, 2, 1)]
    for p in bad_pieces:
        assert call([ok[0], p]) == mi.BAD_ARGS, p
    reserved = mi.compose_pieces(ok)
    reserved[1].reserved = 1
    assert call(recs=reserved) == mi.BAD_ARGS
    for kw in (dict(src_p=None), dict(dst_p=None, flags=1), dict(out_p=None), dict(recs=None), dict(n_dst=0), dict(n_dst=65536), dict(n_src=65536),
               dict(n_src=0), dict(ow=0), dict(oh=0), dict(c=0), dict(iw=0), dict(ih=0), dict(dtype=4), dict(layout=2), dict(flags=2), dict(n_pieces=(1 << 20) + 1),
               dict(fill=[0.0, float("inf"), 0.0]), dict(fill=[float("nan"), 0.0, 0.0]), dict(src_p=src.ctypes.data + 2), dict(out_p=out.ctypes.data + 1),
               dict(src_p=out.ctypes.data + 4, n_src=1), dict(ow=1 << 31, oh=1, pieces=[]), dict(layout=0, ow=1 << 30, c=3, oh=1, pieces=[])):
        assert call(**kw) == mi.BAD_ARGS, kw
    assert call(dtype=0, fill=[1.0, 2.5, 3.0]) == mi.BAD_ARGS and call(dtype=0, fill=[1.0, 256.0, 3.0]) == mi.BAD_ARGS and call(dtype=0, fill=[-1.0, 0.0, 0.0]) == mi.BAD_ARGS
    cap = mi.compose_max_pieces_per_sample()
    assert cap >= 1024
    assert call([ok[0]] * (cap + 1)) == mi.BAD_ARGS
    assert (out == 7.0).all()
    assert call([ok[0]] * cap + [(1, 0, 8, 6, 0, 0, 0, 0)] + [(0, 0, 0, 0, 0, 0, 1, 1)]) == mi.OK  # empty ones do not count, nor another sample's
    assert call(dst_p=None) == mi.OK  # dst_in is not read without KEEP
    assert np.array_equal(bits_of(out), bits_of(compose_spec.apply(src, dst, ok, "chw", "float32")))
    assert call(pieces=[ok[1]], src_p=None, n_src=0, iw=0, ih=0, flags=1) == mi.OK  # no src: FILL pieces only
    assert np.array_equal(bits_of(out), bits_of(compose_spec.apply(None, dst, [ok[1]], "chw", "float32", keep=True)))
    for bad in ([(0, 0, 0)], [dict(dst=0, width=3)], [(0, 0, 0, 0, 0, 0, -1, 1)]):
        with pytest.raises(mi.LlcompError) as e:
            mi.compose_pieces(bad)
        assert e.value.status == mi.BAD_ARGS
    with pytest.raises(mi.LlcompError):
        mi.compose_reference(src, dst[0], ok)  # not 4-D
    with pytest.raises(mi.LlcompError):
        mi.compose_reference(np.zeros(src.shape, np.float16), dst, ok)  # two dtypes
    with pytest.raises(mi.LlcompError):
        mi.compose_plan(2, 5, 4, 2, 8, 6, 3, [(2, 0, 0, 0, 0, 0, 1, 1)])
    recs = mi.compose_pieces([dict(dst=1, w=2, h=3, flags=FILL), (0, 1, 2, 3, 4, 5, 6, 7)])
    assert (recs[0].dst, recs[0].src, recs[0].w, recs[0].h, recs[0].flags, recs[1].sy, recs[1].h, recs[1].flags) == (1, 0, 2, 3, 1, 5, 7, 0)
    assert C.sizeof(recs) == 80 and mi.COMPOSE_FILL == 1 and mi.COMPOSE_KEEP == 1
