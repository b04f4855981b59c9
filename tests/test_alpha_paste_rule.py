"""The batch alpha paste without a GPU: the numpy statement of both rules (tests/alpha_paste_spec.py) and the library's reference
(llcomp_mi_alpha_paste_reference: llcomp_amd/csrc/alpha_rule.hpp through alpha_plan.cpp) against PIL where PIL imports, against recorded
PIL results (tests/golden/alpha_paste_pil.json) where it does not, and against torch's expression on the CPU for the float dtypes; the
painter's order, the refusals one by one, and the plan."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import alpha_paste_spec as spec
import device_domains as dom
from alpha_paste_spec import ALPHA_OVER, ALPHA_VALUE, ALPHA_VALUE_PIXEL
from conftest import GOLDEN


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


def colour_pairs():
    """256 (src, dst) RGB pairs that hold 0 and 255 in every position"""
    rng = np.random.default_rng(99)
    pairs = rng.integers(0, 256, (256, 2, 3), dtype=np.uint8)
    ext = np.array([[[0, 0, 0], [255, 255, 255]], [[255, 255, 255], [0, 0, 0]], [[0, 255, 0], [255, 0, 255]], [[255, 0, 255], [255, 255, 0]],
                    [[0, 0, 0], [0, 0, 0]], [[255, 255, 255], [255, 255, 255]], [[1, 254, 128], [127, 2, 253]], [[128, 127, 1], [254, 129, 126]]], np.uint8)
    pairs[:8] = ext
    return pairs


def over_domain():
    """every (sa, da) pair against the 256 colour pairs: src and dst [256, 65536, 4]"""
    pairs = colour_pairs()
    sa, da = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    src, dst = np.empty((256, 65536, 4), np.uint8), np.empty((256, 65536, 4), np.uint8)
    src[:, :, :3], dst[:, :, :3] = pairs[:, None, 0, :], pairs[:, None, 1, :]
    src[:, :, 3], dst[:, :, 3] = sa.reshape(-1)[None, :], da.reshape(-1)[None, :]
    return src, dst


def test_paste_with_an_l_mask_on_all_triples_as_pil(mi):
    Image = pytest.importorskip("PIL.Image")
    m, d, s = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    m, d, s = (np.ascontiguousarray(a.reshape(4096, 4096)) for a in (m, d, s))
    bg = Image.fromarray(d, "L")
    bg.paste(Image.fromarray(s, "L"), (0, 0), Image.fromarray(m, "L"))
    want = np.asarray(bg)
    assert np.array_equal(spec.paste_rule(d, s, m, "uint8").astype(np.uint8), want)
    got = mi.alpha_paste_reference(s[None, None], m[None], d[None, None], [(0, 0, 0, 0, 0, 0, 4096, 4096)])
    assert np.array_equal(got[0, 0], want)
    comp = np.asarray(Image.composite(Image.fromarray(s, "L"), Image.fromarray(d, "L"), Image.fromarray(m, "L")))
    assert np.array_equal(comp, want)


def test_rgb_under_l_rgba_under_its_own_a_and_a_colour_as_pil(mi):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    h, w = 37, 53
    matte = spec.gen_matte(rng, 1, h, w)
    src, dst = rng.integers(0, 256, (1, h, w, 3), dtype=np.uint8), rng.integers(0, 256, (1, 50, 70, 3), dtype=np.uint8)
    bg = Image.fromarray(dst[0], "RGB")
    bg.paste(Image.fromarray(src[0, 4:, 3:], "RGB"), (9, 2), Image.fromarray(matte[0, 4:, 3:], "L"))
    piece = [(0, 0, 9, 2, 3, 4, w - 3, h - 4)]
    want = np.asarray(bg)[None]
    assert np.array_equal(spec.apply(src, matte, dst, piece, "uint8", "hwc"), want)
    assert np.array_equal(mi.alpha_paste_reference(src, matte, dst, piece, layout="hwc"), want)
    # Image.composite: a whole sample under the matte
    same = rng.integers(0, 256, (1, h, w, 3), dtype=np.uint8)
    comp = np.asarray(Image.composite(Image.fromarray(src[0], "RGB"), Image.fromarray(same[0], "RGB"), Image.fromarray(matte[0], "L")))[None]
    assert np.array_equal(mi.alpha_paste_reference(src, matte, same, [(0, 0, 0, 0, 0, 0, w, h)], layout="hwc"), comp)
    # RGBA under its own A: the batch is its own alpha, 4 bytes per pixel, byte 3
    rgba, canvas = rng.integers(0, 256, (1, h, w, 4), dtype=np.uint8), rng.integers(0, 256, (1, h, w, 4), dtype=np.uint8)
    rgba[..., 3] = matte
    sprite = Image.fromarray(rgba[0], "RGBA")
    bg = Image.fromarray(canvas[0], "RGBA")
    bg.paste(sprite, (0, 0), sprite)
    want = np.asarray(bg)[None]
    piece = [(0, 0, 0, 0, 0, 0, w, h)]
    assert np.array_equal(spec.apply(rgba, rgba, canvas, piece, "uint8", "hwc", alpha_byte=3), want)
    assert np.array_equal(mi.alpha_paste_reference(rgba, rgba, canvas, piece, layout="hwc", alpha_byte=3), want)
    # a colour through a mask: VALUE_PIXEL
    bg = Image.fromarray(dst[0], "RGB")
    bg.paste((200, 17, 255), (5, 6, 5 + w, 6 + h), Image.fromarray(matte[0], "L"))
    piece = [(0, 0, 5, 6, 0, 0, w, h, ALPHA_VALUE | ALPHA_VALUE_PIXEL, 200 | 17 << 8 | 255 << 16)]
    want = np.asarray(bg)[None]
    assert np.array_equal(spec.apply(None, matte, dst, piece, "uint8", "hwc"), want)
    assert np.array_equal(mi.alpha_paste_reference(None, matte, dst, piece, layout="hwc"), want)


def test_alpha_composite_on_every_alpha_pair_as_pil(mi):
    Image = pytest.importorskip("PIL.Image")
    src, dst = over_domain()
    want = np.asarray(Image.alpha_composite(Image.fromarray(dst, "RGBA"), Image.fromarray(src, "RGBA")))
    assert np.array_equal(spec.over_rule(dst, src), want)
    got = mi.alpha_paste_reference(src[None], None, dst[None], [(0, 0, 0, 0, 0, 0, 65536, 256, ALPHA_OVER)], layout="hwc")
    assert np.array_equal(got[0], want)


def test_recorded_pil_results(mi):
    """tests/golden/alpha_paste_pil.json (tools/make_alpha_paste_golden.py): for machines without PIL"""
    with open(os.path.join(GOLDEN, "alpha_paste_pil.json")) as f:
        g = json.load(f)
    p = np.array(g["paste"], np.uint8)  # rows of m, d, s, out
    assert len(p) >= 200 and {0, 255} <= set(p[:, 0].tolist())
    assert np.array_equal(spec.paste_rule(p[:, 1], p[:, 2], p[:, 0], "uint8"), p[:, 3])
    n = len(p)
    got = mi.alpha_paste_reference(p[:, 2].reshape(1, 1, 1, n).copy(), p[:, 0].reshape(1, 1, n).copy(), p[:, 1].reshape(1, 1, 1, n).copy(), [(0, 0, 0, 0, 0, 0, n, 1)])
    assert np.array_equal(got.reshape(-1), p[:, 3])
    o = np.array(g["over"], np.uint8)  # rows of src rgba, dst rgba, out rgba
    assert len(o) >= 200
    assert np.array_equal(spec.over_rule(o[:, 4:8], o[:, 0:4]), o[:, 8:12])
    n = len(o)
    got = mi.alpha_paste_reference(o[:, 0:4].reshape(1, 1, n, 4).copy(), None, o[:, 4:8].reshape(1, 1, n, 4).copy(), [(0, 0, 0, 0, 0, 0, n, 1, ALPHA_OVER)], layout="hwc")
    assert np.array_equal(got.reshape(n, 4), o[:, 8:12])


def float_domain(dtype):
    """(d, s, m) bit patterns and alpha bytes: every own pattern of device_domains (all 65536 of a 16-bit dtype; every exponent of
    float32) x 16 witnesses (signed zeros, infinities, NaNs, subnormals, ties) x alphas; all 256 alphas against a seeded subset"""
    own = dom.own_bits(dtype).reshape(-1)
    wit = np.array(dom.PARTNERS[dtype], np.uint32)
    ms = np.array([0, 1, 2, 127, 128, 129, 253, 254, 255, 85, 170, 51], np.uint32)
    d, s, m = np.meshgrid(own[::1 if dtype == "float32" else 5], wit, ms, indexing="ij")
    sub = np.concatenate([wit, np.random.default_rng(8).choice(own, 240)])
    d2, s2, m2 = np.meshgrid(sub, sub[:64], np.arange(256, dtype=np.uint32), indexing="ij")
    return (np.concatenate([a.reshape(-1), b.reshape(-1)]) for a, b in ((d, d2), (s, s2), (m, m2)))


def torch_expression(d, s, m, dtype):
    """torch's (d * (1 - a) + s * a).to(dtype), a = alpha.float() / 255, on the CPU -> bits; a NaN as the dtype's quiet NaN"""
    import torch

    import mix_spec

    dt, st = mix_spec.from_bits(d, dtype), mix_spec.from_bits(s, dtype)
    a = torch.from_numpy(m.astype(np.uint8)).float() / 255
    out = mix_spec.bits((dt * (1 - a) + st * a).to(mix_spec.DTYPES[dtype])).astype(np.uint32)
    return np.where(dom.is_nan_bits(out, dtype), np.uint32(dom.QUIET_NAN[dtype]), out)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32"])
def test_float_rule_as_torch_on_the_cpu(mi, dtype):
    d, s, m = float_domain(dtype)
    want = torch_expression(d, s, m, dtype)
    ends = (m == 0) | (m == 255)  # the rule keeps or takes the bits there, whatever the other element is
    want = np.where(m == 0, d, np.where(m == 255, s, want))
    got = spec.paste_rule(d, s, m, dtype)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} differ"
    assert ends.any() and (~ends).sum() > 100000
    n = d.size
    t = spec.NP_NAME[dtype]
    bt = spec.BITS[np.dtype(t).itemsize]
    ref = mi.alpha_paste_reference(s.astype(bt).view(t).reshape(1, 1, 1, n), m.astype(np.uint8).reshape(1, 1, n), d.astype(bt).view(t).reshape(1, 1, 1, n),
                                   [(0, 0, 0, 0, 0, 0, n, 1)], dtype=dtype)
    assert np.array_equal(ref.view(bt).reshape(-1), want)


def test_painters_order_three_soft_pieces_as_sequential_pil_pastes(mi):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(11)
    src, matte = rng.integers(0, 256, (3, 20, 24, 3), dtype=np.uint8), spec.gen_matte(rng, 3, 20, 24)
    dst = rng.integers(0, 256, (1, 30, 40, 3), dtype=np.uint8)
    pieces = [(0, 0, 2, 3, 0, 0, 24, 20), (0, 1, 10, 8, 2, 1, 20, 18), (0, 2, 6, 0, 4, 4, 18, 16)]
    bg = Image.fromarray(dst[0], "RGB")
    for _, si, dx, dy, sx, sy, w, h in pieces:
        bg.paste(Image.fromarray(src[si, sy:sy + h, sx:sx + w], "RGB"), (dx, dy), Image.fromarray(matte[si, sy:sy + h, sx:sx + w], "L"))
    want = np.asarray(bg)[None]
    assert np.array_equal(spec.apply(src, matte, dst, pieces, "uint8", "hwc"), want)
    assert np.array_equal(mi.alpha_paste_reference(src, matte, dst, pieces, layout="hwc"), want)
    assert not np.array_equal(mi.alpha_paste_reference(src, matte, dst, pieces[::-1], layout="hwc"), want)


@pytest.mark.parametrize("dtype", ["uint8", "float16", "bfloat16", "float32"])
@pytest.mark.parametrize("layout", ["chw", "hwc"])
def test_reference_equals_the_spec_on_drawn_calls(mi, dtype, layout):
    from batch_support import bits_of, gen_batch

    rng = np.random.default_rng(3)
    for c, apx, ab in ((3, 1, 0), (4, 4, 3), (1, 2, 1), (2, 3, 0)):
        src, dst = gen_batch(dtype, 2, c, 9, 21, layout, 1), gen_batch(dtype, 2, c, 11, 19, layout, 2)
        matte = spec.gen_matte(rng, 2, 9, 21, apx, ab)
        pieces = spec.gen_pieces(rng, 9, 2, 21, 9, 2, 19, 11, dtype, layout, c, over=dtype == "uint8" and layout == "hwc" and c == 4)
        got = mi.alpha_paste_reference(src, matte, dst, pieces, layout=layout, dtype=dtype, alpha_byte=ab)
        assert np.array_equal(bits_of(got), bits_of(spec.apply(src, matte, dst, pieces, dtype, layout, ab)))


def test_refusals_one_by_one(mi):
    L = mi._lib.load()
    src, dst, alpha, out = (np.zeros(4096, np.uint8) for _ in range(4))  # (room for every shape below)
    U8, F32, HWC, CHW = 0, 1, 0, 1

    def call(piece, apx=1, ab=0, c=4, dtype=U8, layout=HWC, s=src.ctypes.data, a=alpha.ctypes.data, d=dst.ctypes.data, n=1, o=None):
        recs = mi.alpha_pieces([piece] * n)
        return L.llcomp_mi_alpha_paste_reference(s, a, apx, ab, 1, 6 if c == 4 else 24 // c, 4, d, 1, 6 if c == 4 else 24 // c, 4, c, dtype, layout, recs, len(recs), out.ctypes.data if o is None else o)

    ok = (0, 0, 0, 0, 0, 0, 3, 2)
    assert call(ok) == mi.OK and call(ok, 4, 3) == mi.OK and call(ok + (ALPHA_OVER,), a=None) == mi.OK and call(ok + (ALPHA_VALUE, 7), s=None) == mi.OK
    for apx, ab in ((0, 0), (5, 0), (1, 1), (4, 4), (2, 2)):
        assert call(ok, apx, ab) == mi.BAD_ARGS
    assert call(ok + (8,)) == mi.BAD_ARGS                                  # an unknown flag bit
    assert call(ok + (ALPHA_OVER | ALPHA_VALUE,)) == mi.BAD_ARGS           # OVER with VALUE
    assert call(ok + (ALPHA_OVER,), c=3) == mi.BAD_ARGS                    # OVER on c != 4
    assert call(ok + (ALPHA_OVER,), layout=CHW) == mi.BAD_ARGS
    assert call(ok + (ALPHA_OVER,), c=1, dtype=F32) == mi.BAD_ARGS
    assert call(ok + (ALPHA_OVER,), s=src.ctypes.data + 1) == mi.BAD_ARGS  # OVER off 4 bytes
    assert call(ok + (ALPHA_OVER,), o=out.ctypes.data + 2) == mi.BAD_ARGS
    assert call(ok + (ALPHA_VALUE_PIXEL,)) == mi.BAD_ARGS                  # VALUE_PIXEL without VALUE
    vp = ALPHA_VALUE | ALPHA_VALUE_PIXEL
    assert call(ok + (vp, 0x04030201)) == mi.OK and call(ok + (vp, 0x030201), c=3) == mi.OK
    assert call(ok + (vp, 0x04030201), c=3) == mi.BAD_ARGS                 # a byte at c
    assert call(ok + (vp, 1), layout=CHW) == mi.BAD_ARGS
    assert call(ok + (vp, 1), c=1, dtype=F32) == mi.BAD_ARGS
    assert call(ok + (vp, 1), c=6) == mi.BAD_ARGS
    assert call(ok + (ALPHA_VALUE, 0x100)) == mi.BAD_ARGS                  # bytes above the element
    assert call(ok + (ALPHA_VALUE, 0x10000), c=1, dtype=2) == mi.BAD_ARGS
    assert call(ok + (0, 1)) == mi.BAD_ARGS                                # value bits without VALUE
    assert call(ok, a=None) == mi.BAD_ARGS                                 # a NULL alpha that a piece needs
    assert call(ok, s=None) == mi.BAD_ARGS
    assert call(ok, d=None) == mi.BAD_ARGS and call(ok, o=0) == mi.BAD_ARGS
    for bad in ((1, 0, 0, 0, 0, 0, 3, 2), (0, 1, 0, 0, 0, 0, 3, 2), (0, 0, 4, 0, 0, 0, 3, 2), (0, 0, 0, 3, 0, 0, 3, 2), (0, 0, 0, 0, 4, 0, 3, 2),
                (0, 0, 0, 0, 0, 3, 3, 2), (0, 0, 0, 0, 0, 0, 7, 2)):
        assert call(bad) == mi.BAD_ARGS                                    # the paste calls' cases
    assert call(ok, dtype=9) == mi.BAD_ARGS and call(ok, layout=2) == mi.BAD_ARGS
    assert call(ok, s=out.ctypes.data) == mi.BAD_ARGS and call(ok, a=out.ctypes.data + 8) == mi.BAD_ARGS  # the written batch overlaps src, alpha
    assert call(ok, n=256) == mi.OK and call(ok, n=257) == mi.BAD_ARGS     # the cap per dst sample
    assert call((0, 0, 0, 0, 0, 0, 0, 2), n=300) == mi.OK                  # ... counts pieces with w and h only
    f32 = np.zeros(64, np.float32)
    assert call(ok, c=1, dtype=F32, s=f32.ctypes.data + 2) == mi.BAD_ARGS  # src off its element


def test_plan_csr_against_the_spec(mi):
    rng = np.random.default_rng(21)
    n_dst, ow, oh, c = 5, 300, 70, 3
    pieces = spec.gen_pieces(rng, 40, 3, 64, 48, n_dst, ow, oh, "uint8", "hwc", c)
    pieces[3] = pieces[3][:6] + (0, 5) + pieces[3][8:]  # ignored: no width
    pieces[17] = pieces[17][:7] + (0,) + pieces[17][8:]
    pieces = [p for p in pieces if p[0] != 2]            # a sample without pieces
    samples, first, order, nwg = mi.alpha_paste_plan(1, 0, 3, 64, 48, n_dst, ow, oh, c, pieces, dtype="uint8", layout="hwc")
    live = [(p[0], i) for i, p in enumerate(pieces) if p[6] and p[7]]
    want_samples = sorted({d for d, _ in live})
    assert samples.tolist() == want_samples and 2 not in want_samples
    assert order.tolist() == [i for d in want_samples for dd, i in live if dd == d]
    assert first.tolist() == [sum(1 for dd, _ in live if dd < d) for d in want_samples] + [len(live)]
    tile, rows = mi.compose_tile(), mi.compose_tile(c)
    assert nwg == len(want_samples) * -(-ow // tile) * -(-oh // rows)
    plain = [q[:8] for q in pieces]  # (the geometry alone: another dtype takes no VALUE_PIXEL)
    assert mi.alpha_paste_plan(1, 0, 3, 64, 48, n_dst, ow, oh, c, plain, dtype="float16", layout="chw")[3] == len(want_samples) * c * -(-ow // tile) * -(-oh // mi.compose_tile(2))
    with pytest.raises(mi.LlcompError):
        mi.alpha_paste_plan(5, 0, 3, 64, 48, n_dst, ow, oh, c, pieces, dtype="uint8", layout="hwc")
