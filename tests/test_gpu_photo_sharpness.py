"""ADJUST_SHARPNESS in the photometric chains on the GPU (include/llcomp_mi.h: "Photometric chains"; k_photo_sharp_save and k_photo_sharp,
llcomp_amd/csrc/photo_kernels.hip).  The way of checking is tests/photo_gpu.py's: the expected bytes of a view are
tests/photo_spec.py -- the rule restated with numpy in integers, itself pinned to PIL by tests/test_photo_sharpness_rule.py --
applied to what the existing call writes for the same view as U8 HWC, then llcomp_mi_output_table for a formatted group, bit for bit.

The kernel's thresholds, each with a shape on either side beside the issue's shapes:
  rows per band, 16 (kSharpBandRows): (20, 16) is one band, (20, 17) two with a last band of one row, (20, 33) three -- a middle band
    reads a saved row on both sides;
  a row's bytes in the LDS ring, 12288 (kSharpRowBytes): ow = 12288 / c is the last whole row in the ring, ow = 12288 / c + 1 the first
    in two column pieces (the second of c bytes), ow = 24576 / c + 8 three pieces; the two piece shapes have 18 and 17 rows, so that
    pieces meet bands;
  dword loads against head and tail bytes: rows of 3 bytes -- (3, 3) on one channel, (1, 1) on three -- have no whole dword at any
    address; (7, 5) has rows whose addresses take every value mod 4, (8, 5) with c = 1 rows that are whole dwords.
kSharpKeepRows (4096 rows of a band whose rows lie in pieces) is the planner's cap, not a path of the kernel: a view with that many rows
of more than 12288 bytes is 50 MB, and tests/helpers/photo_sharp_check.cpp checks the cap on the host."""
import numpy as np
import pytest

import resize_filters_spec as spec
from photo_gpu import FRAMES, GEOS, PG, W, check, close_shared_codecs, flag, mi, run, setup, views_of  # noqa: F401  (mi: the fixture)
from test_gpu_regions_host import make_batch, stream
from test_gpu_resized_output import TOut, same_bits
from test_gpu_resized_regions import packed

pytestmark = pytest.mark.gpu

FACTORS = [0.0, 0.5, 1.0, 1.7, 2.0, 8.0]
# ("ring", oh) / ("two", oh) / ("three", oh): the widths at the ring's threshold, which depend on the channel count
SHAPES = [(1, 1), (2, 3), (3, 2), (3, 3), (4, 3), (20, 12), (70, 33), (300, 5), (5, 300), (20, 16), (20, 17), (7, 5), (8, 5), ("ring", 4),
          ("two", 18), ("three", 17)]
S = ("adjust_sharpness", 1.6)
EIGHT_FIRST = [S, ("brightness", 1.2), ("contrast", 1.5), ("adjust_hue", -0.2), ("equalize", None), ("solarize", 140), ("color", 0.3), ("invert", None)]
EIGHT_MID = EIGHT_FIRST[1:4] + [("adjust_sharpness", 0.4)] + EIGHT_FIRST[4:]
EIGHT_LAST = EIGHT_FIRST[1:5] + [("gaussian_blur", 0.8)] + EIGHT_FIRST[6:] + [("adjust_sharpness", 3.5)]
WARPS = [(0, 0.9, 0.2, 3.0, -0.2, 0.9, 1.0, flag(spec.BILINEAR)), (2, 1.1, -0.3, 20.0, 0.1, 0.5, 0.5, flag(spec.BILINEAR, True)),
         (2, 0.7, 0.0, 5.25, 0.0, 0.4, 0.5, flag(spec.NEAREST))]
PADDED = [(0, -10, -5, 60, 30, flag(spec.BILINEAR)), (2, 70, 30, 40, 20, flag(spec.BICUBIC, True)), (2, 10, 5, 30, 20, flag(spec.BOX))]


def shape_of(shape, c):
    ow, oh = shape
    return ({"ring": 12288 // c, "two": 12288 // c + 1, "three": 24576 // c + 8}.get(ow, ow), oh)


@pytest.mark.parametrize("shape", SHAPES, ids=["%sx%d" % s for s in SHAPES])
@pytest.mark.parametrize("name", list(GEOS))
def test_one_op_per_factor(mi, orc, name, shape):
    """one group, view i with the factor FACTORS[i] (two views mirrored): the op alone -- the chain's last step, which writes the
    output -- and followed by invert, in place; a factor of 1 is the plain output, and sides below 3 are"""
    c, h, imgs, conts, dev, codec = setup(mi, orc, name)
    ow, oh = shape_of(shape, c)
    vs = views_of(h, small=(ow, oh) == (1, 1))
    views = [vs[i % len(vs)] for i in range(len(FACTORS))]
    outs, plain = check(mi, codec, [PG(views, ow, oh, photo=[[("adjust_sharpness", a)] for a in FACTORS])], c, dev)
    assert same_bits(outs[0][2], plain[0][2])  # a = 1
    if ow < 3 or oh < 3:
        assert same_bits(outs[0], plain[0])
    elif (ow, oh) == (70, 33):
        assert not same_bits(outs[0][3], plain[0][3])
    check(mi, codec, [PG(views, ow, oh, photo=[[("adjust_sharpness", a), "invert"] for a in FACTORS])], c, dev)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("kind", ["views", "padded", "warped"])
@pytest.mark.parametrize("name", list(GEOS))
def test_eight_op_chains(mi, orc, name, kind, host):
    """eight ops with the sharpness first, in the middle and last (there behind a blur), one chain per group: u8 HWC, float16 CHW and
    float32 HWC; views, padded views and warped views; mirrored views in every group"""
    c, h, imgs, conts, dev, codec = setup(mi, orc, name)
    warp = kind == "warped"
    vs = WARPS if warp else PADDED if kind == "padded" and h == 44 else views_of(h)[:3]
    fill = dict(warp=True, fill=[200, 30, 90][:c]) if warp else {}
    groups = [PG(vs, 70, 33, photo=EIGHT_MID, **fill), PG(vs, 20, 17, photo=EIGHT_FIRST, dtype="float16", layout="chw", **fill),
              PG(vs, 20, 12, photo=EIGHT_MID, dtype="float32", layout="hwc", **fill), PG(vs, 70, 33, photo=EIGHT_LAST, dtype="float16", layout="chw", **fill),
              PG(vs, 20, 17, photo=EIGHT_LAST, **fill)]
    check(mi, codec, groups, c, dev, pad_mode="edge" if kind == "padded" else None, conts=list(conts) if host else None)


def test_every_kind_of_op_at_one_step(mi, orc):
    """one group whose views have, at step 1, the sharpness, the blur, a table, color, hue and nothing (an ended chain)"""
    c, h, imgs, conts, dev, codec = setup(mi, orc, "100x44_32x16i_c3")
    vs = views_of(h) + views_of(h)[:1]
    first = ("brightness", 1.1)
    mixed = [[first, ("adjust_sharpness", 1.8), "invert"], [first, ("gaussian_blur", 1.5), "invert"], [first, ("solarize", 100), "invert"],
             [first, ("color", 1.6), "invert"], [first, ("adjust_hue", 0.3), "invert"], [first]]
    check(mi, codec, [PG(vs, 70, 33, photo=mixed, dtype="float16", layout="chw"), PG(vs, 20, 12, photo=mixed)], c, dev)
    ends = [[first, ("adjust_sharpness", 0.2)], [first, ("gaussian_blur", 1.5)], [first, "invert"], [first, ("contrast", 1.4), S], [S], []]
    check(mi, codec, [PG(vs, 70, 33, photo=ends), PG(vs, 20, 17, photo=ends, dtype="float32", layout="chw")], c, dev)


def test_chunks_and_the_memory_bound(mi, orc):
    """40 views of 100 x 44 with the op in mid-chain: more than the staging bound holds, the less so with the rows between their bands
    saved beside them; the same group in two calls; then a codec of ONE frame and one view of the frame's size, which fills the
    staging bound by itself and is one band with nothing saved"""
    c, h, tw, th, planar = GEOS["100x44_32x16i_c3"]
    _, _, imgs, conts, dev, _ = setup(mi, orc, "100x44_32x16i_c3")
    chain = [("brightness", 1.3), ("contrast", 0.7), ("adjust_sharpness", 1.9), ("adjust_hue", 0.1), "equalize"]
    codec = mi.Codec(FRAMES, W, h, c, tw, th, planar, device=0)
    try:
        vs = views_of(h)
        many = [vs[i % len(vs)] for i in range(40)]
        groups = [PG(many, 100, 44, photo=chain), PG(vs, 20, 12, photo=EIGHT_LAST, dtype="float32", layout="chw")]
        outs, _ = check(mi, codec, groups, c, dev)
        check(mi, codec, groups, c, dev, pad_mode="edge")
        wviews = [(v[0], 1.0, 0.1, float(v[1]), -0.1, 1.0, float(v[2]), flag(spec.BILINEAR)) for v in many]
        check(mi, codec, [PG(wviews, 100, 44, photo=chain[:3], warp=True)], c, dev)
        run(mi, codec, groups, c, conts=list(conts))
        assert codec.allocated_bytes() <= codec.photo_workspace_bytes(45)
        st_a, a = run(mi, codec, [PG(many[:23], 100, 44, photo=chain)], c, dev=dev)  # (23 and 17: neither a multiple of the chunk)
        st_b, b = run(mi, codec, [PG(many[23:], 100, 44, photo=chain)], c, dev=dev)
        assert st_a == st_b == 0 and same_bits(np.concatenate([a[0], b[0]]), outs[0])
        assert codec.allocated_bytes() <= codec.photo_workspace_bytes(45)
    finally:
        codec.close()
    one_imgs, one_conts = make_batch(orc, 1, W, h, c, tw, th, planar)
    one_dev = packed(mi, one_conts)
    codec = mi.Codec(1, W, h, c, tw, th, planar, device=0)
    try:
        whole = [(0, 0, 0, W, h, flag(spec.NEAREST))]
        outs, plain = check(mi, codec, [PG(whole, W, h, photo=chain)], c, one_dev)
        assert np.array_equal(plain[0][0], one_imgs[0]) and not same_bits(outs[0], plain[0])
        check(mi, codec, [PG(whole, W, h, photo=chain)], c, one_dev, conts=list(one_conts))
        assert codec.allocated_bytes() <= codec.photo_workspace_bytes(1)
    finally:
        codec.close()


def test_a_group_without_chains_beside_a_group_that_sharpens(mi, orc):
    c, h, imgs, conts, dev, codec = setup(mi, orc, "100x44_32x16i_c3")
    vs = views_of(h)
    groups = [PG(vs, 20, 12, dtype="float16", layout="chw"), PG(vs, 70, 33, photo=[S])]
    outs, plain = check(mi, codec, groups, c, dev)
    st, alone = run(mi, codec, groups[:1], c, dev=dev)  # the extended call: the group by itself, no photo= anywhere
    assert st == 0 and same_bits(outs[0], alone[0])


def test_a_bad_factor_leaves_output_and_status_untouched(mi, orc):
    c, h, imgs, conts, dev, codec = setup(mi, orc, "100x44_32x16i_c3")
    vs = views_of(h)[:2]
    for p in (-1e-3, 256.5, float("nan"), float("inf"), -float("inf")):
        for host in (False, True):
            o = TOut(len(vs), 20, 12, c, "uint8", "hwc", status=0x77)
            g = [mi.ViewGroup(vs, 20, 12, o.ptr, photo=[[("adjust_sharpness", 1.0)], [("invert", None), ("adjust_sharpness", p)]])]
            with pytest.raises(mi.LlcompError) as e:
                if host:
                    codec.decode_views_host(conts, g, o.st.data_ptr(), stream())
                else:
                    codec.decode_views(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), g, o.st.data_ptr(), stream())
            assert e.value.status == mi.BAD_ARGS, p
            st, out = o.read()
            assert st == 0x77 and (out == 0x5A).all(), p
    check(mi, codec, [PG(vs, 20, 12, photo=[[("adjust_sharpness", 0.0)], [("adjust_sharpness", 256.0)]])], c, dev)  # (the ends are taken)


def test_close_shared_codecs():
    close_shared_codecs()
