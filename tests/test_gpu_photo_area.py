"""GAUSSIAN_BLUR and ADJUST_HUE in the photometric chains on the GPU (include/llcomp_mi.h: "Photometric chains"; the row and column
kernels of the blur and the hue op of the per-pixel pass, llcomp_amd/csrc/photo_kernels.hip).  The way of checking is
tests/photo_gpu.py's: the expected bytes of a view are tests/photo_spec.py -- both rules restated with numpy, themselves pinned to PIL by
tests/test_photo_area_rule.py -- applied to what the existing call writes for the same view as U8 HWC, then llcomp_mi_output_table for
a formatted group, bit for bit.

The blur's kernels hold at most 256 samples of a line in LDS and do a longer line in pieces of 58 outputs with up to 99 samples of halo
to each side (3 * (r + 1), r <= 32); the column kernel takes strips of 32 byte columns, the row kernel 1024 / min(ow, 256) rows per
workgroup.  So beside the issue's shapes -- 300 crosses five piece boundaries with a tail of 10, and at radius 32 the halo is cut at both
ends of the line -- the shapes 256 and 257 stand on both sides of the threshold between a whole line and pieces, in each direction."""
import ctypes as C

import pytest

import resize_filters_spec as spec
from photo_gpu import FRAMES, GEOS, PG, W, check, close_shared_codecs, flag, mi, run, setup, views_of  # noqa: F401  (mi: the fixture)
from test_gpu_regions_host import stream
from test_gpu_resized_output import TOut, same_bits

pytestmark = pytest.mark.gpu

RADII = [0.0, 0.1, 1.0, 2.0, 32.0]
BLUR_SHAPES = [(1, 1), (2, 3), (20, 12), (70, 33), (300, 5), (5, 300), (256, 2), (257, 2), (2, 256), (2, 257)]
HUES = [0.1, -0.5, 0.5, 1 / 255]
DINO = [("brightness", 1.3), ("contrast", 0.7), ("color", 1.2), ("adjust_hue", 0.07), ("grayscale", None), ("gaussian_blur", 1.0)]
EIGHT_FIRST = [("gaussian_blur", 2.0), ("brightness", 1.2), ("contrast", 1.5), ("adjust_hue", -0.2), ("equalize", None), ("solarize", 140),
               ("color", 0.3), ("invert", None)]
EIGHT_MID = EIGHT_FIRST[1:4] + [("gaussian_blur", 0.6)] + EIGHT_FIRST[4:]
EIGHT_LAST = EIGHT_FIRST[1:] + [("gaussian_blur", 5.5)]
WARPS = [(0, 0.9, 0.2, 3.0, -0.2, 0.9, 1.0, flag(spec.BILINEAR)), (2, 1.1, -0.3, 20.0, 0.1, 0.5, 0.5, flag(spec.BILINEAR, True)),
         (2, 0.7, 0.0, 5.25, 0.0, 0.4, 0.5, flag(spec.NEAREST))]
PADDED = [(0, -10, -5, 60, 30, flag(spec.BILINEAR)), (2, 70, 30, 40, 20, flag(spec.BICUBIC, True)), (2, 10, 5, 30, 20, flag(spec.BOX))]


@pytest.mark.parametrize("shape", BLUR_SHAPES, ids=["%dx%d" % s for s in BLUR_SHAPES])
@pytest.mark.parametrize("name", list(GEOS))
def test_a_single_blur_per_radius(mi, orc, name, shape):
    """one group, view i with the radius RADII[i] (two views mirrored): a line shorter than the window, several strips and pieces in
    each direction with a tail in each; in place (a second op behind it) and as the chain's last op"""
    c, h, imgs, conts, dev, codec = setup(mi, orc, name)
    vs = views_of(h, small=shape == (1, 1))
    views = [vs[i % len(vs)] for i in range(len(RADII))]
    outs, plain = check(mi, codec, [PG(views, *shape, photo=[[("gaussian_blur", r)] for r in RADII])], c, dev)
    assert same_bits(outs[0][0], plain[0][0])  # radius 0
    check(mi, codec, [PG(views, *shape, photo=[[("gaussian_blur", r), "invert"] for r in RADII])], c, dev)


@pytest.mark.parametrize("name", list(GEOS))
def test_a_single_hue_per_factor(mi, orc, name):
    c, h, imgs, conts, dev, codec = setup(mi, orc, name)
    vs = views_of(h)
    for shape in ((20, 12), (70, 33)):
        outs, plain = check(mi, codec, [PG(vs[:len(HUES)], *shape, photo=[[("adjust_hue", f)] for f in HUES])], c, dev)
        if c == 1:
            assert same_bits(outs[0], plain[0])
        else:
            assert not same_bits(outs[0][0], plain[0][0])


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("kind", ["views", "padded", "warped"])
@pytest.mark.parametrize("name", list(GEOS))
def test_dino_and_eight_op_chains(mi, orc, name, kind, host):
    """the DINO global-view chain and eight ops with the blur first, in the middle and last, one chain per group: u8 HWC, float16 CHW
    and float32 HWC; views, padded views and warped views; mirrored views in every group"""
    c, h, imgs, conts, dev, codec = setup(mi, orc, name)
    warp = kind == "warped"
    vs = WARPS if warp else PADDED if kind == "padded" and h == 44 else views_of(h)[:3]
    fill = dict(warp=True, fill=[200, 30, 90][:c]) if warp else {}
    groups = [PG(vs, 70, 33, photo=DINO, **fill), PG(vs, 20, 12, photo=EIGHT_FIRST, dtype="float16", layout="chw", **fill),
              PG(vs, 20, 12, photo=EIGHT_MID, dtype="float32", layout="hwc", **fill), PG(vs, 70, 33, photo=EIGHT_LAST, dtype="float16", layout="chw", **fill)]
    check(mi, codec, groups, c, dev, pad_mode="edge" if kind == "padded" else None, conts=list(conts) if host else None)


def test_every_kind_of_op_at_one_step_and_the_memory_bound(mi, orc):
    """one group whose views have, at step 1, the blur, a table, color, hue and nothing (an ended chain); then the chunked case of
    test_gpu_photo_views.py's memory test with a blur in the chain"""
    c, h, tw, th, planar = GEOS["100x44_32x16i_c3"]
    _, _, imgs, conts, dev, _ = setup(mi, orc, "100x44_32x16i_c3")
    codec = mi.Codec(FRAMES, W, h, c, tw, th, planar, device=0)
    try:
        vs = views_of(h)
        first = ("brightness", 1.1)
        mixed = [[first, ("gaussian_blur", 1.5), "invert"], [first, ("solarize", 100), "invert"], [first, ("color", 1.6), "invert"],
                 [first, ("adjust_hue", 0.3), "invert"], [first]]
        check(mi, codec, [PG(vs, 70, 33, photo=mixed, dtype="float16", layout="chw"), PG(vs, 20, 12, photo=mixed)], c, dev)
        many = [vs[i % len(vs)] for i in range(40)]  # 40 views of 100 x 44: more than the staging buffer's bound holds, so chunks
        chain = [("brightness", 1.3), ("contrast", 0.7), ("gaussian_blur", 1.2), ("adjust_hue", 0.1), "equalize"]
        groups = [PG(many, 100, 44, photo=chain), PG(vs, 20, 12, photo=EIGHT_LAST, dtype="float32", layout="chw")]
        check(mi, codec, groups, c, dev)
        check(mi, codec, groups, c, dev, pad_mode="edge")
        wviews = [(v[0], 1.0, 0.1, float(v[1]), -0.1, 1.0, float(v[2]), flag(spec.BILINEAR)) for v in many]
        check(mi, codec, [PG(wviews, 100, 44, photo=chain[:3], warp=True)], c, dev)
        run(mi, codec, groups, c, conts=list(conts))
        assert codec.allocated_bytes() <= codec.photo_workspace_bytes(45)
    finally:
        codec.close()


def test_a_group_without_chains_beside_a_group_that_blurs(mi, orc):
    c, h, imgs, conts, dev, codec = setup(mi, orc, "100x44_32x16i_c3")
    vs = views_of(h)
    groups = [PG(vs, 20, 12, dtype="float16", layout="chw"), PG(vs, 70, 33, photo=[("gaussian_blur", 1.0)])]
    outs, plain = check(mi, codec, groups, c, dev)
    st, alone = run(mi, codec, groups[:1], c, dev=dev)  # the extended call: the group by itself, no photo= anywhere
    assert st == 0 and same_bits(outs[0], alone[0])


def test_bad_radius_and_factor_leave_output_and_status_untouched(mi, orc):
    c, h, imgs, conts, dev, codec = setup(mi, orc, "100x44_32x16i_c3")
    vs = views_of(h)[:2]
    bad = [("gaussian_blur", -0.5), ("gaussian_blur", 32.5), ("gaussian_blur", float("nan")), ("gaussian_blur", float("inf")),
           ("adjust_hue", 0.51), ("adjust_hue", -0.75), ("adjust_hue", float("nan")), ("adjust_hue", -float("inf")), (9, 1.0), (15, 0.0), (18, 0.0)]
    for op in bad:
        for host in (False, True):
            o = TOut(len(vs), 20, 12, c, "uint8", "hwc", status=0x77)
            g = [mi.ViewGroup(vs, 20, 12, o.ptr, photo=[[("gaussian_blur", 1.0)], [("invert", None), ("adjust_hue", 0.1), op]])]
            with pytest.raises(mi.LlcompError) as e:
                if host:
                    codec.decode_views_host(conts, g, o.st.data_ptr(), stream())
                else:
                    codec.decode_views(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), g, o.st.data_ptr(), stream())
            assert e.value.status == mi.BAD_ARGS, op
            st, out = o.read()
            assert st == 0x77 and (out == 0x5A).all(), op
    from llcomp_amd import _lib

    assert C.sizeof(_lib.PhotoChain) == 68


def test_close_shared_codecs():
    close_shared_codecs()
