"""Photometric chains on the GPU (llcomp_mi_codec_decode_photo_views / _photo_warped_views and their _host forms, through the photo=
keyword of ViewGroup and WarpGroup).  The way of checking is tests/photo_gpu.py's: tests/photo_spec.py over what the existing call writes
for the same view as U8 HWC, bit for bit; and PIL's ImageEnhance / ImageOps themselves where PIL is installed."""
import ctypes as C

import numpy as np
import pytest

import photo_spec
import resize_filters_spec as spec
from photo_gpu import FRAMES, GEOS, PG, W, check, close_shared_codecs, flag, mi, run, setup, views_of  # noqa: F401  (mi: the fixture)
from test_gpu_regions_host import make_batch, stream
from test_gpu_resized_output import TOut, same_bits
from test_gpu_resized_regions import packed

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (16, 8), (20, 12), (70, 33)]  # 70 x 33: several workgroups per view in every kernel, and a tail in each
JITTER = [("brightness", 1.3), ("contrast", 0.7), ("color", 1.6), ("grayscale", None)]
JITTER_B = [("color", 0.4), ("contrast", 1.8), ("brightness", 0.8)]
EIGHT = [("brightness", 1.2), ("contrast", 1.5), ("color", 0.3), ("equalize", None), ("solarize", 140), ("posterize", 3), ("autocontrast", None),
         ("invert", None)]
ONE_OP = [[("brightness", 1.4)], [("contrast", 0.6)], [("color", 1.7)], ["grayscale"], ["invert"], [("solarize", 100)], [("posterize", 3)],
          ["autocontrast"], ["equalize"], [("brightness", 0.0)], [("contrast", 2.5)], [("color", 1.0)], [("solarize", 0)], [("solarize", 256)],
          [("posterize", 8)], [("posterize", 1)]]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("name", list(GEOS))
def test_every_op_alone(mi, orc, name, shape):
    c, h, imgs, conts, dev, codec = setup(mi, orc, name)
    vs = views_of(h, small=shape == (1, 1))
    views = [vs[i % len(vs)] for i in range(len(ONE_OP))]
    check(mi, codec, [PG(views, *shape, photo=[list(ch) for ch in ONE_OP])], c, dev)


@pytest.mark.parametrize("name", list(GEOS))
def test_jitter_chains_and_a_mixed_group(mi, orc, name):
    """the four-op jitter chain in two orders, with and without grayscale, and all eight ops; then ONE group whose views have chains of
    different lengths, empty chains, mirrors and filters of their own (views_of), beside a group without photo="""
    c, h, imgs, conts, dev, codec = setup(mi, orc, name)
    vs = views_of(h)
    for chain in (JITTER, JITTER_B + ["grayscale"], JITTER_B, EIGHT):
        check(mi, codec, [PG(vs, 70, 33, photo=chain), PG(vs[:2], 20, 12, photo=chain)], c, dev)
    mixed = PG(vs, 20, 12, photo=[list(JITTER), [], list(EIGHT), [], ["equalize"]])
    outs, plain = check(mi, codec, [mixed, PG(vs[1:3], 16, 8)], c, dev)
    assert same_bits(outs[0][1], plain[0][1]) and same_bits(outs[0][3], plain[0][3]) and same_bits(outs[1], plain[1])


def test_statistics_are_those_of_the_view(mi, orc):
    """two views of one frame, different rectangles, the same chain: each gets the table of its own mean and histogram"""
    c, h, imgs, conts, dev, codec = setup(mi, orc, "100x44_32x16i_c3")
    chain = [("contrast", 0.5), "equalize", "autocontrast"]
    g = PG([(0, 0, 0, 40, 30, flag(spec.BILINEAR)), (0, 50, 10, 50, 30, flag(spec.BILINEAR))], 20, 12, photo=chain)
    outs, plain = check(mi, codec, [g], c, dev)
    pooled = photo_spec.apply(np.concatenate([plain[0][0], plain[0][1]], axis=0), chain)  # (the group's statistics: NOT the rule)
    assert not np.array_equal(np.concatenate([outs[0][0], outs[0][1]], axis=0), pooled)


def test_formatted_group_beside_plain_groups(mi, orc):
    c, h, imgs, conts, dev, codec = setup(mi, orc, "100x44_32x16i_c3")
    vs = views_of(h)
    groups = [PG(vs, 16, 8, photo=JITTER, dtype="float16", layout="chw"), PG(vs[:3], 20, 12), PG(vs[2:], 70, 33, photo=EIGHT),
              PG(vs[:2], 20, 12, photo=JITTER_B, dtype="float32", layout="hwc"), PG(vs[:2], 16, 8, photo=["equalize"], dtype="uint8", layout="chw")]
    check(mi, codec, groups, c, dev)


@pytest.mark.parametrize("name", ["100x44_32x16i_c3", "100x44_32x16i_c1"])
def test_padded_group(mi, orc, name):
    c, h, imgs, conts, dev, codec = setup(mi, orc, name)
    views = [(0, -10, -5, 60, 30, flag(spec.BILINEAR)), (2, 70, 30, 40, 20, flag(spec.BICUBIC, True)), (2, 10, 5, 30, 20, flag(spec.BOX))]
    check(mi, codec, [PG(views, 20, 12, photo=JITTER + ["equalize"]), PG(views[:2], 16, 8)], c, dev, pad_mode="reflect")


@pytest.mark.parametrize("name", ["100x44_32x16i_c3", "100x6_50x1p_c3", "100x44_32x16i_c1"])
def test_warped_groups(mi, orc, name):
    """bilinear warps with chains; and a view wholly outside the frame -- all fill, constant -- which AUTOCONTRAST and EQUALIZE leave as
    it is"""
    c, h, imgs, conts, dev, codec = setup(mi, orc, name)
    fill = [200, 30, 90][:c]
    views = [(0, 0.9, 0.2, 3.0, -0.2, 0.9, 1.0, flag(spec.BILINEAR)), (2, 1.1, -0.3, 20.0, 0.1, 0.5, 0.5, flag(spec.BILINEAR, True)),
             (0, 1.0, 0.1, 500.0, -0.1, 1.0, 7.0, flag(spec.BILINEAR)), (2, 0.7, 0.0, 5.25, 0.0, 0.4, 0.5, flag(spec.NEAREST))]
    chain = ["autocontrast", "equalize"]
    groups = [PG(views, 20, 12, photo=chain, warp=True, fill=fill), PG(views, 70, 33, photo=JITTER, warp=True, fill=fill, dtype="float16", layout="chw"),
              PG(views[:2], 16, 8, warp=True, fill=fill)]
    outs, plain = check(mi, codec, groups, c, dev)
    assert (plain[0][2] == np.array(fill, np.uint8)).all() and same_bits(outs[0][2], plain[0][2])
    # every view outside: nothing is decoded, the chains still run
    check(mi, codec, [PG([views[2]], 16, 8, photo=EIGHT, warp=True, fill=fill)], c, dev)


def test_host_forms_write_the_same_bytes_and_stage_the_same_payload(mi, orc):
    c, h, imgs, conts, dev, codec = setup(mi, orc, "100x44_32x16i_c3")
    vs = views_of(h)
    rect = [PG(vs, 20, 12, photo=JITTER, dtype="float16", layout="chw"), PG(vs[:2], 16, 8)]
    warp = [PG([(0, 0.9, 0.2, 3.0, -0.2, 0.9, 1.0, flag(spec.BILINEAR)), (2, 1.0, 0.0, 4.0, 0.0, 1.0, 2.0, flag(spec.NEAREST))], 20, 12, photo=EIGHT,
               warp=True)]
    host = [None if f == 1 else d for f, d in enumerate(conts)]  # (frame 1 has no view)
    for groups, pad_mode in ((rect, None), (rect, "reflect"), (warp, None)):
        st, outs = run(mi, codec, groups, c, dev=dev, pad_mode=pad_mode)
        codec.counters(reset=True)
        st_h, outs_h = run(mi, codec, groups, c, conts=host, pad_mode=pad_mode)
        staged = codec.counters(reset=True)["host_staged_bytes"]
        run(mi, codec, groups, c, conts=host, plain=True, pad_mode=pad_mode)
        assert staged == codec.counters(reset=True)["host_staged_bytes"] and staged > 0
        assert st == st_h == 0
        for a, b in zip(outs, outs_h):
            assert same_bits(a, b)


@pytest.mark.parametrize("name", ["100x44_32x16i_c3", "100x6_50x1p_c3"])
def test_empty_chains_are_the_plain_call(mi, orc, name):
    c, h, imgs, conts, dev, codec = setup(mi, orc, name)
    vs = views_of(h)
    for warp in (False, True):
        views = [(v[0], 1.0, 0.0, float(v[1]), 0.0, 1.0, float(v[2]), flag(spec.NEAREST, i == 1)) for i, v in enumerate(vs[:2])] if warp else vs
        none = [PG(views, 20, 12, warp=warp, dtype="float16", layout="chw"), PG(views[:2], 16, 8, warp=warp)]
        empty = [PG(views, 20, 12, photo=[], warp=warp, dtype="float16", layout="chw"), PG(views[:2], 16, 8, photo=[[], []], warp=warp)]
        st, outs = run(mi, codec, none, c, dev=dev)
        st_e, outs_e = run(mi, codec, empty, c, dev=dev)
        assert st == st_e == 0
        for a, b in zip(outs, outs_e):
            assert same_bits(a, b)


def test_two_calls_back_to_back_on_one_stream(mi, orc):
    """no synchronisation in between: the pinned ring, the staging buffer and the statistics are used again behind the first call"""
    c, h, imgs, conts, dev, codec = setup(mi, orc, "100x44_32x16i_c3")
    vs = views_of(h)
    first, second = [PG(vs, 70, 33, photo=EIGHT)], [PG(vs[::-1], 20, 12, photo=JITTER + ["equalize"], dtype="float16", layout="chw")]
    want = [check(mi, codec, g, c, dev)[0] for g in (first, second)]
    o1 = run(mi, codec, first, c, dev=dev, read=False)
    o2 = run(mi, codec, second, c, conts=list(conts), read=False)
    o3 = run(mi, codec, first, c, dev=dev, read=False)
    for o, w in ((o1, want[0]), (o2, want[1]), (o3, want[0])):
        st, out = o[0].read()
        assert st == 0 and same_bits(out, w[0])


def test_memory_stays_within_photo_workspace_bytes(mi, orc):
    c, h, tw, th, planar = GEOS["100x44_32x16i_c3"]
    _, _, imgs, conts, dev, _ = setup(mi, orc, "100x44_32x16i_c3")
    codec = mi.Codec(FRAMES, W, h, c, tw, th, planar, device=0)
    try:
        vs = views_of(h)
        many = [vs[i % len(vs)] for i in range(40)]  # 40 views of 100 x 44: more than the staging buffer's bound holds, so chunks
        groups = [PG(many, 100, 44, photo=JITTER + ["equalize"]), PG(vs, 20, 12, photo=EIGHT, dtype="float32", layout="chw")]
        check(mi, codec, groups, c, dev)
        check(mi, codec, groups, c, dev, pad_mode="edge")
        wviews = [(v[0], 1.0, 0.1, float(v[1]), -0.1, 1.0, float(v[2]), flag(spec.BILINEAR)) for v in many]
        check(mi, codec, [PG(wviews, 100, 44, photo=JITTER, warp=True)], c, dev)
        run(mi, codec, groups, c, conts=list(conts))
        assert codec.allocated_bytes() <= codec.photo_workspace_bytes(45)
        assert codec.photo_workspace_bytes(45) - max(codec.padded_workspace_bytes(45), codec.warp_workspace_bytes(45)) == \
            FRAMES * W * h * c + 45 * (8 + 1280 * c) + 16 + 45 * 68
    finally:
        codec.close()


def test_refusals_leave_output_and_status_untouched(mi, orc):
    c, h, imgs, conts, dev, codec = setup(mi, orc, "100x44_32x16i_c3")
    vs = views_of(h)[:2]

    def refused(call):
        o = TOut(len(vs), 20, 12, c, "uint8", "hwc", status=0x77)
        with pytest.raises(mi.LlcompError) as e:
            call(o)
        assert e.value.status == mi.BAD_ARGS
        st, out = o.read()
        assert st == 0x77 and (out == 0x5A).all()

    def py(photo, host=False, warp=False):
        def call(o):
            if warp:
                g = mi.WarpGroup([(0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, flag(spec.NEAREST))] * 2, 20, 12, o.ptr, photo=photo)
                if host:
                    codec.decode_warped_views_host(conts, [g], o.st.data_ptr(), stream())
                else:
                    codec.decode_warped_views(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), [g], o.st.data_ptr(), stream())
            elif host:
                codec.decode_views_host(conts, [mi.ViewGroup(vs, 20, 12, o.ptr, photo=photo)], o.st.data_ptr(), stream())
            else:
                codec.decode_views(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), [mi.ViewGroup(vs, 20, 12, o.ptr, photo=photo)], o.st.data_ptr(), stream())
        return call

    bad = [[("brightness", float("nan"))], [("contrast", float("inf"))], [("color", -0.5)], [("brightness", 256.5)], [("solarize", 1.5)],
           [("solarize", 257)], [("solarize", -1)], [("posterize", 0)], [("posterize", 9)], [("posterize", 2.5)], [(9, 1.0)], [(0xFFFFFFFF, 1.0)]]
    for chain in bad:
        refused(py([[("invert", None)], chain]))  # (a good chain first: nothing of it may have been queued)
    for host in (False, True):
        for warp in (False, True):
            refused(py([("posterize", 9)], host, warp))

    # what the Python layer refuses by itself goes through the C structs: nine ops, and a struct_size that is not the struct's
    from llcomp_amd import _lib

    def raw(n_ops, struct_size):
        def call(o):
            views = (_lib.View * 2)(*[_lib.View(*v) for v in vs])
            grp = (_lib.ViewGroup * 1)(_lib.ViewGroup(C.sizeof(_lib.ViewGroup), 2, views, 20, 12, None, o.ptr))
            chains = (_lib.PhotoChain * 2)()
            for ch in chains:
                ch.n_ops = n_ops
                for k in range(8):
                    ch.ops[k] = _lib.PhotoOp(mi.PHOTO_INVERT, 0.0)
            pg = (_lib.PhotoGroup * 1)(_lib.PhotoGroup(struct_size, chains))
            rc = _lib.load().llcomp_mi_codec_decode_photo_views(codec._h, dev[0].data_ptr(), dev[1], dev[2].data_ptr(), grp, 1, None, pg,
                                                                o.st.data_ptr(), stream())
            if rc:
                raise mi.LlcompError(rc)
        return call

    refused(raw(9, C.sizeof(_lib.PhotoGroup)))
    refused(raw(1, C.sizeof(_lib.PhotoGroup) + 8))
    raw(8, C.sizeof(_lib.PhotoGroup))(TOut(len(vs), 20, 12, c, "uint8", "hwc"))  # (the same call within the limits is taken)

    # a chain on a codec that is neither L nor RGB; an empty chain there is the plain call
    imgs4, conts4 = make_batch(orc, FRAMES, W, 44, 4, 32, 16, False)
    dev4 = packed(mi, conts4)
    codec4 = mi.Codec(FRAMES, W, 44, 4, 32, 16, False, device=0)
    try:
        for photo, ok in ((["invert"], False), ([], True)):
            o = TOut(len(vs), 20, 12, 4, "uint8", "hwc", status=0x77)
            g = [mi.ViewGroup(vs, 20, 12, o.ptr, photo=photo)]
            if ok:
                codec4.decode_views(dev4[0].data_ptr(), dev4[1], dev4[2].data_ptr(), g, o.st.data_ptr(), stream())
                assert o.read()[0] == 0
            else:
                with pytest.raises(mi.LlcompError) as e:
                    codec4.decode_views(dev4[0].data_ptr(), dev4[1], dev4[2].data_ptr(), g, o.st.data_ptr(), stream())
                assert e.value.status == mi.BAD_ARGS and o.read()[0] == 0x77 and (o.read()[1] == 0x5A).all()
    finally:
        codec4.close()


def test_against_pil_on_the_decoded_crop(mi, orc):
    """identity views (nearest, a rectangle at its own size): the chain's input is the decoded crop itself, and the output PIL's"""
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance, ImageOps

    def pil(a, chain):
        im = Image.fromarray(a[..., 0] if a.shape[2] == 1 else a)
        for o in chain:
            op, p = (o, None) if isinstance(o, str) else o
            p = None if p is None else float(np.float32(p))
            im = {"brightness": lambda: ImageEnhance.Brightness(im).enhance(p), "contrast": lambda: ImageEnhance.Contrast(im).enhance(p),
                  "color": lambda: ImageEnhance.Color(im).enhance(p), "grayscale": lambda: im.convert("L").convert(im.mode),
                  "invert": lambda: ImageOps.invert(im), "solarize": lambda: ImageOps.solarize(im, int(p)),
                  "posterize": lambda: ImageOps.posterize(im, int(p)), "autocontrast": lambda: ImageOps.autocontrast(im),
                  "equalize": lambda: ImageOps.equalize(im)}[op]()
        return np.asarray(im).reshape(a.shape)

    for name in ("100x44_32x16i_c3", "100x44_32x16i_c1"):
        c, h, imgs, conts, dev, codec = setup(mi, orc, name)
        views = [(0, 10, 4, 70, 33, flag(spec.NEAREST)), (2, 30, 11, 70, 33, flag(spec.NEAREST))]
        for chain in (JITTER, EIGHT, ["equalize"], ["autocontrast"], [("contrast", 1.7)]):
            st, outs = run(mi, codec, [PG(views, 70, 33, photo=chain)], c, dev=dev)
            assert st == 0
            for i, (f, x, y, rw, rh, _) in enumerate(views):
                assert np.array_equal(outs[0][i], pil(imgs[f, y:y + rh, x:x + rw], chain)), (name, chain, i)


def test_close_shared_codecs():
    close_shared_codecs()
