"""The arithmetic of the photometric chains as the DEVICE compiler built it, over whole domains (photo_kernels.hip with photo_rule.hpp):
what tests/test_photo_area_rule.py, test_photo_rule.py and test_photo_sharpness_rule.py pin for the host compilation, through the
kernels.  The pixel ops run on a 4096 x 4096 frame that holds every colour once, the hue also with every shift byte a factor can give
on a frame of every (max - min, max) pair; the table ops, the sharpness and the blur's weights run over sweeps of hundreds of
parameters, one chain per view.  Expected values: tests/photo_spec.py (numpy) on the frame itself -- an identity view is asserted to
return it -- bit for bit.  The inputs and their witnesses: tests/device_domains.py.

The frames are encoded by the device encoder (the codec is pinned elsewhere).  Every test prints the seconds its expected values took
on the host ("host s")."""
import time

import numpy as np
import pytest

import device_domains as dd
import photo_spec
import resize_filters_spec as spec
from photo_gpu import PG, flag, mi, run  # noqa: F401  (mi: the fixture)
from test_gpu_resized_regions import packed

pytestmark = pytest.mark.gpu

NEAREST = flag(spec.NEAREST)
_frames = {}


class Frames:
    """frames [n, h, w, c] in HBM as containers of the device encoder, and their codec"""

    def __init__(self, mi, imgs, tw, th, planar):
        n, h, w, c = imgs.shape
        self.imgs, self.c = imgs, c
        conts = [mi.compress_image(f, w, h, c, format=mi.FORMAT_SLICED, tile_w=tw, tile_h=th, planar=planar, device=0) for f in imgs]
        self.dev = packed(mi, conts)
        self.codec = mi.Codec(n, w, h, c, tw, th, planar, device=0)

    def crop(self, v):
        return self.imgs[v[0], v[2]:v[2] + v[4], v[1]:v[1] + v[3]]


def frames(mi, name):
    if name not in _frames:
        kind, c = name[:-1], int(name[-1])
        if kind == "colours":
            made = Frames(mi, (dd.all_colours() if c == 3 else dd.all_levels())[None], 256, 1, True)
        elif kind == "pairs":
            made = Frames(mi, dd.pairs_frame()[None], 128, 1, True)
        elif kind == "white":
            made = Frames(mi, dd.white_heavy(c)[None], 256, 1, True)
        elif kind == "ramp":
            made = Frames(mi, dd.ramp_frame(c)[None], 32, 16, False)
        else:
            made = Frames(mi, {"noise": dd.noise_frames, "blocks": dd.block_frames}[kind](c), 32, 16, False)
        _frames[name] = made
    return _frames[name]


def drop(name):
    if name in _frames:
        _frames.pop(name).codec.close()


def own_size(rects, frame=0):
    """NEAREST views of rectangles (x, y, w, h) at their own size"""
    return [(frame, x, y, w, h, NEAREST) for x, y, w, h in rects]


def check_frame(mi, fr, views, chains):
    """one group per chain of `chains`, every group the same own-size views: each output against photo_spec on the frame's own pixels"""
    ow, oh = views[0][3], views[0][4]
    groups = [PG(views, ow, oh, photo=ch) for ch in chains]
    st, outs = run(mi, fr.codec, groups, fr.c, dev=fr.dev)
    assert st == 0
    t0 = time.perf_counter()
    want = dd.pmap(lambda gv: photo_spec.apply(fr.crop(gv[1]), gv[0]), [(ch, v) for ch in chains for v in views])
    host = time.perf_counter() - t0
    for gi, ch in enumerate(chains):
        for vi, v in enumerate(views):
            exp = want[gi * len(views) + vi]
            if not np.array_equal(outs[gi][vi], exp):
                at = np.argwhere(outs[gi][vi] != exp)[0]
                y, x = int(at[0]), int(at[1])
                raise AssertionError((ch, v, (x, y), fr.crop(v)[y, x].tolist(), outs[gi][vi][y, x].tolist(), exp[y, x].tolist()))
    print("host s %.2f" % host)
    return outs


def check_views(mi, fr, views, ow, oh, chains):
    """a sweep: view i with the one-op chain chains[i], against photo_spec on what the call writes for the view without a chain --
    asserted to be the frame's own pixels.  Returns (outputs, plain outputs)"""
    st0, plain = run(mi, fr.codec, [PG(views, ow, oh)], fr.c, dev=fr.dev)
    st, outs = run(mi, fr.codec, [PG(views, ow, oh, photo=[list(ch) for ch in chains])], fr.c, dev=fr.dev)
    assert st == st0 == 0
    assert all(np.array_equal(plain[0][i], fr.crop(v)) for i, v in enumerate(views))
    t0 = time.perf_counter()
    want = dd.pmap(lambda i: photo_spec.apply(plain[0][i], chains[i]), range(len(views)))
    print("host s %.2f" % (time.perf_counter() - t0))
    for i, exp in enumerate(want):
        assert np.array_equal(outs[0][i], exp), (chains[i], views[i], np.argwhere(outs[0][i] != exp)[:4].tolist())
    return outs[0], plain[0]


# ---- 1. pixel ops on every colour -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["colours3", "colours1", "pairs3"])
def test_identity_views_return_the_frame(mi, name):
    fr = frames(mi, name)
    side = fr.imgs.shape[1]
    views = own_size(dd.tiles(side, min(side, 1024)))
    st, outs = run(mi, fr.codec, [PG(views, views[0][3], views[0][4])], fr.c, dev=fr.dev)
    assert st == 0 and all(np.array_equal(outs[0][i], fr.crop(v)) for i, v in enumerate(views))


HUES = [0.1, -0.5, 0.5, 1 / 255, -1 / 255, 0.0]


@pytest.mark.parametrize("factor", HUES, ids=["%.4f" % f for f in HUES])
def test_hue_on_every_colour(mi, factor):
    outs = check_frame(mi, frames(mi, "colours3"), own_size(dd.tiles()), [[("adjust_hue", factor)]])
    assert not np.array_equal(outs[0][5], dd.all_colours()[1024:2048, 1024:2048])  # (a shift of 0 too: RGB -> HSV -> RGB loses bits)


def test_hue_leaves_one_channel_alone(mi):
    fr = frames(mi, "colours1")
    outs = check_frame(mi, fr, own_size(dd.tiles()), [[("adjust_hue", 0.1)]])
    assert np.array_equal(outs[0][0], fr.imgs[0, :1024, :1024])


SHIFT_PARTS = [dd.SHIFTS[i:i + 64] for i in range(0, len(dd.SHIFTS), 64)]


@pytest.mark.parametrize("shifts", SHIFT_PARTS, ids=["from%d" % p[0] for p in SHIFT_PARTS])
def test_hue_with_every_shift_byte_on_every_pair(mi, shifts):
    """one view of the 512 x 512 frame of every (max - min, max) pair per shift byte, 64 shifts a call: every (H + shift, S, V) that
    HSV -> RGB can meet"""
    chains = [[("adjust_hue", dd.hue_factor(s))] for s in shifts]
    assert [photo_spec.hue_shift(ch[0][1]) for ch in chains] == shifts
    fr = frames(mi, "pairs3")
    check_views(mi, fr, own_size([(0, 0, dd.PAIRS_SIDE, dd.PAIRS_SIDE)]) * len(shifts), dd.PAIRS_SIDE, dd.PAIRS_SIDE, chains)


F_PARTS = [dd.factors()[i:i + 6] for i in range(0, len(dd.factors()), 6)]


@pytest.mark.parametrize("part", range(len(F_PARTS)))
def test_color_on_every_colour(mi, part):
    """every (L, v) pair that COLOR can see, under six factors of F a call; the first call holds the contraction witnesses"""
    outs = check_frame(mi, frames(mi, "colours3"), own_size(dd.tiles()), [[("color", a)] for a in F_PARTS[part]])
    if part == 0:
        for a, d, v, byte, fused in dd.witnesses():
            px = dd.colour_of(d, v)
            i = (px[0] << 16) | (px[1] << 8) | px[2]
            y, x = i >> 12, i & 4095
            got = outs[F_PARTS[0].index(a)][(y >> 10) * 4 + (x >> 10)][y & 1023, x & 1023]
            assert got[px.index(v)] == byte != fused


def test_grayscale_on_every_colour_and_one_channel(mi):
    check_frame(mi, frames(mi, "colours3"), own_size(dd.tiles()), [["grayscale"]])
    fr = frames(mi, "colours1")
    outs = check_frame(mi, fr, own_size(dd.tiles()), [["grayscale"], [("color", dd.factors()[0])], [("color", 1.5)]])
    assert all(np.array_equal(o[3], fr.imgs[0, :1024, 3072:]) for o in outs)


def test_color_on_every_colour_is_pil(mi):
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance

    factors = [dd.factors()[0], 0.5, 1.5]
    fr = frames(mi, "colours3")
    views = own_size(dd.tiles())
    st, outs = run(mi, fr.codec, [PG(views, 1024, 1024, photo=[("color", a)]) for a in factors], fr.c, dev=fr.dev)
    assert st == 0
    enhancer = ImageEnhance.Color(Image.fromarray(dd.all_colours()))
    for a, out in zip(factors, outs):
        want = np.asarray(enhancer.enhance(float(np.float32(a))))
        assert all(np.array_equal(out[i], want[v[2]:v[2] + 1024, v[1]:v[1] + 1024]) for i, v in enumerate(views)), a


def test_close_the_colour_frames():
    for name in ("colours3", "colours1", "pairs3"):
        drop(name)


# ---- 2. table ops, sharpness and blur weights over parameter sweeps -------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
def test_brightness_sweep(mi, c):
    """16 x 16 views of all 256 values in every channel: one per factor of F and 512 seeded ones"""
    factors = dd.factors() + dd.more_factors()
    views = own_size([(0, 16 * (k % dd.BANDS), 16, 16) for k in range(len(factors))])
    out, plain = check_views(mi, frames(mi, "ramp%d" % c), views, 16, 16, [[("brightness", a)] for a in factors])
    assert all(len(np.unique(plain[0][..., ch])) == 256 for ch in range(c))


@pytest.mark.parametrize("c", [1, 3])
def test_contrast_sweep(mi, c):
    """the same views widened by a constant half: every factor of F on four means, the witnesses' on a view whose mean is their d"""
    todo = dd.contrast_views(c)
    views = own_size([(0, 16 * k, 32, 16) for k, _ in todo])
    out, plain = check_views(mi, frames(mi, "ramp%d" % c), views, 32, 16, [[("contrast", a)] for _, a in todo])
    for i, (a, d, v, byte, fused) in enumerate(dd.witnesses()):
        assert dd.mean_l(plain[i]) == d and byte != fused and (out[i][plain[i] == v] == byte).all()


@pytest.mark.parametrize("op", ["contrast", "autocontrast", "equalize"])
@pytest.mark.parametrize("c", [1, 3])
def test_statistics_of_a_view_of_17_million_pixels(mi, c, op):
    """one view of 4352 x 4096: many workgroups merge its histogram and its sum of L, which passes 2^32, through atomics in HBM"""
    fr = frames(mi, "white%d" % c)
    assert int(photo_spec.luma(fr.imgs[0]).sum()) > 1 << 32
    outs = check_frame(mi, fr, own_size([(0, 0, 4352, 4096)]), [[(op, 0.6)]])
    assert not np.array_equal(outs[0][0], fr.imgs[0])


@pytest.mark.parametrize("c", [1, 3])
def test_sharpness_sweep(mi, c):
    factors = dd.factors()
    views = [(f, x, y, 70, 33, NEAREST) for f, x, y in dd.spots(len(factors), 70, 33, 70)]
    check_views(mi, frames(mi, "noise%d" % c), views, 70, 33, [[("adjust_sharpness", a)] for a in factors])


@pytest.mark.parametrize("c", [1, 3])
def test_blur_radius_thresholds(mi, c):
    """the radius at which the box radius steps to r, for every r the limit lets through, with two binary32 neighbours on each side,
    and 64 seeded radii: the device's sqrt, divisions, floorf and truncation of photo_blur_weights"""
    radii = dd.blur_radii()
    at = dd.spots(len(radii), 24, 24, 24)
    views = [(f, x, y, 24, 24, NEAREST) for f, x, y in at]
    check_views(mi, frames(mi, "blocks%d" % c), views, 24, 24, [[("gaussian_blur", r)] for r in radii])


def test_close_the_frames():
    for name in list(_frames):
        drop(name)
