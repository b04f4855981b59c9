"""Views decode (llcomp_mi_codec_decode_views, ..._host): several views of each frame in one call, each frame decoded once.  Containers
come from the oracle; the expected output of a view is the numpy statement of the resampling rule (tests/resize_spec.py for bilinear,
tests/resize_filters_spec.py for every filter) applied to img[frame, y:y+rh, x:x+rw], then llcomp_mi_output_table for a formatted group,
bit for bit -- and what the existing decode_resized_regions writes for that rectangle of that frame."""
import numpy as np
import pytest

import orc as orc_mod
import resize_filters_spec as spec
from conftest import make_image
from resize_spec import resize as bilinear_resize
from test_gpu_regions_host import GUARD, Out, make_batch, stream
from test_gpu_resized_output import TOut, norm, place, same_bits
from test_gpu_resized_regions import FAMILIES, packed

pytestmark = pytest.mark.gpu

MIRROR = 1


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


_batches = {}


def batch(orc, frames, w, h, c, tw, th, planar, small=False):
    key = (frames, w, h, c, tw, th, planar, small)
    if key not in _batches:
        _batches[key] = make_batch(orc, frames, w, h, c, tw, th, planar, small_model=small)
    return _batches[key]


def flag(filt, mirror=False):
    return (filt << 4) | (MIRROR if mirror else 0)


class G:
    """a group of a test: its views (frame, x, y, rw, rh, flags), output shape and format"""

    def __init__(self, views, ow, oh, dtype="uint8", layout="hwc"):
        self.views, self.ow, self.oh, self.dtype, self.layout = list(views), ow, oh, dtype, layout

    def kw(self, c):
        return norm(c, self.dtype)

    def out(self, c, offset=0, status=0):
        return TOut(len(self.views), self.ow, self.oh, c, self.dtype, self.layout, offset, status)

    def group(self, mi, c, ptr):
        plain = self.dtype == "uint8" and self.layout == "hwc"
        return mi.ViewGroup(self.views, self.ow, self.oh, ptr, **({} if plain else dict(dtype=self.dtype, layout=self.layout, **self.kw(c))))

    def expected(self, mi, imgs):
        c = imgs.shape[-1]
        u8 = []
        for f, x, y, rw, rh, fl in self.views:
            crop, filt, mirror = imgs[f, y:y + rh, x:x + rw], (fl >> 4) & 7, bool(fl & 1)
            u8.append(spec.resize(crop, self.ow, self.oh, filt, mirror))
            if filt == 0:  # bilinear: the first statement of the rule says the same
                assert np.array_equal(u8[-1], bilinear_resize(mi, crop, self.ow, self.oh, mirror))
        return place(mi.output_table(c, self.dtype, **self.kw(c)), np.stack(u8), self.layout)


def run_views(mi, codec, groups, c, dev=None, conts=None, order=None):
    """one views call (from HBM: dev; from host containers: conts), the groups passed in `order` -> (status, [output of every group])"""
    outs = [g.out(c) for g in groups]
    order = list(range(len(groups))) if order is None else order
    arg = [groups[i].group(mi, c, outs[i].ptr) for i in order]
    st = outs[0].st
    if conts is not None:
        codec.decode_views_host(conts, arg, st.data_ptr(), stream())
    else:
        codec.decode_views(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), arg, st.data_ptr(), stream())
    got = [o.read() for o in outs]
    return got[0][0], [g[1] for g in got]


def per_view(mi, codec, dev, g, c, frames):
    """the group's views through the existing call, one call per view: its frame gets the view's rectangle, every other frame a 1 x 1"""
    outs = []
    for f, x, y, rw, rh, fl in g.views:
        rects = [(x, y, rw, rh) if i == f else (0, 0, 1, 1) for i in range(frames)]
        flags = np.array([fl if i == f else 0 for i in range(frames)], np.uint8)
        o = TOut(frames, g.ow, g.oh, c, g.dtype, g.layout)
        codec.decode_resized_regions(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), rects, g.ow, g.oh, o.ptr, o.st.data_ptr(), flags=flags,
                                     stream=stream(), dtype=g.dtype, layout=g.layout, **g.kw(c))
        st, out = o.read()
        assert st == 0
        outs.append(out[f])
    return np.stack(outs)


def case_groups(w, h, fmt_b):
    """4 frames with 0, 1, 2 and 5 views in three groups: 24 x 16 u8 HWC; one view at its own size (identity) in format fmt_b; 16 x 24
    float32 CHW normalised.  Frame 1: the full image.  Frame 2: a mirrored 1 x 1 on the last pixel and a rectangle in the last corner
    (the union's window holds the partial last tile column and row).  Frame 3: two identical mirrored views, bicubic and Lanczos views
    in the float group, the identity view -- the same frame in all three groups.  All six filters, three views mirrored."""
    last = (2, w - min(w, 37), h - min(h, 9), min(w, 37), min(h, 9), flag(spec.BOX))
    twin = (3, w // 5, h // 4, min(w - w // 5, 61), min(h - h // 4, 13), flag(spec.HAMMING, True))
    cubic = (3, w // 2, 0, min(w - w // 2, 100), min(h, 20), flag(spec.BICUBIC))
    lanc = (3, 3, h // 3, min(w - 3, 45), min(h - h // 3, 17), flag(spec.LANCZOS, True))
    own = (3, w // 3, h // 2, min(w - w // 3, 31), min(h - h // 2, 11), flag(spec.BILINEAR))
    a = G([(1, 0, 0, w, h, flag(spec.BILINEAR)), (2, w - 1, h - 1, 1, 1, flag(spec.NEAREST, True)), twin, twin], 24, 16)
    b = G([own], own[3], own[4], *fmt_b)
    c_ = G([last, cubic, lanc], 16, 24, "float32", "chw")
    return [a, b, c_]


# the five shapes of test_gpu_resized_regions.FAMILIES (four frames each) and c = 1, 4 and 5 at 160 x 90 in 32 x 16 tiles
CASES = [(f[0], 4, f[2], f[3], f[4], f[5], f[6], f[7], f[8]) for f in FAMILIES] + [
    ("c1_32x16i", 4, 160, 90, 1, 32, 16, False, False), ("c4_32x16i", 4, 160, 90, 4, 32, 16, False, False),
    ("c5_32x16i", 4, 160, 90, 5, 32, 16, False, False)]
FMT_B = [("uint8", "hwc"), ("float16", "hwc"), ("bfloat16", "chw"), ("uint8", "chw"), ("bfloat16", "hwc"), ("float16", "hwc"), ("float16", "chw"),
         ("float32", "hwc")]


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_bytes_per_view(mi, orc, i):
    name, frames, w, h, c, tw, th, planar, small = CASES[i]
    imgs, conts = batch(orc, frames, w, h, c, tw, th, planar, small)
    groups = case_groups(w, h, FMT_B[i])
    uni, win, n_used, n_cls = mi.views_plan(w, h, c, tw, th, planar, frames, [(g.views, g.ow, g.oh) for g in groups])
    assert n_used == 3 and not uni[0].any() and uni[1].tolist() == [0, 0, w, h]
    tw_, th_ = min(tw or w, w), min(th or h, h)
    assert (win[2, 2], win[2, 3]) == (-(-w // tw_), -(-h // th_))  # frame 2's window ends at the last tile column and row
    codec = mi.Codec(frames, w, h, c, tw, th, planar, device=0, small_model=small)
    try:
        dev = packed(mi, conts)
        want = [g.expected(mi, imgs) for g in groups]
        st, outs = run_views(mi, codec, groups, c, dev=dev)
        assert st == 0
        for g, out, exp in zip(groups, outs, want):
            assert same_bits(out, exp), (name, g.dtype, g.layout)
            assert same_bits(out, per_view(mi, codec, dev, g, c, frames)), (name, g.dtype, g.layout)
        assert np.array_equal(outs[0][2], outs[0][3])  # the two identical views
        # the host call (frame 0 has no view: no container), and the groups in another order: the same bytes and status
        st_h, outs_h = run_views(mi, codec, groups, c, conts=[None] + list(conts[1:]))
        st_r, outs_r = run_views(mi, codec, groups, c, dev=dev, order=[2, 0, 1])
        assert st_h == st_r == 0
        for out, a, b in zip(outs, outs_h, outs_r):
            assert same_bits(out, a) and same_bits(out, b), name
        # without the full image the windows are smaller than the tile grid: frames 0 and 1 unused, frame 2's window in the last corner
        groups[0].views.pop(0)
        uni, win, n_used, n_cls = mi.views_plan(w, h, c, tw, th, planar, frames, [(g.views, g.ow, g.oh) for g in groups])
        assert n_used == 2 and not uni[:2].any() and (win[2, 2], win[2, 3]) == (-(-w // tw_), -(-h // th_))
        want = [g.expected(mi, imgs) for g in groups]
        for kw in (dict(dev=dev), dict(conts=[None, None] + list(conts[2:]))):
            st, outs = run_views(mi, codec, groups, c, **kw)
            assert st == 0 and all(same_bits(o, e) for o, e in zip(outs, want)), (name, list(kw))
    finally:
        codec.close()


def overlapping(w, h, frames):
    """three overlapping views of every frame: two "global" ones in a 48 x 48 group, a "local" one in a 24 x 24 group"""
    big, small = [], []
    for f in range(frames):
        x, y = 10 + 30 * f, 5 + 20 * f
        big += [(f, x, y, 120, 90, flag(0, f % 2 == 1)), (f, x + 40, y + 30, 110, 80, flag(spec.BICUBIC))]
        small += [(f, x + 60, y + 20, 40, 50, flag(spec.BOX, True))]
    return [G(big, 48, 48), G(small, 24, 24, "float16", "chw")]


def test_every_frame_is_decoded_once(mi, orc):
    frames, w, h, c, tw, th = 4, 300, 200, 3, 64, 64
    imgs, conts = batch(orc, frames, w, h, c, tw, th, True)
    groups = overlapping(w, h, frames)
    uni, _, n_used, _ = mi.views_plan(w, h, c, tw, th, True, frames, [(g.views, g.ow, g.oh) for g in groups])
    assert n_used == frames
    codec = mi.Codec(frames, w, h, c, tw, th, True, device=0)
    try:
        codec.counters(reset=True)
        codec.get_profile()
        st, outs = run_views(mi, codec, groups, c, conts=conts)
        assert st == 0 and all(same_bits(o, g.expected(mi, imgs)) for o, g in zip(outs, groups))
        staged = codec.counters(reset=True)["host_staged_bytes"]
        assert codec.get_profile()[2] == 1  # one decode, whatever the number of views
        # ... which stages what the existing call stages for the union rectangles
        o = Out(frames, 8, 8, c)
        codec.decode_resized_regions_host(conts, uni, 8, 8, o.ptr, o.st.data_ptr(), stream=stream())
        assert o.read()[0] == 0
        assert staged == codec.counters(reset=True)["host_staged_bytes"] > 0
        # ... and less than the three passes that give the same views through the existing call
        every = [v for g in groups for v in g.views]
        for j in range(3):
            rects = [[v for v in every if v[0] == f][j][1:5] for f in range(frames)]
            o = Out(frames, 8, 8, c)
            codec.decode_resized_regions_host(conts, rects, 8, 8, o.ptr, o.st.data_ptr(), stream=stream())
            assert o.read()[0] == 0
        assert staged < codec.counters()["host_staged_bytes"]
    finally:
        codec.close()


def test_unused_frames_and_verdicts(mi, orc):
    w, h, c, tw, th = 512, 256, 3, 32, 32  # 16 x 8 tiles, interleaved: slice id = tile row * 16 + tile column
    frames = 3
    groups = [G([(0, 100, 70, 60, 50, 0), (0, 130, 100, 40, 30, flag(spec.BOX, True)), (2, 300, 150, 20, 10, 0)], 40, 40),
              G([(2, 310, 155, 30, 20, flag(spec.NEAREST))], 12, 12, "float32", "chw")]
    uni, win, n_used, _ = mi.views_plan(w, h, c, tw, th, False, frames, [(g.views, g.ow, g.oh) for g in groups])
    assert uni.tolist() == [[100, 70, 70, 60], [0, 0, 0, 0], [300, 150, 40, 25]] and n_used == 2
    assert win.tolist() == [[3, 2, 7, 5], [0, 0, 0, 0], [9, 4, 13, 7]]  # frame 2's window is sized for frame 0's union
    imgs = np.stack([make_image(g, w, h, c) for g in ("nat", "g3", "mid")])
    n = len(orc_mod.slice_rects(w, h, c, tw, th, False))
    clean = [orc.compress_sliced(imgs[f], tw, th, False) for f in range(frames)]
    rng = np.random.default_rng(79)

    def damaged(spots):
        conts = []
        for f in range(frames):
            d = clean[f]
            lens = np.frombuffer(d[24:24 + 4 * n], dtype="<u4").astype(np.int64)
            offs = np.concatenate([[0], np.cumsum(lens)]) + 24 + 4 * n
            pays = [d[offs[j]:offs[j + 1]] for j in range(n)]
            for ff, j in spots:
                if ff == f:
                    res = orc_mod.adversarial_residuals(rng, th, tw, c, "small")
                    pays[j] = orc.encode_residuals(res, run_at=th * tw * c // 2, run_len=33)[0]
            conts.append(orc_mod.sliced_container(w, h, c, tw, th, False, pays))
        return conts

    codec = mi.Codec(frames, w, h, c, tw, th, False, device=0)
    try:
        want = [g.expected(mi, imgs) for g in groups]
        # the unused frame: no container, a container that is no container, one damaged in every slice's place -- without effect
        for middle in (None, b"\x00" * 40, damaged([(1, j) for j in range(0, n, 7)])[1]):
            st, outs = run_views(mi, codec, groups, c, conts=[clean[0], middle, clean[2]])
            assert st == 0 and all(same_bits(o, e) for o, e in zip(outs, want))
        conts = damaged([(1, j) for j in range(0, n, 7)])
        st, outs = run_views(mi, codec, groups, c, dev=packed(mi, conts))
        assert st == 0 and all(same_bits(o, e) for o, e in zip(outs, want))
        # frame 2, tile row 6, column 11: inside its union's window, outside every view -- the verdict of the existing call on the unions
        conts = damaged([(2, 6 * 16 + 11)])
        rects = [tuple(uni[0]), (0, 0, 1, 1), tuple(uni[2])]
        o = Out(frames, 8, 8, c)
        codec.decode_resized_regions_host(conts, rects, 8, 8, o.ptr, o.st.data_ptr(), stream=stream())
        st_ref = o.read()[0]
        assert codec.status(st_ref) == mi.BAD_EXPONENT
        st, _ = run_views(mi, codec, groups, c, dev=packed(mi, conts))
        st_h, _ = run_views(mi, codec, groups, c, conts=conts)
        assert codec.status(st) == codec.status(st_h) == codec.status(st_ref)
        # outside every window: OK, exact
        conts = damaged([(0, 0), (2, 7 * 16 + 15), (2, 3 * 16 + 8), (1, 5)])
        for kw in (dict(dev=packed(mi, conts)), dict(conts=conts)):
            st, outs = run_views(mi, codec, groups, c, **kw)
            assert st == 0 and all(same_bits(o, e) for o, e in zip(outs, want))
    finally:
        codec.close()


def test_chunks_and_workspace(mi, orc):
    """one frame, 40 views of the whole image to ow = w: the rows of one view are frames * w * h * c bytes, so the group is resampled a
    view at a time, and the codec stays within what views_workspace_bytes states"""
    w, h, c, tw, th = 100, 70, 3, 32, 32
    imgs, conts = batch(orc, 1, w, h, c, tw, th, True)
    codec = mi.Codec(1, w, h, c, tw, th, True, device=0)
    try:
        assert codec.views_workspace_bytes(0) == codec.views_workspace_bytes(1) == codec.workspace_bytes
        per = 48 + 40 * (w + h) + 16 + 1024 * c  # (the per-view term the header states)
        assert codec.views_workspace_bytes(40) == codec.workspace_bytes + 39 * per
        dev = packed(mi, conts)
        many = G([(0, 0, 0, w, h, flag(j % 6, j % 4 == 1)) for j in range(40)], w, 20)
        st, outs = run_views(mi, codec, [many], c, dev=dev)
        assert st == 0 and same_bits(outs[0], many.expected(mi, imgs))
        held = codec.allocated_bytes()
        assert held <= codec.views_workspace_bytes(40)
        # chunks of several views: 8 views whose rows are a third of the image each, in a formatted group, from host containers
        third = G([(0, j, j, w - 10, h // 3, flag(j % 6, j % 2 == 0)) for j in range(8)], w, 9, "bfloat16", "chw")
        st, outs = run_views(mi, codec, [third, many], c, conts=conts)
        assert st == 0 and same_bits(outs[0], third.expected(mi, imgs)) and same_bits(outs[1], many.expected(mi, imgs))
        assert codec.allocated_bytes() <= codec.views_workspace_bytes(48)
        held = codec.allocated_bytes()
        two = G([(0, 5, 5, 50, 40, 0), (0, 20, 10, 70, 60, 1)], 32, 32)
        st, outs = run_views(mi, codec, [two], c, dev=dev)
        assert st == 0 and same_bits(outs[0], two.expected(mi, imgs))
        assert codec.allocated_bytes() == held  # a smaller call grows nothing
    finally:
        codec.close()


def test_prepare_views(mi, orc):
    frames, w, h, c, tw, th = 4, 100, 70, 3, 32, 32
    imgs, conts = batch(orc, frames, w, h, c, tw, th, True)
    codec = mi.Codec(frames, w, h, c, tw, th, True, device=0)
    try:
        codec.prepare(encode=False, decode=True, views=True)
        held = codec.allocated_bytes()
        assert held <= codec.workspace_bytes
        groups = [G([(0, 0, 0, w, h, 0), (3, 10, 10, 50, 40, flag(spec.LANCZOS, True))], w, h), G([(3, 0, 0, 30, 30, 0), (1, 99, 69, 1, 1, 0)], 24, 16,
                                                                                                     "float32", "chw")]
        st, outs = run_views(mi, codec, groups, c, dev=packed(mi, conts))
        assert st == 0 and all(same_bits(o, g.expected(mi, imgs)) for o, g in zip(outs, groups))
        assert codec.allocated_bytes() == held
    finally:
        codec.close()


def test_bad_args_write_nothing(mi, orc):
    frames, w, h, c, tw, th = 3, 200, 100, 3, 32, 16
    imgs, conts = batch(orc, frames, w, h, c, tw, th, True)
    codec = mi.Codec(frames, w, h, c, tw, th, True, device=0)
    dev = packed(mi, conts)
    good = [(0, 0, 0, 50, 50, 0), (2, 10, 10, 20, 20, 1)]
    bicubic, lanczos = flag(spec.BICUBIC), flag(spec.LANCZOS)
    cases = {  # every refusal of the plan (tests/test_views_plan.py)
        "no groups": [],
        "a group with no views": [G(good, 32, 32), G([], 32, 32)],
        "65536 views": [G([(0, 0, 0, 8, 8, 0)] * 65536, 2, 2)],
        "frame >= frames": [G(good + [(3, 0, 0, 5, 5, 0)], 32, 32)],
        "empty width": [G(good + [(1, 0, 0, 0, 5, 0)], 32, 32)],
        "empty height": [G(good, 32, 32), G([(1, 0, 0, 5, 0, 0)], 8, 8)],
        "past the right edge": [G(good + [(1, 151, 0, 50, 50, 0)], 32, 32)],
        "past the bottom edge": [G(good + [(1, 0, 51, 50, 50, 0)], 32, 32)],
        "filter code 6": [G(good + [(1, 0, 0, 5, 5, 6 << 4)], 32, 32)],
        "downscale above 64x": [G(good, 32, 32), G([(1, 0, 0, 193, 10, 0)], 3, 3)],
        "bicubic above 32x": [G([(1, 0, 0, 97, 10, bicubic)], 3, 3)],
        "lanczos above 64/3": [G(good, 32, 32, "float32", "chw"), G([(1, 0, 0, 10, 65, lanczos)], 3, 3)],
        "ow 0": [G(good, 0, 32)],
    }
    try:
        def refused(groups, outs, host, containers=conts):
            st = outs[0].st if outs else Out(1, 1, 1, 1, status=0x77).st
            arg = [g.group(mi, c, o.ptr) for g, o in zip(groups, outs)]
            with pytest.raises(mi.LlcompError) as e:
                if host:
                    codec.decode_views_host(containers, arg, st.data_ptr(), stream())
                else:
                    codec.decode_views(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), arg, st.data_ptr(), stream())
            assert e.value.status == mi.BAD_ARGS
            import torch

            torch.cuda.synchronize()
            assert int(st.item()) == 0x77
            for o in outs:
                assert (o.read()[1].view(np.uint8) == 0x5A).all()

        for name, groups in cases.items():
            for host in (False, True):
                outs = [TOut(max(1, len(g.views)), max(1, g.ow), max(1, g.oh), c, g.dtype, g.layout, status=0x77) for g in groups]
                refused(groups, outs, host)
        # a formatted output that is not aligned to its element size; a NULL output
        for host in (False, True):
            groups = [G(good, 32, 32), G(good, 16, 16, "float32", "chw")]
            outs = [groups[0].out(c, status=0x77), groups[1].out(c, offset=2, status=0x77)]
            refused(groups, outs, host)
            outs = [groups[0].out(c, status=0x77), groups[1].out(c, status=0x77)]
            outs[1].ptr = 0
            refused(groups, outs, host)
        # a used frame without a container (the unused frame 1 may go without)
        groups = [G(good, 32, 32)]
        refused(groups, [groups[0].out(c, status=0x77)], True, [conts[0], None, None])
        st, outs = run_views(mi, codec, groups, c, conts=[conts[0], None, conts[2]])
        assert st == 0 and same_bits(outs[0], groups[0].expected(mi, imgs))
        # the limits themselves pass
        groups = [G([(1, 0, 0, 192, 64, 0), (1, 0, 0, 96, 10, bicubic)], 3, 1), G([(1, 0, 0, 10, 63, lanczos)], 3, 3)]
        st, outs = run_views(mi, codec, groups, c, dev=dev)
        assert st == 0 and all(same_bits(o, g.expected(mi, imgs)) for o, g in zip(outs, groups))
    finally:
        codec.close()
