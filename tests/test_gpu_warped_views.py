"""Warped views (llcomp_mi_codec_decode_warped_views, ..._host): views of each frame under an affine map, each frame decoded once and only
where its views read.  Containers come from the oracle over noise; the expected output of a view is llcomp_mi_warp_reference -- the rule
of include/llcomp_mi.h, compiled from the functions the kernel is compiled from -- of the frame, mirrored, through llcomp_mi_output_table,
bit for bit; and PIL's Image.transform(AFFINE) itself where PIL is installed."""
import math

import numpy as np
import pytest

import orc as orc_mod
from conftest import load_golden, make_image
from test_gpu_regions_host import Out, stream
from test_gpu_resized_output import TOut, norm, place, same_bits
from test_gpu_resized_regions import packed
from test_gpu_views import G as RectG, run_views

pytestmark = pytest.mark.gpu

FRAMES, W, H = 4, 48, 40
NEAREST, BILINEAR, BICUBIC = 1, 0, 4
NAMES = {NEAREST: "nearest", BILINEAR: "bilinear", BICUBIC: "bicubic"}
# (name, c, tile_w, tile_h, planar): the 2-D family, the row family, and c = 1, 4 and 5 (the generic loop) once each
CODECS = [("tiles_16x16i_c3", 3, 16, 16, False), ("rows_16x1p_c3", 3, 16, 1, True), ("tiles_16x16i_c1", 1, 16, 16, False),
          ("tiles_16x16i_c4", 4, 16, 16, False), ("tiles_16x16i_c5", 5, 16, 16, False)]


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


def sensitive_vector():
    v = [v for v in load_golden("warp_rule.json")["vectors"] if v.get("contraction_sensitive")][0]
    return v, np.array(v["image"], np.uint8).reshape(v["h"], v["w"]), [float.fromhex(t) for t in v["m"]]


_batches = {}


def batch(orc, c, tw, th, planar):
    """4 frames of 48 x 40 noise; the top left corner of frame 0 holds the image of the contraction-sensitive vector in every channel"""
    key = (c, tw, th, planar)
    if key not in _batches:
        imgs = np.stack([make_image("g3@%d" % (900 + f), W, H, c) for f in range(FRAMES)])
        _, patch, _ = sensitive_vector()
        imgs[0, :patch.shape[0], :patch.shape[1], :] = patch[..., None]
        _batches[key] = imgs, [orc.compress_sliced(imgs[f], tw, th, planar) for f in range(FRAMES)]
    return _batches[key]


def flag(filt, mirror=False):
    return (filt << 4) | (1 if mirror else 0)


def rot(deg, cx, cy, ox, oy, s=1.0):
    """output pixel centre (ox, oy) reads (cx, cy); rotated by deg and scaled by s around it"""
    a = math.radians(deg)
    m = [s * math.cos(a), s * math.sin(a), 0.0, -s * math.sin(a), s * math.cos(a), 0.0]
    m[2] = cx - (m[0] * ox + m[1] * oy)
    m[5] = cy - (m[3] * ox + m[4] * oy)
    return m


class WG:
    """a warp group of a test: views (frame, m0..m5, flags), output shape, format, fill"""

    def __init__(self, views, ow, oh, dtype="uint8", layout="hwc", fill=None):
        self.views, self.ow, self.oh, self.dtype, self.layout, self.fill = list(views), ow, oh, dtype, layout, fill

    def out(self, c, status=0):
        return TOut(len(self.views), self.ow, self.oh, c, self.dtype, self.layout, 0, status)

    def fill_of(self, c):
        return None if self.fill is None else [(self.fill + 31 * ch) % 256 for ch in range(c)]

    def group(self, mi, c, ptr):
        plain = self.dtype == "uint8" and self.layout == "hwc"
        return mi.WarpGroup(self.views, self.ow, self.oh, ptr, fill=self.fill_of(c),
                            **({} if plain else dict(dtype=self.dtype, layout=self.layout, **norm(c, self.dtype))))

    def u8(self, imgs, one):
        """the u8 outputs [n, oh, ow, c]: one(frame image, m, filter name, ow, oh, fill) per view, then the mirror"""
        c = imgs.shape[-1]
        outs = []
        for v in self.views:
            o = one(imgs[v[0]], list(v[1:7]), NAMES[(v[7] >> 4) & 7], self.ow, self.oh, self.fill_of(c))
            outs.append(o[:, ::-1] if v[7] & 1 else o)
        return np.stack(outs)

    def expected(self, mi, imgs, one=None):
        c = imgs.shape[-1]
        u8 = self.u8(imgs, one or (lambda img, m, name, ow, oh, fill: mi.warp_reference(img, m, name, ow, oh, fill)))
        return place(mi.output_table(c, self.dtype, **norm(c, self.dtype)), u8, self.layout)


def case_groups():
    """One call: a 30 degree rotation, bilinear; a shear, bicubic; a rotation, nearest (the fixed-point form); a scale and translate,
    nearest (the table form); the identity; the contraction-sensitive vector; a view half outside, with a fill per channel; a view wholly
    outside; a mirrored view -- on frames 0, 1 and 2 (frame 3 has no view) -- in 37 x 29 u8 HWC, and 1 x 1 and 16 x 16 float16 CHW."""
    _, _, m_sens = sensitive_vector()
    a = WG([(0, *rot(30, 24, 20, 18.5, 14.5), flag(BILINEAR)),
            (1, 1.0, 0.35, -3.0, 0.15, 0.9, 2.0, flag(BICUBIC)),
            (2, *rot(-50, 20, 22, 18.5, 14.5, 0.8), flag(NEAREST)),
            (1, 0.75, 0.0, 5.25, 0.0, 1.3, -2.5, flag(NEAREST)),
            (0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, flag(BILINEAR)),
            (0, *m_sens, flag(BILINEAR)),
            (2, *rot(12, 40, 35, 10.0, 8.0), flag(BICUBIC)),
            (0, 1.0, 0.1, 200.0, -0.1, 1.0, 7.0, flag(BILINEAR)),
            (1, *rot(75, 30, 12, 18.5, 14.5, 1.2), flag(BILINEAR, True)),
            (2, -1.1, 0.0, 50.0, 0.0, 0.9, 3.0, flag(NEAREST, True))], 37, 29, fill=200)
    b = WG([(1, *rot(200, 47, 39, 0.5, 0.5), flag(BICUBIC)), (2, 1.0, 0.0, 47.0, 0.0, 1.0, 39.0, flag(NEAREST))], 1, 1, "float16", "chw", fill=7)
    c_ = WG([(0, *rot(45, 10, 10, 8.0, 8.0, 1.5), flag(BICUBIC, True)), (2, *rot(-8, 24, 20, 8.0, 8.0, 2.4), flag(BILINEAR)),
             (1, 2.0, 0.25, 1.0, 0.5, 2.0, 3.0, flag(NEAREST))], 16, 16, "float16", "chw")
    return [a, b, c_]


def run_warp(mi, codec, groups, c, dev=None, conts=None):
    outs = [g.out(c) for g in groups]
    arg = [g.group(mi, c, o.ptr) for g, o in zip(groups, outs)]
    st = outs[0].st
    if conts is not None:
        codec.decode_warped_views_host(conts, arg, st.data_ptr(), stream())
    else:
        codec.decode_warped_views(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), arg, st.data_ptr(), stream())
    got = [o.read() for o in outs]
    return got[0][0], [g[1] for g in got]


def damaged(orc, clean, c, tw, th, planar, spots, seed=79):
    """the containers with the payloads of slices `spots` = [(frame, slice id)] replaced by streams that end in a bad exponent"""
    rects = orc_mod.slice_rects(W, H, c, tw, th, planar)
    n = len(rects)
    rng = np.random.default_rng(seed)
    conts = []
    for f, d in enumerate(clean):
        lens = np.frombuffer(d[24:24 + 4 * n], dtype="<u4").astype(np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)]) + 24 + 4 * n
        pays = [d[offs[j]:offs[j + 1]] for j in range(n)]
        for ff, j in spots:
            if ff == f:
                _, _, sw, sh, plane = rects[j]
                sc = 1 if plane is not None else c
                res = orc_mod.adversarial_residuals(rng, sh, sw, sc, "small")
                pays[j] = orc.encode_residuals(res, run_at=sh * sw * sc // 2, run_len=33)[0]
        conts.append(orc_mod.sliced_container(W, H, c, tw, th, planar, pays))
    return conts


def pil_one(Image):
    from test_warp_rule import pil_warp

    return lambda img, m, name, ow, oh, fill: pil_warp(Image, img, m, name, ow, oh, np.array(fill if fill is not None else [0] * img.shape[-1]))


@pytest.mark.parametrize("case", CODECS, ids=[c[0] for c in CODECS])
def test_bytes_are_the_rule(mi, orc, case):
    name, c, tw, th, planar = case
    imgs, conts = batch(orc, c, tw, th, planar)
    groups = case_groups()
    plan_groups = [(g.views, g.ow, g.oh) for g in groups]
    uni, win, n_used, n_cls = mi.warp_views_plan(W, H, c, tw, th, planar, FRAMES, plan_groups)
    assert n_used == 3 and not uni[3].any() and uni[0].tolist() == [0, 0, W, H]  # (frame 0: the rotation reads to every edge)
    want = [g.expected(mi, imgs) for g in groups]
    # the vector a fused multiply-add changes: output pixel (0, 0) of view 5, every channel
    vec, _, _ = sensitive_vector()
    assert (want[0][5, 0, 0] == vec["bilinear"][0]).all() and vec["bilinear"][0] != vec["bilinear_fused"][0]
    assert (want[0][7] == np.array(groups[0].fill_of(c), np.uint8)).all()  # the view wholly outside
    assert np.array_equal(want[0][4], imgs[0, :29, :37])  # the identity
    # frame 3 has no view: its container is damaged in every slice, and never read
    n = len(orc_mod.slice_rects(W, H, c, tw, th, planar))
    bad = damaged(orc, conts, c, tw, th, planar, [(3, j) for j in range(n)])
    codec = mi.Codec(FRAMES, W, H, c, tw, th, planar, device=0)
    try:
        st, outs = run_warp(mi, codec, groups, c, dev=packed(mi, bad))
        assert st == 0
        for g, out, exp in zip(groups, outs, want):
            assert same_bits(out, exp), (name, g.dtype, g.layout, np.argwhere(out.view(np.uint8) != exp.view(np.uint8))[:4].tolist())
        # the host form: the same bytes and status, with the damaged container, and without one
        for last in (bad[3], None):
            st_h, outs_h = run_warp(mi, codec, groups, c, conts=list(conts[:3]) + [last])
            assert st_h == 0 and all(same_bits(a, b) for a, b in zip(outs_h, want)), name
        assert codec.allocated_bytes() <= codec.warp_workspace_bytes(sum(len(g.views) for g in groups))
    finally:
        codec.close()


@pytest.mark.parametrize("case", CODECS, ids=[c[0] for c in CODECS])
def test_the_rule_is_pil(mi, orc, case):
    """the same comparison against Image.transform itself: what the GPU test above expects is what PIL gives"""
    Image = pytest.importorskip("PIL.Image")
    name, c, tw, th, planar = case
    imgs, conts = batch(orc, c, tw, th, planar)
    groups = case_groups()
    codec = mi.Codec(FRAMES, W, H, c, tw, th, planar, device=0)
    try:
        st, outs = run_warp(mi, codec, groups, c, dev=packed(mi, conts))
        assert st == 0
        for g, out in zip(groups, outs):
            assert same_bits(out, g.expected(mi, imgs, pil_one(Image))), (name, g.dtype, g.layout)
    finally:
        codec.close()


def test_host_form_stages_the_unions_windows(mi, orc):
    name, c, tw, th, planar = CODECS[0]
    imgs, conts = batch(orc, c, tw, th, planar)
    # small views: the unions are parts of the frames
    groups = [WG([(0, *rot(20, 10, 9, 5.5, 5.5, 0.6), flag(BILINEAR)), (2, *rot(-35, 36, 30, 5.5, 5.5, 0.6), flag(BICUBIC, True)),
                  (0, 0.5, 0.0, 6.0, 0.0, 0.5, 5.0, flag(NEAREST))], 12, 12, fill=9),
              WG([(2, *rot(64, 36, 30, 3.5, 3.5, 0.7), flag(NEAREST))], 8, 8, "float16", "chw")]
    uni, win, n_used, _ = mi.warp_views_plan(W, H, c, tw, th, planar, FRAMES, [(g.views, g.ow, g.oh) for g in groups])
    # two used frames, and windows of 2 x 2 of the 3 x 3 tiles: frame 2's in the last corner, with the partial last tile row
    assert n_used == 2 and not uni[1].any() and not uni[3].any() and win[0].tolist() == [0, 0, 2, 2] and win[2].tolist() == [1, 1, 3, 3]
    codec = mi.Codec(FRAMES, W, H, c, tw, th, planar, device=0)
    try:
        want = [g.expected(mi, imgs) for g in groups]
        st_d, outs_d = run_warp(mi, codec, groups, c, dev=packed(mi, conts))
        codec.counters(reset=True)
        codec.get_profile()
        st_h, outs_h = run_warp(mi, codec, groups, c, conts=[conts[0], None, conts[2], None])
        assert st_d == st_h == 0
        assert all(same_bits(a, e) and same_bits(b, e) for a, b, e in zip(outs_d, outs_h, want))
        staged = codec.counters(reset=True)["host_staged_bytes"]
        assert codec.get_profile()[2] == 1  # one decode, whatever the number of views
        # ... what decode_views_host stages for the unions
        rect = [RectG([(f, *[int(v) for v in uni[f]], 0)], int(uni[f][2]), int(uni[f][3])) for f in (0, 2)]
        st, _ = run_views(mi, codec, rect, c, conts=[conts[0], None, conts[2], None])
        assert st == 0 and staged == codec.counters(reset=True)["host_staged_bytes"] > 0
        # every view all fill: nothing is decoded or staged, no container is needed
        none = [WG([(1, 1.0, 0.0, 500.0, 0.0, 1.0, 0.0, flag(BICUBIC)), (3, 0.5, 0.5, -900.0, 0.5, 0.5, 0.0, flag(NEAREST))], 9, 7, fill=33)]
        for kw in (dict(conts=[None] * FRAMES), dict(dev=packed(mi, conts))):
            st, outs = run_warp(mi, codec, none, c, **kw)
            assert st == 0 and (outs[0] == np.array(none[0].fill_of(c), np.uint8)).all()
        assert codec.counters()["host_staged_bytes"] == 0
        assert codec.allocated_bytes() <= codec.warp_workspace_bytes(4)
    finally:
        codec.close()


def test_damage_is_seen_where_the_views_call_sees_it(mi, orc):
    name, c, tw, th, planar = CODECS[0]  # 3 x 3 tiles, interleaved: slice id = tile row * 3 + tile column
    imgs, conts = batch(orc, c, tw, th, planar)
    groups = [WG([(0, *rot(25, 8, 8, 4.0, 4.0, 0.8), flag(BILINEAR)), (1, *rot(-40, 7, 9, 4.0, 4.0, 0.8), flag(BICUBIC))], 8, 8, fill=1)]
    uni, win, n_used, _ = mi.warp_views_plan(W, H, c, tw, th, planar, FRAMES, [(g.views, g.ow, g.oh) for g in groups])
    assert n_used == 2 and win[0].tolist() == win[1].tolist() == [0, 0, 2, 2] and (uni[:2, 0] + uni[:2, 2] <= 16).all() and (uni[:2, 1] + uni[:2, 3] <= 16).all()
    codec = mi.Codec(FRAMES, W, H, c, tw, th, planar, device=0)
    try:
        want = [g.expected(mi, imgs) for g in groups]
        # frame 1, tile row 1, column 1: inside its union's window, outside every view -- the verdict of the views call on the unions
        bad = damaged(orc, conts, c, tw, th, planar, [(1, 4)])
        rect = [RectG([(f, *[int(v) for v in uni[f]], 0)], int(uni[f][2]), int(uni[f][3])) for f in (0, 1)]
        st_ref, _ = run_views(mi, codec, rect, c, dev=packed(mi, bad))
        assert codec.status(st_ref) == mi.BAD_EXPONENT
        st, _ = run_warp(mi, codec, groups, c, dev=packed(mi, bad))
        st_h, _ = run_warp(mi, codec, groups, c, conts=bad)
        assert st == st_h == st_ref
        # outside every window (the third tile column and row, and the unused frames): not seen, exact
        bad = damaged(orc, conts, c, tw, th, planar, [(0, 2), (0, 5), (1, 6), (1, 8), (2, 0), (3, 4)])
        for kw in (dict(dev=packed(mi, bad)), dict(conts=bad)):
            st, outs = run_warp(mi, codec, groups, c, **kw)
            assert st == 0 and all(same_bits(o, e) for o, e in zip(outs, want))
    finally:
        codec.close()


def test_no_collateral_and_bad_args(mi, orc):
    name, c, tw, th, planar = CODECS[1]
    imgs, conts = batch(orc, c, tw, th, planar)
    dev = packed(mi, conts)
    rect = [RectG([(0, 3, 2, 30, 25, 0), (2, 10, 10, 38, 30, (4 << 4) | 1)], 20, 15), RectG([(2, 0, 0, 48, 40, 5 << 4)], 12, 10, "float32", "chw")]
    codec = mi.Codec(FRAMES, W, H, c, tw, th, planar, device=0)
    try:
        st0, before = run_views(mi, codec, rect, c, dev=dev)
        assert st0 == 0 and all(same_bits(o, g.expected(mi, imgs)) for o, g in zip(before, rect))
        groups = case_groups()
        st, outs = run_warp(mi, codec, groups, c, dev=dev)
        assert st == 0 and all(same_bits(o, g.expected(mi, imgs)) for o, g in zip(outs, groups))
        # refusals: before anything is queued, the status word and the outputs untouched
        good = (0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0)
        cases = {
            "no groups": [],
            "a group with no views": [WG([good], 8, 8), WG([], 8, 8)],
            "frame >= frames": [WG([good, (4, *good[1:])], 8, 8)],
            "nan": [WG([good, (1, 1.0, 0.0, float("nan"), 0.0, 1.0, 0.0, 0)], 8, 8)],
            "nearest beyond check_fixed": [WG([good], 8, 8), WG([(1, 1.0, 0.5, 0.0, 0.0, 5000.0, 0.0, flag(NEAREST))], 8, 8, "float16", "chw")],
            "bicubic beyond 2^30": [WG([(1, 1.0, 0.0, 2.0 ** 30, 0.0, 1.0, 0.0, flag(BICUBIC))], 8, 8)],
            "box filter": [WG([good, (1, *good[1:7], 2 << 4)], 8, 8)],
            "ow 0": [WG([good], 0, 8)],
        }
        import torch

        for label, bad in cases.items():
            for host in (False, True):
                outs = [TOut(max(1, len(g.views)), max(1, g.ow), max(1, g.oh), c, g.dtype, g.layout, status=0x77) for g in bad]
                stw = outs[0].st if outs else Out(1, 1, 1, 1, status=0x77).st
                arg = [g.group(mi, c, o.ptr) for g, o in zip(bad, outs)]
                with pytest.raises(mi.LlcompError) as e:
                    if host:
                        codec.decode_warped_views_host(conts, arg, stw.data_ptr(), stream())
                    else:
                        codec.decode_warped_views(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), arg, stw.data_ptr(), stream())
                assert e.value.status == mi.BAD_ARGS, label
                torch.cuda.synchronize()
                assert int(stw.item()) == 0x77, label
                for o in outs:
                    assert (o.read()[1].view(np.uint8) == 0x5A).all(), label
        # a used frame without a container
        with pytest.raises(mi.LlcompError):
            o = groups[0].out(c)
            codec.decode_warped_views_host([None] + list(conts[1:]), [groups[0].group(mi, c, o.ptr)], o.st.data_ptr(), stream())
        st1, after = run_views(mi, codec, rect, c, dev=dev)
        assert st1 == 0 and all(same_bits(a, b) for a, b in zip(before, after))
        assert codec.allocated_bytes() <= codec.warp_workspace_bytes(sum(len(g.views) for g in groups))
    finally:
        codec.close()
