"""Perspective views (llcomp_mi_codec_decode_perspective_views, ..._host, and the _photo_ forms): views of each frame under a projective
map, each frame decoded once and only where its views read.  Containers come from the oracle over noise; the expected output of a view is
llcomp_mi_perspective_reference -- the rule of include/llcomp_mi.h, compiled from the functions the kernel is compiled from -- of the
frame, mirrored, through llcomp_mi_output_table, bit for bit; and PIL's Image.transform(PERSPECTIVE) itself where PIL is installed."""
import math

import numpy as np
import pytest

import orc as orc_mod
from conftest import load_golden, make_image
from perspective_cases import coords, pil_perspective
from test_gpu_regions_host import Out, stream
from test_gpu_resized_output import TOut, norm, place, same_bits
from test_gpu_resized_regions import packed
from test_gpu_views import G as RectG, run_views
from test_gpu_warped_views import BICUBIC, BILINEAR, CODECS, FRAMES, H, NAMES, NEAREST, W, damaged, flag

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


def sensitive_vector():
    v = [v for v in load_golden("perspective_rule.json")["vectors"] if v.get("contraction_sensitive")][0]
    return v, np.array(v["image"], np.uint8).reshape(v["h"], v["w"]), [float.fromhex(t) for t in v["a"]]


_batches = {}


def batch(orc, c, tw, th, planar):
    """4 frames of 48 x 40 noise; the top left corner of frame 0 holds the image of the contraction-sensitive vector in every channel"""
    key = (c, tw, th, planar)
    if key not in _batches:
        imgs = np.stack([make_image("g3@%d" % (1200 + f), W, H, c) for f in range(FRAMES)])
        _, patch, _ = sensitive_vector()
        imgs[0, :patch.shape[0], :patch.shape[1], :] = patch[..., None]
        _batches[key] = imgs, [orc.compress_sliced(imgs[f], tw, th, planar) for f in range(FRAMES)]
    return _batches[key]


def quad(mi, ow, oh, cx, cy, hw, hh, deg=0.0, k=0.0, kv=0.0):
    """the eight numbers that send the ow x oh output onto a quadrilateral of the frame: the rectangle of half sides (hw, hh) around
    (cx, cy), its top edge shortened and its bottom edge lengthened by the fraction k (a keystone), its left and right edges by kv, all
    of it rotated by deg"""
    r = math.radians(deg)
    pts = []
    for sx, sy in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
        x, y = sx * hw * (1 + k * sy), sy * hh * (1 + kv * sx)
        pts.append((cx + x * math.cos(r) - y * math.sin(r), cy + x * math.sin(r) + y * math.cos(r)))
    return mi.perspective_coeffs(pts, [(0, 0), (ow, 0), (ow, oh), (0, oh)])


class PG:
    """a perspective group of a test: views (frame, a0..a7, flags), output shape, format, fill, chains"""

    def __init__(self, views, ow, oh, dtype="uint8", layout="hwc", fill=None, photo=None):
        self.views, self.ow, self.oh, self.dtype, self.layout, self.fill, self.photo = list(views), ow, oh, dtype, layout, fill, photo

    def out(self, c, status=0):
        return TOut(len(self.views), self.ow, self.oh, c, self.dtype, self.layout, 0, status)

    def fill_of(self, c):
        return None if self.fill is None else [(self.fill + 31 * ch) % 256 for ch in range(c)]

    def group(self, mi, c, ptr):
        plain = self.dtype == "uint8" and self.layout == "hwc"
        return mi.PerspectiveGroup(self.views, self.ow, self.oh, ptr, fill=self.fill_of(c), photo=self.photo,
                                   **({} if plain else dict(dtype=self.dtype, layout=self.layout, **norm(c, self.dtype))))

    def u8(self, imgs, one):
        """the u8 outputs [n, oh, ow, c]: one(frame image, a, filter name, ow, oh, fill) per view, then the mirror"""
        c = imgs.shape[-1]
        outs = []
        for v in self.views:
            o = one(imgs[v[0]], list(v[1:9]), NAMES[(v[9] >> 4) & 7], self.ow, self.oh, self.fill_of(c))
            outs.append(o[:, ::-1] if v[9] & 1 else o)
        return np.stack(outs)

    def expected(self, mi, imgs, one=None):
        c = imgs.shape[-1]
        u8 = self.u8(imgs, one or (lambda img, a, name, ow, oh, fill: mi.perspective_reference(img, a, name, ow, oh, fill)))
        if self.photo is not None:
            u8 = np.stack([mi.photo_reference(v, self.photo) for v in u8])
        return place(mi.output_table(c, self.dtype, **norm(c, self.dtype)), u8, self.layout)


KEYSTONE = (1.6, 0.1, 2.0, 0.05, 1.2, 3.0, 0.03, -0.015)  # den = 1 + 0.03 xs - 0.015 ys: 0.59 .. 2.09 over 37 x 29


def case_groups(mi):
    """One call: a keystone whose denominator runs over 0.59 .. 2.09, bilinear; a keystone and a rotation, bicubic; a NEAREST view with
    a6, a7 != 0; a NEAREST view with a6 = a7 = 0; the identity; the contraction-sensitive vector; a view half outside, with a fill per
    channel; a view wholly outside; two mirrored views -- on frames 0, 1 and 2 (frame 3 has no view) -- in 37 x 29 u8 HWC, and 1 x 1 and
    16 x 16 float16 CHW."""
    _, _, a_sens = sensitive_vector()
    a_aff = [float.fromhex(t) for v in load_golden("perspective_rule.json")["vectors"] if v.get("differs_from_affine") for t in v["a"]]
    a = PG([(0, *KEYSTONE, flag(BILINEAR)),
            (1, *quad(mi, 37, 29, 24, 20, 17, 13, deg=25, k=0.25), flag(BICUBIC)),
            (2, *quad(mi, 37, 29, 22, 21, 18, 15, deg=-12, k=-0.2, kv=0.15), flag(NEAREST)),
            (1, *a_aff, flag(NEAREST)),  # (a6 = a7 = 0: the golden vector on which PIL's PERSPECTIVE and AFFINE disagree)
            (0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, flag(BILINEAR)),
            (0, *a_sens, flag(NEAREST)),
            (2, *quad(mi, 37, 29, 44, 36, 14, 12, deg=10, k=0.2), flag(BICUBIC)),
            (0, 1.0, 0.1, 200.0, -0.1, 1.0, 7.0, 0.004, 0.002, flag(BILINEAR)),
            (1, *quad(mi, 37, 29, 28, 14, 16, 11, deg=70, k=0.3), flag(BILINEAR, True)),
            (2, *quad(mi, 37, 29, 20, 20, 22, 18, deg=180, kv=0.25), flag(NEAREST, True))], 37, 29, fill=200)
    b = PG([(1, *quad(mi, 1, 1, 46.5, 38.5, 1.5, 1.5, deg=200, k=0.1), flag(BICUBIC)), (2, 1.0, 0.0, 47.0, 0.0, 1.0, 39.0, 0.25, 0.5, flag(NEAREST))],
           1, 1, "float16", "chw", fill=7)
    c_ = PG([(0, *quad(mi, 16, 16, 12, 12, 11, 11, deg=45, k=0.3), flag(BICUBIC, True)), (2, *quad(mi, 16, 16, 24, 20, 19, 17, deg=-8, kv=-0.3), flag(BILINEAR)),
             (1, 2.0, 0.25, 1.0, 0.5, 2.0, 3.0, 0.01, 0.02, flag(NEAREST))], 16, 16, "float16", "chw")
    return [a, b, c_]


def run_persp(mi, codec, groups, c, dev=None, conts=None):
    outs = [g.out(c) for g in groups]
    arg = [g.group(mi, c, o.ptr) for g, o in zip(groups, outs)]
    st = outs[0].st
    if conts is not None:
        codec.decode_perspective_views_host(conts, arg, st.data_ptr(), stream())
    else:
        codec.decode_perspective_views(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), arg, st.data_ptr(), stream())
    got = [o.read() for o in outs]  # (read() checks the guard bytes on both sides of every output)
    return got[0][0], [g[1] for g in got]


def pil_one(Image):
    return lambda img, a, name, ow, oh, fill: pil_perspective(Image, img, a, name, ow, oh, np.array(fill if fill is not None else [0] * img.shape[-1]))


@pytest.mark.parametrize("case", CODECS, ids=[c[0] for c in CODECS])
def test_bytes_are_the_rule(mi, orc, case):
    name, c, tw, th, planar = case
    imgs, conts = batch(orc, c, tw, th, planar)
    groups = case_groups(mi)
    den, _, _ = coords(KEYSTONE, 37, 29)
    assert den.min() <= 0.6 and den.max() >= 1.6
    uni, win, n_used, n_cls = mi.perspective_views_plan(W, H, c, tw, th, planar, FRAMES, [(g.views, g.ow, g.oh) for g in groups])
    assert n_used == 3 and not uni[3].any()
    want = [g.expected(mi, imgs) for g in groups]
    # the vector a fused multiply-add changes: one pixel of view 5, every channel -- the ramp's column 2, not column 1
    vec, _, _ = sensitive_vector()
    px, py = vec["pixel"]
    assert (want[0][5, py, px] == vec["nearest"][py * 8 + px]).all() and vec["nearest"][py * 8 + px] != vec["nearest_fused"][py * 8 + px]
    assert (want[0][7] == np.array(groups[0].fill_of(c), np.uint8)).all()  # the view wholly outside
    assert np.array_equal(want[0][4], imgs[0, :29, :37])  # the identity
    half = (want[0][6] == np.array(groups[0].fill_of(c), np.uint8)).all(axis=-1).mean()
    assert 0.2 < half < 0.8  # the view half outside
    # a6 = a7 = 0 under NEAREST is not the affine call's fixed-point path
    v3 = groups[0].views[3]
    assert v3[7] == 0.0 and v3[8] == 0.0 and not np.array_equal(want[0][3], mi.warp_reference(imgs[1], v3[1:7], "nearest", 37, 29, groups[0].fill_of(c)))
    # frame 3 has no view: its container is damaged in every slice, and never read
    n = len(orc_mod.slice_rects(W, H, c, tw, th, planar))
    bad = damaged(orc, conts, c, tw, th, planar, [(3, j) for j in range(n)])
    codec = mi.Codec(FRAMES, W, H, c, tw, th, planar, device=0)
    try:
        st, outs = run_persp(mi, codec, groups, c, dev=packed(mi, bad))
        assert st == 0
        for g, out, exp in zip(groups, outs, want):
            assert same_bits(out, exp), (name, g.dtype, g.layout, np.argwhere(out.view(np.uint8) != exp.view(np.uint8))[:4].tolist())
        # the host form: the same bytes and status, with the damaged container, and without one
        for last in (bad[3], None):
            st_h, outs_h = run_persp(mi, codec, groups, c, conts=list(conts[:3]) + [last])
            assert st_h == 0 and all(same_bits(a, b) for a, b in zip(outs_h, want)), name
        assert codec.allocated_bytes() <= codec.perspective_workspace_bytes(sum(len(g.views) for g in groups))
    finally:
        codec.close()


@pytest.mark.parametrize("case", CODECS, ids=[c[0] for c in CODECS])
def test_the_rule_is_pil(mi, orc, case):
    """the same comparison against Image.transform itself: what the GPU test above expects is what PIL gives"""
    Image = pytest.importorskip("PIL.Image")
    name, c, tw, th, planar = case
    imgs, conts = batch(orc, c, tw, th, planar)
    groups = case_groups(mi)
    codec = mi.Codec(FRAMES, W, H, c, tw, th, planar, device=0)
    try:
        st, outs = run_persp(mi, codec, groups, c, dev=packed(mi, conts))
        assert st == 0
        for g, out in zip(groups, outs):
            assert same_bits(out, g.expected(mi, imgs, pil_one(Image))), (name, g.dtype, g.layout)
    finally:
        codec.close()


def small_groups(mi):
    """small views around (8, 8) of frames 0 and 1: the unions stay inside the first 2 x 2 of the 3 x 3 tiles"""
    return [PG([(0, *quad(mi, 8, 8, 8, 8, 3.5, 3.5, deg=25, k=0.2), flag(BILINEAR)), (1, *quad(mi, 8, 8, 7, 9, 3.5, 3.0, deg=-40, kv=0.2), flag(BICUBIC))],
               8, 8, fill=1)]


def test_damage_is_seen_where_the_views_call_sees_it(mi, orc):
    name, c, tw, th, planar = CODECS[0]  # 3 x 3 tiles, interleaved: slice id = tile row * 3 + tile column
    imgs, conts = batch(orc, c, tw, th, planar)
    groups = small_groups(mi)
    uni, win, n_used, _ = mi.perspective_views_plan(W, H, c, tw, th, planar, FRAMES, [(g.views, g.ow, g.oh) for g in groups])
    assert n_used == 2 and win[0].tolist() == win[1].tolist() == [0, 0, 2, 2] and (uni[:2, 0] + uni[:2, 2] <= 16).all() and (uni[:2, 1] + uni[:2, 3] <= 16).all()
    codec = mi.Codec(FRAMES, W, H, c, tw, th, planar, device=0)
    try:
        want = [g.expected(mi, imgs) for g in groups]
        # frame 1, tile row 1, column 1: inside its union's window, outside every view -- the verdict of the views call on the unions
        bad = damaged(orc, conts, c, tw, th, planar, [(1, 4)])
        rect = [RectG([(f, *[int(v) for v in uni[f]], 0)], int(uni[f][2]), int(uni[f][3])) for f in (0, 1)]
        st_ref, _ = run_views(mi, codec, rect, c, dev=packed(mi, bad))
        assert codec.status(st_ref) == mi.BAD_EXPONENT
        st, _ = run_persp(mi, codec, groups, c, dev=packed(mi, bad))
        st_h, _ = run_persp(mi, codec, groups, c, conts=bad)
        assert st == st_h == st_ref
        # outside every window (the third tile column and row, and the unused frames): not seen, exact
        bad = damaged(orc, conts, c, tw, th, planar, [(0, 2), (0, 5), (1, 6), (1, 8), (2, 0), (3, 4)])
        for kw in (dict(dev=packed(mi, bad)), dict(conts=bad)):
            st, outs = run_persp(mi, codec, groups, c, **kw)
            assert st == 0 and all(same_bits(o, e) for o, e in zip(outs, want))
        # every view all fill: nothing is decoded or staged, no container is needed
        codec.counters(reset=True)
        none = [PG([(1, 1.0, 0.0, 500.0, 0.0, 1.0, 0.0, 0.01, 0.0, flag(BICUBIC)), (3, 0.5, 0.5, -900.0, 0.5, 0.5, 0.0, 0.0, 0.02, flag(NEAREST))], 9, 7, fill=33)]
        for kw in (dict(conts=[None] * FRAMES), dict(dev=packed(mi, conts))):
            st, outs = run_persp(mi, codec, none, c, **kw)
            assert st == 0 and (outs[0] == np.array(none[0].fill_of(c), np.uint8)).all()
        assert codec.counters()["host_staged_bytes"] == 0
        assert codec.allocated_bytes() <= codec.perspective_workspace_bytes(2)
    finally:
        codec.close()


def test_no_collateral_and_bad_args(mi, orc):
    import torch

    name, c, tw, th, planar = CODECS[1]
    imgs, conts = batch(orc, c, tw, th, planar)
    dev = packed(mi, conts)
    rect = [RectG([(0, 3, 2, 30, 25, 0), (2, 10, 10, 38, 30, (4 << 4) | 1)], 20, 15), RectG([(2, 0, 0, 48, 40, 5 << 4)], 12, 10, "float32", "chw")]
    codec = mi.Codec(FRAMES, W, H, c, tw, th, planar, device=0)
    try:
        st0, before = run_views(mi, codec, rect, c, dev=dev)
        assert st0 == 0 and all(same_bits(o, g.expected(mi, imgs)) for o, g in zip(before, rect))
        groups = case_groups(mi)
        st, outs = run_persp(mi, codec, groups, c, dev=dev)
        assert st == 0 and all(same_bits(o, g.expected(mi, imgs)) for o, g in zip(outs, groups))
        # refusals: before anything is queued, the status word and the outputs untouched
        good = (0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0)
        cases = {
            "no groups": [],
            "a group with no views": [PG([good], 8, 8), PG([], 8, 8)],
            "frame >= frames": [PG([good, (4, *good[1:])], 8, 8)],
            "nan": [PG([good, (1, 1.0, 0.0, float("nan"), 0.0, 1.0, 0.0, 0.0, 0.0, 0)], 8, 8)],
            "inf a7": [PG([good], 8, 8), PG([(1, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, float("inf"), flag(NEAREST))], 8, 8, "float16", "chw")],
            "den 0 at a corner": [PG([good, (1, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -0.125, -0.125, flag(BILINEAR))], 8, 1)],
            "den < 0 at the last corner": [PG([(1, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -0.07, -0.07, flag(NEAREST))], 8, 8)],
            "den < 0 at the first corner": [PG([(2, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, -3.0, 0.5, flag(BICUBIC))], 8, 8)],
            "beyond 2^30": [PG([(1, 1.0, 0.0, 2.0 ** 30, 0.0, 1.0, 0.0, 0.0, 0.0, flag(BICUBIC))], 8, 8)],
            "box filter": [PG([good, (1, *good[1:9], 2 << 4)], 8, 8)],
            "ow 0": [PG([good], 0, 8)],
        }

        def call(host, arg, n, stw):
            if host:
                codec.decode_perspective_views_host(conts, arg, stw.data_ptr(), stream())
            else:
                codec.decode_perspective_views(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), arg, stw.data_ptr(), stream())

        for label, bad in cases.items():
            for host in (False, True):
                outs = [TOut(max(1, len(g.views)), max(1, g.ow), max(1, g.oh), c, g.dtype, g.layout, status=0x77) for g in bad]
                stw = outs[0].st if outs else Out(1, 1, 1, 1, status=0x77).st
                arg = [g.group(mi, c, o.ptr) for g, o in zip(bad, outs)]
                with pytest.raises(mi.LlcompError) as e:
                    call(host, arg, len(arg), stw)
                assert e.value.status == mi.BAD_ARGS, label
                torch.cuda.synchronize()
                assert int(stw.item()) == 0x77, label
                for o in outs:
                    assert (o.read()[1].view(np.uint8) == 0x5A).all(), label
        # a NULL d_out in the second group, and a struct_size that is not the struct's: through the C entry points themselves
        from llcomp_amd import _warp_groups

        two = [PG([good], 8, 8), PG([good], 8, 8, "float16", "chw")]
        outs = [TOut(1, 8, 8, c, g.dtype, g.layout, status=0x77) for g in two]
        ptrs, lens, _keep_c = mi._frame_containers(conts, FRAMES, allow_none=True)
        for label in ("NULL d_out", "struct_size - 8", "struct_size + 8"):
            arr, n, _keep = _warp_groups([g.group(mi, c, o.ptr) for g, o in zip(two, outs)], c, persp=True)
            if label == "NULL d_out":
                arr[1].d_out = None
            else:
                arr[0].struct_size += 8 if label.endswith("+ 8") else -8
            L, stw = codec._L, outs[0].st
            assert L.llcomp_mi_codec_decode_perspective_views(codec._h, dev[0].data_ptr(), dev[1], dev[2].data_ptr(), arr, n, stw.data_ptr(), stream()) == mi.BAD_ARGS, label
            assert L.llcomp_mi_codec_decode_perspective_views_host(codec._h, ptrs, lens, arr, n, stw.data_ptr(), stream()) == mi.BAD_ARGS, label
            assert L.llcomp_mi_codec_decode_photo_perspective_views(codec._h, dev[0].data_ptr(), dev[1], dev[2].data_ptr(), arr, n, None, stw.data_ptr(), stream()) == mi.BAD_ARGS, label
            torch.cuda.synchronize()
            assert int(stw.item()) == 0x77, label
            for o in outs:
                assert (o.read()[1].view(np.uint8) == 0x5A).all(), label
        # a used frame without a container
        with pytest.raises(mi.LlcompError):
            o = groups[0].out(c)
            codec.decode_perspective_views_host([None] + list(conts[1:]), [groups[0].group(mi, c, o.ptr)], o.st.data_ptr(), stream())
        st1, after = run_views(mi, codec, rect, c, dev=dev)
        assert st1 == 0 and all(same_bits(a, b) for a, b in zip(before, after))
        assert codec.allocated_bytes() <= codec.perspective_workspace_bytes(sum(len(g.views) for g in groups))
    finally:
        codec.close()


def test_photo_chain_on_perspective_groups(mi, orc):
    """brightness then equalize behind the gather: photo_reference on perspective_reference (mirrored), in u8 HWC and float16 CHW, beside
    a group without a chain; the device and the host form"""
    name, c, tw, th, planar = CODECS[0]
    imgs, conts = batch(orc, c, tw, th, planar)
    chain = [("brightness", 1.3), "equalize"]
    full = case_groups(mi)
    groups = [PG(full[0].views, 37, 29, fill=200, photo=chain), PG(full[2].views, 16, 16, "float16", "chw", photo=chain), PG(full[0].views[:3], 20, 12, fill=3)]
    total = sum(len(g.views) for g in groups)
    codec = mi.Codec(FRAMES, W, H, c, tw, th, planar, device=0)
    try:
        want = [g.expected(mi, imgs) for g in groups]
        plain = PG(full[0].views, 37, 29, fill=200).expected(mi, imgs)
        assert not np.array_equal(want[0], plain)  # (the chain does something)
        for kw in (dict(dev=packed(mi, conts)), dict(conts=list(conts[:3]) + [None])):
            st, outs = run_persp(mi, codec, groups, c, **kw)
            assert st == 0
            for g, out, exp in zip(groups, outs, want):
                assert same_bits(out, exp), (g.dtype, g.layout, np.argwhere(out.view(np.uint8) != exp.view(np.uint8))[:4].tolist())
        assert codec.allocated_bytes() <= codec.perspective_workspace_bytes(total, photo=True)
    finally:
        codec.close()
