"""What the GPU tests of the photometric chains share (test_gpu_photo_views.py, test_gpu_photo_area.py, test_gpu_photo_sharpness.py): the
geometries with their batches and codecs, made once and closed by each module's last test; a group of a test and the call that runs a
list of them; and the way of checking -- the expected bytes of a view are tests/photo_spec.py, the rule restated with numpy, applied to
what the existing call writes for the same view as U8 HWC (those bytes are pinned to the oracle and to PIL by the existing tests), then
llcomp_mi_output_table for a formatted group, bit for bit."""
import numpy as np
import pytest

import photo_spec
import resize_filters_spec as spec
from test_gpu_regions_host import make_batch, stream
from test_gpu_resized_output import TOut, norm, place, same_bits
from test_gpu_resized_regions import packed

FRAMES, W = 3, 100
# the two geometries of test_gpu_windows_mixed.py, and the first with one channel: (c, h, tile_w, tile_h, planar)
GEOS = {"100x44_32x16i_c3": (3, 44, 32, 16, False), "100x6_50x1p_c3": (3, 6, 50, 1, True), "100x44_32x16i_c1": (1, 44, 32, 16, False)}


def flag(filt, mirror=False):
    return (filt << 4) | (1 if mirror else 0)


def views_of(h, small=False):
    """five views of frames 0 and 2 (frame 1 has none), every one under a filter of its own, two mirrored; small: rectangles that a 1 x 1
    output may take under every filter's downscale limit"""
    if small:
        return [(0, 5, 1, 20, min(h - 1, 12), flag(spec.BILINEAR)), (2, 96, 2, 4, 4, flag(spec.NEAREST, True)), (2, 50, 0, 9, 5, flag(spec.LANCZOS))]
    if h == 6:
        return [(0, 5, 1, 60, 4, flag(spec.BILINEAR)), (2, 50, 2, 50, 4, flag(spec.BOX, True)), (0, 40, 0, 30, 5, flag(spec.LANCZOS)),
                (2, 0, 0, 100, 6, flag(spec.HAMMING, True)), (2, 96, 2, 4, 4, flag(spec.NEAREST))]
    return [(0, 5, 3, 60, 30, flag(spec.BILINEAR)), (2, 50, 20, 50, 24, flag(spec.BOX, True)), (0, 40, 10, 30, 20, flag(spec.LANCZOS)),
            (2, 0, 0, 100, 44, flag(spec.HAMMING, True)), (2, 96, 40, 4, 4, flag(spec.NEAREST))]


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


_state = {}


def setup(mi, orc, name):
    """(c, h, imgs, containers, the batch in HBM, codec) of a geometry, made once"""
    if name not in _state:
        c, h, tw, th, planar = GEOS[name]
        imgs, conts = make_batch(orc, FRAMES, W, h, c, tw, th, planar)
        _state[name] = (c, h, imgs, conts, packed(mi, conts), mi.Codec(FRAMES, W, h, c, tw, th, planar, device=0))
    return _state[name]


def close_shared_codecs():
    """every module's last test: what setup() opened is closed"""
    for s in _state.values():
        s[5].close()
    _state.clear()


class PG:
    """a group of a test: rectangle views (frame, x, y, rw, rh, flags) or, warp=True, affine views (frame, m0..m5, flags); photo: None, one
    chain, or one chain per view"""

    def __init__(self, views, ow, oh, photo=None, dtype="uint8", layout="hwc", warp=False, fill=None):
        self.views, self.ow, self.oh, self.photo, self.dtype, self.layout, self.warp, self.fill = list(views), ow, oh, photo, dtype, layout, warp, fill

    def chains(self):
        if self.photo is None:
            return [[]] * len(self.views)
        per_view = len(self.photo) == len(self.views) and all(isinstance(ch, list) for ch in self.photo)
        return list(self.photo) if per_view else [self.photo] * len(self.views)

    def group(self, mi, c, ptr, plain=False):
        """plain: the same views as U8 HWC without chains -- what the existing calls take"""
        fmt = {} if plain or (self.dtype == "uint8" and self.layout == "hwc") else dict(dtype=self.dtype, layout=self.layout, **norm(c, self.dtype))
        kw = {} if plain or self.photo is None else dict(photo=self.photo)
        if self.warp:
            return mi.WarpGroup(self.views, self.ow, self.oh, ptr, fill=self.fill, **fmt, **kw)
        return mi.ViewGroup(self.views, self.ow, self.oh, ptr, **fmt, **kw)


def run(mi, codec, groups, c, dev=None, conts=None, plain=False, pad_mode=None, read=True):
    outs = [TOut(len(g.views), g.ow, g.oh, c, "uint8" if plain else g.dtype, "hwc" if plain else g.layout) for g in groups]
    arg = [g.group(mi, c, o.ptr, plain) for g, o in zip(groups, outs)]
    st = outs[0].st.data_ptr()
    kw = dict(pad_mode=pad_mode) if pad_mode else {}
    if groups[0].warp:
        if conts is not None:
            codec.decode_warped_views_host(conts, arg, st, stream())
        else:
            codec.decode_warped_views(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), arg, st, stream())
    elif conts is not None:
        codec.decode_views_host(conts, arg, st, stream(), **kw)
    else:
        codec.decode_views(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), arg, st, stream(), **kw)
    if not read:
        return outs
    got = [o.read() for o in outs]
    return got[0][0], [g[1] for g in got]


def expected(mi, groups, plain_outs, c):
    want = []
    for g, u8 in zip(groups, plain_outs):
        v = np.stack([photo_spec.apply(u8[i], ch) for i, ch in enumerate(g.chains())])
        want.append(place(mi.output_table(c, g.dtype, **norm(c, g.dtype)), v, g.layout))
    return want


def check(mi, codec, groups, c, dev, pad_mode=None, conts=None):
    """the call with chains against photo_spec over the existing call's U8 HWC output; conts: the _host form.  Returns (outputs, the
    plain outputs)"""
    st0, plain = run(mi, codec, groups, c, dev=dev, plain=True, pad_mode=pad_mode)
    st, outs = run(mi, codec, groups, c, dev=None if conts is not None else dev, conts=conts, pad_mode=pad_mode)
    assert st == st0 == 0
    for i, (out, exp) in enumerate(zip(outs, expected(mi, groups, plain, c))):
        assert same_bits(out, exp), (i, np.argwhere(out != exp)[:4].tolist())
    return outs, plain
