"""Every decode entry point through ONE codec on one stream with no synchronisation in between: ten calls -- nine uses of the four-slot
pinned ring, so it wraps twice, and the first host call grows d_stage while earlier work is still queued -- each byte for byte what the
same call gives alone on a fresh codec (those single calls are what the other GPU tests pin to the oracle and to the PIL golden), every
status word 0, and the codec's device memory within views_workspace_bytes."""
import numpy as np
import pytest

import resize_filters_spec as spec
from test_gpu_regions_host import Out, make_batch, stream
from test_gpu_resized_output import TOut, norm, same_bits
from test_gpu_resized_regions import packed
from test_gpu_views import flag

pytestmark = pytest.mark.gpu

FRAMES, W, C = 3, 100, 3


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


# 3 frames of 100 x 44 x 3 in 32 x 16 tiles, interleaved: partial last tile column and row, so the windows fall into several classes;
# 3 frames of 100 x 6 x 3 in 50 x 1 tiles, planar: the fused row path (whole tiles: one class).  Per geometry the rectangles of the calls:
GEOMETRIES = {
    "100x44_32x16i": dict(
        h=44, tw=32, th=16, planar=False,
        regions=([(0, 0), (60, 24), (30, 10)], 40, 20), regions_again=([(59, 0), (0, 23), (59, 23)], 41, 21),
        resized_host=([(0, 0, 50, 20), (55, 20, 45, 24), (10, 5, 33, 17)], 24, 16), resized=([(3, 2, 90, 40), (70, 30, 30, 14), (0, 0, 9, 9)], 31, 13),
        views=[([(0, 5, 3, 60, 30, flag(spec.BILINEAR)), (2, 50, 20, 50, 24, flag(spec.BOX, True))], 20, 12),
               ([(0, 40, 10, 30, 20, flag(spec.LANCZOS)), (2, 0, 0, 100, 44, flag(spec.HAMMING, True)), (2, 96, 40, 4, 4, flag(spec.NEAREST))], 16, 8)],
        region=(33, 13, 50, 25), update=(10, 5, 30, 12)),
    "100x6_50x1p": dict(
        h=6, tw=50, th=1, planar=True,
        regions=([(0, 0), (60, 3), (30, 2)], 40, 3), regions_again=([(59, 0), (0, 2), (59, 1)], 41, 4),
        resized_host=([(0, 0, 50, 4), (55, 2, 45, 4), (10, 1, 33, 5)], 24, 4), resized=([(3, 1, 90, 5), (70, 3, 30, 3), (0, 0, 9, 2)], 31, 3),
        views=[([(0, 5, 1, 60, 4, flag(spec.BILINEAR)), (2, 50, 2, 50, 4, flag(spec.BOX, True))], 20, 3),
               ([(0, 40, 0, 30, 5, flag(spec.LANCZOS)), (2, 0, 0, 100, 6, flag(spec.HAMMING, True)), (2, 96, 2, 4, 4, flag(spec.NEAREST))], 16, 2)],
        region=(33, 1, 50, 4), update=(10, 1, 30, 3)),
}
VIEW_FORMATS = [("uint8", "hwc"), ("float16", "hwc")]  # group 0 plain, group 1 formatted; frame 1 has no view


class Updated:
    """the outputs of update_region: the new payload, table and total"""

    def __init__(self, codec):
        import torch

        self.cap = codec.max_payload_bytes
        self.pay = torch.zeros(self.cap + 16, dtype=torch.uint8, device="cuda")
        self.len = torch.zeros(codec.n_slices, dtype=torch.int32, device="cuda")
        self.total = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.st = torch.full((1,), 0x7F, dtype=torch.int32, device="cuda")

    def read(self):
        import torch

        torch.cuda.synchronize()
        n = int(self.total.item())
        assert 0 < n <= self.cap
        return int(self.st.item()) & 0xFFFFFFFF, np.concatenate([self.len.cpu().numpy().view(np.uint8), self.pay.cpu().numpy()[:n]])


def calls(mi, codec, geo, conts, dev, d_rect):
    """the ten calls in the issue's order as (name, outputs, queue): every output buffer exists before anything is queued"""
    h, c, s = geo["h"], C, stream()
    pay, n, lens = dev[0].data_ptr(), dev[1], dev[2].data_ptr()

    def regions(key, host):
        xy, rw, rh = geo[key]
        o = Out(FRAMES, rw, rh, c, status=0x7F)
        if host:
            return [o], lambda: codec.decode_regions_host(conts, xy, rw, rh, o.ptr, o.st.data_ptr(), s)
        return [o], lambda: codec.decode_regions(pay, n, lens, xy, rw, rh, o.ptr, o.st.data_ptr(), s)

    def resized(host):
        rects, ow, oh = geo["resized_host" if host else "resized"]
        if host:  # bicubic, float32 CHW, normalised
            o = TOut(FRAMES, ow, oh, c, "float32", "chw", status=0x7F)
            return [o], lambda: codec.decode_resized_regions_host(conts, rects, ow, oh, o.ptr, o.st.data_ptr(), flags=[0, 1, 0], stream=s, dtype="float32",
                                                                   layout="chw", filter="bicubic", **norm(c, "float32"))
        o = Out(FRAMES, ow, oh, c, status=0x7F)
        return [o], lambda: codec.decode_resized_regions(pay, n, lens, rects, ow, oh, o.ptr, o.st.data_ptr(), flags=[1, 0, 0], stream=s)

    def views(host):
        outs = [TOut(len(v), ow, oh, c, d, lay, status=0x7F) for (v, ow, oh), (d, lay) in zip(geo["views"], VIEW_FORMATS)]
        groups = [mi.ViewGroup(v, ow, oh, o.ptr, **({} if d == "uint8" else dict(dtype=d, layout=lay, **norm(c, d))))
                  for (v, ow, oh), (d, lay), o in zip(geo["views"], VIEW_FORMATS, outs)]
        if host:
            return outs, lambda: codec.decode_views_host([conts[0], None, conts[2]], groups, outs[0].st.data_ptr(), s)
        return outs, lambda: codec.decode_views(pay, n, lens, groups, outs[0].st.data_ptr(), s)

    def region():
        x, y, rw, rh = geo["region"]
        o = Out(FRAMES, rw, rh, c, status=0x7F)
        return [o], lambda: codec.decode_region(pay, n, lens, x, y, rw, rh, o.ptr, o.st.data_ptr(), s)

    def full():
        o = Out(FRAMES, W, h, c, status=0x7F)
        return [o], lambda: codec.decode(pay, n, lens, o.ptr, o.st.data_ptr(), s)

    def update():
        x, y, rw, rh = geo["update"]
        o = Updated(codec)
        return [o], lambda: codec.update_region(pay, n, lens, x, y, rw, rh, d_rect.data_ptr(), o.pay.data_ptr(), o.cap, o.len.data_ptr(),
                                                o.total.data_ptr(), o.st.data_ptr(), s)

    made = [("decode_regions", regions("regions", False)), ("decode_resized_regions_host", resized(True)), ("decode_views", views(False)),
            ("decode_regions_host", regions("regions", True)), ("decode_views_host", views(True)), ("decode_region", region()),
            ("decode_resized_regions", resized(False)), ("decode", full()), ("update_region", update()),
            ("decode_regions again", regions("regions_again", False))]
    return [(name, outs, queue) for name, (outs, queue) in made]


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_ten_calls_queued_on_one_codec_equal_each_call_alone(mi, orc, name):
    import torch

    geo = GEOMETRIES[name]
    h, tw, th, planar = geo["h"], geo["tw"], geo["th"], geo["planar"]
    imgs, conts = make_batch(orc, FRAMES, W, h, C, tw, th, planar)
    dev = packed(mi, conts)
    x, y, rw, rh = geo["update"]
    assert x % tw and rw % tw  # (the rectangle is not a whole box: the box is decoded and the rectangle pasted over it)
    d_rect = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (FRAMES, rh, rw, C), dtype=np.uint8)).cuda()
    n_classes = mi.regions_plan(W, h, C, tw, th, planar, geo["regions"][1], geo["regions"][2], geo["regions"][0])[1]
    assert n_classes >= (2 if W % tw or h % th else 1)
    total_views = sum(len(v) for v, _, _ in geo["views"])

    codec = mi.Codec(FRAMES, W, h, C, tw, th, planar, device=0)
    try:
        mixed = calls(mi, codec, geo, conts, dev, d_rect)
        torch.cuda.synchronize()
        for _, _, queue in mixed:  # no synchronisation from here ...
            queue()
        torch.cuda.synchronize()  # ... to here
        got = [[o.read() for o in outs] for _, outs, _ in mixed]
        assert codec.allocated_bytes() <= codec.views_workspace_bytes(total_views)
    finally:
        codec.close()

    for i, (call, _, _) in enumerate(mixed):
        fresh = mi.Codec(FRAMES, W, h, C, tw, th, planar, device=0)
        try:
            _, outs, queue = calls(mi, fresh, geo, conts, dev, d_rect)[i]
            queue()
            alone = [o.read() for o in outs]
        finally:
            fresh.close()
        # (the groups of a views call share the first group's status word)
        assert got[i][0][0] == 0 and alone[0][0] == 0, (call, got[i][0][0], alone[0][0])
        for (_, a), (_, b) in zip(got[i], alone):
            assert same_bits(a, b), call
    # what the first and the last call read is the images' own pixels (one anchor outside the library; the rest is the other tests')
    for key, i in (("regions", 0), ("regions_again", 9)):
        xy, rw, rh = geo[key]
        assert np.array_equal(got[i][0][1], np.stack([imgs[f, y:y + rh, x:x + rw] for f, (x, y) in enumerate(xy)]))
    assert np.array_equal(got[7][0][1], imgs)
