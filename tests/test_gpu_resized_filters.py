"""The resampling filters of the resized regions decode on the GPU: PIL's bilinear, box, hamming, bicubic and lanczos and the
centre-aligned nearest neighbour, chosen per frame through bits 4-6 of the flags.  Every comparison is np.array_equal against the rule
restated with `math` (tests/resize_filters_spec.py) applied to the oracle-coded images' crops: it needs neither PIL nor the library's own
weights."""
import zlib

import numpy as np
import pytest

import resize_filters_spec as spec
from test_gpu_regions_host import Out, make_batch, stream
from test_gpu_resized_output import TOut, place, same_bits
from test_gpu_resized_regions import packed

pytestmark = pytest.mark.gpu

FILTERS = list(range(6))
MIRROR = 1


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


_batches = {}


def batch(orc, frames, w, h, c, tw, th, planar):
    key = (frames, w, h, c, tw, th, planar)
    if key not in _batches:
        _batches[key] = make_batch(orc, frames, w, h, c, tw, th, planar)
    return _batches[key]


def flag(filt, mirror=False):
    return (filt << 4) | (MIRROR if mirror else 0)


def expected(imgs, rects, ow, oh, flags):
    """frame f's crop under the filter of its flags' bits 4-6, mirrored where bit 0 is set"""
    return np.stack([spec.resize(imgs[f, y:y + rh, x:x + rw], ow, oh, (int(flags[f]) >> 4) & 7, bool(int(flags[f]) & 1))
                     for f, (x, y, rw, rh) in enumerate(rects)])


def run_device(codec, dev, rects, ow, oh, c, **kw):
    d_pay, n, d_len = dev
    o = Out(len(rects), ow, oh, c)
    codec.decode_resized_regions(d_pay.data_ptr(), n, d_len.data_ptr(), rects, ow, oh, o.ptr, o.st.data_ptr(), stream=stream(), **kw)
    return o.read()


def run_host(codec, conts, rects, ow, oh, c, **kw):
    o = Out(len(rects), ow, oh, c)
    codec.decode_resized_regions_host(conts, rects, ow, oh, o.ptr, o.st.data_ptr(), stream=stream(), **kw)
    return o.read()


def limit_rects(filt, w, h, ow, oh, frames):
    """rectangles at the filter's downscale limit on x, on y and on both (as far as the image goes), a 1 x 1 and an upscale"""
    r = spec.REACH[filt]
    rw, rh = min(w, 64 * ow // r), min(h, 64 * oh // r)
    rects = [(0, 0, rw, rh), (w - rw, h - rh, rw, min(rh, 2 * oh)), (3, h - rh, min(rw, 3 * ow), rh), (w - 1, h - 1, 1, 1), (5, 7, 2, 2),
             (w // 3, h // 3, rw // 2 + 1, rh // 2 + 1)]
    return [rects[f % len(rects)] for f in range(frames)]


def mixed_rects(rng, w, h, frames):
    """upscales and downscales for an output of some tens of pixels: sides from 1 to the whole image"""
    rects = []
    for f in range(frames):
        rw = int(rng.integers(1, w + 1)) if f % 2 else int(rng.integers(1, 40))
        rh = int(rng.integers(1, h + 1)) if f % 3 else int(rng.integers(1, 30))
        rects.append((int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1)), rw, rh))
    rects[0] = (0, 0, w, h)
    return rects


# (name, frames, w, h, c, tile_w, tile_h, planar, classes the "two" rectangles give or None)
SHAPES = [
    ("rows_480x1p_c3", 6, 1100, 120, 3, 480, 1, True, None),
    ("rows_480x1p_c1", 6, 1100, 120, 1, 480, 1, True, None),
    ("tiles_64x64i_c3", 6, 300, 200, 3, 64, 64, False, None),
    ("tiles_64x64i_c4", 6, 300, 200, 4, 64, 64, False, None),
    ("tiles_64x64i_c1", 6, 300, 200, 1, 64, 64, False, None),
    ("tiles_32x16i_c5", 6, 160, 90, 5, 32, 16, False, None),
    ("two_classes_64x64p_c3", 4, 300, 200, 3, 64, 64, True, 2),
]


@pytest.mark.parametrize("filt", FILTERS, ids=spec.NAMES)
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_every_filter(mi, orc, shape, filt):
    """one filter for the whole batch, through filter= and through the flags: rectangles at the filter's downscale limit, upscales,
    1 x 1, the whole image, with and without the mirror"""
    name, frames, w, h, c, tw, th, planar, n_cls = shape
    imgs, conts = batch(orc, frames, w, h, c, tw, th, planar)
    rng = np.random.default_rng(zlib.crc32(f"{name}{filt}".encode()))
    codec = mi.Codec(frames, w, h, c, tw, th, planar, device=0)
    try:
        dev = packed(mi, conts)
        if n_cls:
            rects = [(0, 0, 60, 40), (w - 60, 10, 60, 40), (5, 70, 33, 21), (w - 1, 0, 1, 1)]
            assert mi.resized_regions_plan(w, h, c, tw, th, planar, rects)[1] == n_cls
            calls = [(rects, 224, 224), (rects, 7, 5)]
        else:
            calls = [(limit_rects(filt, w, h, 4, 3, frames), 4, 3), (mixed_rects(rng, w, h, frames), 57, 43)]
        for rects, ow, oh in calls:
            mirror = np.array([f % 2 for f in range(frames)], np.uint8)
            flags = np.array([flag(filt, f % 2) for f in range(frames)], np.uint8)
            want = expected(imgs, rects, ow, oh, flags)
            st, out = run_device(codec, dev, rects, ow, oh, c, flags=flags)  # the filter in the flags' bits 4-6
            assert st == 0 and np.array_equal(out, want), (rects, ow, oh)
            st, out = run_host(codec, conts, rects, ow, oh, c, flags=mirror, filter=spec.NAMES[filt])  # ... and as filter=, by name
            assert st == 0 and np.array_equal(out, want), (rects, ow, oh)
            st, out = run_device(codec, dev, rects, ow, oh, c, filter=filt)  # no mirror
            assert st == 0 and np.array_equal(out, expected(imgs, rects, ow, oh, [flag(filt)] * frames)), (rects, ow, oh)
            # bits 1-3 and 7 stay ignored
            st, out = run_device(codec, dev, rects, ow, oh, c, flags=flags | 0x8E)
            assert st == 0 and np.array_equal(out, want)
    finally:
        codec.close()


def test_a_flags_byte_of_0x40_is_bicubic_not_bilinear(mi, orc):
    w, h, c = 300, 200, 3
    imgs, conts = batch(orc, 6, w, h, c, 64, 64, False)
    codec = mi.Codec(6, w, h, c, 64, 64, False, device=0)
    try:
        rects = [(10, 20, 200, 150)] * 6
        st, out = run_device(codec, packed(mi, conts), rects, 64, 48, c, flags=np.full(6, 0x40, np.uint8))
        assert st == 0 and np.array_equal(out, expected(imgs, rects, 64, 48, [0x40] * 6))
        assert not np.array_equal(out, expected(imgs, rects, 64, 48, [0] * 6))
    finally:
        codec.close()


@pytest.mark.parametrize("c,tw,th,planar", [(3, 480, 1, True), (4, 64, 64, False)], ids=["rows_c3", "tiles_c4"])
def test_one_batch_with_all_six_filters(mi, orc, c, tw, th, planar):
    """frame f uses filter f: the device call, the host-container call and a pipeline job give the same bytes -- the spec's"""
    w, h = (1100, 120) if th == 1 else (300, 200)
    frames = 6
    imgs, conts = batch(orc, frames, w, h, c, tw, th, planar)
    rng = np.random.default_rng(c)
    # every frame the same rectangle size: the axes' weights may only be shared between frames of one filter
    rects = [(int(rng.integers(0, w - 150)), int(rng.integers(0, h - 100)), 150, 100) for _ in range(frames)]
    flags = np.array([flag(f, f % 2) for f in range(frames)], np.uint8)
    ow, oh = 40, 30
    want = expected(imgs, rects, ow, oh, flags)
    assert len({want[f].tobytes() for f in range(frames)}) == frames
    codec = mi.Codec(frames, w, h, c, tw, th, planar, device=0)
    s = mi.Stream(w, h, c, tw, th, planar, depth=2, device=0, frames_per_job=frames)
    try:
        st, out = run_device(codec, packed(mi, conts), rects, ow, oh, c, flags=flags)
        assert st == 0 and np.array_equal(out, want)
        st, out = run_host(codec, conts, rects, ow, oh, c, flags=flags)
        assert st == 0 and np.array_equal(out, want)
        st, out = run_host(codec, conts, rects, ow, oh, c, flags=flags & 1, filter=list(spec.NAMES))
        assert st == 0 and np.array_equal(out, want)
        assert s.submit_decode_resized_regions(list(conts), rects, ow, oh, flags=flags, tag=7)
        job = s.wait()
        assert (job.status, job.kind, job.tag) == (mi.OK, mi.JOB_DECODE_RESIZED_REGIONS, 7) and np.array_equal(job.data, want)
        s.release(job)
        assert s.submit_decode_resized_regions(list(conts), rects, ow, oh, flags=flags & 1, filter=list(range(6)), tag=8)
        job = s.wait()
        assert job.status == mi.OK and np.array_equal(job.data, want)
        s.release(job)
        # pictures and their label images in one batch: the nearest frames hold only values their crops held
        mask_flags = np.array([flag(spec.NEAREST if f % 2 else spec.BICUBIC) for f in range(frames)], np.uint8)
        st, out = run_device(codec, packed(mi, conts), rects, ow, oh, c, flags=mask_flags)
        assert st == 0 and np.array_equal(out, expected(imgs, rects, ow, oh, mask_flags))
        for f in range(1, frames, 2):
            x, y, rw, rh = rects[f]
            assert set(np.unique(out[f])) <= set(np.unique(imgs[f, y:y + rh, x:x + rw]))
    finally:
        s.close()
        codec.close()


@pytest.mark.parametrize("dtype,layout,filt", [("float32", "chw", spec.BICUBIC), ("float16", "hwc", spec.LANCZOS), ("bfloat16", "chw", spec.NEAREST),
                                               ("uint8", "chw", spec.HAMMING)], ids=["f32_chw_bicubic", "f16_hwc_lanczos", "bf16_chw_nearest",
                                                                                     "u8_chw_hamming"])
def test_output_formats_are_the_table_over_the_u8_result(mi, orc, dtype, layout, filt):
    w, h, c = 300, 200, 3
    frames = 6
    imgs, conts = batch(orc, frames, w, h, c, 64, 64, False)
    rng = np.random.default_rng(filt)
    rects = mixed_rects(rng, w, h, frames)
    flags = np.array([flag(filt, f % 2) for f in range(frames)], np.uint8)
    kw = {} if dtype == "uint8" else dict(scale=True, mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
    want = place(mi.output_table(c, dtype, **kw), expected(imgs, rects, 57, 43, flags), layout)
    codec = mi.Codec(frames, w, h, c, 64, 64, False, device=0)
    try:
        o = TOut(frames, 57, 43, c, dtype, layout)
        codec.decode_resized_regions_host(conts, rects, 57, 43, o.ptr, o.st.data_ptr(), flags=flags, stream=stream(), dtype=dtype, layout=layout,
                                          **kw)
        st, out = o.read()
        assert st == 0 and same_bits(out, want)
        d_pay, n, d_len = packed(mi, conts)
        o = TOut(frames, 57, 43, c, dtype, layout)
        codec.decode_resized_regions(d_pay.data_ptr(), n, d_len.data_ptr(), rects, 57, 43, o.ptr, o.st.data_ptr(), flags=flags & 1, stream=stream(),
                                     dtype=dtype, layout=layout, filter=filt, **kw)
        st, out = o.read()
        assert st == 0 and same_bits(out, want)
    finally:
        codec.close()


def test_bad_filter_arguments_write_nothing(mi, orc):
    """filter codes 6 and 7 and a downscale above the frame's own filter's limit: BAD_ARGS with d_px and d_status untouched"""
    w, h, c = 300, 200, 3
    imgs, conts = batch(orc, 6, w, h, c, 64, 64, False)
    codec = mi.Codec(6, w, h, c, 64, 64, False, device=0)
    s = mi.Stream(w, h, c, 64, 64, False, depth=2, device=0, frames_per_job=6)
    dev = packed(mi, conts)
    good = [(5, 5, 30, 20)] * 5
    try:
        cases = [([(0, 0, 100, 100)] + good, [0x60, 0, 0, 0, 0, 0], 32, 32), (good + [(0, 0, 100, 100)], [0, 0, 0, 0, 0, 0x71], 32, 32),
                 # 4 x 3 output: bicubic takes 128 x 96 at most, Lanczos 85 x 64; bilinear in the same batch takes 256 x 192
                 ([(0, 0, 129, 96)] + good, [flag(spec.BICUBIC)] + [0] * 5, 4, 3), ([(0, 0, 128, 97)] + good, [flag(spec.BICUBIC)] + [0] * 5, 4, 3),
                 ([(0, 0, 86, 64)] + good, [flag(spec.LANCZOS)] + [0] * 5, 4, 3), ([(0, 0, 85, 65)] + good, [flag(spec.LANCZOS, True)] + [0] * 5, 4, 3),
                 ([(0, 0, 257, 10)] + good, [flag(spec.NEAREST)] + [0] * 5, 4, 3), ([(0, 0, 257, 10)] + good, [flag(spec.BOX)] + [0] * 5, 4, 3)]
        for rects, flags, ow, oh in cases:
            flags = np.array(flags, np.uint8)
            for host in (False, True):
                o = Out(6, ow, oh, c, status=0x77)
                with pytest.raises(mi.LlcompError) as e:
                    if host:
                        codec.decode_resized_regions_host(conts, rects, ow, oh, o.ptr, o.st.data_ptr(), flags=flags, stream=stream())
                    else:
                        codec.decode_resized_regions(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), rects, ow, oh, o.ptr, o.st.data_ptr(), flags=flags,
                                                     stream=stream())
                assert e.value.status == mi.BAD_ARGS, (rects, flags, host)
                st, out = o.read()
                assert st == 0x77 and (out == 0x5A).all()
            with pytest.raises(mi.LlcompError) as e:
                s.submit_decode_resized_regions(list(conts), rects, ow, oh, flags=flags)
            assert e.value.status == mi.BAD_ARGS
        assert s.pending() == 0
        for bad in ("cubic", 6, ["box"] * 5):
            o = Out(6, 8, 8, c, status=0x77)
            with pytest.raises(mi.LlcompError) as e:
                codec.decode_resized_regions_host(conts, [(0, 0, 100, 100)] + good, 8, 8, o.ptr, o.st.data_ptr(), stream=stream(), filter=bad)
            assert e.value.status == mi.BAD_ARGS
            st, out = o.read()
            assert st == 0x77 and (out == 0x5A).all()
        # exactly at every filter's limit, in one batch
        rects = [(0, 0, 256, 192), (0, 0, 256, 192), (0, 0, 256, 192), (0, 0, 256, 192), (0, 0, 128, 96), (0, 0, 85, 64)]
        flags = np.array([flag(f) for f in range(6)], np.uint8)
        st, out = run_device(codec, dev, rects, 4, 3, c, flags=flags)
        assert st == 0 and np.array_equal(out, expected(imgs, rects, 4, 3, flags))
    finally:
        s.close()
        codec.close()


def test_lanczos_at_the_limit_stays_within_workspace_bytes(mi, orc):
    """Lanczos has the longest weight tables; calls whose rectangles keep growing, every frame another size (nothing shared), up to the
    whole image at the filter's limit: the codec never holds more than workspace_bytes"""
    frames, w, h, c = 8, 600, 400, 3
    imgs, conts = batch(orc, frames, w, h, c, 64, 64, True)
    codec = mi.Codec(frames, w, h, c, 64, 64, True, device=0)
    try:
        dev = packed(mi, conts)
        flags = np.array([flag(spec.LANCZOS, f % 2) for f in range(frames)], np.uint8)
        for hmax, (ow, oh) in ((90, (600, 400)), (150, (300, 200)), (250, (100, 60)), (380, (29, 19)), (400, (29, 19))):
            rects = [(f, 0, min(w - f, 21 * ow) - f, min(hmax, 21 * oh) - f) for f in range(frames)]
            want = expected(imgs, rects, ow, oh, flags)
            # what this call's tables take in the staging buffer (48 bytes and out * (K + 1) int32 per axis and frame; no two frames
            # share an axis) against the bound's share for them, 10 sides per axis -- and, for the first call (an upscale to the
            # image's size: 7 taps and lo per output), against the 6 sides that the triangle filter needed
            staged = sum(48 + 4 * (ow * (mi.resize_weights(rw, ow, "lanczos")[1].shape[1] + 1) + oh * (mi.resize_weights(rh, oh, "lanczos")[1].shape[1] + 1))
                         for _, _, rw, rh in rects)
            assert staged <= frames * (48 + 4 * 10 * (w + h))
            if hmax == 90:
                assert staged > frames * (48 + 4 * 6 * (w + h)), staged
            st, out = run_device(codec, dev, rects, ow, oh, c, flags=flags)
            assert st == 0 and np.array_equal(out, want), hmax
            assert codec.allocated_bytes() <= codec.workspace_bytes, (hmax, codec.allocated_bytes(), codec.workspace_bytes)
            st, out = run_host(codec, conts, rects, ow, oh, c, flags=flags)
            assert st == 0 and np.array_equal(out, want), hmax
            assert codec.allocated_bytes() <= codec.workspace_bytes, (hmax, codec.allocated_bytes(), codec.workspace_bytes)
    finally:
        codec.close()


# (name, frames, w, h, c, tile_w, tile_h, planar, [(ow, oh), ...]): scales from an upscale to the filters' limits; 8 x 6 on 1100 x 120 and
# 4 x 3 on 300 x 200 are power-of-two strides between the lanes of the horizontal pass where the rectangle is 1024, 512 or 256 wide
SCALE_GRID = [
    ("c1", 6, 1100, 120, 1, 480, 1, True, [(300, 40), (64, 15), (8, 6)]),
    ("c3", 6, 1100, 120, 3, 480, 1, True, [(300, 40), (64, 15), (8, 6)]),
    ("c4", 6, 300, 200, 4, 64, 64, False, [(224, 224), (57, 43), (4, 3)]),
    ("c5", 6, 160, 90, 5, 32, 16, False, [(224, 100), (31, 17), (3, 2)]),
]


@pytest.mark.parametrize("case", SCALE_GRID, ids=[g[0] for g in SCALE_GRID])
def test_filter_channel_scale_grid(mi, orc, case):
    """every filter over a range of scales, every rectangle as large as the filter allows for the output"""
    name, frames, w, h, c, tw, th, planar, outs = case
    imgs, conts = batch(orc, frames, w, h, c, tw, th, planar)
    codec = mi.Codec(frames, w, h, c, tw, th, planar, device=0)
    try:
        dev = packed(mi, conts)
        for ow, oh in outs:
            for filt in FILTERS:
                r = spec.REACH[filt]
                rw, rh = min(w, 64 * ow // r), min(h, 64 * oh // r)
                rects = [(0, 0, rw, rh), (w - rw, h - rh, rw, rh), (1, 1, max(rw // 2, 1), max(rh // 3, 1)), (w - 1, 0, 1, 1),
                         (min(7, w - min(rw, 512)), min(3, h - min(rh, 64)), min(rw, 512), min(rh, 64)),
                         (min(2, w - min(rw, 1024)), 0, min(rw, 1024), 1)]
                flags = np.array([flag(filt, f % 2) for f in range(frames)], np.uint8)
                st, out = run_device(codec, dev, rects, ow, oh, c, flags=flags)
                assert st == 0 and np.array_equal(out, expected(imgs, rects, ow, oh, flags)), (ow, oh, filt)
    finally:
        codec.close()


# (name, w, h, c, tile_w, tile_h, planar): rows of more than 16 KiB
LONG_ROWS = [("c4_4400", 4400, 8, 4, 64, 64, False), ("c3_6000", 6000, 4, 3, 480, 1, True), ("c5_3400", 3400, 6, 5, 64, 64, False)]


@pytest.mark.parametrize("case", LONG_ROWS, ids=[r[0] for r in LONG_ROWS])
def test_long_rows_at_every_filters_limit(mi, orc, case):
    """every filter at its own downscale limit over a whole long row, at a quarter of it and to 300 outputs"""
    name, w, h, c, tw, th, planar = case
    frames = 2
    imgs, conts = batch(orc, frames, w, h, c, tw, th, planar)
    codec = mi.Codec(frames, w, h, c, tw, th, planar, device=0)
    try:
        dev = packed(mi, conts)
        for filt in FILTERS:
            least = -(-w * spec.REACH[filt] // 64)  # the fewest outputs the whole row may go to
            for ow in (least, 4 * least, 300):
                rects = [(0, 0, w, h), (7, h - 1, w - 7, 1)]
                flags = np.array([flag(filt, f % 2) for f in range(frames)], np.uint8)
                st, out = run_device(codec, dev, rects, ow, 2, c, flags=flags)
                assert st == 0 and np.array_equal(out, expected(imgs, rects, ow, 2, flags)), (filt, ow)
    finally:
        codec.close()
