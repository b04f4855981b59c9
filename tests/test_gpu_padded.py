"""Crops that leave the image (llcomp_mi_codec_decode_padded_regions(_host), llcomp_mi_codec_decode_padded_views(_host); pad_mode= and
fill= of Codec.decode_resized_regions(_host) and Codec.decode_views(_host)).  Everything is byte-exact: the expected pixels come from
the ORIGINAL frames (the codec is lossless), np.pad with the mode's name (constant: an array of the fill with the frame pasted in), a
slice, and tests/resize_filters_spec.py's resize with the mirror; float outputs go through output_table."""
import ctypes as C

import numpy as np
import pytest

import resize_filters_spec as spec
from test_gpu_regions_host import make_batch, stream
from test_gpu_resized_output import TOut, place, same_bits
from test_gpu_resized_regions import packed

pytestmark = pytest.mark.gpu

MODES = ("constant", "edge", "reflect", "symmetric")
FILL = (124, 116, 104, 7)
# the smallest geometries with a partial last tile column and / or row, so two or more classes, in each kernel family:
# (name, frames, w, h, c, tile_w, tile_h, planar)
GEOMS = {
    "a_rows_32x1p_c3": (6, 97, 24, 3, 32, 1, True),      # the fused row path
    "b_2d_40x8i_c4": (4, 70, 41, 4, 40, 8, False),       # 2-D, both partial edges
    "c_16x4i_c2": (3, 33, 17, 2, 16, 4, False),          # the generic resample path
    "c_16x1p_c1": (3, 33, 17, 1, 16, 1, True),           # the c = 1 resample path
}
FILTERS = (spec.BILINEAR, spec.BICUBIC, spec.LANCZOS, spec.NEAREST)  # mixed per frame through the flags


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


_BATCHES = {}


@pytest.fixture
def batch(mi, orc, request):
    """(geometry, frames [F, h, w, c], containers, the packed batch in HBM, a codec) of a geometry: made once, shared, never changed"""
    name = request.param
    if name not in _BATCHES:
        frames, w, h, c, tw, th, planar = GEOMS[name]
        imgs, conts = make_batch(orc, frames, w, h, c, tw, th, planar)
        imgs.setflags(write=False)
        _BATCHES[name] = (GEOMS[name], imgs, conts, packed(mi, conts), mi.Codec(frames, w, h, c, tw, th, planar, device=0))
    return _BATCHES[name]


def limit(mode, n):
    return n - 1 if mode == "reflect" else n


def axis(kind, n, lim, rng):
    """(x, r) of one axis: "in" inside the image, "lo" / "hi" out by that side alone, "both", "lo_limit" / "hi_limit" at the mode's limit"""
    some = lambda: int(rng.integers(1, max(1, min(lim, n // 2)) + 1))  # noqa: E731
    a = {"lo": -some(), "both": -some(), "lo_limit": -lim}.get(kind)
    b = {"hi": n + some(), "both": n + some(), "hi_limit": n + lim}.get(kind)
    if a is None:
        a = int(rng.integers(0, n - 1)) if n > 1 else 0
    if b is None:
        b = int(rng.integers(max(a, 0) + 1, n + 1))
    return a, b - a


# a frame's rectangle by kind: (the x axis' kind, the y axis' kind)
KINDS = {"inside": ("in", "in"), "left": ("lo", "in"), "right": ("hi", "in"), "top": ("in", "lo"), "bottom": ("in", "hi"),
         "all_four": ("both", "both"), "limit_x": ("lo_limit", "in"), "limit_y": ("in", "hi_limit")}


def rect_of(kind, mode, w, h, rng):
    kx, ky = KINDS[kind]
    (x, rw), (y, rh) = axis(kx, w, limit(mode, w), rng), axis(ky, h, limit(mode, h), rng)
    return x, y, rw, rh


def calls_of(mode, frames, w, h, rng):
    """every kind of rectangle, spread over as few calls of `frames` rectangles as it takes, an inside frame in every call"""
    others = [k for k in KINDS if k != "inside"]
    out = []
    for n, i in enumerate(range(0, len(others), frames - 1)):
        kinds = (others[i:i + frames - 1] + others)[:frames - 1]
        kinds.insert(n % frames, "inside")
        out.append((kinds, [rect_of(k, mode, w, h, rng) for k in kinds]))
    return out


def padded_crop(img, rect, mode, fill):
    """np.pad with the mode's name, then the slice"""
    h, w, c = img.shape
    x, y, rw, rh = rect
    pl, pr, pt, pb = max(-x, 0), max(x + rw - w, 0), max(-y, 0), max(y + rh - h, 0)
    if mode == "constant":
        big = np.empty((h + pt + pb, w + pl + pr, c), np.uint8)
        big[:] = np.asarray(fill, np.uint8)[:c]
        big[pt:pt + h, pl:pl + w] = img
    else:
        big = np.pad(img, ((pt, pb), (pl, pr), (0, 0)), mode=mode)
    return big[y + pt:y + pt + rh, x + pl:x + pl + rw]


def expected(imgs, frame_rects, ow, oh, mode, fill, flags):
    """[(frame, rect)] -> u8 [n, oh, ow, c]; flags: per entry, bit 0 the mirror and bits 4-6 the filter"""
    return np.stack([spec.resize(padded_crop(imgs[f], r, mode, fill), ow, oh, (int(fl) >> 4) & 7, bool(int(fl) & 1))
                     for (f, r), fl in zip(frame_rects, flags)])


def flags_of(n, shift=0):
    """bilinear, bicubic, Lanczos and nearest in turn, the mirror on every other frame"""
    return np.array([(FILTERS[(i + shift) % 4] << 4) | ((i + shift) % 2) for i in range(n)], np.uint8)


def run(codec, src, rects, ow, oh, c, mode, fill=None, flags=None, dtype="uint8", layout="hwc", status=0, **kw):
    """(status, output) of the padded resized call from the packed batch in HBM (a tuple) or from host containers (a list)"""
    o = TOut(len(rects), ow, oh, c, dtype, layout, 0, status)
    fmt = dict(dtype=dtype, layout=layout, **kw) if (dtype, layout) != ("uint8", "hwc") else {}
    if isinstance(src, tuple):
        codec.decode_resized_regions(src[0].data_ptr(), src[1], src[2].data_ptr(), rects, ow, oh, o.ptr, o.st.data_ptr(), flags=flags,
                                     stream=stream(), pad_mode=mode, fill=fill, **fmt)
    else:
        codec.decode_resized_regions_host(src, rects, ow, oh, o.ptr, o.st.data_ptr(), flags=flags, stream=stream(), pad_mode=mode, fill=fill, **fmt)
    return o.read()


def run_plain(codec, dev, rects, ow, oh, c, flags):
    """the existing unpadded call"""
    o = TOut(len(rects), ow, oh, c, "uint8", "hwc")
    codec.decode_resized_regions(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), rects, ow, oh, o.ptr, o.st.data_ptr(), flags=flags, stream=stream())
    return o.read()


def seed_of(name, mode):
    return 1000 * sorted(GEOMS).index(name) + MODES.index(mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("batch", sorted(GEOMS), indirect=True, ids=sorted(GEOMS))
def test_padded_crops_equal_np_pad_then_resize(mi, batch, mode, request):
    """per geometry and mode: rectangles out by each side alone, by all four, at the mode's limit, beside an inside frame; ow = rw, oh = rh
    (the np.pad slice itself), a downscale and an upscale; four filters and the mirror mixed per frame; device and host sources give the
    same bytes and status; the inside frame equals the unpadded call on the same rectangle"""
    (frames, w, h, c, *_), imgs, conts, dev, codec = batch
    rng = np.random.default_rng(seed_of(request.node.callspec.params["batch"], mode))
    fill = FILL[:c] if mode == "constant" else None
    lx, ly = limit(mode, w), limit(mode, h)
    px, py = min(3, lx), min(2, ly)

    def check(rects, ow, oh, flags, inside=None):
        want = expected(imgs, list(enumerate(rects)), ow, oh, mode, fill, flags)
        st_d, out_d = run(codec, dev, rects, ow, oh, c, mode, fill, flags)
        st_h, out_h = run(codec, conts, rects, ow, oh, c, mode, fill, flags)
        assert st_d == 0 and st_h == 0
        assert np.array_equal(out_d, want), (mode, rects, ow, oh)
        assert np.array_equal(out_h, out_d)
        if inside is not None:
            st_p, out_p = run_plain(codec, dev, [rects[inside]] * frames, ow, oh, c, flags)
            assert st_p == 0 and np.array_equal(out_p[inside], out_d[inside])

    # RandomCrop with padding: one size, ow = rw, oh = rh -- the output is the np.pad slice itself, whatever the filter
    rw, rh = w - 4, h - 3
    shifts = [(2, 1), (-px, 1), (w - rw + px, 1), (2, -py), (2, h - rh + py), (-px, -py)]
    rects = [(*shifts[f % len(shifts)], rw, rh) for f in range(frames)]
    check(rects, rw, rh, flags_of(frames), inside=0)
    want = np.stack([padded_crop(imgs[f], r, mode, fill) for f, r in enumerate(rects)])
    assert np.array_equal(run(codec, dev, rects, rw, rh, c, mode, fill)[1], want)
    # ... larger than the image (a CenterCrop of a smaller picture), and at the mode's limit on both sides of the x axis
    rects = [(-px - f % 2, -py, w + 2 * px + 1, h + 2 * py) for f in range(frames)]
    check(rects, w + 2 * px + 1, h + 2 * py, flags_of(frames, 1))
    rects = [(-lx, 1 - f % 2, w + 2 * lx, h - 1) for f in range(frames)]
    check(rects, w + 2 * lx, h - 1, flags_of(frames))
    # every kind of rectangle, each frame its own size: a downscale and an upscale
    for n, (kinds, rects) in enumerate(calls_of(mode, frames, w, h, rng)):
        inside = kinds.index("inside")
        check(rects, (w * 29 + 63) // 64, (h * 31 + 63) // 64, flags_of(frames, n), inside)
        check(rects, w + 9, h + 5, flags_of(frames, n + 1), inside)


@pytest.mark.parametrize("batch", sorted(GEOMS), indirect=True, ids=sorted(GEOMS))
def test_constant_fills_and_the_bias_kernels(mi, batch):
    """fill 0, fill 255 and a fill per channel: the latter two run the kernels' bias forms (LLCOMP_MI_CTR_BIAS_LAUNCHES counts the launches
    that did), fill 0, a NULL fill and a call whose rectangles all lie inside the image do not; every mode but "constant" never does"""
    (frames, w, h, c, *_), imgs, conts, dev, codec = batch
    rng = np.random.default_rng(31)
    kinds, rects = calls_of("constant", frames, w, h, rng)[0]
    inside = [rect_of("inside", "constant", w, h, rng) for _ in range(frames)]
    flags = flags_of(frames)
    ow, oh = (w * 3 + 3) // 4, (h * 3 + 3) // 4

    def launches(mode, fill, rs):
        codec.counters(reset=True)
        st, out = run(codec, dev, rs, ow, oh, c, mode, fill, flags)
        assert st == 0
        assert np.array_equal(out, expected(imgs, list(enumerate(rs)), ow, oh, mode, fill if fill is not None else (0,) * 4, flags)), (mode, fill)
        return codec.counters()["bias_launches"]

    assert launches("constant", (0,) * c, rects) == 0
    assert launches("constant", None, rects) == 0
    assert launches("constant", (255,) * c, rects) == 1
    assert launches("constant", FILL[:c], rects) == 1
    assert launches("constant", (0,) * (c - 1) + (9,), rects) == 1
    assert launches("constant", FILL[:c], inside) == 0
    for mode in MODES[1:]:
        assert launches(mode, FILL[:c], rects) == 0  # (the fill is ignored)
    # one value stands for every channel; the host source runs the same kernels
    codec.counters(reset=True)
    st, out = run(codec, conts, rects, ow, oh, c, "constant", 200, flags)
    assert st == 0 and np.array_equal(out, expected(imgs, list(enumerate(rects)), ow, oh, "constant", (200,) * 4, flags))
    assert codec.counters()["bias_launches"] == 1


@pytest.mark.parametrize("batch", ["a_rows_32x1p_c3", "b_2d_40x8i_c4"], indirect=True)
def test_output_formats(mi, batch):
    """u8 HWC, float32 CHW with scale, mean and std, and bfloat16 HWC once: the table of the format over the u8 bytes, with and without
    the bias kernels"""
    (frames, w, h, c, *_), imgs, conts, dev, codec = batch
    rng = np.random.default_rng(8)
    flags = flags_of(frames)
    ow, oh = (w * 5 + 7) // 8, (h * 5 + 7) // 8
    norm = dict(scale=True, mean=[0.485, 0.456, 0.406, 0.5][:c], std=[0.229, 0.224, 0.225, 0.25][:c])
    formats = [("float32", "chw", norm)] + ([("bfloat16", "hwc", dict(scale=True))] if c == 4 else [])
    for mode in ("constant", "reflect"):
        fill = FILL[:c] if mode == "constant" else None
        kinds, rects = calls_of(mode, frames, w, h, rng)[0]
        u8 = expected(imgs, list(enumerate(rects)), ow, oh, mode, fill, flags)
        for dtype, layout, kw in formats:
            want = place(mi.output_table(c, dtype, **kw), u8, layout)
            for src in (dev, conts):
                st, out = run(codec, src, rects, ow, oh, c, mode, fill, flags, dtype, layout, **kw)
                assert st == 0 and same_bits(out, want), (mode, dtype, layout, isinstance(src, tuple))


@pytest.mark.parametrize("batch", ["a_rows_32x1p_c3", "b_2d_40x8i_c4"], indirect=True)
def test_padded_views(mi, batch):
    """two groups; frame 1 has one view out by the left and one out by the right: every view equals the padded resized call for its
    rectangle, device and host sources agree, and the host call stages what the unpadded call stages for the unions of the source
    rectangles, which padded_regions_plan + views_plan state"""
    (frames, w, h, c, tw, th, planar), imgs, conts, dev, codec = batch
    rng = np.random.default_rng(13)
    for mode in MODES:
        fill = FILL[:c] if mode == "constant" else None
        # group 0: one view per frame (what one padded resized call gives); group 1: a second view of frames 0 and 1 and a third of frame 1
        _, g0 = calls_of(mode, frames, w, h, rng)[0]
        g0[1] = rect_of("left", mode, w, h, rng)
        g1 = [(1, *rect_of("right", mode, w, h, rng)), (0, *rect_of("all_four", mode, w, h, rng)), (1, *rect_of("top", mode, w, h, rng))]
        f0, f1 = flags_of(frames), flags_of(3, 1)
        o0, o1 = ((w * 3) // 4, (h * 3) // 4), ((w + 1) // 2, (h + 3) // 2)
        views0 = [(f, *r, int(f0[f])) for f, r in enumerate(g0)]
        views1 = [(*v, int(f1[i])) for i, v in enumerate(g1)]
        want0 = expected(imgs, list(enumerate(g0)), *o0, mode, fill, f0)
        want1 = expected(imgs, [(v[0], v[1:]) for v in g1], *o1, mode, fill, f1)
        norm = dict(dtype="float32", layout="chw", scale=True, mean=[0.5] * c, std=[0.25] * c)
        table = mi.output_table(c, "float32", scale=True, mean=[0.5] * c, std=[0.25] * c)
        st_r, resized = run(codec, dev, g0, *o0, c, mode, fill, f0)
        assert st_r == 0 and np.array_equal(resized, want0)
        got = {}
        for src in (dev, conts):
            a, b = TOut(frames, *o0, c, "uint8", "hwc"), TOut(3, *o1, c, "float32", "chw")
            groups = [mi.ViewGroup(views0, *o0, a.ptr), mi.ViewGroup(views1, *o1, b.ptr, **norm)]
            codec.counters(reset=True)
            if isinstance(src, tuple):
                codec.decode_views(src[0].data_ptr(), src[1], src[2].data_ptr(), groups, a.st.data_ptr(), stream=stream(), pad_mode=mode, fill=fill)
            else:
                codec.decode_views_host(src, groups, a.st.data_ptr(), stream=stream(), pad_mode=mode, fill=fill)
            (st, out0), (_, out1) = a.read(), b.read()
            assert st == 0 and np.array_equal(out0, resized) and same_bits(out1, place(table, want1, "chw")), (mode, isinstance(src, tuple))
            got[isinstance(src, tuple)] = codec.counters()["host_staged_bytes"]
        # what was staged: the unpadded host call on the unions of the source rectangles
        rects = [r for r in g0] + [v[1:] for v in g1]
        owner = list(range(frames)) + [v[0] for v in g1]
        src_rects = mi.padded_regions_plan(w, h, rects, mode).astype(np.int64)
        unions = []
        for f in range(frames):
            mine = src_rects[[i for i, o in enumerate(owner) if o == f]]
            x0, y0 = mine[:, 0].min(), mine[:, 1].min()
            unions.append((int(x0), int(y0), int((mine[:, 0] + mine[:, 2]).max() - x0), int((mine[:, 1] + mine[:, 3]).max() - y0)))
        planned, windows, n_used, _ = mi.views_plan(w, h, c, tw, th, planar, frames, [([(o, *map(int, r)) for o, r in zip(owner, src_rects)], 8, 8)])
        assert n_used == frames and planned.tolist() == [list(u) for u in unions]
        codec.counters(reset=True)
        o = TOut(frames, 8, 8, c, "uint8", "hwc")
        codec.decode_resized_regions_host(conts, unions, 8, 8, o.ptr, o.st.data_ptr(), flags=[spec.NEAREST << 4] * frames, stream=stream())
        assert o.read()[0] == 0
        assert got[True] == 0 and got[False] == codec.counters()["host_staged_bytes"] > 0


def test_memory_stays_within_padded_workspace_bytes(mi, orc):
    """growing Lanczos calls at the pad limit, every frame another size, to the image's own size: the codec never holds more than
    padded_workspace_bytes(), which is more than workspace_bytes by the tables alone"""
    frames, w, h, c, tw, th, planar = GEOMS["a_rows_32x1p_c3"]
    imgs, conts = make_batch(orc, frames, w, h, c, tw, th, planar)
    codec = mi.Codec(frames, w, h, c, tw, th, planar, device=0)
    try:
        bound = codec.padded_workspace_bytes()
        assert bound == codec.padded_workspace_bytes(frames) == codec.workspace_bytes + frames * 52 * (w + h) + 4 * c
        assert codec.padded_workspace_bytes(frames + 5) == codec.views_workspace_bytes(frames + 5) + (frames + 5) * 52 * (w + h) + 4 * c
        flags = [spec.LANCZOS << 4] * frames
        for mode in ("constant", "symmetric"):
            for step in range(4, -1, -1):
                rects = [(-(w - step - f), -(h - step - f), 3 * w - 2 * (step + f), 3 * h - 2 * (step + f)) for f in range(frames)]
                for src in (conts, None):
                    o = TOut(frames, w, h, c, "float32", "chw")
                    if src is None:
                        dev = packed(mi, conts)
                        codec.decode_resized_regions(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), rects, w, h, o.ptr, o.st.data_ptr(), flags=flags,
                                                     stream=stream(), dtype="float32", layout="chw", pad_mode=mode, fill=FILL[:c])
                    else:
                        codec.decode_resized_regions_host(src, rects, w, h, o.ptr, o.st.data_ptr(), flags=flags, stream=stream(), dtype="float32",
                                                          layout="chw", pad_mode=mode, fill=FILL[:c])
                    st, out = o.read()
                    assert st == 0 and codec.allocated_bytes() <= bound, (mode, step, codec.allocated_bytes(), bound)
        st, out = run(codec, conts, rects, w, h, c, "symmetric", None, flags)
        assert st == 0 and np.array_equal(out, expected(imgs, list(enumerate(rects)), w, h, "symmetric", None, flags))
    finally:
        codec.close()


@pytest.mark.parametrize("batch", ["b_2d_40x8i_c4"], indirect=True)
def test_refusals_leave_output_and_status_untouched(mi, batch):
    """every BAD_ARGS case of the padded calls, from HBM and from host containers: nothing is queued, d_out and d_status keep their bytes"""
    (frames, w, h, c, *_), imgs, conts, dev, codec = batch
    good = [(-2, -1, w, h)] * frames

    def refused(call):
        o = TOut(frames, 16, 16, c, "uint8", "hwc", 0, 0x7777)
        rc = call(o)
        if rc is not None:
            assert rc == mi.BAD_ARGS
        import torch

        torch.cuda.synchronize()
        assert (o.buf.cpu().numpy() == 0x5A).all() and int(o.st.item()) == 0x7777

    def py(rects, mode="edge", fill=None, ow=16, oh=16, flags=None, views=False):
        def call(o):
            for src in (dev, conts):
                with pytest.raises(mi.LlcompError) as e:
                    if views:
                        groups = [mi.ViewGroup([(f, *r) for f, r in enumerate(rects)], ow, oh, o.ptr)]
                        if isinstance(src, tuple):
                            codec.decode_views(src[0].data_ptr(), src[1], src[2].data_ptr(), groups, o.st.data_ptr(), stream=stream(), pad_mode=mode, fill=fill)
                        else:
                            codec.decode_views_host(src, groups, o.st.data_ptr(), stream=stream(), pad_mode=mode, fill=fill)
                    elif isinstance(src, tuple):
                        codec.decode_resized_regions(src[0].data_ptr(), src[1], src[2].data_ptr(), rects, ow, oh, o.ptr, o.st.data_ptr(), flags=flags,
                                                     stream=stream(), pad_mode=mode, fill=fill)
                    else:
                        codec.decode_resized_regions_host(src, rects, ow, oh, o.ptr, o.st.data_ptr(), flags=flags, stream=stream(), pad_mode=mode,
                                                          fill=fill)
                assert e.value.status == mi.BAD_ARGS
        return call

    def one(rect):
        return [rect] + good[1:]

    for views in (False, True):
        for mode in MODES:
            lx, ly = limit(mode, w), limit(mode, h)
            refused(py(one((-lx - 1, 0, lx + 2, h)), mode, views=views))        # a pad above the mode's limit: left
            refused(py(one((w - 1, 0, lx + 2, h)), mode, views=views))          # right
            refused(py(one((0, -ly - 1, w, ly + 2)), mode, views=views))        # top
            refused(py(one((0, h - 1, w, ly + 2)), mode, views=views))          # bottom
            refused(py(one((-5, 0, 5, h)), mode, views=views))                  # no image pixel: left of the image
            refused(py(one((w, 0, 4, h)), mode, views=views))                   # ... starting at its right edge
            refused(py(one((0, h, w, 1)), mode, views=views))                   # ... below it
        refused(py(one((0, 0, 0, h)), views=views))                             # every case of the unpadded call: an empty rectangle,
        refused(py(good, ow=0, views=views))                                    # an output side of 0,
    refused(py(good, flags=[6 << 4] * frames))                                  # a filter code of 6,
    refused(py(one((-w, 0, 3 * w, h)), "edge", ow=w // 8, flags=[spec.LANCZOS << 4] * frames))  # a downscale above the limit: r -> out's
    refused(py([(-w, 0, 3 * w, h, spec.LANCZOS << 4)] * frames, "edge", ow=w // 8, views=True))
    # without pad_mode and fill nothing changes: a negative origin is refused before the library sees it, one past the edge by the library
    refused(py(good, mode=None))
    refused(py([(w - 3, 0, 4, h)] + [(0, 0, w, h)] * (frames - 1), mode=None))
    # a NULL pad, a struct_size below the struct's, a mode above 3: through the C ABI itself
    L, Pad = codec._L, mi._lib.Pad
    tab = (C.c_int32 * (4 * frames))(*[v for r in good for v in r])
    ptrs, lens, _keep = mi._containers(conts)
    views = (mi._lib.View * frames)(*[mi._lib.View(f, *[v & 0xFFFFFFFF for v in r], 0) for f, r in enumerate(good)])
    for pad in (None, Pad(C.sizeof(Pad) - 1, 1, None), Pad(C.sizeof(Pad), 4, None)):
        p = C.byref(pad) if pad is not None else None
        refused(lambda o: L.llcomp_mi_codec_decode_padded_regions(codec._h, dev[0].data_ptr(), dev[1], dev[2].data_ptr(), tab, None, 16, 16, p, None, o.ptr,
                                                                  o.st.data_ptr(), stream()))
        refused(lambda o: L.llcomp_mi_codec_decode_padded_regions_host(codec._h, ptrs, lens, tab, None, 16, 16, p, None, o.ptr, o.st.data_ptr(), stream()))

        def group(o):
            return mi._lib.ViewGroup(C.sizeof(mi._lib.ViewGroup), frames, C.cast(views, C.POINTER(mi._lib.View)), 16, 16, None, o.ptr)

        refused(lambda o: L.llcomp_mi_codec_decode_padded_views(codec._h, dev[0].data_ptr(), dev[1], dev[2].data_ptr(), C.byref(group(o)), 1, p,
                                                                o.st.data_ptr(), stream()))
        refused(lambda o: L.llcomp_mi_codec_decode_padded_views_host(codec._h, ptrs, lens, C.byref(group(o)), 1, p, o.st.data_ptr(), stream()))
    # the same arguments with a good pad are taken
    ok = Pad(C.sizeof(Pad), 1, None)
    o = TOut(frames, 16, 16, c, "uint8", "hwc")
    assert L.llcomp_mi_codec_decode_padded_regions(codec._h, dev[0].data_ptr(), dev[1], dev[2].data_ptr(), tab, None, 16, 16, C.byref(ok), None, o.ptr,
                                                   o.st.data_ptr(), stream()) == mi.OK
    st, out = o.read()
    assert st == 0 and np.array_equal(out, expected(imgs, list(enumerate(good)), 16, 16, "edge", None, [0] * frames))


def test_close_shared_codecs():
    """(the codecs the tests above share)"""
    for *_, codec in _BATCHES.values():
        codec.close()
    _BATCHES.clear()
