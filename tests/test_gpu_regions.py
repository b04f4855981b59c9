"""Regions decode on the GPU (llcomp_mi_codec_decode_regions): a rectangle of one size at an offset of its own in every frame of a
batch, bit for bit, into one dense [frames][rh][rw][c] buffer.  Containers come from the oracle, so none of this depends on the HIP
encoder; the expected output of frame f is img[f, y_f:y_f+rh, x_f:x_f+rw]."""
import zlib

import numpy as np
import pytest

import orc as orc_mod
from conftest import make_image

pytestmark = pytest.mark.gpu

GUARD = 4096


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


@pytest.fixture
def set_hook(mi, monkeypatch):
    """the library reads its LLCOMP_MI_* hooks once per process: a test that changes one has them read again"""
    def _set(name, value):
        monkeypatch.setenv(name, value)
        mi.reload_tuning()

    yield _set
    monkeypatch.undo()
    mi.reload_tuning()


class Batch:
    """frames of one shape as the codec takes them: the oracle's containers, packed by pack_batch, in HBM"""

    def __init__(self, mi, orc, frames, w, h, c, tw, th, planar, gens, small_model=False, containers=None):
        self.shape = (w, h, c, tw, th, planar)
        self.small_model = small_model
        self.imgs = np.stack([np.ascontiguousarray(np.roll(make_image(gens[i % len(gens)], w, h, c), 7 * i, axis=1)) for i in range(frames)])
        if containers is None:
            orc.set_small_model(small_model)
            try:
                containers = [orc.compress_sliced(self.imgs[f], tw, th, planar) for f in range(frames)]
            finally:
                orc.set_small_model(False)
        self.containers = containers
        self.upload(*mi.pack_batch(containers))

    def upload(self, pay, lens):
        import torch

        self.pay, self.lens = pay, lens
        self.total = len(pay)
        self.d_pay = torch.from_numpy(np.concatenate([pay, np.zeros(16, np.uint8)])).cuda()
        self.d_len = torch.from_numpy(lens.view(np.int32).copy()).cuda()
        self.d_st = torch.zeros(1, dtype=torch.int32, device="cuda")

    def codec(self, mi):
        w, h, c, tw, th, planar = self.shape
        return mi.Codec(len(self.imgs), w, h, c, tw, th, planar, device=0, small_model=self.small_model)


def decode_regions(mi, codec, b, xy, rw, rh, want=None, payload_bytes=None):
    """codec.decode_regions into a buffer with sentinel guard bytes on both sides -> (status, [frames][rh][rw][c] host array); the
    guards must stay untouched, and with want=OK every frame's rectangle must be exact"""
    import torch

    frames, c = b.imgs.shape[0], b.imgs.shape[3]
    n = frames * rh * rw * c
    buf = torch.full((n + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    codec.decode_regions(b.d_pay.data_ptr(), b.total if payload_bytes is None else payload_bytes, b.d_len.data_ptr(), xy, rw, rh,
                         buf.data_ptr() + GUARD, b.d_st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    status = codec.status(int(b.d_st.item()) & 0xFFFFFFFF)
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 0x5A).all() and (host[GUARD + n:] == 0x5A).all(), "a byte outside the output was written"
    out = host[GUARD:GUARD + n].reshape(frames, rh, rw, c)
    if want is not None:
        assert status == want, (status, want)
    if status == mi.OK:
        for f, (x, y) in enumerate(xy):
            assert np.array_equal(out[f], b.imgs[f, y:y + rh, x:x + rw]), (f, x, y, rw, rh)
    return status, out


def offsets(rng, w, h, rw, rh, frames):
    """the origin, the last partial tile column, the last partial tile row, both, and random offsets for the rest"""
    edges = [(0, 0), (w - rw, 0), (0, h - rh), (w - rw, h - rh)]
    return [edges[f] if f < len(edges) else (int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1))) for f in range(frames)]


def tile_offsets(rng, w, h, tw, th, frames):
    """a rectangle that is exactly one whole tile, at tile-aligned offsets"""
    return [(int(rng.integers(0, (w - tw) // tw + 1)) * tw, int(rng.integers(0, (h - th) // th + 1)) * th) for _ in range(frames)]


# (name, w, h, c, tile_w, tile_h, planar, generator, rw, rh, key that must be set in every class's family)
FAMILIES = [
    ("rows_480x1p", 1100, 24, 3, 480, 1, True, "nat", 300, 11, "rows"),
    ("tiles_64x64i", 300, 200, 3, 64, 64, False, "mid", 100, 70, None),
    ("planes_128x128p", 600, 300, 3, 128, 128, True, "nat", 200, 150, None),
    ("clamped_40x2_on_160x41p", 160, 41, 3, 40, 2, True, "nat", 100, 1, None),
    ("clamped_40x2_on_160x41i", 160, 41, 3, 40, 2, False, "nat", 70, 3, None),
    ("c5_interleaved_32x16", 160, 90, 5, 32, 16, False, "g1", 50, 30, None),
    ("c7_planar_rows_40x1", 160, 30, 7, 40, 1, True, "g1", 70, 20, "rows"),
    ("c7_interleaved_24x16", 100, 50, 7, 24, 16, False, "mid", 40, 20, None),
]


@pytest.mark.parametrize("case", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_regions_equal_crops_per_family(mi, orc, case):
    name, w, h, c, tw, th, planar, gen, rw, rh, key = case
    frames = 6
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    b = Batch(mi, orc, frames, w, h, c, tw, th, planar, [gen, "g3", "mid", "checker", "nat", "g1"])
    codec = b.codec(mi)
    try:
        for xy, (rrw, rrh) in ((offsets(rng, w, h, rw, rh, frames), (rw, rh)),
                               (tile_offsets(rng, w, h, min(tw, w), min(th, h), frames), (min(tw, w), min(th, h))),
                               ([(0, 0)] * frames, (w, h)),
                               (offsets(rng, w, h, 1, 1, frames), (1, 1))):
            fams = codec.regions_family(xy, rrw, rrh)
            _, n_classes = mi.regions_plan(w, h, c, tw, th, planar, rrw, rrh, xy)
            assert fams is not None and len(fams) == n_classes
            if key and (rrw, rrh) == (rw, rh):
                assert all(f[key] for f in fams), (name, fams)
            decode_regions(mi, codec, b, xy, rrw, rrh, want=mi.OK)
    finally:
        codec.close()


def test_clamped_tile_classes_run_different_families(mi, orc):
    """160x41 in 40x2 tiles, 1-row rectangles: a window in the 1-row remainder runs the row kernels, the others the 2-D ones, in one call"""
    b = Batch(mi, orc, 3, 160, 41, 3, 40, 2, True, ["nat"])
    codec = b.codec(mi)
    xy = [(10, 40), (0, 3), (60, 40)]
    fams = codec.regions_family(xy, 100, 1)
    assert len(fams) == 2 and not fams[0]["rows"] and fams[1]["rows"], fams
    decode_regions(mi, codec, b, xy, 100, 1, want=mi.OK)
    codec.close()


def test_equal_offsets_equal_decode_region(mi, orc):
    import torch

    for (w, h, c, tw, th, planar, rw, rh) in ((300, 200, 3, 64, 64, False, 100, 70), (1100, 24, 3, 480, 1, True, 300, 11),
                                              (160, 90, 5, 32, 16, False, 50, 30)):
        b = Batch(mi, orc, 4, w, h, c, tw, th, planar, ["nat", "mid", "g3", "g1"])
        codec = b.codec(mi)
        for (x, y) in ((0, 0), (w - rw, h - rh), (w // 3, h // 5)):
            _, got = decode_regions(mi, codec, b, [(x, y)] * 4, rw, rh, want=mi.OK)
            one = torch.empty((4, rh, rw, c), dtype=torch.uint8, device="cuda")
            codec.decode_region(b.d_pay.data_ptr(), b.total, b.d_len.data_ptr(), x, y, rw, rh, one.data_ptr(), b.d_st.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert int(b.d_st.item()) == 0
            assert np.array_equal(got, one.cpu().numpy())
        codec.close()


def test_one_two_and_four_classes(mi, orc):
    w, h, c, tw, th = 300, 200, 3, 32, 16  # 300 % 32 and 200 % 16 are both non-zero
    b = Batch(mi, orc, 4, w, h, c, tw, th, False, ["nat", "mid", "g3", "g1"])
    codec = b.codec(mi)
    rw, rh = 40, 20
    for xy, want in (([(0, 0), (10, 5), (100, 100), (200, 40)], 1), ([(0, 0), (260, 0), (10, 5), (255, 3)], 2),
                     ([(0, 0), (0, 180), (100, 7), (1, 170)], 2), ([(0, 0), (260, 0), (0, 180), (260, 180)], 4)):
        assert mi.regions_plan(w, h, c, tw, th, False, rw, rh, xy)[1] == want
        assert len(codec.regions_family(xy, rw, rh)) == want
        decode_regions(mi, codec, b, xy, rw, rh, want=mi.OK)
    codec.close()
    # tile-aligned images have one class: 4K-like widths at 480x1
    b = Batch(mi, orc, 3, 960, 8, 3, 480, 1, True, ["nat"])
    codec = b.codec(mi)
    xy = [(0, 0), (736, 4), (300, 2)]
    assert len(codec.regions_family(xy, 224, 4)) == 1
    decode_regions(mi, codec, b, xy, 224, 4, want=mi.OK)
    codec.close()


def test_small_model(mi, orc):
    b = Batch(mi, orc, 4, 300, 100, 3, 40, 16, True, ["mid", "nat"], small_model=True)
    codec = b.codec(mi)
    rng = np.random.default_rng(3)
    decode_regions(mi, codec, b, offsets(rng, 300, 100, 90, 33, 4), 90, 33, want=mi.OK)
    codec.close()


@pytest.mark.parametrize("hook", [("LLCOMP_MI_NOCACHE", "1"), ("LLCOMP_MI_FORCE_REPLAY", "1"), ("LLCOMP_MI_LANE_SHIFT", "3"),
                                  ("LLCOMP_MI_NOLDSTAB", "1")], ids=["nocache", "force_replay", "lane_shift3", "noldstab"])
def test_hooks(mi, orc, set_hook, hook):
    set_hook(*hook)
    rng = np.random.default_rng(5)
    for (w, h, c, tw, th, planar, rw, rh) in ((800, 420, 3, 32, 32, False, 300, 200), (300, 200, 3, 64, 64, False, 100, 70),
                                              (600, 20, 3, 120, 1, True, 250, 9)):
        b = Batch(mi, orc, 4, w, h, c, tw, th, planar, ["g3", "nat", "mid"])
        codec = b.codec(mi)
        xy = offsets(rng, w, h, rw, rh, 4)
        fams = codec.regions_family(xy, rw, rh)
        if hook[0] == "LLCOMP_MI_NOCACHE":
            assert not any(f["bank_cache"] for f in fams)
        if hook[0] == "LLCOMP_MI_NOLDSTAB":
            assert not any(f["lds_table"] for f in fams)
        if hook[0] == "LLCOMP_MI_LANE_SHIFT":
            assert all(f["lane_shift"] == 3 for f in fams)
        decode_regions(mi, codec, b, xy, rw, rh, want=mi.OK)
        codec.close()


def _spans(lens):
    return np.concatenate([[0], np.cumsum(lens.astype(np.int64))])


def _bad_stream(orc, rng, sw, sh, nch):
    """a slice stream the decoders reject with BAD_EXPONENT: a unary run of 33 ones halfway"""
    res = orc_mod.adversarial_residuals(rng, sh, sw, nch, "small")
    return orc.encode_residuals(res, run_at=sh * sw * nch // 2, run_len=33)[0]


def test_damage_inside_and_outside_the_windows(mi, orc):
    w, h, c, tw, th = 512, 256, 3, 32, 32  # 16 x 8 tiles, interleaved: slice id = tile row * 16 + tile column
    rw, rh = 60, 50                        # windows of 3 x 3 tiles
    xy = [(100, 70), (300, 150)]           # frame 0: window columns 3..5, rows 2..4; frame 1: columns 9..11, rows 4..6
    assert mi.regions_plan(w, h, c, tw, th, False, rw, rh, xy)[0].tolist() == [[3, 2, 6, 5], [9, 4, 12, 7]]
    imgs = [make_image("nat", w, h, c), make_image("mid", w, h, c)]
    rects = orc_mod.slice_rects(w, h, c, tw, th, False)
    rng = np.random.default_rng(77)

    def batch(damaged):
        conts = []
        for f in range(2):
            d = orc.compress_sliced(imgs[f], tw, th, False)
            n = len(rects)
            lens = np.frombuffer(d[24:24 + 4 * n], dtype="<u4")
            offs = _spans(lens) + 24 + 4 * n
            pays = [d[offs[j]:offs[j + 1]] for j in range(n)]
            for (ff, j) in damaged:
                if ff == f:
                    pays[j] = _bad_stream(orc, rng, tw, th, c)
            conts.append(orc_mod.sliced_container(w, h, c, tw, th, False, pays))
        b = Batch(mi, orc, 2, w, h, c, tw, th, False, ["nat"], containers=conts)
        b.imgs = np.stack(imgs)
        return b

    codec = mi.Codec(2, w, h, c, tw, th, False, device=0)
    # a window tile outside the rectangle (frame 0, tile row 4, column 5): reported
    b = batch([(0, 4 * 16 + 5)])
    assert orc.decompress(b.containers[0])[0] == orc_mod.BAD_EXPONENT
    decode_regions(mi, codec, b, xy, rw, rh, want=mi.BAD_EXPONENT)
    # outside every window -- including a tile of frame 0's window damaged in frame 1: never seen, the pixels are exact
    b = batch([(0, 0), (0, 7 * 16 + 15), (1, 3 * 16 + 4), (1, 4 * 16 + 8), (1, 7 * 16 + 10)])
    decode_regions(mi, codec, b, xy, rw, rh, want=mi.OK)
    # a covered slice cut short: the last slice of frame 1's window (row 6, column 11) ends the payload
    b = batch([])
    sp = _spans(b.lens)
    last = 128 + 6 * 16 + 11
    assert b.lens[last] > 2
    decode_regions(mi, codec, b, xy, rw, rh, want=mi.TRUNCATED, payload_bytes=int(sp[last] + b.lens[last] // 2))
    decode_regions(mi, codec, b, xy, rw, rh, want=mi.OK, payload_bytes=int(sp[last + 1]))
    codec.close()


def test_bad_arguments_launch_nothing(mi, orc):
    import torch

    w, h, c = 160, 90, 3
    b = Batch(mi, orc, 3, w, h, c, 32, 16, True, ["nat"])
    codec = b.codec(mi)
    buf = torch.full((3 * 20 * 30 * c,), 0x5A, dtype=torch.uint8, device="cuda")
    b.d_st.fill_(0x77)
    st = torch.cuda.current_stream().cuda_stream
    for xy, rw, rh in (([(0, 0), (131, 0), (0, 0)], 30, 20), ([(0, 0), (0, 71), (0, 0)], 30, 20), ([(0, 0)] * 3, 0, 20),
                       ([(0, 0)] * 3, 30, 0), ([(160, 0)] * 3, 1, 1), ([(10, 0)] * 3, 2**32 - 5, 1), ([(0, 0)] * 2, 30, 20),
                       ([(0, 0)] * 4, 30, 20)):
        with pytest.raises(mi.LlcompError) as e:
            codec.decode_regions(b.d_pay.data_ptr(), b.total, b.d_len.data_ptr(), xy, rw, rh, buf.data_ptr(), b.d_st.data_ptr(), st)
        assert e.value.status == mi.BAD_ARGS, (xy, rw, rh)
        if len(xy) == 3:
            assert codec.regions_family(xy, rw, rh) is None
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0x5A).all() and int(b.d_st.item()) == 0x77
    codec.close()


def test_prepare_ahead(mi, orc):
    b = Batch(mi, orc, 3, 160, 90, 3, 32, 16, True, ["nat"])
    codec = b.codec(mi)
    codec.prepare(encode=False, decode=False, regions=True)
    codec.prepare(encode=False, decode=True, regions=True)  # (idempotent)
    decode_regions(mi, codec, b, [(0, 0), (130, 70), (33, 17)], 30, 20, want=mi.OK)
    codec.close()


def test_state_tables_across_generation_wraps(mi, orc):
    """one codec with state tables in HBM, ~200 calls alternating full decodes with two-class regions decodes (two generations each):
    more than 255 generations, the tagged tables are shared safely, every output is exact"""
    import torch

    w, h, c, tw, th = 650, 330, 3, 32, 32
    b = Batch(mi, orc, 4, w, h, c, tw, th, False, ["nat", "mid", "g3", "g1"])
    codec = b.codec(mi)
    assert not codec.family["rows"] and not codec.family["lds_table"]
    codec.prepare(encode=False, decode=True, regions=True)
    st = torch.cuda.current_stream().cuda_stream
    rw, rh = 500, 250
    shapes = [[(0, 0), (10, 5), (140, 0), (150, 60)], [(0, 70), (3, 3), (20, 80), (100, 10)]]  # classes {0, 1} and {0, 2}
    wants = []
    for xy in shapes:
        fams = codec.regions_family(xy, rw, rh)
        assert len(fams) == 2 and all(not f["rows"] and not f["lds_table"] for f in fams), fams
        wants.append(torch.from_numpy(np.stack([b.imgs[f, y:y + rh, x:x + rw] for f, (x, y) in enumerate(xy)])).cuda())
    want_full = torch.from_numpy(b.imgs).cuda()
    full = torch.empty_like(want_full)
    out = torch.empty((4, rh, rw, c), dtype=torch.uint8, device="cuda")
    codec.counters(reset=True)
    for i in range(200):
        if i % 2 == 0:
            full.fill_(0)
            codec.decode(b.d_pay.data_ptr(), b.total, b.d_len.data_ptr(), full.data_ptr(), b.d_st.data_ptr(), st)
            ok = torch.equal(full, want_full)
        else:
            k = (i // 2) % 2
            out.fill_(0)
            codec.decode_regions(b.d_pay.data_ptr(), b.total, b.d_len.data_ptr(), np.array(shapes[k], np.uint32), rw, rh, out.data_ptr(),
                                 b.d_st.data_ptr(), st)
            ok = torch.equal(out, wants[k])
        assert ok and int(b.d_st.item()) == 0, i
    assert codec.counters()["generation_wraps"] >= 1
    codec.close()


def test_many_calls_in_flight(mi, orc):
    """more calls queued than the staging ring has slots, none waited for in between: every call's table is its own"""
    import torch

    w, h, c = 300, 200, 3
    b = Batch(mi, orc, 3, w, h, c, 64, 64, False, ["nat", "mid", "g1"])
    codec = b.codec(mi)
    rng = np.random.default_rng(12)
    st = torch.cuda.current_stream().cuda_stream
    xys = [offsets(rng, w, h, 100, 70, 3)[::-1] if i % 3 == 0 else [(int(rng.integers(0, 201)), int(rng.integers(0, 131))) for _ in range(3)]
           for i in range(11)]
    outs = [torch.empty((3, 70, 100, c), dtype=torch.uint8, device="cuda") for _ in xys]
    for xy, o in zip(xys, outs):
        codec.decode_regions(b.d_pay.data_ptr(), b.total, b.d_len.data_ptr(), xy, 100, 70, o.data_ptr(), b.d_st.data_ptr(), st)
    torch.cuda.synchronize()
    assert int(b.d_st.item()) == 0
    for xy, o in zip(xys, outs):
        got = o.cpu().numpy()
        for f, (x, y) in enumerate(xy):
            assert np.array_equal(got[f], b.imgs[f, y:y + 70, x:x + 100]), (xy, f)
    codec.close()
