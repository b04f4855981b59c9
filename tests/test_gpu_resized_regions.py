"""Resized regions decode (llcomp_mi_codec_decode_resized_regions, ..._host, llcomp_mi_stream_submit_decode_resized_regions): a rectangle
of its own size per frame, resampled to one output shape, optionally mirrored.  Containers come from the oracle; the expected output of
frame f is the numpy statement of the rule (tests/resize_spec.py) applied to img[f, y_f:y_f+rh_f, x_f:x_f+rw_f], byte for byte."""
import zlib

import numpy as np
import pytest

import orc as orc_mod
from conftest import make_image
from resize_spec import random_resized_crop, resize
from test_gpu_regions_host import GUARD, Out, make_batch, stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


def packed(mi, conts):
    import torch

    pay, lens = mi.pack_batch(conts)
    d_pay = torch.from_numpy(np.concatenate([pay, np.zeros(16, np.uint8)])).cuda()
    d_len = torch.from_numpy(lens.view(np.int32).copy()).cuda()
    return d_pay, len(pay), d_len


def expected(mi, imgs, rects, ow, oh, flags=None):
    return np.stack([resize(mi, imgs[f, y:y + rh, x:x + rw], ow, oh, bool(flags[f] & 1) if flags is not None else False)
                     for f, (x, y, rw, rh) in enumerate(rects)])


def run_device(mi, codec, dev, rects, ow, oh, c, flags=None):
    d_pay, n, d_len = dev
    o = Out(len(rects), ow, oh, c)
    codec.decode_resized_regions(d_pay.data_ptr(), n, d_len.data_ptr(), rects, ow, oh, o.ptr, o.st.data_ptr(), flags=flags, stream=stream())
    return o.read()


def run_host(mi, codec, conts, rects, ow, oh, c, flags=None):
    o = Out(len(rects), ow, oh, c)
    codec.decode_resized_regions_host(conts, rects, ow, oh, o.ptr, o.st.data_ptr(), flags=flags, stream=stream())
    return o.read()


# (name, frames, w, h, c, tile_w, tile_h, planar, small model, rw, rh, offsets)
FAMILIES = [
    ("rows_480x1p", 4, 1100, 24, 3, 480, 1, True, False, 300, 11, [(0, 0), (800, 13), (17, 5), (480, 0)]),
    ("tiles_64x64i", 4, 300, 200, 3, 64, 64, False, False, 100, 70, [(0, 0), (200, 130), (17, 90), (150, 3)]),
    ("partial_32x32p", 4, 100, 70, 3, 32, 32, True, False, 45, 30, [(0, 0), (55, 40), (30, 33), (3, 39)]),
    ("clamped_40x2_on_160x41p", 3, 160, 41, 3, 40, 2, True, False, 100, 1, [(10, 40), (0, 3), (60, 40)]),
    ("small_model_40x16p", 4, 300, 100, 3, 40, 16, True, True, 90, 33, [(0, 0), (210, 67), (100, 20), (45, 50)]),
]


@pytest.mark.parametrize("case", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_equal_rects_at_their_own_size_equal_decode_regions(mi, orc, case):
    name, frames, w, h, c, tw, th, planar, small, rw, rh, xy = case
    imgs, conts = make_batch(orc, frames, w, h, c, tw, th, planar, small_model=small)
    codec = mi.Codec(frames, w, h, c, tw, th, planar, device=0, small_model=small)
    try:
        dev = packed(mi, conts)
        st, out = run_device(mi, codec, dev, [(x, y, rw, rh) for x, y in xy], rw, rh, c)
        ref = Out(frames, rw, rh, c)
        codec.decode_regions(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), xy, rw, rh, ref.ptr, ref.st.data_ptr(), stream())
        st_r, out_r = ref.read()
        assert st == st_r == 0
        assert np.array_equal(out, out_r)
        assert np.array_equal(out, np.stack([imgs[f, y:y + rh, x:x + rw] for f, (x, y) in enumerate(xy)]))
    finally:
        codec.close()


def _batch_rects(rng, w, h, frames, kind):
    rects = [random_resized_crop(rng, w, h, scale=(0.02, 0.15) if kind == "corners" else (0.08, 1.0)) for _ in range(frames)]
    if kind == "corners":  # small rectangles, windows at the partial last tile column / row: 4 classes; a 1x1 rectangle and upscales
        rects[0] = (w - 1, h - 1, 1, 1)
        rects[1] = (0, h - 20, 25, 20)
        rects[2] = (w - 30, 0, 30, 17)
        rects[3] = (0, 0, 20, 20)
    elif kind == "full":  # the full image: every window is the whole image, one class
        rects[0] = (0, 0, w, h)
    elif kind == "two":  # only the x split
        rects = [(0, 0, 60, 40), (w - 60, 10, 60, 40), (5, 70, 33, 21), (w - 1, 0, 1, 1)][:frames]
    return rects


CROPS = [  # (name, w, h, c, tile_w, tile_h, planar, frames, kind, (ow, oh), classes)
    ("c3_224_corners", 300, 200, 3, 64, 64, True, 6, "corners", (224, 224), 4),
    ("c3_96x160_full", 300, 200, 3, 64, 64, True, 4, "full", (96, 160), 1),
    ("c1_224_two", 300, 200, 1, 64, 64, False, 4, "two", (224, 224), 2),
    ("c4_96x160_corners", 300, 200, 4, 64, 64, False, 5, "corners", (96, 160), 4),
    ("c5_224_random", 160, 90, 5, 32, 16, False, 4, "random", (224, 224), None),
    ("c3_rows_480x1p_224", 1100, 300, 3, 480, 1, True, 8, "random", (224, 224), None),
]


@pytest.mark.parametrize("case", CROPS, ids=[c[0] for c in CROPS])
def test_random_resized_crops(mi, orc, case):
    name, w, h, c, tw, th, planar, frames, kind, (ow, oh), n_cls = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    imgs, conts = make_batch(orc, frames, w, h, c, tw, th, planar)
    rects = _batch_rects(rng, w, h, frames, kind)
    flags = np.array([f % 2 for f in range(frames)], np.uint8)
    win, k = mi.resized_regions_plan(w, h, c, tw, th, planar, rects)
    if n_cls:
        assert k == n_cls, (k, win)
    codec = mi.Codec(frames, w, h, c, tw, th, planar, device=0)
    try:
        dev = packed(mi, conts)
        want = expected(mi, imgs, rects, ow, oh, flags)
        st, out = run_device(mi, codec, dev, rects, ow, oh, c, flags)
        assert st == 0 and np.array_equal(out, want)
        st, out = run_device(mi, codec, dev, rects, ow, oh, c)  # no flags: nothing mirrored
        assert st == 0 and np.array_equal(out, expected(mi, imgs, rects, ow, oh))
        # the host call: same bytes and status, fewer bytes staged than the payload
        codec.counters(reset=True)
        st_h, out_h = run_host(mi, codec, conts, rects, ow, oh, c, flags)
        assert st_h == 0 and np.array_equal(out_h, want)
        if kind in ("corners", "two"):
            assert 0 < codec.counters()["host_staged_bytes"] < dev[1]
    finally:
        codec.close()


def test_prepare_and_workspace(mi, orc):
    w, h, c = 300, 200, 3
    imgs, conts = make_batch(orc, 2, w, h, c, 64, 64, True)
    codec = mi.Codec(2, w, h, c, 64, 64, True, device=0)
    try:
        codec.prepare(encode=False, decode=False, resized=True)
        rects = [(0, 0, w, h), (10, 20, 3, 2)]
        st, out = run_host(mi, codec, conts, rects, 128, 96, c)
        assert st == 0 and np.array_equal(out, expected(mi, imgs, rects, 128, 96))
    finally:
        codec.close()


def test_containers_reusable_and_ring_in_flight(mi, orc):
    w, h, c = 300, 200, 3
    imgs, conts = make_batch(orc, 3, w, h, c, 64, 64, False)
    codec = mi.Codec(3, w, h, c, 64, 64, False, device=0)
    rng = np.random.default_rng(5)
    try:
        # nine calls queued (more than the ring has slots), none waited for; the host containers / rects overwritten at once
        jobs = []
        for i in range(9):
            rects = [random_resized_crop(rng, w, h) for _ in range(3)]
            flags = rng.integers(0, 2, size=3).astype(np.uint8)
            o = Out(3, 64, 48, c)
            mine, r_arr, f_arr = [bytearray(d) for d in conts], np.array(rects, np.uint32), flags.copy()
            if i % 2:
                codec.decode_resized_regions_host(mine, r_arr, 64, 48, o.ptr, o.st.data_ptr(), flags=f_arr, stream=stream())
            else:
                dev = packed(mi, conts)
                codec.decode_resized_regions(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), r_arr, 64, 48, o.ptr, o.st.data_ptr(), flags=f_arr,
                                             stream=stream())
            for d in mine:
                d[:] = bytes(len(d))
            r_arr[:] = 0
            f_arr[:] = 0
            jobs.append((rects, flags, o, dev if i % 2 == 0 else None))
        for rects, flags, o, _ in jobs:
            st, out = o.read()
            assert st == 0 and np.array_equal(out, expected(mi, imgs, rects, 64, 48, flags)), rects
    finally:
        codec.close()


def test_bad_args_write_nothing(mi, orc):
    w, h, c = 300, 200, 3
    imgs, conts = make_batch(orc, 2, w, h, c, 64, 64, True)
    codec = mi.Codec(2, w, h, c, 64, 64, True, device=0)
    dev = packed(mi, conts)
    good = [(0, 0, 100, 100), (5, 5, 30, 20)]
    try:
        for rects, ow, oh in (([(0, 0, 0, 10), good[1]], 32, 32), ([(201, 0, 100, 100), good[1]], 32, 32), ([(0, 101, 100, 100), good[1]], 32, 32),
                              (good, 0, 32), (good, 32, 0), ([(0, 0, 300, 10), good[1]], 4, 4), ([(0, 0, 10, 200), good[1]], 4, 3)):
            for host in (False, True):
                o = Out(2, max(ow, 1), max(oh, 1), c, status=0x77)
                with pytest.raises(mi.LlcompError) as e:
                    if host:
                        codec.decode_resized_regions_host(conts, rects, ow, oh, o.ptr, o.st.data_ptr(), stream=stream())
                    else:
                        codec.decode_resized_regions(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), rects, ow, oh, o.ptr, o.st.data_ptr(),
                                                     stream=stream())
                assert e.value.status == mi.BAD_ARGS, (rects, ow, oh, host)
                st, out = o.read()
                assert st == 0x77 and (out == 0x5A).all()
        # exactly 64x on both axes is allowed
        st, out = run_device(mi, codec, dev, [(0, 0, 256, 192), good[1]], 4, 3, c)
        assert st == 0 and np.array_equal(out, expected(mi, imgs, [(0, 0, 256, 192), good[1]], 4, 3))
    finally:
        codec.close()


def test_damage_inside_a_window(mi, orc):
    w, h, c, tw, th = 512, 256, 3, 32, 32  # 16 x 8 tiles, interleaved: slice id = tile row * 16 + tile column
    rects = [(100, 70, 60, 50), (300, 150, 20, 10)]
    win, _ = mi.resized_regions_plan(w, h, c, tw, th, False, rects)
    assert win.tolist() == [[3, 2, 6, 5], [9, 4, 12, 7]]  # frame 1's window is sized for frame 0's rectangle
    imgs = np.stack([make_image("nat", w, h, c), make_image("mid", w, h, c)])
    n = len(orc_mod.slice_rects(w, h, c, tw, th, False))
    clean = [orc.compress_sliced(imgs[f], tw, th, False) for f in range(2)]
    rng = np.random.default_rng(78)

    def damaged(spots):
        conts = []
        for f in range(2):
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

    codec = mi.Codec(2, w, h, c, tw, th, False, device=0)
    try:
        # frame 1, tile row 6, column 11: inside its window, outside its rectangle -- reported, as decode_regions reports window damage
        conts = damaged([(1, 6 * 16 + 11)])
        st, _ = run_device(mi, codec, packed(mi, conts), rects, 40, 40, c)
        st_h, _ = run_host(mi, codec, conts, rects, 40, 40, c)
        assert codec.status(st) == codec.status(st_h) == mi.BAD_EXPONENT
        # outside every window: OK, exact
        conts = damaged([(0, 0), (1, 7 * 16 + 15), (1, 3 * 16 + 8)])
        for st, out in (run_device(mi, codec, packed(mi, conts), rects, 40, 40, c), run_host(mi, codec, conts, rects, 40, 40, c)):
            assert st == 0 and np.array_equal(out, expected(mi, imgs, rects, 40, 40))
    finally:
        codec.close()


@pytest.mark.parametrize("fpj,devices", [(1, None), (4, None), (2, [0, 0])], ids=["fpj1", "fpj4", "fpj2_devices00"])
def test_stream_resized_jobs(mi, orc, fpj, devices):
    w, h, c, tw, th = 320, 48, 3, 80, 1
    n_jobs = 4
    imgs, conts = make_batch(orc, n_jobs * fpj, w, h, c, tw, th, True)
    s = mi.Stream(w, h, c, tw, th, True, depth=2, device=0, frames_per_job=fpj, devices=devices)
    codec = mi.Codec(fpj, w, h, c, tw, th, True, device=0)
    rng = np.random.default_rng(fpj)
    ow, oh = 56, 40
    try:
        for j in range(n_jobs):
            part = conts[j * fpj:(j + 1) * fpj]
            rects = [random_resized_crop(rng, w, h) for _ in range(fpj)]
            flags = np.array([(j + f) % 2 for f in range(fpj)], np.uint8)
            assert s.submit_decode_resized_regions(list(part), rects, ow, oh, flags=flags, tag=j)
            job = s.wait()
            assert (job.status, job.kind, job.tag) == (mi.OK, mi.JOB_DECODE_RESIZED_REGIONS, j)
            st, want = run_host(mi, codec, list(part), rects, ow, oh, c, flags)  # the codec call's bytes
            assert st == 0 and np.array_equal(want, expected(mi, imgs[j * fpj:(j + 1) * fpj], rects, ow, oh, flags))
            assert np.array_equal(job.data, want[0] if fpj == 1 else want)
            s.release(job)
        # an output larger than a slot holds, and a bad rectangle: the submit's own BAD_ARGS, nothing queued
        for rects, ow_, oh_ in (([(0, 0, 10, 10)] * fpj, w + 1, h), ([(w - 5, 0, 10, 10)] * fpj, ow, oh)):
            with pytest.raises(mi.LlcompError) as e:
                s.submit_decode_resized_regions(list(conts[:fpj]), rects, ow_, oh_)
            assert e.value.status == mi.BAD_ARGS
        assert s.pending() == 0
    finally:
        s.close()
        codec.close()


def test_buffers_stay_within_workspace_bytes(mi, orc):
    """calls whose largest rectangle keeps growing: the boxes and the horizontal pass's rows grow geometrically, but never past
    frames * w * h * c each, so the codec never holds more than workspace_bytes"""
    frames, w, h, c = 8, 600, 400, 3
    imgs, conts = make_batch(orc, frames, w, h, c, 64, 64, True)
    codec = mi.Codec(frames, w, h, c, 64, 64, True, device=0)
    try:
        codec.prepare(encode=False, decode=True, region=True, regions=True)
        before = codec.allocated_bytes()
        samples = frames * w * h * c
        tables = 2 * (16 + frames * (32 + 48 + 24 * (w + h)))  # (the staging buffer's share: tables and weights, doubled at most)
        dev = packed(mi, conts)
        rng = np.random.default_rng(11)
        # full-width rectangles: boxes and rows are both frames * 600 * hmax * c, and 90 -> 150 -> 250 -> 380 rows doubles them past the bound
        for hmax in (90, 150, 250, 380, 400):
            rects = [(0, int(rng.integers(0, h - hmax + 1)), w, hmax)] + [random_resized_crop(rng, w, h, scale=(0.02, 0.2)) for _ in range(frames - 1)]
            rects[1:] = [(x, y, min(rw, w), min(rh, hmax)) for x, y, rw, rh in rects[1:]]
            st, out = run_device(mi, codec, dev, rects, w, 64, c)
            assert st == 0 and np.array_equal(out, expected(mi, imgs, rects, w, 64)), hmax
            assert codec.allocated_bytes() <= codec.workspace_bytes
            assert codec.allocated_bytes() - before <= 2 * samples + tables, (hmax, codec.allocated_bytes() - before)
    finally:
        codec.close()


class OddOut:
    """an output buffer that starts one byte past a 4-byte boundary, with guard bytes on both sides, and a status word"""

    def __init__(self, frames, ow, oh, c):
        import torch

        self.n = frames * oh * ow * c
        self.shape = (frames, oh, ow, c)
        self.buf = torch.full((self.n + 2 * GUARD + 1,), 0x5A, dtype=torch.uint8, device="cuda")
        self.st = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD + 1
        assert self.ptr % 4 == 1

    def read(self):
        import torch

        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        assert (host[:GUARD + 1] == 0x5A).all() and (host[GUARD + 1 + self.n:] == 0x5A).all(), "a byte outside the output was written"
        return int(self.st.item()) & 0xFFFFFFFF, host[GUARD + 1:GUARD + 1 + self.n].reshape(self.shape)


def test_c4_unaligned_output(mi, orc):
    """c = 4 into an output that is not 4-byte aligned: the vertical pass takes its generic path, with the same bytes"""
    w, h, c = 300, 200, 4
    imgs, conts = make_batch(orc, 3, w, h, c, 64, 64, False)
    codec = mi.Codec(3, w, h, c, 64, 64, False, device=0)
    rects = [(0, 0, 120, 90), (150, 60, 40, 33), (299, 199, 1, 1)]
    flags = np.array([1, 0, 1], np.uint8)
    try:
        o = OddOut(3, 57, 43, c)
        codec.decode_resized_regions_host(conts, rects, 57, 43, o.ptr, o.st.data_ptr(), flags=flags, stream=stream())
        st, out = o.read()
        assert st == 0 and np.array_equal(out, expected(mi, imgs, rects, 57, 43, flags))
    finally:
        codec.close()
