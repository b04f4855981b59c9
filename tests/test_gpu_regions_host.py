"""Regions decode from HOST containers (llcomp_mi_codec_decode_regions_host, llcomp_mi_stream_submit_decode_regions): only the windows'
bytes cross PCIe, and the output and the status word are those of llcomp_mi_codec_decode_regions on pack_batch of the same containers.
Containers come from the oracle; the expected output of frame f is img[f, y_f:y_f+rh, x_f:x_f+rw]."""
import ctypes as C
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
    def _set(name, value):
        monkeypatch.setenv(name, value)
        mi.reload_tuning()

    yield _set
    monkeypatch.undo()
    mi.reload_tuning()


def make_batch(orc, frames, w, h, c, tw, th, planar, gens=("nat", "g3", "mid", "g1"), small_model=False):
    imgs = np.stack([np.ascontiguousarray(np.roll(make_image(gens[f % len(gens)], w, h, c), 7 * f, axis=1)) for f in range(frames)])
    orc.set_small_model(small_model)
    try:
        conts = [orc.compress_sliced(imgs[f], tw, th, planar) for f in range(frames)]
    finally:
        orc.set_small_model(False)
    return imgs, conts


def crops(imgs, xy, rw, rh):
    return np.stack([imgs[f, y:y + rh, x:x + rw] for f, (x, y) in enumerate(xy)])


class Out:
    """an output buffer with sentinel guard bytes on both sides, and a status word"""

    def __init__(self, frames, rw, rh, c, status=0):
        import torch

        self.n = frames * rh * rw * c
        self.shape = (frames, rh, rw, c)
        self.buf = torch.full((self.n + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        self.st = torch.full((1,), status, dtype=torch.int32, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD

    def read(self):
        import torch

        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        assert (host[:GUARD] == 0x5A).all() and (host[GUARD + self.n:] == 0x5A).all(), "a byte outside the output was written"
        return int(self.st.item()) & 0xFFFFFFFF, host[GUARD:GUARD + self.n].reshape(self.shape)


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def both(mi, codec, conts, xy, rw, rh, c):
    """(status word, output) of decode_regions_host and of decode_regions on pack_batch of the same containers"""
    import torch

    frames = len(conts)
    a, b = Out(frames, rw, rh, c), Out(frames, rw, rh, c)
    codec.decode_regions_host(conts, xy, rw, rh, a.ptr, a.st.data_ptr(), stream())
    pay, lens = mi.pack_batch(conts)
    d_pay = torch.from_numpy(np.concatenate([pay, np.zeros(16, np.uint8)])).cuda()
    d_len = torch.from_numpy(lens.view(np.int32).copy()).cuda()
    codec.decode_regions(d_pay.data_ptr(), len(pay), d_len.data_ptr(), xy, rw, rh, b.ptr, b.st.data_ptr(), stream())
    return a.read(), b.read()


def offsets(rng, w, h, rw, rh, frames):
    edges = [(0, 0), (w - rw, 0), (0, h - rh), (w - rw, h - rh)]
    return [edges[f] if f < len(edges) else (int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1))) for f in range(frames)]


# (name, frames, w, h, c, tile_w, tile_h, planar, small model, rw, rh, offsets (None: edges + random), key set in every class's family)
FAMILIES = [
    ("rows_480x1p", 4, 1100, 24, 3, 480, 1, True, False, 300, 11, None, "rows"),
    ("lds_table_128x128p", 6, 600, 300, 3, 128, 128, True, False, 200, 150, None, "lds_table"),
    ("bank_cache_64x64p_2cls", 8, 404, 328, 3, 64, 64, True, False, 300, 250, [(0, 0), (100, 0)] * 4, "bank_cache"),
    ("bank_cache_64x64p_4cls", 12, 404, 328, 3, 64, 64, True, False, 300, 250, [(0, 0), (100, 0), (0, 70), (100, 70)] * 3, "bank_cache"),
    ("clamped_40x2_on_160x41p", 3, 160, 41, 3, 40, 2, True, False, 100, 1, [(10, 40), (0, 3), (60, 40)], None),
    ("c5_interleaved_32x16", 6, 160, 90, 5, 32, 16, False, False, 50, 30, None, None),
    ("small_model_40x16p", 4, 300, 100, 3, 40, 16, True, True, 90, 33, None, None),
]


@pytest.mark.parametrize("case", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_equal_to_decode_regions_per_family(mi, orc, case):
    name, frames, w, h, c, tw, th, planar, small, rw, rh, xy, key = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    imgs, conts = make_batch(orc, frames, w, h, c, tw, th, planar, small_model=small)
    codec = mi.Codec(frames, w, h, c, tw, th, planar, device=0, small_model=small)
    try:
        xy = xy or offsets(rng, w, h, rw, rh, frames)
        fams = codec.regions_family(xy, rw, rh)
        if key:
            assert all(f[key] for f in fams), (name, fams)
        if name.startswith("clamped"):
            assert len(fams) == 2 and fams[0]["rows"] != fams[1]["rows"], fams
        if "cls" in name:
            assert len(fams) == int(name[-4]), fams
        for (sa, oa), (sb, ob) in [both(mi, codec, conts, xy, rw, rh, c)]:
            assert sa == sb == 0, (sa, sb)
            assert np.array_equal(oa, ob)
            assert np.array_equal(oa, crops(imgs, xy, rw, rh))
    finally:
        codec.close()


def test_forced_lane_shift(mi, orc, set_hook):
    set_hook("LLCOMP_MI_LANE_SHIFT", "3")
    w, h, c = 300, 200, 3
    imgs, conts = make_batch(orc, 4, w, h, c, 64, 64, False)
    codec = mi.Codec(4, w, h, c, 64, 64, False, device=0)
    xy = [(0, 0), (200, 0), (0, 130), (200, 130)]
    assert all(f["lane_shift"] == 3 for f in codec.regions_family(xy, 100, 70))
    (sa, oa), (sb, ob) = both(mi, codec, conts, xy, 100, 70, c)
    assert sa == sb == 0 and np.array_equal(oa, ob) and np.array_equal(oa, crops(imgs, xy, 100, 70))
    codec.close()


def _bad_stream(orc, rng, sw, sh, nch):
    res = orc_mod.adversarial_residuals(rng, sh, sw, nch, "small")
    return orc.encode_residuals(res, run_at=sh * sw * nch // 2, run_len=33)[0]


def test_damage_and_gather_errors(mi, orc):
    w, h, c, tw, th = 512, 256, 3, 32, 32  # 16 x 8 tiles, interleaved: slice id = tile row * 16 + tile column
    rw, rh = 60, 50
    xy = [(100, 70), (300, 150)]           # windows: frame 0 columns 3..5, rows 2..4; frame 1 columns 9..11, rows 4..6
    assert mi.regions_plan(w, h, c, tw, th, False, rw, rh, xy)[0].tolist() == [[3, 2, 6, 5], [9, 4, 12, 7]]
    imgs = np.stack([make_image("nat", w, h, c), make_image("mid", w, h, c)])
    rects = orc_mod.slice_rects(w, h, c, tw, th, False)
    rng = np.random.default_rng(78)
    clean = [orc.compress_sliced(imgs[f], tw, th, False) for f in range(2)]

    def damaged(spots):
        conts = []
        for f in range(2):
            d = clean[f]
            n = len(rects)
            lens = np.frombuffer(d[24:24 + 4 * n], dtype="<u4").astype(np.int64)
            offs = np.concatenate([[0], np.cumsum(lens)]) + 24 + 4 * n
            pays = [d[offs[j]:offs[j + 1]] for j in range(n)]
            for (ff, j) in spots:
                if ff == f:
                    pays[j] = _bad_stream(orc, rng, tw, th, c)
            conts.append(orc_mod.sliced_container(w, h, c, tw, th, False, pays))
        return conts

    codec = mi.Codec(2, w, h, c, tw, th, False, device=0)
    # inside a window (frame 0, tile row 4, column 5: outside the rectangle, inside the window): the verdict of decode_regions
    (sa, _), (sb, _) = both(mi, codec, damaged([(0, 4 * 16 + 5)]), xy, rw, rh, c)
    assert codec.status(sa) == codec.status(sb) == mi.BAD_EXPONENT
    # outside every window: OK, the pixels are exact
    (sa, oa), (sb, ob) = both(mi, codec, damaged([(0, 0), (0, 7 * 16 + 15), (1, 3 * 16 + 4), (1, 4 * 16 + 8)]), xy, rw, rh, c)
    assert sa == sb == 0 and np.array_equal(oa, ob) and np.array_equal(oa, crops(imgs, xy, rw, rh))
    # a gather error leaves d_px and d_status untouched: a window slice cut short, a rectangle outside the image, a foreign container
    t = np.frombuffer(clean[1][24:24 + 4 * len(rects)], dtype="<u4").astype(np.int64)
    end6_11 = 24 + 4 * len(rects) + int(t[:6 * 16 + 12].sum())
    for conts, xy_, want in (([clean[0], clean[1][:end6_11 - 1]], xy, mi.TRUNCATED), (clean, [(100, 70), (460, 0)], mi.BAD_ARGS),
                             ([clean[0], orc.compress_sliced(imgs[1], 32, 16, False)], xy, mi.BAD_ARGS)):
        o = Out(2, rw, rh, c, status=0x77)
        with pytest.raises(mi.LlcompError) as e:
            codec.decode_regions_host(conts, xy_, rw, rh, o.ptr, o.st.data_ptr(), stream())
        assert e.value.status == want
        st, out = o.read()
        assert st == 0x77 and (out == 0x5A).all()
    # cut right behind the last window slice of frame 1 (the rest lies outside every window): OK
    o = Out(2, rw, rh, c)
    codec.decode_regions_host([clean[0], clean[1][:end6_11]], xy, rw, rh, o.ptr, o.st.data_ptr(), stream())
    st, out = o.read()
    assert st == 0 and np.array_equal(out, crops(imgs, xy, rw, rh))
    codec.close()


def test_containers_reusable_when_the_call_returns(mi, orc):
    w, h, c = 300, 200, 3
    imgs, conts = make_batch(orc, 4, w, h, c, 64, 64, True)
    codec = mi.Codec(4, w, h, c, 64, 64, True, device=0)
    xy = [(0, 0), (200, 130), (17, 90), (150, 3)]
    o = Out(4, 100, 70, c)
    mine = [bytearray(d) for d in conts]
    xy_arr = np.array(xy, np.uint32)
    codec.decode_regions_host(mine, xy_arr, 100, 70, o.ptr, o.st.data_ptr(), stream())
    for d in mine:  # before any synchronise
        d[:] = bytes(len(d))
    xy_arr[:] = 0
    st, out = o.read()
    assert st == 0 and np.array_equal(out, crops(imgs, xy, 100, 70))
    codec.close()


def test_ring_many_calls_in_flight(mi, orc):
    """more calls queued than the ring has slots, none waited for in between, each with its own offsets and output"""
    w, h, c = 300, 200, 3
    imgs, conts = make_batch(orc, 3, w, h, c, 64, 64, False)
    codec = mi.Codec(3, w, h, c, 64, 64, False, device=0)
    rng = np.random.default_rng(21)
    xys = [[(int(rng.integers(0, 201)), int(rng.integers(0, 131))) for _ in range(3)] for _ in range(9)]
    outs = [Out(3, 100, 70, c) for _ in xys]
    for xy, o in zip(xys, outs):
        codec.decode_regions_host(conts, xy, 100, 70, o.ptr, o.st.data_ptr(), stream())
    for xy, o in zip(xys, outs):
        st, out = o.read()
        assert st == 0 and np.array_equal(out, crops(imgs, xy, 100, 70)), xy
    codec.close()


def test_staging_grows_and_counts_the_staged_bytes(mi, orc):
    import torch

    w, h, c, tw, th = 480, 64, 3, 96, 1
    imgs, conts = make_batch(orc, 4, w, h, c, tw, th, True)
    codec = mi.Codec(4, w, h, c, tw, th, True, device=0)
    codec.counters(reset=True)
    staged = 0
    for rw, rh, xy in ((1, 1, [(0, 0), (479, 63), (100, 5), (7, 40)]), (30, 4, [(0, 0), (450, 60), (96, 8), (191, 3)]),
                       (w, h, [(0, 0)] * 4)):
        o = Out(4, rw, rh, c)
        codec.decode_regions_host(conts, xy, rw, rh, o.ptr, o.st.data_ptr(), stream())
        st, out = o.read()
        assert st == 0 and np.array_equal(out, crops(imgs, xy, rw, rh)), (rw, rh)
        staged += len(mi.regions_gather(conts, xy, rw, rh)[0])
        assert codec.counters()["host_staged_bytes"] == staged
    # the whole-image crop is a full decode
    pay, lens = mi.pack_batch(conts)
    assert staged > len(pay)  # (the last call alone staged every payload byte)
    full = torch.empty((4, h, w, c), dtype=torch.uint8, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_pay = torch.from_numpy(pay).cuda()
    d_len = torch.from_numpy(lens.view(np.int32).copy()).cuda()
    codec.decode(d_pay.data_ptr(), len(pay), d_len.data_ptr(), full.data_ptr(), st.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.array_equal(full.cpu().numpy(), imgs) and np.array_equal(out, imgs)
    assert codec.counters()["host_staged_bytes"] == staged  # (a decode from HBM stages nothing)
    codec.close()


def _parts(mi, s, job, n):
    from llcomp_amd import _lib

    sizes = []
    for f in range(n):
        p, m = C.c_void_p(), C.c_uint64()
        assert _lib.load().llcomp_mi_stream_result_part(s._h, job.slot, f, C.byref(p), C.byref(m)) == mi.OK
        sizes.append(m.value)
    return sizes


@pytest.mark.parametrize("fpj,devices", [(1, None), (4, None), (2, [0, 0])], ids=["fpj1", "fpj4", "fpj2_devices00"])
def test_stream_region_jobs(mi, orc, fpj, devices):
    w, h, c, tw, th = 320, 48, 3, 80, 1
    n_jobs = 5
    imgs, conts = make_batch(orc, n_jobs * fpj, w, h, c, tw, th, True)
    s = mi.Stream(w, h, c, tw, th, True, depth=2, device=0, frames_per_job=fpj, devices=devices)
    rng = np.random.default_rng(fpj)
    rw, rh = 70, 9
    try:
        # region jobs mixed with full decode jobs, taken one at a time
        for j in range(n_jobs):
            part = conts[j * fpj:(j + 1) * fpj]
            xy = [(int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1))) for _ in range(fpj)]
            assert s.submit_decode_regions(list(part), xy, rw, rh, tag=2 * j)
            assert s.submit_decode(np.frombuffer(part[0], np.uint8).copy() if fpj == 1 else [np.frombuffer(d, np.uint8).copy() for d in part],
                                   tag=2 * j + 1)
            job = s.wait()
            assert (job.status, job.kind, job.tag) == (mi.OK, mi.JOB_DECODE_REGIONS, 2 * j)
            want = crops(imgs[j * fpj:(j + 1) * fpj], xy, rw, rh)
            assert np.array_equal(job.data, want[0] if fpj == 1 else want)
            assert _parts(mi, s, job, fpj) == [rw * rh * c] * fpj
            s.release(job)
            job = s.wait()
            assert (job.status, job.kind, job.tag) == (mi.OK, mi.JOB_DECODE, 2 * j + 1)
            assert np.array_equal(job.data, imgs[j * fpj] if fpj == 1 else imgs[j * fpj:(j + 1) * fpj])
            s.release(job)
        # back-pressure: every slot holds a region job -> BUSY (False) until one is released
        xy = [(0, 0)] * fpj
        part = conts[:fpj]
        taken = 0
        while s.submit_decode_regions(part, xy, rw, rh, tag=100 + taken):
            taken += 1
        assert taken == 2 * (len(devices) if devices else 1)
        jobs = [s.wait() for _ in range(taken)]
        assert all(jb.status == mi.OK and np.array_equal(jb.data.reshape(fpj, rh, rw, c), crops(imgs[:fpj], xy, rw, rh)) for jb in jobs)
        assert not s.submit_decode_regions(part, xy, rw, rh)
        s.release(jobs[0])
        assert s.submit_decode_regions(part, xy, rw, rh, tag=200)
        for jb in jobs[1:]:
            s.release(jb)
        job = s.wait()
        assert job.tag == 200 and job.status == mi.OK
        s.release(job)
        # a gather error is the submit's own, nothing is queued
        with pytest.raises(mi.LlcompError) as e:
            s.submit_decode_regions(part, [(w - rw + 1, 0)] * fpj, rw, rh)
        assert e.value.status == mi.BAD_ARGS
        assert s.pending() == 0
    finally:
        s.close()
