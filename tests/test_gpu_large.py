"""Batches and frames past 2^31 and 2^32 samples, checked byte for byte against the oracle's per-slice streams.

The oracle cannot code gigasamples, but every slice of a SLICED container is an independent stream: the batches here
are tile-periodic (tests/tiled_batch.py, whose shortcut tests/test_tiled_batch.py checks against whole-image oracle containers), so the
expected slice-length table and payload are assembled from a few bank streams by index arithmetic.  The pixels are built on the GPU from
the bank; only the host-API legs build them on the host.

Every leg frees what it holds before the next starts, and skips (stating both numbers) when the device has less free memory than the
codec's workspace_bytes plus the leg's own buffers.  Legs a-d and f print one "LARGE" line each: the codec's workspace bytes ("n/a" for
the host-API legs d), the least free device memory seen, wall time.

The batch calls (mix_batch to label_targets) and the formatted view outputs at these sizes: tests/test_gpu_large_batches.py."""
import os
import time
import zlib

import numpy as np
import pytest

from resize_spec import resize
from tiled_batch import TiledBatch

pytestmark = pytest.mark.gpu

GUARD = 4096
NOISY = ("noise",) * 11 + ("grad", "flat")  # 13 entries: payload volume above all
MIXED = ("noise", "grad", "flat", "noise", "grad", "noise", "flat", "noise", "grad", "noise", "flat")  # 11 entries
PIECE = 1 << 28  # payload bytes compared per step


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


class Leg:
    """memory bookkeeping and the report line of one leg"""

    def __init__(self, mi, name):
        import torch

        self.mi, self.name, self.t0, self.ws = mi, name, time.time(), None  # (None: a host-API leg, no codec of its own)
        torch.cuda.synchronize()
        self.min_free = torch.cuda.mem_get_info()[0]

    def seen(self):
        import torch

        torch.cuda.synchronize()
        self.min_free = min(self.min_free, torch.cuda.mem_get_info()[0])

    def codec(self, own, *args, **kw):
        """a Codec, or a skip when its workspace plus `own` bytes does not fit what the device has free.  Only NOMEM skips: any other
        status of the creation (a size limit or size arithmetic that rejects these valid shapes) is a failure."""
        import torch

        free0 = torch.cuda.mem_get_info()[0]
        try:
            codec = self.mi.Codec(*args, device=0, **kw)
        except self.mi.LlcompError as e:
            if e.status != self.mi.NOMEM:
                raise
            pytest.skip(f"{self.name}: the codec's workspace could not be allocated ({e}); {free0} bytes free")
        self.ws = codec.workspace_bytes
        free = torch.cuda.mem_get_info()[0]
        need = codec.workspace_bytes - codec.allocated_bytes() + own
        if free < need:
            codec.close()
            pytest.skip(f"{self.name}: needs {codec.workspace_bytes} workspace bytes + {own} own bytes; "
                        f"{free + codec.allocated_bytes()} bytes free")
        return codec

    def report(self):
        self.seen()
        ws = "n/a (host API)" if self.ws is None else self.ws
        print(f"\nLARGE {self.name}: workspace_bytes={ws} min_free_bytes={self.min_free} wall_s={time.time() - self.t0:.1f}")


def _release(mi):
    import torch

    torch.cuda.synchronize()
    mi.trim()
    torch.cuda.empty_cache()


def check_payload(tb, d_pay, sids=None, f0=0, f1=None):
    """the device payload d_pay (u8, at least the expected bytes) equals the assembly of frames [f0, f1), compared piece by piece on the
    device"""
    import torch

    dev = d_pay.device
    if sids is None:
        sids = torch.from_numpy(tb.stream_ids(f0, f1)).to(dev)
    bank = tb.stream_tensors(dev)
    cum = torch.cumsum(bank[2][sids], 0)
    n = sids.numel()
    s0, b0 = 0, 0
    while s0 < n:
        s1 = int(torch.searchsorted(cum, b0 + PIECE, right=True))
        s1 = min(n, max(s1, s0 + 1))
        b1 = int(cum[s1 - 1])
        want = tb.payload(sids[s0:s1], *bank)
        if not torch.equal(d_pay[b0:b1], want):
            bad = int((d_pay[b0:b1] != want).to(torch.uint8).argmax())
            slice_at = int(torch.searchsorted(cum, b0 + bad, right=True))
            raise AssertionError(f"payload differs at byte {b0 + bad} (slice {slice_at} of the batch, frame {slice_at // tb.slices_per_frame})")
        s0, b0 = s1, b1
    return b0


def encode_and_check(mi, leg, tb, codec):
    """encode the batch on the device, check the table and the payload against the assembly; -> (px, payload, lens) on the device"""
    import torch

    F, h, w, c = tb.frames, tb.h, tb.w, tb.c
    total = tb.payload_bytes()
    px = torch.empty((F, h, w, c), dtype=torch.uint8, device="cuda")
    tb.fill_device(px)
    pay = torch.full((total + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    lens = torch.empty(codec.n_slices, dtype=torch.int32, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    codec.encode(px.data_ptr(), pay.data_ptr(), total + GUARD, lens.data_ptr(), d_total.data_ptr(), st.data_ptr(), _stream())
    leg.seen()
    assert int(st.item()) == 0, f"encode status {int(st.item()):#x}"
    want = torch.from_numpy(tb.lengths().view(np.int32)).cuda()
    if not torch.equal(lens, want):
        bad = torch.nonzero(lens != want).reshape(-1)
        b = int(bad[0])
        raise AssertionError(f"{bad.numel()} slice lengths differ, the first is slice {b} (frame {b // tb.slices_per_frame}): "
                             f"{int(lens[b])} != {int(want[b])}")
    del want
    assert int(d_total.item()) == total
    assert bool((pay[total:] == 0x5A).all()), "the encoder wrote past the payload"
    assert check_payload(tb, pay) == total
    leg.seen()
    return px, pay, lens


def decode_and_check(leg, tb, codec, px, pay, lens):
    import torch

    out = torch.full_like(px, 0xA5)
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    codec.decode(pay.data_ptr(), tb.payload_bytes(), lens.data_ptr(), out.data_ptr(), st.data_ptr(), _stream())
    leg.seen()
    assert int(st.item()) == 0, f"decode status {int(st.item()):#x}"
    for f in range(tb.frames):  # (frame by frame: bounded memory however much differs)
        if not torch.equal(out[f], px[f]):
            bad = int((out[f] != px[f]).reshape(-1).to(torch.uint8).argmax())
            raise AssertionError(f"decoded sample {bad} of frame {f} differs from the source")


def _edge_rects(w, h, rw, rh):
    """rectangles of rw x rh at the right edge, the bottom edge and the corners (the partial last tile column / row, where there is one)"""
    return [(w - rw, h - rh), (w - rw, 0), (0, h - rh), (w - rw, (h - rh) // 3), ((w - rw) // 2, h - rh)]


def check_regions(mi, leg, tb, codec, px, pay, lens, late, rng, rw=500, rh=300):
    """decode_regions of the encoded batch: random rectangles, the frames `late` at the edges; the output must be the source crops.
    -> (xy, rw, rh, expected output on the device)"""
    import torch

    F, w, h = tb.frames, tb.w, tb.h
    xy = np.stack([rng.integers(0, w - rw + 1, F), rng.integers(0, h - rh + 1, F)], 1).astype(np.int64)
    edge = _edge_rects(w, h, rw, rh)
    for i, f in enumerate(late):
        xy[f] = edge[i % len(edge)]
    out = torch.full((F, rh, rw, tb.c), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    codec.decode_regions(pay.data_ptr(), tb.payload_bytes(), lens.data_ptr(), xy, rw, rh, out.data_ptr(), st.data_ptr(), _stream())
    leg.seen()
    assert int(st.item()) == 0
    want = torch.stack([px[f, y:y + rh, x:x + rw] for f, (x, y) in enumerate(xy.tolist())])
    assert torch.equal(out, want), [f for f in range(F) if not torch.equal(out[f], want[f])][:8]
    return xy, rw, rh, want


def check_resized_regions(mi, leg, tb, codec, px, pay, lens, late, rng, ow=224, oh=160):
    """decode_resized_regions of the encoded batch: rectangles of their own sizes, the frames `late` at the edges, every other frame
    mirrored; the output must be resize_spec.resize of the source crops"""
    import torch

    F, w, h = tb.frames, tb.w, tb.h
    rects = []
    for f in range(F):
        rw_f, rh_f = int(rng.integers(1, 600)), int(rng.integers(1, 500))
        rects.append((int(rng.integers(0, w - rw_f + 1)), int(rng.integers(0, h - rh_f + 1)), rw_f, rh_f))
    for i, f in enumerate(late):
        rw_f, rh_f = rects[f][2:]
        x, y = _edge_rects(w, h, rw_f, rh_f)[i % 5]
        rects[f] = (x, y, rw_f, rh_f)
    flags = np.array([f % 2 for f in range(F)], np.uint8)
    out = torch.full((F, oh, ow, tb.c), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    codec.decode_resized_regions(pay.data_ptr(), tb.payload_bytes(), lens.data_ptr(), rects, ow, oh, out.data_ptr(), st.data_ptr(),
                                 flags=flags, stream=_stream())
    leg.seen()
    assert int(st.item()) == 0
    got = out.cpu().numpy()
    for f, (x, y, rw_f, rh_f) in enumerate(rects):
        crop = px[f, y:y + rh_f, x:x + rw_f].cpu().numpy()
        assert np.array_equal(got[f], resize(mi, crop, ow, oh, bool(flags[f]))), f"frame {f}, rect {rects[f]}"


def _straddlers(tb):
    """the frames that hold sample 2^31 and 2^32, which must not repeat frame 0 or the frame before them"""
    fs = [f for f in ((1 << 31) // tb.samples_per_frame, (1 << 32) // tb.samples_per_frame) if f < tb.frames]
    for f in fs:
        assert tb.frames_differ(f, 0) and tb.frames_differ(f, f - 1), f
    return fs


# ---- a + b: the headline family past 2^32 samples, then regions on the same batch -------------------------------------------------
class TestHeadline:
    """4K RGB, planar 480x1 (the fused row kernels), 176 frames: 4.38 G samples, frames 86 and 172 hold samples 2^31 and 2^32, a payload
    above 4 GiB"""

    @pytest.fixture(scope="class")
    def batch(self, mi, orc):
        import torch

        tb = TiledBatch(orc, 176, 3840, 2160, 3, 480, 1, True, NOISY, seed=1)
        assert _straddlers(tb) == [86, 172]
        assert tb.payload_bytes() > 1 << 32, "precondition: the payload passes 4 GiB"
        leg = Leg(mi, "a_rows_480x1p_176x4K")
        samples = tb.frames * tb.samples_per_frame
        own = 2 * samples + tb.payload_bytes() + 12 * tb.frames * tb.slices_per_frame + 24 * PIECE
        codec = leg.codec(own, tb.frames, tb.w, tb.h, tb.c, 480, 1, True)
        assert codec.family["rows"]
        state = dict(tb=tb, leg=leg, codec=codec)
        try:
            state["px"], state["pay"], state["lens"] = encode_and_check(mi, leg, tb, codec)
        except BaseException as e:
            state["error"] = e
        yield state
        codec.close()
        state.clear()
        _release(mi)

    def test_a_encode_decode_past_2_32(self, mi, batch):
        if "error" in batch:
            raise batch["error"]
        decode_and_check(batch["leg"], batch["tb"], batch["codec"], batch["px"], batch["pay"], batch["lens"])
        batch["leg"].report()

    def test_b_regions_beyond_4_gib(self, mi, batch):
        import torch

        if "error" in batch:
            pytest.fail(f"the batch did not encode: {batch['error']}")
        tb, codec, px, pay, lens = batch["tb"], batch["codec"], batch["px"], batch["pay"], batch["lens"]
        leg = Leg(mi, "b_regions_176x4K")
        leg.ws = codec.workspace_bytes
        F = tb.frames
        per_frame = tb.stream_len[tb.stream_ids()].reshape(F, -1).sum(1)
        beyond = [f for f in range(F) if per_frame[:f].sum() > 1 << 32]  # frames whose payload starts past 4 GiB
        assert len(beyond) >= 8
        # (4K in 480x1 tiles has no partial tile: the edge rectangles here touch the last tile column and row, leg c's the partial ones)
        xy, rw, rh, want = check_regions(mi, leg, tb, codec, px, pay, lens, beyond, np.random.default_rng(5))
        # the same from per-frame containers assembled on the host (frames repeat with the bank size: assembled once per residue)
        conts = {}
        for f in range(F):
            key = (tb.a * f) % tb.K
            if key not in conts:
                conts[key] = tb.container(f)
        host = [conts[(tb.a * f) % tb.K] for f in range(F)]
        out = torch.full(want.shape, 0xA5, dtype=torch.uint8, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        codec.decode_regions_host(host, xy, rw, rh, out.data_ptr(), st.data_ptr(), _stream())
        leg.seen()
        assert int(st.item()) == 0
        assert torch.equal(out, want)
        del out, want, host, conts
        check_resized_regions(mi, leg, tb, codec, px, pay, lens, beyond, np.random.default_rng(6))
        leg.report()


# ---- c: the other families past 2^31 samples ------------------------------------------------------------------------------------
# (name, frames, w, h, c, tile_w, tile_h, planar, small model, family key)
FAMILIES = [
    ("c_tiles_64x64i", 88, 3900, 2100, 3, 64, 64, False, False, "snapshot"),
    ("c_chunked_128x128p", 88, 3900, 2100, 3, 128, 128, True, False, "snapshot"),
    ("c_c5_32x16i_small_model", 55, 3900, 2004, 5, 32, 16, False, True, None),
]


@pytest.mark.parametrize("case", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_c_families_past_2_31(mi, orc, case):
    name, F, w, h, c, tw, th, planar, small, fam = case
    tb = TiledBatch(orc, F, w, h, c, tw, th, planar, NOISY, small_model=small, seed=zlib.crc32(name.encode()))
    assert F * tb.samples_per_frame > 1 << 31 and len(_straddlers(tb)) == 1
    leg = Leg(mi, name)
    samples = F * tb.samples_per_frame
    own = 2 * samples + tb.payload_bytes() + 12 * F * tb.slices_per_frame + 24 * PIECE
    codec = leg.codec(own, F, w, h, c, tw, th, planar, small_model=small)
    try:
        if fam:
            assert codec.family[fam], codec.family
        px, pay, lens = encode_and_check(mi, leg, tb, codec)
        decode_and_check(leg, tb, codec, px, pay, lens)
        # regions and resized regions: the last five frames (the one holding sample 2^31 among them) get rectangles on the partial last
        # tile column / row and the partial corner
        late = list(range(F - 5, F))
        assert _straddlers(tb)[0] in late
        assert tb.w % tb.tile_w and tb.h % tb.tile_h
        check_regions(mi, leg, tb, codec, px, pay, lens, late, np.random.default_rng(len(name)))
        check_resized_regions(mi, leg, tb, codec, px, pay, lens, late, np.random.default_rng(len(name) + 1))
        del px, pay, lens
        leg.report()
    finally:
        codec.close()
        _release(mi)


# ---- d: one frame just under the 2^31-sample limit, through the host API --------------------------------------------------------
FRAMES_D = [  # (name, w, h, c, tile_w, tile_h, planar)
    ("d_46340sq_c1_64x64", 46340, 46340, 1, 64, 64, False),
    ("d_26754sq_c3_480x1p", 26754, 26754, 3, 480, 1, True),
]


@pytest.mark.parametrize("case", FRAMES_D, ids=[f[0] for f in FRAMES_D])
def test_d_frame_near_2_31_host_api(mi, orc, case):
    import torch

    name, w, h, c, tw, th, planar = case
    assert (1 << 31) - 3 * 2**20 < w * h * c < 1 << 31
    tb = TiledBatch(orc, 1, w, h, c, tw, th, planar, MIXED, seed=zlib.crc32(name.encode()))
    leg = Leg(mi, name)
    free = torch.cuda.mem_get_info()[0]
    need = 40 * w * h * c  # the host API's lane (13 B/sample scratch and its arrays) plus the comparison on the device
    if free < need:
        pytest.skip(f"{name}: needs about {need} bytes; {free} bytes free")
    img = tb.frames_host()[0]
    try:
        data = mi.compress_image(img, w, h, c, format=mi.FORMAT_SLICED, tile_w=tw, tile_h=th, planar=planar, device=0)
        leg.seen()
        n = tb.slices_per_frame
        body = 24 + 4 * n
        assert data[:24] == tb.header()
        assert np.array_equal(np.frombuffer(data, "<u4", count=n, offset=24), tb.lengths())
        assert len(data) == body + tb.payload_bytes()
        d_pay = torch.from_numpy(np.frombuffer(data, np.uint8, offset=body).copy()).cuda()
        assert check_payload(tb, d_pay) == len(data) - body
        del d_pay
        leg.seen()
        px = mi.decompress_image(data, device=0).pixels
        leg.seen()
        assert px.shape == img.shape and np.array_equal(px, img)
        del px
        rw, rh = 333, 77
        reg = mi.decompress_region(data, w - rw, h - rh, rw, rh, device=0).pixels
        assert np.array_equal(reg, img[h - rh:, w - rw:])
        leg.report()
    finally:
        _release(mi)


# ---- e: channel counts past the specialised kernels ---------------------------------------------------------------------------
def _wide(c, w=37, h=23, seed=0):
    rng = np.random.default_rng(seed + c)
    img = rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    img[:, :, 1::3] = ((x * 3 + y * 5)[:, :, None] + np.arange(img[:, :, 1::3].shape[2])[None, None, :]).astype(np.uint8)
    img[: h // 2, : w // 2, 2::3] = 77
    return img


@pytest.fixture
def nosnap(mi):
    old = os.environ.get("LLCOMP_MI_NOSNAP")

    def _set(on):
        os.environ["LLCOMP_MI_NOSNAP"] = "1" if on else "0"
        mi.reload_tuning()

    yield _set
    if old is None:
        os.environ.pop("LLCOMP_MI_NOSNAP", None)
    else:
        os.environ["LLCOMP_MI_NOSNAP"] = old
    mi.reload_tuning()


@pytest.mark.parametrize("c", [8, 16, 32, 64, 128, 255])
def test_e_many_channels(mi, orc, nosnap, c):
    w, h = 37, 23
    img = _wide(c, w, h)
    for ns in (False, True):
        nosnap(ns)
        for small in (False, True):
            orc.set_small_model(small)
            try:
                for tw, th, planar in ((16, 16, False), (0, 1, False), (0, 0, False), (16, 16, True), (8, 5, True)):
                    got = mi.compress_image(img, w, h, c, format=mi.FORMAT_SLICED, tile_w=tw, tile_h=th, planar=planar, device=0,
                                            small_model=small)
                    assert got == orc.compress_sliced(img, tw, th, planar), (ns, small, tw, th, planar)
                    assert np.array_equal(mi.decompress_image(got, device=0).pixels, img), (ns, small, tw, th, planar)
                legacy = mi.compress_image(img, w, h, c, device=0, small_model=small)
                assert legacy == orc.compress_image(img), (ns, small)
                assert np.array_equal(mi.decompress_image(legacy, device=0, small_model=small).pixels, img), (ns, small)
            finally:
                orc.set_small_model(False)


def test_e_regions_at_255_channels(mi, orc):
    import torch

    c, w, h, F = 255, 37, 23, 3
    imgs = np.stack([_wide(c, w, h, seed=f) for f in range(F)])
    conts = [orc.compress_sliced(imgs[f], 16, 8, False) for f in range(F)]
    for x, y, rw, rh in ((0, 0, 37, 23), (30, 20, 7, 3), (5, 9, 20, 10), (36, 22, 1, 1)):
        reg = mi.decompress_region(conts[1], x, y, rw, rh, device=0).pixels
        assert np.array_equal(reg, imgs[1, y:y + rh, x:x + rw]), (x, y, rw, rh)
    codec = mi.Codec(F, w, h, c, 16, 8, False, device=0)
    try:
        pay, lens = mi.pack_batch(conts)
        dev = (torch.from_numpy(np.concatenate([pay, np.zeros(16, np.uint8)])).cuda(), len(pay),
               torch.from_numpy(lens.view(np.int32).copy()).cuda())
        rects = [(0, 0, 37, 23), (21, 15, 16, 8), (3, 2, 9, 17)]
        flags = np.array([0, 1, 1], np.uint8)
        ow, oh = 20, 13
        out = torch.full((F, oh, ow, c), 0xA5, dtype=torch.uint8, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        codec.decode_resized_regions(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), rects, ow, oh, out.data_ptr(), st.data_ptr(), flags=flags,
                                     stream=_stream())
        torch.cuda.synchronize()
        assert int(st.item()) == 0
        got = out.cpu().numpy()
        for f, (x, y, rw, rh) in enumerate(rects):
            assert np.array_equal(got[f], resize(mi, imgs[f, y:y + rh, x:x + rw], ow, oh, bool(flags[f]))), f
    finally:
        codec.close()


# ---- f: the frame limit of resized regions ----------------------------------------------------------------------------------------
def test_f_resized_regions_frame_limit(mi, orc):
    import torch

    w, h, c, F = 6, 5, 3, 65535
    tb = TiledBatch(orc, F, w, h, c, 4, 4, True, MIXED, seed=7)
    leg = Leg(mi, "f_65535_frames")
    codec = leg.codec(0, F, w, h, c, 4, 4, True)
    try:
        px, pay, lens = encode_and_check(mi, leg, tb, codec)
        rects = [(1, 0, 5, 4) if f % 2 else (0, 1, 3, 4) for f in range(F)]
        flags = np.array([(f // 2) % 2 for f in range(F)], np.uint8)
        ow, oh = 7, 3
        out = torch.full((F, oh, ow, c), 0xA5, dtype=torch.uint8, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        codec.decode_resized_regions(pay.data_ptr(), tb.payload_bytes(), lens.data_ptr(), rects, ow, oh, out.data_ptr(), st.data_ptr(),
                                     flags=flags, stream=_stream())
        torch.cuda.synchronize()
        assert int(st.item()) == 0
        got = out.cpu().numpy()
        src = px.cpu().numpy()
        # frames repeat with the bank size and the rectangles with period 2, the flags with period 4: K * 4 distinct outputs
        memo = {}
        for f in range(F):
            key = ((tb.a * f) % tb.K, f % 4)
            if key not in memo:
                x, y, rw, rh = rects[f]
                memo[key] = resize(mi, src[f, y:y + rh, x:x + rw], ow, oh, bool(flags[f]))
            assert np.array_equal(got[f], memo[key]), f
        leg.report()
    finally:
        codec.close()
    # one frame more: a valid batch of F + 1 frames (the last repeats frame 0), so that nothing is read past a buffer if the limit ever
    # went missing
    f0_bytes = int(tb.lengths(0, 1).sum(dtype=np.uint64))
    pay1 = torch.cat([pay[:tb.payload_bytes()], pay[:f0_bytes], torch.zeros(GUARD, dtype=torch.uint8, device="cuda")])
    lens1 = torch.cat([lens, lens[:tb.slices_per_frame]])
    big = mi.Codec(F + 1, w, h, c, 4, 4, True, device=0)
    try:
        assert big.n_slices == lens1.numel()
        out = torch.full((F + 1, 3, 7, c), 0xA5, dtype=torch.uint8, device="cuda")
        with pytest.raises(mi.LlcompError) as e:
            big.decode_resized_regions(pay1.data_ptr(), tb.payload_bytes() + f0_bytes, lens1.data_ptr(), [(0, 0, 1, 1)] * (F + 1), 7, 3,
                                       out.data_ptr(), st.data_ptr(), stream=_stream())
        assert e.value.status == mi.BAD_ARGS
        torch.cuda.synchronize()
        assert bool((out == 0xA5).all())
    finally:
        big.close()
        _release(mi)
