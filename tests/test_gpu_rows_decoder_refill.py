"""The hand-written sample of the 1-row-slice decoder (csrc/dec_rows_asm.hpp) keeps `low` and its private copy of the window's next
three bytes in one register pair (a refill is one 64-bit shift; the copy ends in a 0xFF sentinel, and what is left of it says how many
bytes went), and its unary phase alternates between two range registers (the lanes that left on the second one are moved over once,
behind the phase).  Nothing of that may show: every case encodes and compares the container with the oracle's, byte by byte, then
decodes and compares the pixels with the source -- and does both again under LLCOMP_MI_FORCE_REPLAY=1, where every sample is rolled
back from the block's untouched inputs and replayed on the checked path.

Contents.  Noise: every lane refills at nearly every bin, and samples consume 0 to 3 bytes (none wants a fourth, at any width: the
replay counter of the noise frames is 0 before and after; the samples that do want one come from the spikes image below).  A flat image: long stretches with no refill and no top-up.  A clean gradient and the photo-like `nat`: short, ragged
unary runs, so lanes leave the phase on either parity of the run and on each of slots 1..3 (which register holds their range).
Three frames of 40 rows: lane groups start and end inside frames and planes.  The interleaved layouts run k_decode_slices<2..4,true>,
which share the block."""
import numpy as np
import pytest

import orc as orc_mod
from conftest import make_image

pytestmark = pytest.mark.gpu

FRAMES, ROWS = 3, 40
WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 480]


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1
    return llcomp_amd


@pytest.fixture
def set_hook(mi, monkeypatch):
    def _set(name, value):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
        mi.reload_tuning()

    yield _set
    monkeypatch.undo()
    mi.reload_tuning()


def frames_of(w, c, gen="g3"):
    """u8 [FRAMES, ROWS, w, c]: noise with another seed per frame; `flat` = one value per frame; the others rolled by rows"""
    if gen == "g3":
        return np.stack([make_image("g3@%d" % (77 + f), w, ROWS, c) for f in range(FRAMES)])
    if gen == "flat":
        return np.stack([np.full((ROWS, w, c), 90 + 40 * f, np.uint8) for f in range(FRAMES)])
    return np.stack([np.ascontiguousarray(np.roll(make_image(gen, w, ROWS, c), 3 * f, axis=0)) for f in range(FRAMES)])


_wanted = {}


def wanted(orc, gen, w, c, planar, small):
    """the oracle's containers of frames_of(w, c, gen) at one tile column per row (computed once, shared, never changed)"""
    key = (gen, w, c, planar, small)
    if key not in _wanted:
        imgs = frames_of(w, c, gen)
        orc.set_small_model(small)
        try:
            _wanted[key] = (imgs, [orc.compress_sliced(np.ascontiguousarray(f), w, 1, planar) for f in imgs])
        finally:
            orc.set_small_model(False)
    return _wanted[key]


def check(mi, orc, gen, w, c, planar, small, n_frames=FRAMES):
    """every frame: container == the oracle's, pixels == the source"""
    imgs, want = wanted(orc, gen, w, c, planar, small)
    for f, wnt in list(zip(imgs, want))[:n_frames]:
        got = mi.compress_image(f, w, ROWS, c, format=mi.FORMAT_SLICED, tile_w=w, tile_h=1, planar=planar, small_model=small)
        assert got == wnt, ("container differs from the oracle's", gen, w, c, planar, small)
        assert np.array_equal(mi.decompress_image(got, small_model=small).pixels, f), ("pixels", gen, w, c, planar, small)


def both_ways(mi, orc, set_hook, gen, w, c):
    """planar and interleaved, both models; then all of it again with every sample replayed"""
    for force in (None, "1"):
        set_hook("LLCOMP_MI_FORCE_REPLAY", force)
        for small in (False, True):
            check(mi, orc, gen, w, c, True, small)
            if c > 1:
                check(mi, orc, gen, w, c, False, small, n_frames=1)


@pytest.mark.parametrize("c", [1, 2, 3, 4])
@pytest.mark.parametrize("w", WIDTHS)
def test_noise(mi, orc, set_hook, w, c):
    """widths 1..9 give the peel alone, peel + odd / even bulk and the leftover pixel (the two register pairs in every order);
    63 / 64 / 65 and 480 a bulk long enough for every refill count per sample"""
    both_ways(mi, orc, set_hook, "g3", w, c)


@pytest.mark.parametrize("gen", ["flat", "g2", "nat"])
@pytest.mark.parametrize("w", [5, 64, 65, 480])
def test_other_contents(mi, orc, set_hook, gen, w):
    both_ways(mi, orc, set_hook, gen, w, 3)


class Batch:
    """frames [F,h,w,c] on the GPU behind one codec object: the round trip of the whole batch, and the codec's event counters"""

    def __init__(self, mi, imgs, tw, planar, small=False):
        import torch

        self.torch = torch
        F, h, w, c = imgs.shape
        self.codec = mi.Codec(F, w, h, c, tw, 1, planar, small_model=small)
        self.st = torch.cuda.current_stream().cuda_stream
        self.d_px = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
        self.cap = min(self.codec.max_payload_bytes, 2 * imgs.size + 64 * self.codec.n_slices + 4096)
        self.d_pay = torch.empty(self.cap, dtype=torch.uint8, device="cuda")
        self.d_len = torch.empty(self.codec.n_slices, dtype=torch.int32, device="cuda")
        self.d_tot = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.d_out = torch.zeros_like(self.d_px)

    def roundtrip(self):
        self.codec.encode(self.d_px.data_ptr(), self.d_pay.data_ptr(), self.cap, self.d_len.data_ptr(), self.d_tot.data_ptr(), self.d_st.data_ptr(), self.st)
        self.torch.cuda.synchronize()
        assert int(self.d_st.item()) == 0
        self.d_out.zero_()
        self.codec.decode(self.d_pay.data_ptr(), int(self.d_tot.item()), self.d_len.data_ptr(), self.d_out.data_ptr(), self.d_st.data_ptr(), self.st)
        self.torch.cuda.synchronize()
        assert int(self.d_st.item()) == 0 and self.torch.equal(self.d_out, self.d_px), "round trip is not lossless"
        return self.codec.counters()

    def close(self):
        self.codec.close()


def spikes(w, h):
    """the hostile-statistics image of test_gpu_rows_loop_pairs.py (long constant runs saturate the models, then a maximal spike costs
    more bytes in one sample than the sample's three): spikes at x = 96, 193, 290, 387 -- odd and even sample indices"""
    y, x, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    return np.ascontiguousarray(np.where((x % 97 == 96) & (k != 1), 255, np.where((x % 2 == 0) & (k == 0), 128, 0)).astype(np.uint8))


def replay_input(kind, w, c):
    return frames_of(w, c) if kind == "g3" else spikes(w, 24)[None]


# dec_replays of one round trip without the hook, one tile column: the samples that wanted a fourth byte.  Which samples those are
# is a property of the stream, not of the block -- every figure was read on the parent of this change (commit b34385e, the block with
# the 32-bit copy under a sentinel 1) and must not move.  The noise frames at the widest tile give none there (a noise sample costs
# about a byte, never four); the spikes do, at an even and an odd width (both samples of a loop turn), planar under both models and interleaved.
PARENT_REPLAYS = {
    # (content, width, c, planar, small_model): dec_replays
    ("g3", 480, 1, True, False): 0,
    ("g3", 480, 3, True, False): 0,
    ("g3", 480, 4, False, False): 0,
    ("g3", 480, 4, False, True): 0,
    ("spikes", 400, 3, True, False): 72,
    ("spikes", 401, 3, True, False): 72,
    ("spikes", 401, 3, True, True): 48,
    ("spikes", 401, 3, False, True): 72,
}


def replays_of(mi, kind, w, c, planar, small):
    b = Batch(mi, replay_input(kind, w, c), w, planar, small)
    try:
        return b.roundtrip()["dec_replays"]
    finally:
        b.close()


@pytest.mark.parametrize("key", sorted(PARENT_REPLAYS), ids=lambda k: "%s_%d_c%d%s%s" % (k[0], k[1], k[2], "p" if k[3] else "i", "_small" if k[4] else ""))
def test_fourth_byte_replays(mi, key):
    """a sample that wants a fourth byte finds its copy used up (it took the sentinel) and is replayed -- the same samples as before"""
    got = replays_of(mi, *key)
    print("dec_replays", key, got)
    assert key[0] == "g3" or PARENT_REPLAYS[key] > 0
    assert got == PARENT_REPLAYS[key], (key, got)


@pytest.mark.parametrize("force", [None, "1"])
def test_invalid_exponent(mi, orc, set_hook, force):
    """a unary run of 33 ones in one slice (exponent above 31): the block zeroes the lane's copy, the replay gives the verdict -- the
    oracle's, with the oracle's status"""
    import test_gpu_adversarial as adv

    set_hook("LLCOMP_MI_FORCE_REPLAY", force)
    geo = adv.Geo(72, 20, 1, 36, 1, True)
    rng = np.random.default_rng(1911)
    data = geo.container(geo.payloads(orc, rng, False, ["small", "sparse", "ex31"], bad=(5, lambda m: m // 2, 33)), False)
    codec = mi.Codec(1, geo.w, geo.h, geo.c, geo.tw, geo.th, geo.planar)
    try:
        assert codec.family["rows"]
        status, px = adv._decode_codec(mi, codec, data)
    finally:
        codec.close()
    assert adv._same_as_oracle(orc, status, px, data, ("run33", force)) == orc_mod.BAD_EXPONENT
