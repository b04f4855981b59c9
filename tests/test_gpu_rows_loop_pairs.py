"""The sample loops of the two 1-row-slice kernels code the first pixel (decoder) / the first two samples (encoder) of a slice in
front of their bulk loop, the bulk two samples per turn with the registers of consecutive samples swapping roles, and what is left --
an odd sample, the tail whose pixel reads need tests, ragged wavefronts -- in the loop with the per-lane tests.  The model
(LargeModel, llcomp.hpp:21) is a template flag of the kernels.  The shapes here are the smallest at which that structure can go
wrong: every case encodes and compares the container with the oracle's, byte by byte, then decodes and compares the pixels with
the source.

Which widths take which path.  Decoder: pixel 0 alone, then pairs while two pixels are left, then singles -- widths 1..7 give the
peel alone, peel + odd / even bulk and the leftover pixel.  Encoder (planar, reads the pixels itself): samples 0 and 1 alone, pairs
up to width - rows_px_tail(C) (5 / 3 / 3 / 2 for C = 1..4: csrc/geometry.hpp), singles for the rest -- the first pair runs at width
9 / 7 / 7 / 6, so the widths go on to 14.  Interleaved slices (planar=False) run the decoder with C samples per pixel and the encoder
on 16-bit symbols, whose bulk stops two samples before the end."""
import numpy as np
import pytest

from conftest import make_image

pytestmark = pytest.mark.gpu


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


FRAMES, ROWS = 3, 40  # 120 rows x C planes: lane groups of 64 slices start and end inside frames and inside planes


def frames_of(w, c, gen="g3"):
    """u8 [FRAMES, ROWS, w, c]: noise (every sample costs bytes: renormalisations, refills, top-ups in every lane), another seed per frame"""
    if gen == "g3":
        return np.stack([make_image("g3@%d" % (77 + f), w, ROWS, c) for f in range(FRAMES)])
    return np.stack([np.ascontiguousarray(np.roll(make_image(gen, w, ROWS, c), 3 * f, axis=0)) for f in range(FRAMES)])


def check_frames(mi, orc, imgs, tw, planar, small=False):
    """every frame: container == the oracle's, pixels == the source"""
    orc.set_small_model(small)
    try:
        want = [orc.compress_sliced(np.ascontiguousarray(f), tw, 1, planar) for f in imgs]
    finally:
        orc.set_small_model(False)
    for f, wanted in zip(imgs, want):
        h, w, c = f.shape
        got = mi.compress_image(f, w, h, c, format=mi.FORMAT_SLICED, tile_w=tw, tile_h=1, planar=planar, small_model=small)
        assert got == wanted, ("container differs from the oracle's", w, c, tw, planar, small)
        assert np.array_equal(mi.decompress_image(got, small_model=small).pixels, f), ("pixels", w, c, tw, planar, small)


class Batch:
    """frames [F,h,w,c] on the GPU behind one codec object: the round trip of the whole batch, and the codec's event counters"""

    def __init__(self, mi, imgs, tw, planar, small=False):
        import torch

        self.torch, self.imgs = torch, imgs
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

    def payload(self):
        """(slice lengths, payload bytes) as the encoder left them"""
        return self.d_len.cpu().numpy().copy(), self.d_pay[: int(self.d_tot.item())].cpu().numpy().copy()

    def close(self):
        self.codec.close()


@pytest.mark.parametrize("c", [1, 2, 3, 4])
@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14])
def test_uniform_widths(mi, orc, w, c):
    """one tile column (tile_w = w): every wavefront is uniform and takes peel + bulk + leftovers; planar and interleaved"""
    imgs = frames_of(w, c)
    check_frames(mi, orc, imgs, w, True)
    if c > 1:
        check_frames(mi, orc, imgs[:1], w, False)


@pytest.mark.parametrize("planar", [True, False])
def test_width_480(mi, orc, planar):
    """the headline's slice width, once: a long bulk"""
    check_frames(mi, orc, frames_of(480, 3)[:1], 480, planar)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("tw", [4, 5])
@pytest.mark.parametrize("r", [1, 2, 3])
def test_ragged_last_column(mi, orc, tw, r, c):
    """w = 2 tile_w + r: wavefronts that hold slices of both widths take the loop with the per-lane tests, next to uniform ones"""
    imgs = frames_of(2 * tw + r, c)
    check_frames(mi, orc, imgs, tw, True)
    if c > 1:
        check_frames(mi, orc, imgs[:1], tw, False)


@pytest.mark.parametrize("tw", [12, 13])
def test_ragged_last_column_with_a_bulk(mi, orc, tw):
    """the same where the full tiles are wide enough for the encoder's pairs: uniform wavefronts in the bulk, mixed ones beside them"""
    check_frames(mi, orc, frames_of(2 * tw + 3, 3), tw, True)


@pytest.mark.parametrize("planar", [True, False])
@pytest.mark.parametrize("w", [1, 2, 5, 33])
def test_small_model(mi, orc, w, planar):
    """LargeModel = false: the kernels' other template instance (no difference, context 0, no fold)"""
    check_frames(mi, orc, frames_of(w, 3), w, planar, small=True)


@pytest.mark.parametrize("w", [1, 2, 5, 6, 33])
def test_forced_replay(mi, orc, set_hook, w):
    """LLCOMP_MI_FORCE_REPLAY=1: every sample is rolled back and replayed on the checked path -- from the inputs the fast path left
    untouched, at both register roles.  Pixels unchanged, and the replay counter equals the sample count."""
    imgs = frames_of(w, 3)
    set_hook("LLCOMP_MI_FORCE_REPLAY", "1")
    for planar in (True, False):
        check_frames(mi, orc, imgs[:1], w, planar)
        b = Batch(mi, imgs, w, planar)
        counters = b.roundtrip()
        b.close()
        assert counters["dec_replays"] == imgs.size, (w, planar, counters)


def spikes(w, h):
    """the hostile-statistics image of test_decoder_rollback_and_checked_replay (long constant runs saturate the models, then a maximal
    spike costs more bytes in one sample than the window is guaranteed to hold), at another size"""
    y, x, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    return np.ascontiguousarray(np.where((x % 97 == 96) & (k != 1), 255, np.where((x % 2 == 0) & (k == 0), 128, 0)).astype(np.uint8))


@pytest.mark.parametrize("w", [400, 401])
def test_natural_replays(mi, orc, w):
    """samples that outrun the window without the hook, at an even and an odd width: spikes sit at x = 96, 193, 290, 387 -- odd and
    even sample indices, so both roles of the pair roll back"""
    img = spikes(w, 24)
    check_frames(mi, orc, img[None], w, True)
    b = Batch(mi, img[None], w, True)
    counters = b.roundtrip()
    b.close()
    assert counters["dec_replays"] > 0, counters


@pytest.mark.parametrize("w", [300, 301])
def test_carry_heavy_streams(mi, orc, w):
    """tiles whose stream holds a carry through 33 undecided 0xFF bytes (tests/carry_streams.py), at an even and an odd width: more than
    the 28 bytes the staging area ever holds, so the carry goes on into bytes that have left for HBM -- the rare path behind the
    encoder's block, in the bulk"""
    import carry_streams as cs

    base = cs.natural(orc, w, 1)
    found = cs.search(lambda seed: cs.craft_tile(orc, base, 0, 33, True, seed), cs.run_of(33, True))
    assert found is not None, "no seed of the budget gives a carry through 33 bytes at this width"
    row = cs.pixels(orc, found.tile, 1)  # (1, w, 1) grey pixels
    # the crafted row in every fourth slice, ordinary rows between them (neighbours that renormalise at other samples)
    rows = [row if i % 4 == 0 else cs.filler(w, 1, 1, i) for i in range(96)]
    img = np.ascontiguousarray(np.concatenate(rows, axis=0))
    check_frames(mi, orc, img[None], w, True)
    b = Batch(mi, img[None], w, True)
    counters = b.roundtrip()
    b.close()
    assert counters["enc_carry_backs"] > 0, counters


@pytest.mark.parametrize("tw", [5, 6, 33])
def test_region_decode(mi, orc, tw):
    """a rectangle of a container the encoder wrote: the same decoder kernel on a sub-geometry (whole tiles of some rows)"""
    img = make_image("g3@5", 4 * tw + 2, 37, 3)
    h, w, c = img.shape
    data = mi.compress_image(img, w, h, c, format=mi.FORMAT_SLICED, tile_w=tw, tile_h=1, planar=True)
    assert data == orc.compress_sliced(img, tw, 1, True)
    for x, y, rw, rh in ((tw + 1, 3, 2 * tw, 20), (0, 0, w, 1), (3 * tw + 1, 30, tw + 1, 7)):
        got = mi.decompress_region(data, x, y, rw, rh)
        got = got.pixels if hasattr(got, "pixels") else got
        assert np.array_equal(np.asarray(got).reshape(rh, rw, c), img[y:y + rh, x:x + rw]), (tw, x, y, rw, rh)
