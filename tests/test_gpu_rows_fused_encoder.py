"""The encoder of planar 1-row slices reads the pixel batch itself (stage A runs inside the coder, no 16-bit symbol array in
between): its containers against the oracle's for every shape that family meets -- ragged last tile columns, tiles whose planes
straddle two lane groups, 1 to 4 channels, one and many frames, noise, the small model, tiles of one and two pixels at the end of the
batch (where the encoder reads pixels byte by byte) -- and region decodes of what it wrote.  These check the results only: the device
buffers come from an allocator that leaves slack behind them, so a read past the batch would go unseen here; that bound is checked on
the host (test_rows_px_reads.py)."""
import numpy as np
import pytest
from conftest import make_image

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


def frames_of(gen, frames, w, h, c):
    imgs = np.stack([make_image(gen, w, h, c) for _ in range(frames)])
    for i in range(frames):
        imgs[i] = np.roll(imgs[i], 11 * i, axis=1)
    return imgs


def encode_batch(mi, imgs, tw, small_model=False):
    """one Codec.encode of the whole batch -> (slice lengths, payload)"""
    import torch

    frames, h, w, c = imgs.shape
    k = mi.Codec(frames, w, h, c, tw, 1, True, device=0, small_model=small_model)
    try:
        assert k.family["rows"]
        d_px = torch.from_numpy(np.ascontiguousarray(imgs).reshape(-1)).cuda()
        d_pay = torch.zeros(k.max_payload_bytes + 16, dtype=torch.uint8, device="cuda")
        d_len = torch.zeros(k.n_slices, dtype=torch.int32, device="cuda")
        d_tot = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
        k.encode(d_px.data_ptr(), d_pay.data_ptr(), k.max_payload_bytes, d_len.data_ptr(), d_tot.data_ptr(), d_st.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert int(d_st.item()) == 0
        total = int(d_tot.item())
        return d_len.cpu().numpy().view(np.uint32), d_pay[:total].cpu().numpy().tobytes()
    finally:
        k.close()


def oracle_batch(orc, imgs, tw, small_model=False):
    lens, pays = [], []
    orc.set_small_model(small_model)
    try:
        for img in imgs:
            d = orc.compress_sliced(np.ascontiguousarray(img), tw, 1, True)
            n = int.from_bytes(d[20:24], "little")
            lens.append(np.frombuffer(d[24:24 + 4 * n], dtype="<u4"))
            pays.append(d[24 + 4 * n:])
    finally:
        orc.set_small_model(False)
    return np.concatenate(lens), b"".join(pays)


# (name, generator, frames, w, h, c, tile_w): with 64 slices per lane group and 3 planes per tile, groups start and end inside tiles
CASES = [
    ("ragged_c3_1frame", "nat", 1, 1100, 6, 3, 480),
    ("ragged_c3_frames", "g3", 5, 1100, 6, 3, 480),
    ("straddle_c3_many_groups", "mid", 3, 640, 40, 3, 32),
    ("c1_ragged", "g3", 3, 700, 8, 1, 96),
    ("c2_ragged", "mid", 2, 333, 7, 2, 64),
    ("c4_ragged", "nat", 3, 250, 9, 4, 50),
    ("c4_straddle", "g3", 2, 300, 30, 4, 20),
    ("tile_of_one_pixel_at_the_end", "g3", 2, 5, 4, 3, 2),
    ("one_pixel_c1", "g3", 1, 1, 1, 1, 1),
    ("two_pixels_c2", "nat", 1, 2, 1, 2, 1),
    ("one_row_c3", "checker", 1, 97, 1, 3, 97),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fused_encoder_equals_oracle(mi, orc, case):
    _, gen, frames, w, h, c, tw = case
    imgs = frames_of(gen, frames, w, h, c)
    lens, pay = encode_batch(mi, imgs, tw)
    want_lens, want_pay = oracle_batch(orc, imgs, tw)
    assert np.array_equal(lens, want_lens)
    assert pay == want_pay


@pytest.mark.parametrize("c", [1, 3, 4])
def test_fused_encoder_carry_heavy_noise(mi, orc, c):
    """uniform noise: long residuals, many carries through the held byte"""
    rng = np.random.default_rng(1234 + c)
    imgs = rng.integers(0, 256, size=(3, 12, 517, c), dtype=np.uint8)
    lens, pay = encode_batch(mi, imgs, 128)
    want_lens, want_pay = oracle_batch(orc, imgs, 128)
    assert np.array_equal(lens, want_lens)
    assert pay == want_pay


@pytest.mark.parametrize("c", [1, 3])
def test_fused_encoder_small_model(mi, orc, c):
    imgs = frames_of("nat", 2, 301, 10, c)
    lens, pay = encode_batch(mi, imgs, 64, small_model=True)
    want_lens, want_pay = oracle_batch(orc, imgs, 64, small_model=True)
    assert np.array_equal(lens, want_lens)
    assert pay == want_pay


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_fused_container_region_and_full_decode(mi, orc, c):
    """containers the fused encoder wrote: equal to the oracle's, and their rectangles and whole frames decode to the pixels"""
    w, h, tw = 777, 23, 480
    img = make_image("nat", w, h, c)
    s = mi.compress_image(img, w, h, c, format=mi.FORMAT_SLICED, tile_w=tw, tile_h=1, planar=True, device=0)
    assert s == orc.compress_sliced(img, tw, 1, True)
    assert np.array_equal(mi.decompress_image(s, device=0).pixels, img)
    for (x, y, rw, rh) in [(0, 0, w, h), (470, 3, 20, 9), (481, 0, 296, 1), (776, 22, 1, 1), (5, 7, 300, 16)]:
        got = mi.decompress_region(s, x, y, rw, rh, device=0)
        assert np.array_equal(got.pixels, img[y:y + rh, x:x + rw]), (x, y, rw, rh)
