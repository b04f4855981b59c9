"""The 1-row-slice encoder flushes its staging areas in batches (a wavefront enters the flush region only when one of its lanes holds
kFlushAt bytes; every lane with a whole unit then stores one), forms stage A with two byte dot products, and its hand-written sample
narrows the lane sets with v_cmpx and tests its two run loops at the bottom (csrc/slice_kernels.hip, enc_rows_asm.hpp,
enc_sample_asm.inc -- the latter shared with the 2-D snapshot encoder).  Every case is a container compared with the oracle's byte by
byte, plus the decode round trip."""
import numpy as np
import pytest

from conftest import make_image

import rows_flush_model as fm

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


ROWS = 70  # more than 64 slices per plane: a full wavefront and a partial one


def check(mi, orc, img, tw, th=1, planar=True, small=False):
    """container == the oracle's, pixels == the source"""
    img = np.ascontiguousarray(img)
    h, w, c = img.shape
    orc.set_small_model(small)
    try:
        want = orc.compress_sliced(img, tw, th, planar)
    finally:
        orc.set_small_model(False)
    got = mi.compress_image(img, w, h, c, format=mi.FORMAT_SLICED, tile_w=tw, tile_h=th, planar=planar, small_model=small)
    assert got == want, ("container differs from the oracle's", w, h, c, tw, th, planar, small)
    assert np.array_equal(mi.decompress_image(got, small_model=small).pixels, img), ("pixels", w, h, c, tw, th, planar, small)
    return want


# ---- flush policy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 31, 33, 480])
def test_widths_channels_models(mi, orc, w, small):
    """one frame, planar one-row tiles of one column, 1..4 channels: slices that never fill a unit, that fill one at the very end, that
    flush many times; every plane position of stage A"""
    for c in (1, 2, 3, 4):
        check(mi, orc, make_image("g3@%d" % (11 + c), w, ROWS, c), w, small=small)


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("tw,r", [(13, 1), (13, 3), (33, 2), (33, 17)])
def test_ragged_last_column(mi, orc, tw, r, c):
    """w = 2 tile_w + r: wavefronts that hold slices of both widths run the loop with the per-lane tests, where the flush test sees only
    the lanes still coding"""
    check(mi, orc, make_image("g3@31", 2 * tw + r, ROWS, c), tw)


def test_symbol_forms(mi, orc):
    """interleaved one-row tiles: the same loops on 16-bit (3 channels) and 32-bit symbols"""
    for c in (1, 3, 4):
        check(mi, orc, make_image("g3@41", 97, ROWS, c), 97, planar=False)
        check(mi, orc, make_image("g3@41", 2 * 33 + 5, ROWS, c), 33, planar=False)


# ---- lanes of one wavefront that fill at different rates ---------------------------------------------------------------------------
def mixed_rows(w, c, period):
    """noise rows next to flat rows, rows of small noise and rows that are flat in their first half: at a flush event the lanes of a
    wavefront stand on both sides of 16 and of kFlushAt bytes, and a flat lane's first renormalisation (its dummy byte) comes while
    its neighbour's area is full"""
    rng = np.random.default_rng(100 + period)
    img = rng.integers(0, 256, size=(ROWS, w, c), dtype=np.uint8)
    for y in range(ROWS):
        k = y % period
        if k == 1:
            img[y] = 128
        elif k == 2:
            img[y] = 128 + rng.integers(-2, 3, size=(w, c))
        elif k == 3:
            img[y, : w // 2] = 37
    return img


@pytest.mark.parametrize("shift", [None, "6"])
@pytest.mark.parametrize("period", [2, 3, 4, 5])
def test_mixed_fill_rates(mi, orc, set_hook, period, shift):
    set_hook("LLCOMP_MI_LANE_SHIFT", shift)
    for c in (1, 3):
        check(mi, orc, mixed_rows(480, c, period), 480)
    check(mi, orc, mixed_rows(150, 3, period), 150, planar=False)


# ---- what finish() finds in the staging area -------------------------------------------------------------------------------------------
def test_slices_that_end_on_both_sides_of_a_unit(mi, orc, set_hook):
    """16 consecutive widths of noise, 64 slices = one wavefront each.  The policy's model on the oracle's byte counts says what every
    lane holds when finish() begins: lanes with a whole unit still staged (finish stores it first, then adds its two bytes: the tail
    flush sees one unit more) and lanes without, at every width; every container equals the oracle's."""
    set_hook("LLCOMP_MI_LANE_SHIFT", "6")
    stage, most, at = fm.constants()
    seen, peak = set(), 0
    for w in range(40, 56):
        img = make_image("g3@%d" % (500 + w), w, 64, 1)
        check(mi, orc, img, w)
        m = fm.Wave([fm.renorms_per_sample(orc, img[y, :, 0].astype(np.int16)) for y in range(64)]).run()
        seen |= set(m.unit_at_finish)
        peak = max(peak, m.peak)
    print("largest fill of a staging area:", peak, "of", stage)
    assert seen == {True, False} and at <= peak <= stage - 1


# ---- carries ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", [1, 2, 3])
def test_carry_streams(mi, orc, set_hook, placement):
    """the crafted streams of tests/carry_streams.py: carries through 17..64 undecided 0xFF bytes -- into staged bytes, and into bytes
    that have left for HBM (later than before: a unit now waits for a flush event)"""
    import carry_streams as cs

    for c in (1, 3):
        img, tw, th, at = cs.rows_mosaic(orc, placement, c)
        for shift in (None, "6"):
            set_hook("LLCOMP_MI_LANE_SHIFT", shift)
            check(mi, orc, img, tw)
            if c == 1:
                check(mi, orc, img, tw, planar=False)


def test_carries_into_flushed_bytes_are_counted(mi, orc):
    import torch

    import carry_streams as cs

    img, tw, th, at = cs.rows_mosaic(orc, 1, 1)
    h, w, c = img.shape
    codec = mi.Codec(1, w, h, c, tw, 1, True)
    st = torch.cuda.current_stream().cuda_stream
    d_px = torch.from_numpy(img).cuda()
    cap = codec.max_payload_bytes
    d_pay = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_len = torch.empty(codec.n_slices, dtype=torch.int32, device="cuda")
    d_tot = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
    codec.encode(d_px.data_ptr(), d_pay.data_ptr(), cap, d_len.data_ptr(), d_tot.data_ptr(), d_st.data_ptr(), st)
    torch.cuda.synchronize()
    counters = codec.counters()
    codec.close()
    assert int(d_st.item()) == 0 and counters["enc_carry_backs"] > 0, counters


# ---- capacity -------------------------------------------------------------------------------------------------------------------------
def test_payload_capacity_overflow_is_reported(mi):
    import torch

    w, h, c = 480, 40, 3
    img = np.random.default_rng(3).integers(0, 256, size=(h, w, c), dtype=np.uint8)
    codec = mi.Codec(1, w, h, c, 480, 1, True)
    st = torch.cuda.current_stream().cuda_stream
    d_px = torch.from_numpy(img).cuda()
    cap = 5000  # far too small for noise
    d_pay = torch.full((cap + 4096,), 0xAB, dtype=torch.uint8, device="cuda")
    d_len = torch.empty(codec.n_slices, dtype=torch.int32, device="cuda")
    d_tot = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
    codec.encode(d_px.data_ptr(), d_pay.data_ptr(), cap, d_len.data_ptr(), d_tot.data_ptr(), d_st.data_ptr(), st)
    torch.cuda.synchronize()
    assert codec.status(int(d_st.item())) == mi.OUTPUT_OVERFLOW
    assert int(d_tot.item()) > cap
    assert bool((d_pay[cap:] == 0xAB).all()), "nothing may be written past the caller's capacity"
    codec.close()


# ---- the shared block in the 2-D snapshot encoder ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [16, 64])
@pytest.mark.parametrize("gen", ["nat", "g3"])
def test_snapshot_encoder(mi, orc, set_hook, tile, gen):
    """16x16 and 64x64 tiles of one small frame (the 36 big tiles share wavefronts only under a forced lane shift)"""
    if tile == 64:
        set_hook("LLCOMP_MI_LANE_SHIFT", "6")
    img = make_image(gen, 256, 192, 3)
    for planar in (True, False):
        k = mi.Codec(1, 256, 192, 3, tile, tile, planar)
        fam = dict(k.family)
        k.close()
        assert fam["snapshot"], fam
        check(mi, orc, img, tile, tile, planar)


# ---- the decoder's checked replay on what this encoder wrote ----------------------------------------------------------------------------
def test_forced_replay(mi, orc, set_hook):
    set_hook("LLCOMP_MI_FORCE_REPLAY", "1")
    check(mi, orc, mixed_rows(480, 3, 4), 480)
