"""The encoders' carry walks on runs that noise never produces (carry_streams.py; every crafted tile is checked on the CPU by
test_carry_streams.py): a carry through 17, 33 and 64 undecided 0xFF bytes -- through whole 16-byte units already stored, across two unit
boundaries, beyond the 28 staged bytes --, runs that long that must STAY FF, runs still open when the slice ends, runs that reach the first
bytes of a stream, runs that open in one launch of the segmented coder and go out in the next, and runs that end at offsets 15, 0 and 1
modulo 16.  Every kernel family that has a walk of its own codes them (csrc/slice_kernels.hip: enc_carry_back, the hand-written carry
subroutine with enc_carry_back_flushed behind it, the segmented coder's parked state, enc_finish_and_count), asserted through Codec.family.
Every container == the oracle's byte for byte, every round trip gives the input back.

Placements (carry_streams.py): 1 = crafted tiles at chosen slices among ordinary ones (lane 0, a middle lane, lane 63 and the last, partial
lane group of 64-lane groups); 2 = every tile the same crafted tile; 3 = the family's cases in turn."""
import numpy as np
import pytest

import carry_streams as cs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


@pytest.fixture
def set_hook(mi, monkeypatch):
    """The library reads its LLCOMP_MI_* test hooks once per process; a test that changes one says so (reload_tuning)."""
    def _set(name, value):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
        mi.reload_tuning()

    yield _set
    monkeypatch.undo()
    mi.reload_tuning()


def family_of(mi, w, h, c, tw, th, planar):
    """the kernel family the library picks for this geometry under the hooks in force"""
    k = mi.Codec(1, w, h, c, tw, th, planar)
    fam = dict(k.family)
    k.close()
    return fam


_wants = {}


def oracle_of(orc, key, img, tw, th, planar):
    """(the oracle's container, its runs >= 17 bytes or None where there are more than the log holds), once per mosaic"""
    if key not in _wants:
        orc.carry_log(min_run=17)
        try:
            orc.carry_stats(reset=True)
            want = orc.compress_sliced(img, tw, th, planar)
            try:
                log = orc.carry_log()
            except OverflowError:
                log = None
        finally:
            orc.carry_log(min_run=1)
        _wants[key] = (want, log)
    return _wants[key]


def same(got, want, ns, what):
    """containers equal; if not, say where: the first differing byte as (slice, offset in its stream) for the event log to locate"""
    if got == want:
        return
    n = min(len(got), len(want))
    at = next((i for i in range(n) if got[i] != want[i]), n)
    lens = np.frombuffer(want[24:24 + 4 * ns], dtype="<u4").astype(np.int64)
    ends = 24 + 4 * ns + np.cumsum(lens)
    sl = int(np.searchsorted(ends, at, side="right"))
    off = at - (int(ends[sl - 1]) if sl else 24 + 4 * ns)
    raise AssertionError(f"{what}: differs from the oracle's at byte {at} = slice {sl}, stream offset {off} (lengths {len(got)} / {len(want)}); "
                         f"got {got[at:at + 8].hex()} want {want[at:at + 8].hex()}" if at >= 24 + 4 * ns else f"{what}: the slice table differs at byte {at}")


def check(mi, orc, key, mosaic, planar, what, expect):
    """the mosaic through the library as the hooks in force have it: family as expected, container == the oracle's, round trip"""
    img, tw, th, at = mosaic
    h, w, c = img.shape
    fam = family_of(mi, w, h, c, tw, th, planar)
    for k, v in expect.items():
        assert fam[k] == v, (what, k, fam)
    want, log = oracle_of(orc, key + (planar,), img, tw, th, planar)
    assert log is None or len(log) >= len(at), (what, "the mosaic does not hold the runs it is meant to", len(log), len(at))
    got = mi.compress_image(img, w, h, c, format=mi.FORMAT_SLICED, tile_w=tw, tile_h=th, planar=planar)
    same(got, want, orc.slice_count(w, h, c, tw, th, planar), what)
    assert np.array_equal(mi.decompress_image(got).pixels, img), (what, "round trip")
    return fam


def lanes_of(at, planes=1, plane=0):
    return {(s * planes + plane) % 64 for s in at}, {(s * planes + plane) // 64 for s in at}


# ---- one-row slices ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", [1, 2, 3])
def test_one_row_slices(mi, orc, set_hook, placement):
    """tiles 600 and 300 wide.  Planar, 1 / 3 / 4 channels (grey: the Y and the alpha plane are the crafted plane): the row encoder that
    reads the pixels itself; interleaved one channel: the row encoder on u32 symbols; LLCOMP_MI_NOROWS=1: the same slices through the 2-D
    kernels, snapshot and table encoder."""
    for c in (1, 3, 4):
        m = cs.rows_mosaic(orc, placement, c)
        if placement == 1 and c == 1:
            lanes, groups = lanes_of(m[3])
            assert {0, 31, 63} <= lanes and 3 in groups and 210 < 4 * 64  # lane 0, a middle one, 63; group 3 = slices 192..209 is partial
        for shift in (None, "6"):
            set_hook("LLCOMP_MI_LANE_SHIFT", shift)
            check(mi, orc, ("rows", placement, c), m, True, f"rows planar c={c} placement {placement} shift {shift}", {"rows": True})
            if c == 1:
                check(mi, orc, ("rows", placement, c), m, False, f"rows interleaved placement {placement} shift {shift}", {"rows": True})
    m = cs.rows_mosaic(orc, placement, 1)
    set_hook("LLCOMP_MI_NOROWS", "1")
    for shift, nosnap in ((None, "0"), ("6", "0"), ("6", "1")):
        set_hook("LLCOMP_MI_LANE_SHIFT", shift)
        set_hook("LLCOMP_MI_NOSNAP", nosnap)
        check(mi, orc, ("rows", placement, 1), m, True, f"rows through the 2-D kernels, placement {placement} shift {shift} nosnap {nosnap}",
              {"rows": False, "lds_table": False, "snapshot": nosnap == "0"})


# ---- 2-D tiles up to 4096 samples: the snapshot encoder (hand-written sample) and the table encoder (C++ walk) -----------------------
@pytest.mark.parametrize("placement", [1, 2, 3])
@pytest.mark.parametrize("tile", [(64, 16), (64, 64)], ids=lambda t: "%dx%d" % t)
def test_2d_tiles(mi, orc, set_hook, tile, placement):
    for c in (1, 3):
        m = cs.tiles_mosaic(orc, tile[0], tile[1], placement, c)
        if placement == 1 and c == 1:
            lanes, groups = lanes_of(m[3])
            assert {0, 31, 63} <= lanes and max(groups) == 3 and len(m[3]) >= 10
        for shift, nosnap in ((None, "0"), ("6", "0"), ("6", "1"), (None, "1")):
            set_hook("LLCOMP_MI_LANE_SHIFT", shift)
            set_hook("LLCOMP_MI_NOSNAP", nosnap)
            fam = check(mi, orc, ("tiles", tile, placement, c), m, True, f"{tile} planar c={c} placement {placement} shift {shift} nosnap {nosnap}",
                        {"rows": False, "lds_table": False, "snapshot": nosnap == "0"})
            assert fam["slices_per_wave"] == 1 << fam["lane_shift"] and fam["slices_per_wave"] == (64 if shift else fam["slices_per_wave"]) > 1, fam


# ---- tiles above 4096 samples: the segmented coder parks low, range, the staged bytes and `flushed` between its launches -------------
@pytest.mark.parametrize("placement", [1, 2, 3])
@pytest.mark.parametrize("tile", [(128, 48), (96, 64)], ids=lambda t: "%dx%d" % t)
def test_segmented_coder(mi, orc, set_hook, tile, placement):
    """runs that open before sample 4096 and go out behind it, among ragged tiles that end in the first launch"""
    m = cs.segmented_mosaic(orc, tile[0], tile[1], placement)
    for shift, overlap, nosnap in (("2", None, "0"), ("6", None, "0"), ("2", "0", "0"), ("6", "0", "0"), ("2", "1", "0"), ("6", "1", "0"), ("6", None, "1")):
        set_hook("LLCOMP_MI_LANE_SHIFT", shift)
        set_hook("LLCOMP_MI_OVERLAP", overlap)
        set_hook("LLCOMP_MI_NOSNAP", nosnap)
        check(mi, orc, ("seg", tile, placement), m, True, f"{tile} placement {placement} shift {shift} overlap {overlap} nosnap {nosnap}",
              {"rows": False, "lds_table": False, "snapshot": nosnap == "0", "lane_shift": int(shift)})


# ---- one slice per wavefront, its table in LDS; also the LEGACY format ----------------------------------------------------------------
@pytest.mark.parametrize("name", cs.names("64x64-"))
def test_one_slice_per_wavefront(mi, orc, set_hook, name):
    tile = cs.build(orc, name).tile
    img = cs.pixels(orc, tile, 1)
    orc.carry_stats(reset=True)
    legacy = orc.compress_image(img)
    assert any(e.run >= cs.CASES[name].min_run for e in orc.carry_log())
    for noldstab in (None, "1"):
        set_hook("LLCOMP_MI_NOLDSTAB", noldstab)
        fam = family_of(mi, 64, 64, 1, 64, 64, False)
        assert fam["lds_table"] == (noldstab is None) and not fam["rows"], fam
        got = mi.compress_image(img, 64, 64, 1)
        assert got == legacy, (name, noldstab, "legacy stream")
        assert np.array_equal(mi.decompress_image(got).pixels, img)
        for planar in (False, True):
            s = mi.compress_image(img, 64, 64, 1, format=mi.FORMAT_SLICED, tile_w=64, tile_h=64, planar=planar)
            same(s, orc.compress_sliced(img, 64, 64, planar), 1, f"{name} one slice, noldstab {noldstab}")
            assert np.array_equal(mi.decompress_image(s).pixels, img)


# ---- fewer active lanes per wavefront --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lpw", ["1", "7"])
def test_lanes_per_wave(mi, orc, set_hook, lpw):
    set_hook("LLCOMP_MI_LANE_SHIFT", "6")
    set_hook("LLCOMP_MI_LPW", lpw)
    want = 1 if lpw == "1" else 4  # (rounded down to a power of two)
    fam = check(mi, orc, ("rows", 3, 1), cs.rows_mosaic(orc, 3, 1), True, f"rows lpw {lpw}", {"rows": True})
    assert fam["slices_per_wave"] == want, fam
    set_hook("LLCOMP_MI_NOLDSTAB", "1")  # (one active lane per wavefront would otherwise take the table into LDS: another encoder)
    fam = check(mi, orc, ("tiles", (64, 16), 3, 1), cs.tiles_mosaic(orc, 64, 16, 3, 1), True, f"64x16 lpw {lpw}", {"rows": False, "snapshot": True})
    assert fam["slices_per_wave"] == want, fam


# ---- interleaved colour: three and five channels in one stream (five: the generic kernels) ---------------------------------------------
def test_interleaved_colour(mi, orc, set_hook):
    for c, tw, th, prefix, rows in ((3, 64, 16, "il3-64x16-", False), (5, 40, 16, "il5-40x16-", False), (3, 200, 1, "il3-200x1-", True), (5, 120, 1, "il5-120x1-", False)):
        if th == 1:
            pool = cs.names(prefix)
            at = {i: pool[i % len(pool)] for i in range(0, 3 * 70, 2)}
            m = (cs.grid_image(orc, 3, 70, tw, 1, at, c), tw, 1, at)
        else:
            m = cs.tiles_mosaic(orc, tw, th, 3, c, prefix)
        for shift, nosnap in ((None, "0"), ("6", "0"), ("6", "1")):
            set_hook("LLCOMP_MI_LANE_SHIFT", shift)
            set_hook("LLCOMP_MI_NOSNAP", nosnap)
            check(mi, orc, ("il", prefix), m, False, f"{prefix} interleaved shift {shift} nosnap {nosnap}",
                  {"rows": rows, "lds_table": False} if rows else {"rows": False, "lds_table": False, "snapshot": nosnap == "0"})
    # ... and one interleaved tile alone as a LEGACY stream
    img = cs.pixels(orc, cs.build(orc, "il3-64x16-carry").tile, 3)
    got = mi.compress_image(img, 64, 16, 3)
    assert got == orc.compress_image(img)
    assert np.array_equal(mi.decompress_image(got).pixels, img)


# ---- the counter of carries that left the staging area ----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["rows", "64x64", "128x48"])
def test_long_carries_are_counted(mi, orc, set_hook, which):
    """enc_carry_backs counts the carries that went on into bytes already stored to HBM.  A carry through 28 bytes or more has left the
    staging area, which never holds more than 28 (slice_kernels.hip: kStageBytes): the counter is at least the number of those in the
    oracle's log of the batch, and at most the number of all carries through undecided bytes."""
    import torch

    set_hook("LLCOMP_MI_LANE_SHIFT", "6")
    img, tw, th, at = {"rows": lambda: cs.rows_mosaic(orc, 1, 1), "64x64": lambda: cs.tiles_mosaic(orc, 64, 64, 1, 1),
                       "128x48": lambda: cs.segmented_mosaic(orc, 128, 48, 1)}[which]()
    orc.carry_log(min_run=28)
    try:
        orc.carry_stats(reset=True)
        want = orc.compress_sliced(img, tw, th, True)
        long_carries = sum(e.carried for e in orc.carry_log())
        all_carries, longest = orc.carry_stats()
    finally:
        orc.carry_log(min_run=1)
    assert long_carries >= 3 and longest >= 33, (long_carries, longest)
    h, w, c = img.shape
    codec = mi.Codec(1, w, h, c, tw, th, True)
    assert codec.family["rows"] == (which == "rows") and not codec.family["lds_table"], codec.family
    st = torch.cuda.current_stream().cuda_stream
    d_px = torch.from_numpy(img).cuda()
    cap = codec.max_payload_bytes
    d_pay = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_len = torch.empty(codec.n_slices, dtype=torch.int32, device="cuda")
    d_tot = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
    codec.encode(d_px.data_ptr(), d_pay.data_ptr(), cap, d_len.data_ptr(), d_tot.data_ptr(), d_st.data_ptr(), st)
    torch.cuda.synchronize()
    assert int(d_st.item()) == 0
    n = codec.n_slices
    assert d_len.cpu().numpy().astype("<u4").tobytes() == want[24:24 + 4 * n] and d_pay[:int(d_tot.item())].cpu().numpy().tobytes() == want[24 + 4 * n:]
    got = codec.counters()["enc_carry_backs"]
    print(f"{which}: enc_carry_backs {got}, carries through >= 28 bytes {long_carries}, all carries through undecided bytes {all_carries}")
    assert long_carries <= got <= all_carries, (which, long_carries, got, all_carries)
    codec.close()
