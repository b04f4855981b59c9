"""The crafted tiles of carry_streams.CASES, checked with the oracle alone: every row meets its condition ON THE ORACLE'S EVENT LOG
(orc.carry_log), with the seed, the run length and the way out that the table states.  A tile that does not is a failure here, never a
case that the GPU tests skip.  The conditions (what each makes an eager encoder do, csrc/slice_kernels.hip):

  (a) a carry through a run >= 17: through a whole 16-byte unit already stored
  (b) a carry through a run >= 33: across two unit boundaries, and longer than the 28 staging bytes ever in use
  (c) a run >= 33 that stays FF: nothing may touch it
  (d) a run >= 17 still open when the slice ends: finish() resolves it, once by its carry, once as FF
  (e) a run whose held byte is among the first two bytes of the stream: the walk reaches the start
  (f) tiles above 4096 samples: the run opens in one launch of the segmented coder and goes out in the next, with a carry and without
  (g) carries whose run ends at byte offsets 15, 0 and 1 modulo 16
"""
import numpy as np
import pytest

import carry_streams as cs


def test_event_log_describes_the_stream(orc):
    """the log against the bytes: a run that carried reads `held + 1, 00 x run` in the stream, one that stayed `held, FF x run`; runs of
    noise are logged one by one (count and longest == the counters'), a reset empties the log, and min_run filters it"""
    rng = np.random.default_rng(5)
    tile = rng.integers(0, 256, size=(40, 64, 1)).astype(np.int16)
    stream, log = cs.encode_logged(orc, tile)
    runs, longest = orc.carry_stats()
    assert runs == sum(e.carried for e in log) > 3 and longest == max(e.run for e in log if e.carried)
    for e in log:
        body = stream[e.offset + 1:e.offset + 1 + e.run]
        assert body == (b"\x00" if e.carried else b"\xff") * e.run, e
        assert 0 <= e.opened <= e.resolved <= tile.size and e.stream == 0
    assert any(not e.carried for e in log)
    orc.carry_log(min_run=2)
    try:
        _, log2 = cs.encode_logged(orc, tile)
        assert log2 == [e for e in log if e.run >= 2]
    finally:
        orc.carry_log(min_run=1)
    orc.carry_stats(reset=True)
    assert orc.carry_log() == []
    # more runs than the log holds: reading it says so
    orc.encode_samples(rng.integers(0, 256, size=(512, 512, 1)).astype(np.int16))
    with pytest.raises(OverflowError):
        orc.carry_log()
    # streams of a container are numbered in its order
    orc.carry_stats(reset=True)
    img = rng.integers(0, 256, size=(32, 64, 1), dtype=np.uint8)
    orc.compress_sliced(img, 16, 16, True)
    assert {e.stream for e in orc.carry_log()} <= set(range(8)) and len({e.stream for e in orc.carry_log()}) > 1


@pytest.mark.parametrize("name", sorted(cs.CASES))
def test_case_meets_its_condition(orc, name):
    c = cs.CASES[name]
    got = cs.build(orc, name)
    assert got is not None, f"{name}: no seed of the budget of {cs.BUDGET} gives a legal tile that meets the condition"
    e = got.event
    print(f"{name}: seed {got.seed}, run {e.run} at offset {e.offset}, {cs.how_of(e)}, samples {e.opened}..{e.resolved}")
    assert (got.seed, e.run, cs.how_of(e)) == (c.seed, c.run, c.how), "the case table does not say what the search finds"
    assert got.seed < cs.BUDGET and got.tile.shape == (c.h, c.w, c.nch) and cs.legal(orc, got.tile)
    # the condition itself, spelled out once more from the table
    cond = dict(c.cond)
    assert e.run >= c.min_run and e.carried == c.carry and e.in_finish == bool(cond.get("open_end"))
    if "first" in cond:
        assert e.offset <= 1 and e.run >= 2
    if "crosses" in cond:
        assert c.w * c.h * c.nch > cs.SEG and e.opened < cs.SEG <= e.resolved
    if "ends" in cond:
        assert (e.offset + e.run) % 16 == cond["ends"]
    if cond.get("open_end"):
        assert e.resolved == c.w * c.h * c.nch
    # ... and the bytes agree with the log
    stream = orc.encode_samples(got.tile)
    assert stream[e.offset + 1:e.offset + 1 + e.run] == (b"\x00" if e.carried else b"\xff") * e.run
    # the pixels of the tile code to the same stream (the tile is what a container's slice sees)
    px = cs.pixels(orc, got.tile, max(c.nch, 1))
    assert np.array_equal(orc.forward_rct(px), got.tile)


def test_the_table_covers_every_condition():
    """the letters above, per tile family"""
    by = lambda pred: [n for n, c in cs.CASES.items() if pred(c, dict(c.cond))]  # noqa: E731
    plain = lambda k: not k  # noqa: E731
    for w, h in ((600, 1), (300, 1), (64, 16), (64, 64)):
        here = lambda c: (c.w, c.h, c.nch) == (w, h, 1)  # noqa: E731
        assert by(lambda c, k: here(c) and c.carry and c.min_run >= 17 and plain(k)), (w, h, "a")
        assert by(lambda c, k: here(c) and c.carry and c.min_run >= 33 and plain(k)), (w, h, "b")
        assert by(lambda c, k: here(c) and not c.carry and c.min_run >= 33 and plain(k)), (w, h, "c")
    for carry in (True, False):
        assert by(lambda c, k: k.get("open_end") and c.carry == carry and c.min_run >= 17), "d"
        for w, h in ((128, 48), (96, 64)):
            assert by(lambda c, k: (c.w, c.h) == (w, h) and k.get("crosses") == 4096 and c.carry == carry and c.min_run >= 17), "f"
    assert by(lambda c, k: k.get("first") == 1 and c.run >= 2), "e"
    for r in (15, 0, 1):
        assert by(lambda c, k: k.get("ends") == r and c.carry), "g"
