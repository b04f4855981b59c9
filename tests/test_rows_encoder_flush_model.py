"""The batched flush policy of the 1-row-slice encoder, replayed on the oracle's per-sample byte counts (tests/rows_flush_model.py):
the fill of a lane's staging area never reaches the area's last byte -- the neighbour's dummy byte lands there --, no sample adds more
than kSampleBytesMax bytes, and one 16-byte unit per lane and flush event is enough.  No GPU."""
import numpy as np
import pytest

import carry_streams as cs
import rows_flush_model as fm


def test_constants_fit():
    stage, most, at = fm.constants()
    assert at >= 16 and at - 1 + most <= stage - 1 and (at - 1 + most) - 16 <= at - 1


def noise_rows(w, n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, w), dtype=np.uint8).astype(np.int16)


def adversarial_rows(w):
    """long constant runs saturate the models, then full-scale steps: the dearest samples an 8-bit plane can give, alone and in bursts"""
    x = np.arange(w)
    rows = [np.where(x % 97 == 96, 255, 0), np.where((x // 40) % 2 == 0, 0, np.where(x % 2 == 0, 255, 0)),
            np.where(x < w // 2, 7, np.where(x % 3 == 0, 0, 255)), np.where(x % 2 == 0, 0, 255), np.zeros(w), np.full(w, 255)]
    return np.array(rows).astype(np.int16)


def carry_rows(orc):
    """the crafted 600-sample rows whose streams carry through (or hold) long runs of 0xFF"""
    out = []
    for name in ("row600-carry33", "row600-ff33", "row600-carry64"):
        got = cs.build(orc, name)
        assert got is not None, name
        out.append(got.tile.reshape(-1))
    return np.array(out)


@pytest.mark.parametrize("kind", ["noise", "carry", "adversarial"])
def test_fill_stays_inside_the_area(orc, kind):
    rows = {"noise": lambda: noise_rows(480, 6, 5), "carry": lambda: carry_rows(orc), "adversarial": lambda: adversarial_rows(480)}[kind]()
    counts = [fm.renorms_per_sample(orc, r) for r in rows]
    stage, most, at = fm.constants()
    assert max(int(c.max()) for c in counts) <= most
    for alone in (True, False):
        m = fm.Wave(counts, alone=alone).run()
        assert m.peak <= stage - 1 and m.events > 0, (kind, alone, m.peak, m.events)


def test_the_dummy_byte_can_come_late(orc):
    """why the fill stops one byte short of the area: a flat neighbour renormalises for the first time -- the dummy byte, into the last
    byte of this lane's area -- after more samples than a busy lane needs to fill its area"""
    stage, most, at = fm.constants()
    flat = fm.renorms_per_sample(orc, np.full(480, 128, dtype=np.int16))
    first = int(np.argmax(flat > 0))
    assert flat[first] > 0 and first * most > stage, first


def test_batches_store_less_often_than_every_sample(orc):
    """64 noise lanes: a flush event about every third sample (every sample under the old policy: some lane has a unit in nearly all)"""
    counts = [fm.renorms_per_sample(orc, r) for r in noise_rows(200, 64, 9)]
    m = fm.Wave(counts).run()
    old_events = 0
    fill = np.full(64, -1)
    for s in range(200):
        go = fill >= 16
        old_events += bool(go.any())
        fill[go] -= 16
        fill += np.array([c[s] for c in counts])
    print("events per 200 samples: batched", m.events, "every-sample", old_events, "stores", m.stores)
    assert m.events * 2 < old_events
