"""The torch formulations of tests/large_wide_formulations.py, which the large legs of the wide id-map calls
(tests/test_gpu_large_wide_id_maps.py) take for their expectations, against the numpy specs of the small tests, on the CPU: ids_of and
wide_maps (tests/test_wide_id_maps_rule.py), target_spec (tests/test_gpu_wide_id_maps.py), apply32 and select
(tests/test_wide_id_paste_rule.py).  Every comparison is exact."""
import numpy as np
import pytest

import large_wide_formulations as F
from batch_support import gen_batch
from test_gpu_wide_id_maps import target_spec
from test_wide_id_maps_rule import HIGH_BYTES, TOP, WIDTHS, draw, ids_of, wide_maps
from test_wide_id_paste_rule import POOL, Window, apply32, gen_ids, select

DEV = "cpu"


def dev_maps(ids, mb):
    """host ids [...] -> the maps as the legs view them on the device: uint8 [..., 3] or int32 [...]"""
    import torch

    m = wide_maps(ids, mb)
    return torch.from_numpy(m.copy() if mb == 3 else m.view(np.int32).copy()).to(DEV)


@pytest.mark.parametrize("mb", WIDTHS)
def test_ids_rebuilt_from_the_pixels_bytes(mb):
    rng = np.random.default_rng(mb)
    ids = rng.integers(0, TOP[mb] + 1, size=(2, 9, 31))
    ids[0, 0, :4] = (0, TOP[mb], TOP[mb] - 1, 1 << (8 * mb - 1))  # the ends, and the top bit alone (negative as int32)
    got = F.ids_of_maps(dev_maps(ids, mb), mb)
    assert np.array_equal(got.numpy(), ids) and np.array_equal(got.numpy(), ids_of(wide_maps(ids, mb)))


@pytest.mark.parametrize("mb", WIDTHS)
def test_index_and_planes_of_a_band_per_listed_id(mb):
    import torch

    rng = np.random.default_rng(10 + mb)
    ids, lists = draw(rng, mb, 3, 13, 37)
    lists[2] = sorted(set(lists[2]) | {TOP[mb], HIGH_BYTES[mb][1]})
    assert lists[1] == [] and max(max(l) for l in lists if l) > 0xFFFF
    values = [rng.integers(-3, 4, size=len(l)).tolist() for l in lists]
    values[2][0] = -(1 << 31)
    for i in range(3):
        m = F.ids_of_maps(dev_maps(ids[i], mb), mb)
        for dtype, tdtype, default in (("int32", torch.int32, -100), ("uint8", torch.uint8, 255), ("int64", torch.int64, -100)):
            vals = [[v & 0xFF for v in l] for l in values] if dtype == "uint8" else values
            want = target_spec(ids[i:i + 1], lists[i:i + 1], vals[i:i + 1], dtype=dtype, default=default)
            got = F.index_of(m, lists[i], vals[i], default, tdtype)
            assert np.array_equal(got.numpy().reshape(-1).view(np.uint8), want), (i, dtype)
        for dtype, tdtype, on, off, bits in (("uint8", torch.uint8, 255, 7, (255, 7)), ("float16", torch.int16, 0.9, 0.05, (0x3B33, 0x2A66))):
            want = target_spec(ids[i:i + 1], lists[i:i + 1], values[i:i + 1], kind="planes", dtype=dtype, default=1, planes=[3], on=on, off=off)
            got = F.planes_of(m, lists[i], values[i], 1, 3, bits[0], bits[1], tdtype)
            assert np.array_equal(got.numpy().reshape(-1).view(np.uint8), want), (i, dtype)
    assert np.array_equal(np.array([0.9, 0.05], np.float16).view(np.uint16), [0x3B33, 0x2A66])


def windows_of(rng, mb):
    """windows at the bases the legs use, the last passing the top id; every one with bits set and bits clear"""
    bases = [0, 0x00FF00, 0xFF0001, TOP[mb] - 100] + ([0x80000000] if mb == 4 else [])
    return [Window(b, rng.integers(0, 3, size=256) > 0) for b in bases]


@pytest.mark.parametrize("mb", WIDTHS)
def test_a_windowed_piece_and_a_window_past_the_top_id(mb):
    import torch

    rng = np.random.default_rng(20 + mb)
    top = TOP[mb]
    pool = np.array(sorted(set(POOL[mb]) | {0, 5, 255, 256, 0x00FF00, 0x00FF80, 0x00FFFF, 0x010000, 0xFF0001, 0xFF0100, 0xFF0101, top - 101, top - 100, top - 1, top}
                           | ({0x7FFFFFFF, 0x80000000, 0x800000FF, 0x80000100} if mb == 4 else set())), np.int64)
    ids = pool[rng.integers(0, len(pool), size=(1, 9, 41))]
    m = F.ids_of_maps(dev_maps(ids[0], mb), mb)
    for win in windows_of(rng, mb) + [Window(top - 9, np.ones(256, bool)), Window(top, np.ones(256, bool))]:
        want = select(ids[0], win)
        assert np.array_equal(F.window_selects(m, win.base, win.lut).numpy(), want) and (win.base == top - 9 or want.any()), hex(win.base)
        if win.base + 255 > top:  # nothing below the base, which 32-bit arithmetic would wrap into the window
            assert not want[ids[0] < win.base].any() and want[ids[0] == top].all()
    c = 3
    src, dst = gen_batch("uint8", 1, c, 9, 41, "hwc", 1), gen_batch("uint8", 1, c, 11, 43, "hwc", 2)
    wins = windows_of(rng, mb)
    recs = [(0, 0, 1, 2, 3, 0, 30, 8, wins[0]), (0, 0, 2, 1, 0, 2, 41, 7, wins[3]), (0, 0, 10, 3, 5, 1, 25, 6, wins[2], 0xC7),
            (0, 0, 2, 0, 1, 1, 33, 8, wins[1], 0xC0B0A1, True), (0, 0, 13, 10, 11, 8, 30, 1, wins[-1])]
    dv, sv = torch.from_numpy(dst[0].copy()), torch.from_numpy(src[0].copy())
    for r in recs:
        F.paste_piece32(dv, sv, (m[r[5]:r[5] + r[7]], r[5]) if r is recs[1] else m, r[2:8], r[8], *r[9:])
    want = apply32(src, ids, dst, recs, "hwc")
    assert np.array_equal(dv.numpy(), want[0]) and not np.array_equal(want[0], dst[0])
    # a map that is its own source (uint8 HWC, c = 3), and 2-byte elements beside a map of their own
    if mb == 3:
        own = wide_maps(gen_ids(rng, 3, 1, 9, 41), 3)
        ids = ids_of(own)
        wins3 = [Window(0, np.ones(256, bool)), Window(0xFF0001, np.ones(256, bool))]
        recs = [(0, 0, 1, 2, 3, 0, 30, 8, wins3[0]), (0, 0, 2, 0, 1, 1, 33, 8, wins3[1], 0x030201, True)]
        dv, sv = torch.from_numpy(dst[0].copy()), torch.from_numpy(own[0].copy())
        for r in recs:
            F.paste_piece32(dv, sv, F.ids_of_bytes(sv), r[2:8], r[8], *r[9:])
        assert np.array_equal(dv.numpy(), apply32(own, ids, dst, recs, "hwc")[0])
    else:
        s16, d16 = gen_batch("float16", 1, 1, 9, 41, "hwc", 3), gen_batch("float16", 1, 1, 11, 43, "hwc", 4)
        recs = [(0, 0, 1, 2, 3, 0, 30, 8, wins[4]), (0, 0, 10, 3, 5, 1, 25, 6, wins[0], 0xFC01)]
        dv, sv = torch.from_numpy(d16[0].view(np.int16).copy()), torch.from_numpy(s16[0].view(np.int16).copy())
        for r in recs:
            F.paste_piece32(dv, sv, m, r[2:8], r[8], *r[9:])
        assert np.array_equal(dv.numpy().view(np.uint16), apply32(s16, ids, d16, recs, "hwc").view(np.uint16)[0])


@pytest.mark.parametrize("c", (1, 2, 3, 4))
def test_the_value_pixel_bytes(c):
    value = 0xD4C3B2A1 & ((1 << (8 * c)) - 1)
    ids = np.zeros((1, 2, 5), np.int64)
    dst = gen_batch("uint8", 1, c, 2, 5, "hwc", 5)
    want = apply32(dst, ids, dst, [(0, 0, 0, 0, 0, 0, 5, 2, [0], value, True)], "hwc")
    assert (want == np.array(F.value_pixel_bytes(value, c), np.uint8)).all() and F.value_pixel_bytes(value, c) == [0xA1, 0xB2, 0xC3, 0xD4][:c]
