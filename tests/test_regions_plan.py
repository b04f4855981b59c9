"""Regions decode (a rectangle of one size at an offset of its own in every frame), host side: llcomp_mi_regions_plan against the
covered boxes of llcomp_mi_region_plan and a brute-force class count, pack_batch, and the class sub-geometries of geometry.hpp
(compiled helper).  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd
    from llcomp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "llcomp_amd", "csrc")])
    return llcomp_amd


def check_plan(mi, w, h, c, tw, th, planar, rw, rh, xy):
    """every window has Wx x Wy tiles, lies in the image and contains region_plan's box; n_classes = the distinct window pixel sizes"""
    windows, n_classes = mi.regions_plan(w, h, c, tw, th, planar, rw, rh, xy)
    ttw = w if tw == 0 or tw > w else tw
    tth = h if th == 0 or th > h else th
    ntx, nty = -(-w // ttw), -(-h // tth)
    wx, wy = min(ntx, (rw + ttw - 2) // ttw + 1), min(nty, (rh + tth - 2) // tth + 1)
    assert windows.shape == (len(xy), 4)
    sizes = set()
    for (x, y), (wx0, wy0, wx1, wy1) in zip(xy, windows.tolist()):
        (bx0, by0, bx1, by1), _ = mi.region_plan(w, h, c, tw, th, planar, x, y, rw, rh)
        assert (wx1 - wx0, wy1 - wy0) == (wx, wy), (w, h, tw, th, rw, rh, x, y)
        assert 0 <= wx0 <= bx0 and bx1 <= wx1 <= ntx and 0 <= wy0 <= by0 and by1 <= wy1 <= nty, (w, h, tw, th, rw, rh, x, y)
        assert (wx0, wy0) == (min(x // ttw, ntx - wx), min(y // tth, nty - wy))
        sizes.add((min(wx1 * ttw, w) - wx0 * ttw, min(wy1 * tth, h) - wy0 * tth))
    assert n_classes == len(sizes), (w, h, tw, th, rw, rh, xy)
    assert 1 <= n_classes <= (2 if w % ttw else 1) * (2 if h % tth else 1)
    return n_classes


def test_regions_plan_random_and_edge_shapes(mi):
    rng = np.random.default_rng(1016)
    n = 0
    for _ in range(300):
        w, h = int(rng.integers(1, 3000)), int(rng.integers(1, 2000))
        c, planar = int(rng.integers(1, 6)), bool(rng.integers(0, 2))
        kind = int(rng.integers(0, 5))
        if kind == 0:
            tw, th = 0, 0                                               # one tile
        elif kind == 1:
            tw, th = int(rng.integers(1, w + 1)), int(rng.integers(1, 3))  # 1- and 2-row tiles
        elif kind == 2:
            tw, th = 64, 64
            w, h = 64 * max(1, w // 64), 64 * max(1, h // 64)           # tile multiples
        else:
            tw, th = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
        for rw, rh in ((int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))), (w, h), (1, 1), (w, 1), (min(w, tw or w), min(h, th or h))):
            frames = int(rng.integers(1, 9))
            xy = [(int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1))) for _ in range(frames)]
            xy += [(0, 0), (w - rw, 0), (0, h - rh), (w - rw, h - rh)]
            check_plan(mi, w, h, c, tw, th, planar, rw, rh, xy)
            n += 1
    assert n >= 1500


def test_regions_plan_class_counts(mi):
    # 4K at 480x1: tile-aligned, one class whatever the offsets
    assert check_plan(mi, 3840, 2160, 3, 480, 1, True, 224, 224, [(0, 0), (3616, 1936), (1000, 7)]) == 1
    # 4K at 64x64: 2160 % 64 != 0 -- a crop whose window reaches the last tile row is the second class
    assert check_plan(mi, 3840, 2160, 3, 64, 64, False, 224, 224, [(0, 0), (3616, 1936)]) == 2
    assert check_plan(mi, 3840, 2160, 3, 64, 64, False, 224, 224, [(0, 0), (3616, 100)]) == 1
    # partial last column and row: two classes when every window holds the last tile row, four when not
    assert check_plan(mi, 100, 37, 3, 32, 16, True, 40, 20, [(0, 0), (60, 0), (0, 17), (60, 17)]) == 2  # (Wy = nty: every window has the last row)
    assert check_plan(mi, 300, 200, 3, 32, 16, False, 40, 20, [(0, 0), (260, 0), (0, 180), (260, 180)]) == 4
    # windows capped at ntx / nty, rw = w: one window, the whole frame
    windows, k = mi.regions_plan(160, 41, 3, 40, 2, True, 160, 41, [(0, 0)] * 3)
    assert k == 1 and (windows == [0, 0, 4, 21]).all()
    # the clamped-tile case: the 1-row remainder of 2-row tiles is a window of its own
    windows, k = mi.regions_plan(160, 41, 3, 40, 2, True, 100, 1, [(10, 40), (10, 39), (10, 0)])
    assert k == 2 and windows.tolist() == [[0, 20, 4, 21], [0, 19, 4, 20], [0, 0, 4, 1]]


def test_regions_plan_refuses_bad_arguments(mi):
    good = (100, 50, 3, 16, 16, False)
    for rw, rh, xy in ((0, 10, [(0, 0)]), (10, 0, [(0, 0)]), (10, 10, [(0, 0), (91, 0)]), (10, 10, [(0, 41)]), (10, 10, [(100, 0)]),
                       (2**32 - 5, 1, [(10, 0)]), (1, 2**32 - 5, [(0, 10)])):
        with pytest.raises(mi.LlcompError) as e:
            mi.regions_plan(*good, rw, rh, xy)
        assert e.value.status == mi.BAD_ARGS, (rw, rh, xy)
    with pytest.raises(mi.LlcompError) as e:
        mi.regions_plan(100, 50, 0, 16, 16, False, 1, 1, [(0, 0)])  # no channels
    assert e.value.status == mi.BAD_ARGS
    for xy in ([], [(1, 2, 3)], np.zeros((2, 2), np.float32), [(-1, 0)]):  # the binding's own checks of the table
        with pytest.raises(mi.LlcompError) as e:
            mi.regions_plan(*good, 1, 1, xy)
        assert e.value.status == mi.BAD_ARGS
    # the C entry point itself: n = 0, NULL table, NULL n_classes
    import ctypes as C

    L = mi._lib.load()
    k = C.c_uint32()
    tab = (C.c_uint32 * 2)(0, 0)
    assert L.llcomp_mi_regions_plan(100, 50, 3, 16, 16, 0, 1, 1, tab, 0, None, C.byref(k)) == mi.BAD_ARGS
    assert L.llcomp_mi_regions_plan(100, 50, 3, 16, 16, 0, 1, 1, None, 1, None, C.byref(k)) == mi.BAD_ARGS
    assert L.llcomp_mi_regions_plan(100, 50, 3, 16, 16, 0, 1, 1, tab, 1, None, None) == mi.BAD_ARGS
    assert L.llcomp_mi_regions_plan(100, 50, 3, 16, 16, 0, 1, 1, tab, 1, None, C.byref(k)) == mi.OK and k.value == 1
    # nothing is written when one rectangle is bad
    win = (C.c_uint32 * 8)(*([7] * 8))
    tab2 = (C.c_uint32 * 4)(0, 0, 95, 0)
    assert L.llcomp_mi_regions_plan(100, 50, 3, 16, 16, 0, 10, 1, tab2, 2, win, C.byref(k)) == mi.BAD_ARGS
    assert list(win) == [7] * 8


def hand_rolled(containers):
    """the concatenation tests/test_gpu_region.py's Batch builds by hand"""
    lens, pays = [], []
    for d in containers:
        n = int.from_bytes(d[20:24], "little")
        lens.append(np.frombuffer(d[24:24 + 4 * n], dtype="<u4"))
        pays.append(d[24 + 4 * n:])
    return np.frombuffer(b"".join(pays), np.uint8), np.concatenate(lens)


def test_pack_batch_matches_the_hand_rolled_concatenation(mi, orc):
    from conftest import make_image

    for (w, h, c, tw, th, planar) in ((100, 37, 3, 32, 16, True), (90, 40, 5, 32, 8, False), (300, 12, 3, 64, 1, True)):
        conts = [orc.compress_sliced(np.ascontiguousarray(np.roll(make_image(g, w, h, c), 7 * i, axis=1)), tw, th, planar)
                 for i, g in enumerate(["g1", "g3", "mid", "checker", "nat"])]
        pay, lens = mi.pack_batch(conts)
        want_pay, want_lens = hand_rolled(conts)
        assert pay.dtype == np.uint8 and lens.dtype == np.uint32
        assert np.array_equal(pay, want_pay) and np.array_equal(lens, want_lens)
        assert len(lens) == 5 * mi.slice_count(w, h, c, tw, th, planar) and int(lens.sum()) == len(pay)
    # bytes after the last slice are dropped: the next container's payload still starts where its table says
    a, b = conts[0], conts[1]
    pay, lens = mi.pack_batch([a + b"\xee" * 5, b])
    assert np.array_equal(pay, hand_rolled([a, b])[0])


def test_pack_batch_refuses_mismatches(mi, orc):
    from conftest import make_image

    img = make_image("nat", 64, 40, 3)
    base = orc.compress_sliced(img, 32, 8, True)
    others = [orc.compress_sliced(make_image("nat", 64, 48, 3), 32, 8, True),          # another shape
              orc.compress_sliced(img, 16, 8, True),                                   # another tiling
              orc.compress_sliced(img, 32, 8, False),                                  # interleaved
              orc.compress_sliced(make_image("nat", 64, 40, 4), 32, 8, True),          # another channel count
              orc.compress_image(img)]                                                 # LEGACY
    orc.set_small_model(True)
    try:
        others.append(orc.compress_sliced(img, 32, 8, True))                           # the small model
    finally:
        orc.set_small_model(False)
    for o in others:
        with pytest.raises(mi.LlcompError) as e:
            mi.pack_batch([base, o])
        assert e.value.status == mi.BAD_ARGS
    with pytest.raises(mi.LlcompError) as e:
        mi.pack_batch([])
    assert e.value.status == mi.BAD_ARGS
    with pytest.raises(mi.LlcompError) as e:
        mi.pack_batch([base, base[:-3]])
    assert e.value.status == mi.TRUNCATED


def test_class_sub_geometries_fit_the_codec_workspace(tmp_path):
    """geometry.hpp: every window contains its covered box, every class's sub-slice j is full slice regions_full_id(j) (same rectangle,
    frame, plane; no slice twice in a batch), and the class sub-geometries fit the full geometry's workspace -- always with the default
    tuning; under forced LANE_SHIFT / LPW they fit or are refused (never written past)"""
    exe = str(tmp_path / "regions_fit_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "llcomp_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "helpers", "regions_fit_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, cases, fits, refused = out.stdout.split()
    assert word == "ok" and int(cases) >= 20000 and int(fits) + int(refused) == int(cases)

