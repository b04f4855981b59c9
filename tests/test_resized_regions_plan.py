"""llcomp_mi_resized_regions_plan (host only): the windows of a rectangle of its own size per frame, all sized for the batch's largest
rectangle -- llcomp_mi_regions_plan's rule, so equal sizes give its plan window for window."""
import ctypes as C

import numpy as np
import pytest

import llcomp_amd as mi
from resize_spec import random_resized_crop

SHAPES = [  # w, h, c, tile_w, tile_h, planar
    (3840, 2160, 3, 480, 1, True), (3840, 2160, 3, 64, 64, False), (32, 32, 3, 12, 10, True), (160, 41, 3, 40, 2, True),
    (1100, 24, 3, 480, 1, True), (404, 328, 4, 64, 64, True), (97, 61, 1, 0, 0, False),
]


def _tiles(w, h, tw, th):
    tw = w if tw == 0 or tw > w else tw
    th = h if th == 0 or th > h else th
    return tw, th, -(-w // tw), -(-h // th)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}_{s[3]}x{s[4]}" for s in SHAPES])
def test_windows_contain_rects_and_share_one_size(shape):
    w, h, c, tw, th, planar = shape
    rng = np.random.default_rng(w * 7 + h)
    tw_, th_, ntx, nty = _tiles(w, h, tw, th)
    for _ in range(20):
        n = int(rng.integers(1, 9))
        rects = np.array([random_resized_crop(rng, w, h) for _ in range(n)], np.int64)
        if rng.integers(0, 3) == 0:
            rects[0] = (int(rng.integers(0, w)), int(rng.integers(0, h)), 1, 1)
            rects[0, 0] = min(rects[0, 0], w - 1)
        win, ncls = mi.resized_regions_plan(w, h, c, tw, th, planar, rects)
        sizes = {(int(b[2] - b[0]), int(b[3] - b[1])) for b in win}
        assert len(sizes) == 1
        wmax, hmax = rects[:, 2].max(), rects[:, 3].max()
        classes = set()
        for (x, y, rw, rh), b in zip(rects.tolist(), win.tolist()):
            assert b[0] * tw_ <= x and x + rw <= min(b[2] * tw_, w)
            assert b[1] * th_ <= y and y + rh <= min(b[3] * th_, h)
            # the window's tile count is the one of regions_plan for the largest rectangle
            assert b[2] - b[0] == min(ntx, (wmax + tw_ - 2) // tw_ + 1)
            assert b[3] - b[1] == min(nty, (hmax + th_ - 2) // th_ + 1)
            assert b[0] == min(x // tw_, ntx - (b[2] - b[0])) and b[1] == min(y // th_, nty - (b[3] - b[1]))
            # a box of the largest size that holds the rectangle fits in the window
            assert min(b[2] * tw_, w) - b[0] * tw_ >= wmax and min(b[3] * th_, h) - b[1] * th_ >= hmax
            classes.add((1 if w % tw_ and b[2] == ntx else 0) | (2 if h % th_ and b[3] == nty else 0))
        assert ncls == len(classes)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}_{s[3]}x{s[4]}" for s in SHAPES])
def test_equal_sizes_equal_regions_plan(shape):
    w, h, c, tw, th, planar = shape
    rng = np.random.default_rng(h)
    for _ in range(10):
        rw, rh = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
        n = int(rng.integers(1, 7))
        xy = [(int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1))) for _ in range(n)]
        a = mi.regions_plan(w, h, c, tw, th, planar, rw, rh, xy)
        b = mi.resized_regions_plan(w, h, c, tw, th, planar, [(x, y, rw, rh) for x, y in xy])
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def test_bad_args():
    w, h = 200, 100
    good = [(0, 0, 50, 50), (10, 10, 20, 20)]
    mi.resized_regions_plan(w, h, 3, 32, 16, True, good)
    for rects in ([(0, 0, 0, 5)], [(0, 0, 5, 0)], [(151, 0, 50, 50)], [(0, 51, 50, 50)], [(0, 0, 201, 1)], good + [(0xFFFFFFFF, 0, 2, 1)]):
        with pytest.raises(mi.LlcompError) as e:
            mi.resized_regions_plan(w, h, 3, 32, 16, True, rects)
        assert e.value.status == mi.BAD_ARGS, rects
    L = mi._lib.load()
    tab = (C.c_uint32 * 4)(0, 0, 5, 5)
    win, k = (C.c_uint32 * 4)(), C.c_uint32()
    assert L.llcomp_mi_resized_regions_plan(w, h, 3, 32, 16, 1, tab, 0, win, C.byref(k)) == mi.BAD_ARGS
    assert L.llcomp_mi_resized_regions_plan(w, h, 3, 32, 16, 1, None, 1, win, C.byref(k)) == mi.BAD_ARGS
    assert L.llcomp_mi_resized_regions_plan(w, h, 3, 32, 16, 1, tab, 1, win, None) == mi.BAD_ARGS
    # a downscale above 64x has no weights: the codec call refuses it (test_gpu_resized_regions) with the rule's BAD_ARGS
    assert L.llcomp_mi_resize_weights(200, 3, None, None) == 0
    assert L.llcomp_mi_resize_weights(192, 3, None, None) > 0
