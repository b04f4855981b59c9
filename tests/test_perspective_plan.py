"""The host planner of the perspective views (llcomp_mi_perspective_source_rect, llcomp_mi_perspective_views_plan;
llcomp_amd/csrc/warp_plan.cpp): a view's source rectangle is a BOUND -- it contains the brute-force box of every pixel the rule reads,
exceeds it by no more than 1 + ceil(s) a side (s: the largest step of a source coordinate between neighbouring output pixels), and is
empty exactly when the brute force is; the plan is llcomp_mi_views_plan on those rectangles; and every refusal of the header.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest
from perspective_cases import FILTERS, coords, keystone


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


def taps(w, h, a, name, ow, oh):
    """((x0, y0, x1, y1) inclusive, s): the bounding box of every pixel the rule reads for a view, by brute force over all output pixels
    from the rule's own coordinates (perspective_cases.coords), or None when no output pixel is inside; s = the largest |step| of xin
    or yin between horizontally or vertically adjacent output pixels"""
    _, xin, yin = coords(a, ow, oh)
    steps = [np.abs(np.diff(t, axis=ax)) for t in (xin, yin) for ax in (0, 1)]
    s = max([float(d.max()) for d in steps if d.size] + [0.0])
    ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    if not ok.any():
        return None, s
    if name == "nearest":
        xi, yi = np.trunc(xin[ok]).astype(np.int64), np.trunc(yin[ok]).astype(np.int64)
        return (xi.min(), yi.min(), xi.max(), yi.max()), s
    X, Y = np.floor(xin[ok] - 0.5).astype(np.int64), np.floor(yin[ok] - 0.5).astype(np.int64)
    lo, hi = (-1, 2) if name == "bicubic" else (0, 1)
    cols = np.clip(np.stack([X + d for d in range(lo, hi + 1)]), 0, w - 1)
    rows = [np.clip(Y + lo, 0, h - 1)] + [(Y + d)[(Y + d >= 0) & (Y + d < h)] for d in range(lo + 1, hi + 1)]  # rows past the edge are not read
    rows = np.concatenate(rows)
    return (cols.min(), rows.min(), cols.max(), rows.max()), s


def random_views(mi, seed, n):
    """images up to 64 x 64, outputs up to 40 x 40: keystones inside the image, partly outside (the corners moved by up to 0.4 of a
    side, every third one shifted by up to a side) and, every seventh, wholly outside"""
    rng = np.random.default_rng(seed)
    for i in range(n):
        w, h = int(rng.integers(1, 65)), int(rng.integers(1, 65))
        ow, oh = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        shift = rng.uniform(-1, 1, 2) if i % 3 == 0 else (0.0, 0.0)
        if i % 7 == 0:
            shift = (3.0, -2.5)
        a = keystone(mi, rng, w, h, ow, oh, spread=(0.1, 0.25, 0.4)[i % 3], shift=shift)
        if i % 5 == 0:  # the source quadrilateral well inside the image: every pixel inside
            sp = np.array([[0.3, 0.3], [0.7, 0.25], [0.75, 0.7], [0.2, 0.8]]) * [w, h]
            a = mi.perspective_coeffs(sp, [[0, 0], [ow, 0], [ow, oh], [0, oh]])
        yield w, h, a, ow, oh


def test_source_rect_bounds_the_taps(mi):
    empties = full = seen = 0
    for w, h, a, ow, oh in random_views(mi, 23, 400):
        den, _, _ = coords(a, ow, oh)
        if not (den > 0).all():
            continue
        for name in FILTERS:
            box, s = taps(w, h, a, name, ow, oh)
            (x, y, rw, rh), empty = mi.perspective_source_rect(w, h, a, name, ow, oh)
            seen += 1
            assert empty == (box is None), (w, h, a, name, ow, oh)  # empty exactly when no output pixel is inside
            if box is None:
                assert (x, y, rw, rh) == (0, 0, 0, 0)
                empties += 1
                continue
            full += (x, y, rw, rh) == (0, 0, w, h)
            assert rw >= 1 and rh >= 1 and x + rw <= w and y + rh <= h
            got = (x, y, x + rw - 1, y + rh - 1)
            assert got[0] <= box[0] and got[1] <= box[1] and got[2] >= box[2] and got[3] >= box[3], (w, h, a, name, ow, oh, box, got)
            slack = 1 + math.ceil(s)
            assert max(box[0] - got[0], box[1] - got[1], got[2] - box[2], got[3] - box[3]) <= slack, (w, h, a, name, ow, oh, box, got, s)
    assert seen > 1000 and 100 < empties < seen / 2 and full < seen / 2  # all three kinds were seen, and the bound is not "the whole image"


def test_rows_along_the_image_edge(mi):
    """maps whose rows or columns run exactly along the image's edge, where the planner's margins decide nothing: integer translates
    of -1 .. 1 pixels, and the constant map"""
    for w, h, ow, oh in ((9, 7, 9, 7), (5, 5, 8, 3), (1, 1, 4, 4)):
        for tx in (-1.0, -0.5, 0.0, 0.5, 1.0):
            for ty in (-1.0, -0.5, 0.0, 0.5, float(h) - 0.5, float(h)):
                for a in ([1, 0, tx, 0, 1, ty, 0, 0], [0, 0, tx, 0, 0, ty, 0, 0], [1, 0, tx, 0, 0, ty, 0, 0.125]):
                    for name in FILTERS:
                        box, _ = taps(w, h, a, name, ow, oh)
                        (x, y, rw, rh), empty = mi.perspective_source_rect(w, h, a, name, ow, oh)
                        assert empty == (box is None), (w, h, a, name)
                        if box is not None:
                            assert x <= box[0] and y <= box[1] and x + rw - 1 >= box[2] and y + rh - 1 >= box[3], (w, h, a, name, box, (x, y, rw, rh))


def groups_of(mi, seed, frames, w, h, skip=()):
    """two groups of random views of a w x h batch; frames in `skip` get none, frame 1 only views that read nothing"""
    rng = np.random.default_rng(seed)
    out = []
    for ow, oh, n in ((20, 14, 7), (9, 9, 5)):
        views = []
        for j in range(n):
            f = int(rng.integers(0, frames))
            while f in skip:
                f = (f + 1) % frames
            a = keystone(mi, rng, w / 2, h / 2, ow, oh, shift=(5.0, 5.0) if f == 1 else rng.uniform(0, 1, 2))
            views.append((f, *a, (mi.filter_code(FILTERS[j % 3]) << 4) | (j & 1)))
        out.append((views, ow, oh))
    return out


@pytest.mark.parametrize("geo", [(100, 70, 3, 32, 32, True), (64, 48, 1, 16, 16, False), (300, 40, 4, 40, 1, True)], ids=lambda g: "x".join(map(str, g[:5])))
def test_plan_is_views_plan_on_the_source_rectangles(mi, geo):
    w, h, c, tw, th, planar = geo
    frames = 6
    for seed in range(5):
        groups = groups_of(mi, seed, frames, w, h, skip=(4,))
        uni, win, n_used, n_cls = mi.perspective_views_plan(w, h, c, tw, th, planar, frames, groups)
        rect_groups = []
        for views, ow, oh in groups:
            for v in views:
                (x, y, rw, rh), empty = mi.perspective_source_rect(w, h, v[1:9], (v[9] >> 4) & 7, ow, oh)
                assert empty == (v[0] == 1)
                if not empty:
                    rect_groups.append(([(v[0], x, y, rw, rh, mi.FILTER_NEAREST << 4)], rw, rh))
        uni2, win2, n_used2, n_cls2 = mi.views_plan(w, h, c, tw, th, planar, frames, rect_groups)
        assert np.array_equal(uni, uni2) and np.array_equal(win, win2) and (n_used, n_cls) == (n_used2, n_cls2)
        assert not uni[4].any() and not win[4].any() and not uni[1].any() and not win[1].any()
        assert n_used == len({v[0] for g in groups for v in g[0]} - {1})
    # every view empty: nothing is decoded, and that is no error
    far = [([(0, 1.0, 0.0, 10.0 * w, 0.0, 1.0, 0.0, 0.001, 0.0), (2, 1.0, 0.2, 0.0, 0.0, 1.0, -3.0 * h - 40, 0.0, 0.002, 1 << 4)], 8, 8)]
    uni, win, n_used, n_cls = mi.perspective_views_plan(w, h, c, tw, th, planar, frames, far)
    assert not uni.any() and not win.any() and (n_used, n_cls) == (0, 0)


BIG = 2.0 ** 30
BAD_VIEWS = {  # (a, filter code, ow, oh): every limit of the header
    "nan": ([1, 0, float("nan"), 0, 1, 0, 0, 0], 0, 8, 8),
    "inf": ([float("inf"), 0, 0, 0, 1, 0, 0, 0], 4, 8, 8),
    "-inf a7 nearest": ([1, 0, 0, 0, 1, 0, 0, float("-inf")], 1, 8, 8),
    "nan a6": ([1, 0, 0, 0, 1, 0, float("nan"), 0], 1, 8, 8),
    "den 0 at (ow - 1, 0)": ([1, 0, 0, 0, 1, 0, -0.125, -0.125], 0, 8, 1),
    "den < 0 at (0, oh - 1)": ([1, 0, 0, 0, 1, 0, 0.01, -0.2], 4, 8, 8),
    "den < 0 at (0, 0)": ([1, 0, 0, 0, 1, 0, -1.5, -1.5], 1, 8, 8),
    "den < 0 at the last corner": ([1, 0, 0, 0, 1, 0, -0.07, -0.07], 1, 8, 8),
    "|xin| = 2^30": ([1, 0, BIG, 0, 1, 0, 0, 0], 0, 8, 8),
    "nearest |xin| beyond 2^30": ([1, 0, -BIG - 8, 0, 1, 0, 0, 0], 1, 8, 8),
    "|yin| at the last corner": ([1, 0, 0, BIG / 8, BIG / 8, 0, 0, 0], 4, 8, 8),
    "|yin| through a small den": ([1, 0, 0, 0, 1, 0, 0, -(1 - 2.0 ** -40) / 7.5], 0, 8, 8),
    "box": ([1, 0, 0, 0, 1, 0, 0, 0], 2, 8, 8),
    "hamming": ([1, 0, 0, 0, 1, 0, 0, 0], 3, 8, 8),
    "lanczos": ([1, 0, 0, 0, 1, 0, 0, 0], 5, 8, 8),
    "filter 6": ([1, 0, 0, 0, 1, 0, 0, 0], 6, 8, 8),
    "ow 0": ([1, 0, 0, 0, 1, 0, 0, 0], 0, 0, 8),
    "oh 0": ([1, 0, 0, 0, 1, 0, 0, 0], 1, 8, 0),
}


@pytest.mark.parametrize("name", list(BAD_VIEWS))
def test_bad_args_leave_the_outputs_untouched(mi, name):
    from llcomp_amd import _lib

    L = _lib.load()
    a, filt, ow, oh = BAD_VIEWS[name]
    coef = (C.c_double * 8)(*a)
    rect, empty = (C.c_uint32 * 4)(7, 7, 7, 7), C.c_uint32(7)
    assert L.llcomp_mi_perspective_source_rect(20, 10, coef, filt, ow, oh, rect, C.byref(empty)) == mi.BAD_ARGS
    assert list(rect) == [7, 7, 7, 7] and empty.value == 7
    src, out = np.zeros((10, 20, 3), np.uint8), np.full((max(oh, 1), max(ow, 1), 3), 0x5A, np.uint8)
    assert L.llcomp_mi_perspective_reference(src.ctypes.data, 20, 10, 3, coef, filt, None, ow, oh, out.ctypes.data) == mi.BAD_ARGS
    assert (out == 0x5A).all()
    # ... as one view among good ones of a plan
    ident = (C.c_double * 8)(1, 0, 0, 0, 1, 0, 0, 0)
    views = (_lib.PerspectiveView * 2)(_lib.PerspectiveView(0, 0, ident), _lib.PerspectiveView(1, filt << 4, coef))
    grp = (_lib.PerspectiveGroup * 1)(_lib.PerspectiveGroup(C.sizeof(_lib.PerspectiveGroup), 2, views, ow, oh, None, None, None))
    uni, win, used, cls = (C.c_uint32 * 8)(*[9] * 8), (C.c_uint32 * 8)(*[9] * 8), C.c_uint32(9), C.c_uint32(9)
    assert L.llcomp_mi_perspective_views_plan(20, 10, 3, 8, 8, 0, 2, grp, 1, uni, win, C.byref(used), C.byref(cls)) == mi.BAD_ARGS
    assert list(uni) == [9] * 8 and list(win) == [9] * 8 and used.value == cls.value == 9


def test_the_limits_themselves_pass(mi):
    assert mi.perspective_source_rect(20, 10, [1, 0, math.nextafter(BIG, 0.0) - 8, 0, 1, 0, 0, 0], "bilinear", 8, 8) == ((0, 0, 0, 0), True)
    assert mi.perspective_source_rect(20, 10, [1, 0, 0, 0, 1, 0, 0, 0], "bicubic", 20, 10) == ((0, 0, 20, 10), False)
    # a denominator that all but vanishes at the last corner (2^-26 there): still a map, planned pixel by pixel
    a = [1, 0, 0, 0, 1, 0, 0, -(1 - 2.0 ** -26) / 7.5]
    box, _ = taps(20, 10, a, "nearest", 8, 8)
    (x, y, rw, rh), empty = mi.perspective_source_rect(20, 10, a, "nearest", 8, 8)
    assert not empty and x <= box[0] and y <= box[1] and x + rw - 1 >= box[2] and y + rh - 1 >= box[3]


def test_bad_groups_leave_the_outputs_untouched(mi):
    from llcomp_amd import _lib

    L = _lib.load()
    ident = (C.c_double * 8)(1, 0, 0, 0, 1, 0, 0, 0)
    one = (_lib.PerspectiveView * 1)(_lib.PerspectiveView(0, 0, ident))
    late = (_lib.PerspectiveView * 1)(_lib.PerspectiveView(2, 0, ident))
    G = _lib.PerspectiveGroup
    size = C.sizeof(G)
    assert size == 48 and C.sizeof(_lib.PerspectiveView) == 72
    cases = {
        "no groups": ((G * 1)(G(size, 1, one, 8, 8, None, None, None)), 0),
        "struct_size": ((G * 1)(G(size - 8, 1, one, 8, 8, None, None, None)), 1),
        "struct_size above": ((G * 1)(G(size + 8, 1, one, 8, 8, None, None, None)), 1),
        "no views": ((G * 1)(G(size, 0, one, 8, 8, None, None, None)), 1),
        "65536 views": ((G * 1)(G(size, 65536, one, 8, 8, None, None, None)), 1),
        "NULL views": ((G * 1)(G(size, 1, None, 8, 8, None, None, None)), 1),
        "frame >= frames": ((G * 2)(G(size, 1, one, 8, 8, None, None, None), G(size, 1, late, 8, 8, None, None, None)), 2),
    }
    for name, (grp, n) in cases.items():
        uni, win, used, cls = (C.c_uint32 * 8)(*[9] * 8), (C.c_uint32 * 8)(*[9] * 8), C.c_uint32(9), C.c_uint32(9)
        assert L.llcomp_mi_perspective_views_plan(20, 10, 3, 8, 8, 0, 2, grp, n, uni, win, C.byref(used), C.byref(cls)) == mi.BAD_ARGS, name
        assert list(uni) == [9] * 8 and list(win) == [9] * 8 and used.value == cls.value == 9, name
    grp = cases["no groups"][0]
    assert L.llcomp_mi_perspective_views_plan(20, 10, 3, 8, 8, 0, 2, None, 1, None, None, C.byref(used), C.byref(cls)) == mi.BAD_ARGS
    assert L.llcomp_mi_perspective_views_plan(20, 10, 3, 8, 8, 0, 2, grp, 1, None, None, None, C.byref(cls)) == mi.BAD_ARGS
    assert L.llcomp_mi_perspective_views_plan(20, 10, 3, 8, 8, 0, 2, grp, 1, None, None, C.byref(used), C.byref(cls)) == mi.OK
    assert (used.value, cls.value) == (1, 1)
