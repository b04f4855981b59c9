"""The host planner of the warped views (llcomp_mi_warp_source_rect, llcomp_mi_warp_views_plan; llcomp_amd/csrc/warp_plan.cpp): a view's
source rectangle against a brute-force numpy statement of which pixels the rule reads, the plan against llcomp_mi_views_plan on the
source rectangles, and every refusal of the header.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

FILTERS = ("nearest", "bilinear", "bicubic")


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


def taps(w, h, m, name, ow, oh):
    """(x0, y0, x1, y1) inclusive: the bounding box of every pixel the rule reads for a view, by brute force over all output pixels in
    numpy's binary64 (one rounding per operation); None when no output pixel is inside"""
    x, y = np.meshgrid(np.arange(ow), np.arange(oh))
    m = [np.float64(v) for v in m]
    if name == "nearest":
        if m[1] == 0 and m[3] == 0:
            def table(scale, off, n_out, n_in):
                o, t = off + scale * np.float64(0.5), []
                for _ in range(n_out):
                    t.append(-1 if o < 0 or o >= n_in else int(o))
                    o = o + scale
                return np.array(t)
            xi, yi = table(m[0], m[2], ow, w)[x], table(m[4], m[5], oh, h)[y]
        else:
            fix = lambda t: int(math.floor(t * 65536.0 + 0.5))
            A = [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]
            wrap = lambda v: ((v + 2 ** 31) % 2 ** 32 - 2 ** 31) >> 16
            xi, yi = wrap(A[2] + x.astype(object) * A[0] + y.astype(object) * A[1]), wrap(A[5] + x.astype(object) * A[3] + y.astype(object) * A[4])
            xi, yi = xi.astype(np.int64), yi.astype(np.int64)
        ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
        return (xi[ok].min(), yi[ok].min(), xi[ok].max(), yi[ok].max()) if ok.any() else None
    xs, ys = x + np.float64(0.5), y + np.float64(0.5)
    xin, yin = (m[0] * xs + m[1] * ys) + m[2], (m[3] * xs + m[4] * ys) + m[5]
    ok = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    if not ok.any():
        return None
    X, Y = np.floor(xin[ok] - 0.5).astype(np.int64), np.floor(yin[ok] - 0.5).astype(np.int64)
    lo, hi = (-1, 2) if name == "bicubic" else (0, 1)
    cols = np.clip(np.stack([X + d for d in range(lo, hi + 1)]), 0, w - 1)
    rows = [np.clip(Y + lo, 0, h - 1)] + [(Y + d)[(Y + d >= 0) & (Y + d < h)] for d in range(lo + 1, hi + 1)]  # rows past the edge are not read
    rows = np.concatenate(rows)
    return cols.min(), rows.min(), cols.max(), rows.max()


def random_views(seed, n):
    rng = np.random.default_rng(seed)
    for i in range(n):
        w, h = int(rng.integers(1, 65)), int(rng.integers(1, 49))
        ow, oh = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        ang, sx, sy, sh = rng.uniform(0, 2 * math.pi), rng.uniform(0.3, 3.0), rng.uniform(0.3, 3.0), rng.uniform(-0.8, 0.8)
        m = [sx * math.cos(ang), sx * (math.sin(ang) + sh), rng.uniform(-w, 1.5 * w), -sy * math.sin(ang), sy * math.cos(ang), rng.uniform(-h, 1.5 * h)]
        if i % 4 == 0:
            m[0], m[1], m[3], m[4] = sx * (1 if i % 8 else -1), 0.0, 0.0, sy * (1 if i % 3 else -1)
        if i % 9 == 0:
            m = [1.0, 0.0, float(rng.integers(-w, w + 1)), 0.0, 1.0, float(rng.integers(-h, h + 1))]
        if i % 11 == 0:  # far away: nothing inside
            m[2] += 5 * w + 50
        yield w, h, m, ow, oh


def test_source_rect_is_the_bounding_box_of_the_taps(mi):
    empties = 0
    for w, h, m, ow, oh in random_views(11, 400):
        for name in FILTERS:
            box = taps(w, h, m, name, ow, oh)
            (x, y, rw, rh), empty = mi.warp_source_rect(w, h, m, name, ow, oh)
            assert empty == (box is None), (w, h, m, name, ow, oh)  # empty exactly when no output pixel is inside
            if box is None:
                assert (x, y, rw, rh) == (0, 0, 0, 0)
                empties += 1
                continue
            assert rw >= 1 and rh >= 1 and x + rw <= w and y + rh <= h
            # it contains every tap, and exceeds their bounding box by at most 2 pixels a side
            assert x <= box[0] and y <= box[1] and x + rw - 1 >= box[2] and y + rh - 1 >= box[3], (w, h, m, name, ow, oh, box, (x, y, rw, rh))
            assert box[0] - x <= 2 and box[1] - y <= 2 and x + rw - 1 - box[2] <= 2 and y + rh - 1 - box[3] <= 2, (w, h, m, name, ow, oh, box, (x, y, rw, rh))
    assert 100 < empties < 900  # both kinds were seen


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
            ang, s = rng.uniform(0, 2 * math.pi), rng.uniform(0.5, 1.5)
            m = [s * math.cos(ang), s * math.sin(ang), rng.uniform(0, w / 2), -s * math.sin(ang), s * math.cos(ang), rng.uniform(0, h / 2)]
            if f == 1:
                m[2] = 10.0 * w
            views.append((f, *m, (mi.filter_code(FILTERS[j % 3]) << 4) | (j & 1)))
        out.append((views, ow, oh))
    return out


@pytest.mark.parametrize("geo", [(100, 70, 3, 32, 32, True), (64, 48, 1, 16, 16, False), (300, 40, 4, 40, 1, True)], ids=lambda g: "x".join(map(str, g[:5])))
def test_plan_is_views_plan_on_the_source_rectangles(mi, geo):
    w, h, c, tw, th, planar = geo
    frames = 6
    for seed in range(5):
        groups = groups_of(mi, seed, frames, w, h, skip=(4,))
        uni, win, n_used, n_cls = mi.warp_views_plan(w, h, c, tw, th, planar, frames, groups)
        rect_groups = []
        for views, ow, oh in groups:
            for v in views:
                (x, y, rw, rh), empty = mi.warp_source_rect(w, h, v[1:7], (v[7] >> 4) & 7, ow, oh)
                assert empty == (v[0] == 1)
                if not empty:
                    rect_groups.append(([(v[0], x, y, rw, rh, mi.FILTER_NEAREST << 4)], rw, rh))
        uni2, win2, n_used2, n_cls2 = mi.views_plan(w, h, c, tw, th, planar, frames, rect_groups)
        assert np.array_equal(uni, uni2) and np.array_equal(win, win2) and (n_used, n_cls) == (n_used2, n_cls2)
        # the unused frame, and the frame whose views are all empty, have zero rows
        assert not uni[4].any() and not win[4].any() and not uni[1].any() and not win[1].any()
        assert n_used == len({v[0] for g in groups for v in g[0]} - {1})
    # every view empty: nothing is decoded, and that is no error
    far = [([(0, 1.0, 0.0, 10.0 * w, 0.0, 1.0, 0.0), (2, 1.0, 0.2, 0.0, 0.0, 1.0, -3.0 * h - 40, 1 << 4)], 8, 8)]
    uni, win, n_used, n_cls = mi.warp_views_plan(w, h, c, tw, th, planar, frames, far)
    assert not uni.any() and not win.any() and (n_used, n_cls) == (0, 0)


BIG = 2.0 ** 30
BAD_VIEWS = {  # (m, filter code, ow, oh): every limit of the header
    "nan": ([1, 0, float("nan"), 0, 1, 0], 0, 8, 8),
    "inf": ([float("inf"), 0, 0, 0, 1, 0], 4, 8, 8),
    "-inf nearest": ([1, 0, 0, 0, 1, float("-inf")], 1, 8, 8),
    "nearest |m2| = 32768": ([1, 0.5, 32768.0, 0, 1, 0], 1, 8, 8),
    "nearest x at (ow, 0)": ([4096.0, 0.5, 0, 0, 1, 0], 1, 8, 8),
    "nearest y at (0, oh)": ([1, 0.5, 0, 0, -4096.0, 0], 1, 8, 8),
    "nearest y at (ow, oh)": ([1, 0.5, 0, 2048.0, 2048.0, 0], 1, 8, 8),
    "nearest pure scale beyond the limit": ([1, 0, -40000.0, 0, 1, 0], 1, 8, 8),
    "bilinear |xin| = 2^30": ([1, 0, BIG, 0, 1, 0], 0, 8, 8),
    "bicubic |yin| at the last corner": ([1, 0, 0, BIG / 8, BIG / 8, 0], 4, 8, 8),
    "box": ([1, 0, 0, 0, 1, 0], 2, 8, 8),
    "hamming": ([1, 0, 0, 0, 1, 0], 3, 8, 8),
    "lanczos": ([1, 0, 0, 0, 1, 0], 5, 8, 8),
    "filter 6": ([1, 0, 0, 0, 1, 0], 6, 8, 8),
    "ow 0": ([1, 0, 0, 0, 1, 0], 0, 0, 8),
    "oh 0": ([1, 0, 0, 0, 1, 0], 1, 8, 0),
}


@pytest.mark.parametrize("name", list(BAD_VIEWS))
def test_bad_args_leave_the_outputs_untouched(mi, name):
    from llcomp_amd import _lib

    L = _lib.load()
    m, filt, ow, oh = BAD_VIEWS[name]
    mat = (C.c_double * 6)(*m)
    rect, empty = (C.c_uint32 * 4)(7, 7, 7, 7), C.c_uint32(7)
    assert L.llcomp_mi_warp_source_rect(20, 10, mat, filt, ow, oh, rect, C.byref(empty)) == mi.BAD_ARGS
    assert list(rect) == [7, 7, 7, 7] and empty.value == 7
    src, out = np.zeros((10, 20, 3), np.uint8), np.full((max(oh, 1), max(ow, 1), 3), 0x5A, np.uint8)
    assert L.llcomp_mi_warp_reference(src.ctypes.data, 20, 10, 3, mat, filt, None, ow, oh, out.ctypes.data) == mi.BAD_ARGS
    assert (out == 0x5A).all()
    # ... as one view among good ones of a plan
    good = (0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0)
    views = (_lib.WarpView * 2)(_lib.WarpView(*good[:1], good[7], (C.c_double * 6)(*good[1:7])), _lib.WarpView(1, filt << 4, mat))
    grp = (_lib.WarpGroup * 1)(_lib.WarpGroup(C.sizeof(_lib.WarpGroup), 2, views, ow, oh, None, None, None))
    uni, win, used, cls = (C.c_uint32 * 8)(*[9] * 8), (C.c_uint32 * 8)(*[9] * 8), C.c_uint32(9), C.c_uint32(9)
    assert L.llcomp_mi_warp_views_plan(20, 10, 3, 8, 8, 0, 2, grp, 1, uni, win, C.byref(used), C.byref(cls)) == mi.BAD_ARGS
    assert list(uni) == [9] * 8 and list(win) == [9] * 8 and used.value == cls.value == 9


def test_the_limits_themselves_pass(mi):
    just = math.nextafter(32768.0, 0.0)
    assert mi.warp_source_rect(20, 10, [1, 0.5, just - 12, 0, 1, 0], "nearest", 8, 8) == ((0, 0, 0, 0), True)
    assert mi.warp_source_rect(20, 10, [1, 0, math.nextafter(BIG, 0.0) - 8, 0, 1, 0], "bilinear", 8, 8) == ((0, 0, 0, 0), True)
    assert mi.warp_source_rect(20, 10, [1, 0, 0, 0, 1, 0], "bicubic", 20, 10) == ((0, 0, 20, 10), False)


def test_bad_groups_leave_the_outputs_untouched(mi):
    from llcomp_amd import _lib

    L = _lib.load()
    ident = (C.c_double * 6)(1, 0, 0, 0, 1, 0)
    one = (_lib.WarpView * 1)(_lib.WarpView(0, 0, ident))
    late = (_lib.WarpView * 1)(_lib.WarpView(2, 0, ident))
    size = C.sizeof(_lib.WarpGroup)
    assert size == 48 and C.sizeof(_lib.WarpView) == 56
    cases = {
        "no groups": ((_lib.WarpGroup * 1)(_lib.WarpGroup(size, 1, one, 8, 8, None, None, None)), 0),
        "struct_size": ((_lib.WarpGroup * 1)(_lib.WarpGroup(size - 8, 1, one, 8, 8, None, None, None)), 1),
        "no views": ((_lib.WarpGroup * 1)(_lib.WarpGroup(size, 0, one, 8, 8, None, None, None)), 1),
        "65536 views": ((_lib.WarpGroup * 1)(_lib.WarpGroup(size, 65536, one, 8, 8, None, None, None)), 1),
        "NULL views": ((_lib.WarpGroup * 1)(_lib.WarpGroup(size, 1, None, 8, 8, None, None, None)), 1),
        "frame >= frames": ((_lib.WarpGroup * 2)(_lib.WarpGroup(size, 1, one, 8, 8, None, None, None), _lib.WarpGroup(size, 1, late, 8, 8, None, None, None)), 2),
    }
    for name, (grp, n) in cases.items():
        uni, win, used, cls = (C.c_uint32 * 8)(*[9] * 8), (C.c_uint32 * 8)(*[9] * 8), C.c_uint32(9), C.c_uint32(9)
        assert L.llcomp_mi_warp_views_plan(20, 10, 3, 8, 8, 0, 2, grp, n, uni, win, C.byref(used), C.byref(cls)) == mi.BAD_ARGS, name
        assert list(uni) == [9] * 8 and list(win) == [9] * 8 and used.value == cls.value == 9, name
    grp = cases["no groups"][0]
    assert L.llcomp_mi_warp_views_plan(20, 10, 3, 8, 8, 0, 2, None, 1, None, None, C.byref(used), C.byref(cls)) == mi.BAD_ARGS
    assert L.llcomp_mi_warp_views_plan(20, 10, 3, 8, 8, 0, 2, grp, 1, None, None, None, C.byref(cls)) == mi.BAD_ARGS
    assert L.llcomp_mi_warp_views_plan(20, 10, 3, 8, 8, 0, 2, grp, 1, None, None, C.byref(used), C.byref(cls)) == mi.OK
    assert (used.value, cls.value) == (1, 1)
