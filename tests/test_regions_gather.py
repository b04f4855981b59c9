"""Regions gather (llcomp_mi_regions_gather): the table entries and payload bytes of every frame's window, taken from host containers,
against a NumPy restatement built from regions_plan's windows and the containers' own tables.  Containers come from the oracle.  No GPU
needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import make_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd
    from llcomp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "llcomp_amd", "csrc")])
    return llcomp_amd


def containers(orc, frames, w, h, c, tw, th, planar, small_model=False, gens=("nat", "mid", "g3", "g1")):
    orc.set_small_model(small_model)
    try:
        return [orc.compress_sliced(np.ascontiguousarray(np.roll(make_image(gens[f % len(gens)], w, h, c), 5 * f, axis=1)), tw, th, planar)
                for f in range(frames)]
    finally:
        orc.set_small_model(False)


def table(d):
    n = int.from_bytes(d[20:24], "little")
    t = np.frombuffer(d, dtype="<u4", count=n, offset=24).astype(np.int64)
    return t, 24 + 4 * n + np.concatenate([[0], np.cumsum(t)])


def restate(mi, conts, xy, rw, rh):
    """(payload, slice_len, n_classes) as the issue defines them: class by class, frame order inside a class, and inside a frame the
    window's slices by tile row, tile column, plane -- from regions_plan's windows and each container's table"""
    info = mi.probe(conts[0])
    w, h, c, tw, th, planar = info.width, info.height, info.channels, info.tile_w, info.tile_h, info.planar
    windows, n_classes = mi.regions_plan(w, h, c, tw, th, planar, rw, rh, xy)
    ntx, nty = -(-w // tw), -(-h // th)
    planes = c if planar else 1

    def cls(win):
        return (1 if w % tw and win[2] == ntx else 0) | (2 if h % th and win[3] == nty else 0)

    pays, lens, seen = [], [], set()
    for k in range(4):
        for f, win in enumerate(windows.tolist()):
            if cls(win) != k:
                continue
            seen.add(k)
            t, starts = table(conts[f])
            wx0, wy0, wx1, wy1 = win
            for ty in range(wy0, wy1):
                for tx in range(wx0, wx1):
                    for p in range(planes):
                        s = (ty * ntx + tx) * planes + p
                        lens.append(int(t[s]))
                        pays.append(bytes(conts[f][starts[s]:starts[s] + t[s]]))
    assert len(seen) == n_classes
    return b"".join(pays), np.array(lens, np.uint32), n_classes


def check(mi, conts, xy, rw, rh):
    pay, sl, k = mi.regions_gather(conts, xy, rw, rh)
    want_pay, want_sl, want_k = restate(mi, conts, xy, rw, rh)
    assert k == want_k
    assert np.array_equal(sl, want_sl)
    assert pay.tobytes() == want_pay
    return k


def edge_offsets(rng, w, h, rw, rh, frames):
    edges = [(0, 0), (w - rw, 0), (0, h - rh), (w - rw, h - rh), ((w - rw) // 2, 0), (0, (h - rh) // 2)]
    return [edges[f] if f < len(edges) else (int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1))) for f in range(frames)]


# (w, h, c, tile_w, tile_h, planar): tile multiples, a partial last column, partial both ways, one tile, one-row slices, 5 channels
SHAPES = [
    (64, 48, 3, 16, 16, False),
    (70, 48, 3, 16, 16, True),
    (70, 45, 3, 16, 8, False),
    (70, 45, 3, 16, 8, True),
    (40, 30, 3, 0, 0, True),
    (40, 30, 3, 0, 0, False),
    (50, 9, 4, 12, 1, True),
    (33, 20, 5, 8, 6, False),
    (160, 41, 3, 40, 2, True),
]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_layout_matches_restatement(mi, orc, shape):
    w, h, c, tw, th, planar = shape
    frames = 7
    conts = containers(orc, frames, w, h, c, tw, th, planar)
    rng = np.random.default_rng(w * 1000 + h * 10 + c)
    classes = set()
    for rw, rh in ((w, h), (1, 1), (max(1, w // 3), max(1, h // 2)), (w, 1), (1, h), (min(w, tw or w), min(h, th or h)),
                   (int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1)))):
        xy = edge_offsets(rng, w, h, rw, rh, frames)
        classes.add(check(mi, conts, xy, rw, rh))
    if w % (tw or w) and h % (th or h):
        assert 4 in classes, classes
    if (w % (tw or w)) or (h % (th or h)):
        assert 2 in classes, classes
    assert 1 in classes


def test_class_counts_and_small_model(mi, orc):
    w, h, c, tw, th = 70, 45, 3, 16, 8  # partial last tile column and row
    conts = containers(orc, 4, w, h, c, tw, th, False, small_model=True)
    assert mi.probe(conts[0]).small_model == 1
    for xy, want in (([(0, 0), (10, 5), (20, 10), (3, 3)], 1), ([(0, 0), (50, 0), (10, 5), (45, 3)], 2),
                     ([(0, 0), (50, 0), (0, 25), (50, 25)], 4)):
        assert check(mi, conts, xy, 20, 20) == want


def test_inputs_of_every_buffer_kind(mi, orc):
    conts = containers(orc, 3, 70, 45, 3, 16, 8, True)
    xy = [(0, 0), (50, 25), (13, 7)]
    want = mi.regions_gather(conts, xy, 20, 20)
    for kind in (bytearray, lambda d: np.frombuffer(d, np.uint8).copy(), memoryview):
        got = mi.regions_gather([kind(d) for d in conts], np.array(xy, np.uint32), 20, 20)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def _raw(mi, conts, xy, rw, rh, pay=None, pay_cap=0, sl=None, sl_cap=0):
    """llcomp_mi_regions_gather through ctypes -> (status, payload_bytes, n_slices, n_classes)"""
    from llcomp_amd import _lib

    L = _lib.load()
    ptrs, lens, keep = mi._containers(conts)
    tab = (C.c_uint32 * (2 * len(xy)))(*[v for p in xy for v in p]) if xy is not None else None
    nb, ns, nc = C.c_uint64(77), C.c_uint32(77), C.c_uint32(77)
    rc = L.llcomp_mi_regions_gather(ptrs, lens, len(keep), tab, rw, rh, None if pay is None else pay.ctypes.data, pay_cap,
                                    None if sl is None else sl.ctypes.data, sl_cap, C.byref(nb), C.byref(ns), C.byref(nc))
    return rc, nb.value, ns.value, nc.value


def test_size_query_and_overflow_write_nothing(mi, orc):
    conts = containers(orc, 4, 70, 45, 3, 16, 8, False)
    xy = [(0, 0), (50, 0), (0, 25), (50, 25)]
    want_pay, want_sl, want_k = restate(mi, conts, xy, 20, 20)
    nb, ns = len(want_pay), len(want_sl)
    assert _raw(mi, conts, xy, 20, 20) == (mi.OK, nb, ns, want_k)
    pay, sl = np.full(nb + 64, 0xAB, np.uint8), np.full(ns + 16, 0xABABABAB, np.uint32)
    assert _raw(mi, conts, xy, 20, 20, sl=sl, sl_cap=ns) == (mi.OK, nb, ns, want_k)            # (payload == NULL: a query)
    assert _raw(mi, conts, xy, 20, 20, pay=pay, pay_cap=nb) == (mi.OK, nb, ns, want_k)          # (slice_len == NULL: a query)
    assert (pay == 0xAB).all() and (sl == 0xABABABAB).all()
    for pay_cap, sl_cap in ((nb - 1, ns), (nb, ns - 1), (0, 0)):
        assert _raw(mi, conts, xy, 20, 20, pay, pay_cap, sl, sl_cap) == (mi.OUTPUT_OVERFLOW, nb, ns, want_k)
        assert (pay == 0xAB).all() and (sl == 0xABABABAB).all(), "an overflowing call wrote"
    assert _raw(mi, conts, xy, 20, 20, pay, nb, sl, ns) == (mi.OK, nb, ns, want_k)
    assert pay[:nb].tobytes() == want_pay and np.array_equal(sl[:ns], want_sl)
    assert (pay[nb:] == 0xAB).all() and (sl[ns:] == 0xABABABAB).all()
    # a failing call reports zero sizes
    assert _raw(mi, conts, xy, 200, 20) == (mi.BAD_ARGS, 0, 0, 0)
    assert _raw(mi, conts, None, 20, 20)[0] == mi.BAD_ARGS


def _status(mi, conts, xy, rw, rh):
    try:
        mi.regions_gather(conts, xy, rw, rh)
    except mi.LlcompError as e:
        return e.status
    return mi.OK


def test_truncation_inside_and_outside_the_windows(mi, orc):
    w, h, c, tw, th = 64, 48, 3, 16, 16  # 4 x 3 tiles, interleaved: slice id = tile row * 4 + tile column
    conts = containers(orc, 2, w, h, c, tw, th, False)
    xy = [(0, 0), (20, 0)]  # 16 x 16 rectangles: windows of 2 x 2 tiles -- frame 0 tiles 0, 1, 4, 5; frame 1 tiles 1, 2, 5, 6
    assert mi.regions_plan(w, h, c, tw, th, False, 16, 16, xy)[0].tolist() == [[0, 0, 2, 2], [1, 0, 3, 2]]
    t, starts = table(conts[1])
    # cut inside frame 1's last window slice (6): TRUNCATED
    cut = conts[1][:int(starts[6] + t[6] - 1)]
    assert _status(mi, [conts[0], cut], xy, 16, 16) == mi.TRUNCATED
    # cut right behind it (slices 7..11 are outside every window): OK, and the bytes are the same
    cut = conts[1][:int(starts[7])]
    assert check(mi, [conts[0], cut], xy, 16, 16) == 1
    pay, sl, _ = mi.regions_gather([conts[0], cut], xy, 16, 16)
    want = mi.regions_gather(conts, xy, 16, 16)
    assert np.array_equal(pay, want[0]) and np.array_equal(sl, want[1])
    # a header or table cut short fails as in probe
    assert _status(mi, [conts[0], conts[1][:10]], xy, 16, 16) == mi.TRUNCATED
    assert _status(mi, [conts[0], conts[1][:24 + 4 * 5]], xy, 16, 16) == mi.TRUNCATED


def test_entry_above_the_sliced_limit(mi, orc):
    import orc as orc_mod

    w, h, c, tw, th = 64, 48, 3, 16, 16
    conts = containers(orc, 2, w, h, c, tw, th, False)
    xy = [(0, 0), (20, 0)]
    limit = (13 * tw * th * c + 16 + 15) & ~15
    t, starts = table(conts[1])
    pays = [conts[1][starts[s]:starts[s + 1]] for s in range(len(t))]

    def with_entry(s, n):
        p = list(pays)
        p[s] = p[s] + bytes(n - len(p[s]))  # (the bytes are there: only the entry is at issue)
        return orc_mod.sliced_container(w, h, c, tw, th, False, p)

    assert _status(mi, [conts[0], with_entry(5, limit + 1)], xy, 16, 16) == mi.TRUNCATED   # inside frame 1's window
    assert _status(mi, [conts[0], with_entry(5, limit)], xy, 16, 16) == mi.OK              # at the limit
    assert _status(mi, [conts[0], with_entry(11, limit + 1)], xy, 16, 16) == mi.OK         # outside every window
    assert _status(mi, [conts[0], with_entry(0, limit + 1)], xy, 16, 16) == mi.OK          # in frame 0's window, not frame 1's
    # the staged bytes never exceed the window slices x the slice capacity
    pay, sl, _ = mi.regions_gather([conts[0], with_entry(5, limit)], xy, 16, 16)
    assert pay.size <= sl.size * (limit + 16)


def test_bad_arguments(mi, orc):
    w, h, c, tw, th = 64, 48, 3, 16, 16
    conts = containers(orc, 2, w, h, c, tw, th, True)
    xy = [(0, 0), (20, 10)]
    assert _status(mi, conts, xy, 20, 20) == mi.OK
    img = make_image("nat", w, h, c)
    legacy = orc.compress_image(img)
    others = [orc.compress_sliced(img, 32, 16, True), orc.compress_sliced(img, 16, 16, False), containers(orc, 1, 64, 40, 3, 16, 16, True)[0],
              containers(orc, 1, w, h, 4, 16, 16, True)[0], containers(orc, 1, w, h, c, 16, 16, True, small_model=True)[0]]
    assert _status(mi, [conts[0], legacy], xy, 20, 20) == mi.BAD_ARGS
    assert _status(mi, [legacy, conts[0]], xy, 20, 20) == mi.BAD_ARGS
    for o in others:
        assert _status(mi, [conts[0], o], xy, 20, 20) == mi.BAD_ARGS
    for xy_, rw, rh in (([(0, 0), (45, 0)], 20, 20), ([(0, 0), (0, 29)], 20, 20), (xy, 0, 20), (xy, 20, 0), (xy, 65, 1),
                        ([(10, 0), (0, 0)], 2**32 - 5, 1)):
        assert _status(mi, conts, xy_, rw, rh) == mi.BAD_ARGS, (xy_, rw, rh)
    from llcomp_amd import _lib

    nb, ns, nc = C.c_uint64(), C.c_uint32(), C.c_uint32()
    tab = (C.c_uint32 * 2)(0, 0)
    assert _lib.load().llcomp_mi_regions_gather(None, None, 0, tab, 1, 1, None, 0, None, 0, C.byref(nb), C.byref(ns), C.byref(nc)) == mi.BAD_ARGS
    ptrs, lens, _keep = mi._containers(conts)
    assert _lib.load().llcomp_mi_regions_gather(ptrs, lens, 0, tab, 1, 1, None, 0, None, 0, C.byref(nb), C.byref(ns), C.byref(nc)) == mi.BAD_ARGS
    assert _lib.load().llcomp_mi_regions_gather(ptrs, lens, 1, tab, 1, 1, None, 0, None, 0, None, C.byref(ns), C.byref(nc)) == mi.BAD_ARGS
