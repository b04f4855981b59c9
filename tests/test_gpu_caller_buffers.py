"""Every device entry point on caller buffers that sit at ANY byte address, with nothing but the call's own bytes around them.

Every other GPU test hands the codec pointers that come straight from the allocator: 256-byte aligned, with slack behind them.  Real
callers do not: frame 1 of a uint8 batch of 73x21x3 frames starts at an odd address, a container in HBM has its payload 24 + 4n bytes
in, the sharded path decodes out of a receive buffer.  Here all buffers of a call are carved out of ONE arena (tests/arena.py): pixels
and payloads at the skews of TRIPLES (pixels in, payload, pixels out -- address modulo 256), outputs at exactly the size the call may
write, so the byte behind an output is a red-zone byte; the tables and result words keep their natural alignment, which is the
contract (include/llcomp_mi.h, "Alignment of the device pointers").  What a kernel can get wrong then shows as a wrong byte (a
dword access that silently drops the low address bits) or as a damaged red zone (a tail stored as a whole dword, a 16-byte unit past
the capacity, four pixels stored where three remain).

Expected values come from the oracle's sliced containers of each frame and from the source pixels, never from another GPU result.
Three frames per codec (noise, `nat`, flat): the frames of the odd-sized shapes start at odd addresses on their own, and one lane
group holds streams of a few bytes next to streams of several hundred.  The shapes are the smallest that reach each kernel family
(asserted through Codec.family).  With three frames of these sizes the default lane groups are narrow and the 64x64 / 65x64 tiles would
run one slice per wavefront, so the snapshot cases force LLCOMP_MI_LANE_SHIFT=3 (several slices per wavefront, as in a real batch) and
two extra row cases force the full 64-lane groups of a real batch; no hook changes an output byte.

llcomp_mi_device_copy_segments, which otherwise runs only under llcomp_amd/sharding.py, is compared with numpy here."""
import zlib

import numpy as np
import pytest
from arena import Arena
from conftest import make_image
from resize_spec import resize

pytestmark = pytest.mark.gpu

FRAMES = 3
TRIPLES = [(0, 0, 0), (1, 7, 3), (2, 1, 13), (3, 15, 1)]  # address % 256 of (pixels in, payload, pixels out)
TRIPLE_IDS = ["-".join(map(str, t)) for t in TRIPLES]


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


@pytest.fixture
def set_hooks(mi, monkeypatch):
    """the library reads its LLCOMP_MI_* hooks once per process: a test that changes one has them read again"""
    def _set(hooks):
        for name, value in hooks:
            monkeypatch.setenv(name, value)
        mi.reload_tuning()

    yield _set
    monkeypatch.undo()
    mi.reload_tuning()


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def sync():
    import torch

    torch.cuda.synchronize()


class Case:
    def __init__(self, name, w, h, c, tw, th, planar, want, hooks=(), small=False):
        self.name, self.w, self.h, self.c, self.tw, self.th, self.planar = name, w, h, c, tw, th, planar
        self.want, self.hooks, self.small = want, tuple(hooks), small  # want: the keys of Codec.family that are asserted

    def codec(self, mi, frames=FRAMES):
        k = mi.Codec(frames, self.w, self.h, self.c, self.tw, self.th, self.planar, device=0, small_model=self.small)
        got = {key: k.family[key] for key in self.want}
        if got != self.want:
            k.close()
            raise AssertionError(f"{self.name} runs another kernel family than it is meant to: {k.family}")
        return k


ROWS, TABLES_HBM = {"rows": True}, {"rows": False, "lds_table": False}
CASES = (
    # one-row planar slices: the encoder reads the pixels itself, the batched row inverse writes them; the last tile column is one
    # pixel wide and the planes of a tile straddle lane groups
    [Case(f"rows_planar_c{c}", 73, 21, c, 36, 1, True, ROWS) for c in (1, 2, 3, 4)]
    # ... in the 64-lane groups of a real batch (the dword rows of the row kernels; three frames alone give narrow groups)
    + [Case(f"rows_planar_c{c}_groups64", 73, 21, c, 36, 1, True, dict(ROWS, lane_shift=6), [("LLCOMP_MI_LANE_SHIFT", "6")]) for c in (3, 4)]
    # one-row interleaved slices
    + [Case(f"rows_interleaved_c{c}", 73, 21, c, 73, 1, False, ROWS) for c in (1, 2, 3, 4)]
    # 2-D slices with their state tables in HBM: lane groups of 64 and of 8, the decoder's bank cache on and off
    + [Case(f"tables_8x8_{'c3p' if planar else 'c4i'}_shift{shift}{'_nocache' if nocache else ''}", 97, 65, c, 8, 8, planar,
            dict(TABLES_HBM, lane_shift=shift, bank_cache=not nocache),
            [("LLCOMP_MI_LANE_SHIFT", str(shift))] + ([("LLCOMP_MI_NOCACHE", "1")] if nocache else []))
       for (c, planar) in ((3, True), (4, False)) for shift in (6, 3) for nocache in (False, True)]
    # the encoder's snapshot pass in one go (4096 samples a slice) and in chunks (4160), and the table encoder in its place
    + [Case("snapshot_64x64p", 131, 129, 3, 64, 64, True, dict(TABLES_HBM, snapshot=True), [("LLCOMP_MI_LANE_SHIFT", "3")]),
       Case("snapshot_chunked_65x64p", 131, 129, 3, 65, 64, True, dict(TABLES_HBM, snapshot=True), [("LLCOMP_MI_LANE_SHIFT", "3")]),
       Case("nosnap_64x64p", 131, 129, 3, 64, 64, True, dict(TABLES_HBM, snapshot=False), [("LLCOMP_MI_LANE_SHIFT", "3"), ("LLCOMP_MI_NOSNAP", "1")])]
    # one slice per wavefront, its state table in LDS
    + [Case("lds_table_80x24i", 161, 49, 3, 80, 24, False, {"rows": False, "lds_table": True, "slices_per_wave": 1})]
    # more than four channels: the _any model kernels
    + [Case("c5_planar_rows", 41, 19, 5, 20, 1, True, ROWS), Case("c5_interleaved_16x8", 41, 19, 5, 16, 8, False, {"rows": False})]
    # the small model
    + [Case("small_rows_planar_c3", 73, 21, 3, 36, 1, True, ROWS, small=True),
       Case("small_tables_8x8_c3p", 97, 65, 3, 8, 8, True, TABLES_HBM, small=True)]
)
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}

_CACHE = {}


def cached(key, make):
    """expected values are computed once, shared among the tests that need them and left unchanged"""
    if key not in _CACHE:
        v = make()
        for a in v if isinstance(v, tuple) else (v,):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def frames_of(case, frames=FRAMES):
    """noise, `nat`, a flat frame (and round again)"""
    def make():
        rng = np.random.default_rng(zlib.crc32(case.name.encode()))
        shape = (case.h, case.w, case.c)
        three = [rng.integers(0, 256, size=shape, dtype=np.uint8), make_image("nat", case.w, case.h, case.c), np.full(shape, 90, np.uint8)]
        return np.stack([three[f % 3] for f in range(frames)])

    return cached((case.name, "frames", frames), make)


def oracle_pack(mi, orc, case, imgs):
    """(payload u8, slice lengths u32, the containers) of the batch as llcomp_mi_codec_encode writes them: the oracle's container of every frame"""
    orc.set_small_model(case.small)
    try:
        conts = [orc.compress_sliced(np.ascontiguousarray(f), case.tw, case.th, case.planar) for f in imgs]
    finally:
        orc.set_small_model(False)
    # a container is header (24 bytes, its last dword the slice count), table, payload: cut by hand, not by the package under test
    pays, lens = [], []
    for d in conts:
        n = int.from_bytes(d[20:24], "little")
        lens.append(np.frombuffer(d, dtype="<u4", count=n, offset=24).astype(np.uint32))
        pays.append(np.frombuffer(d, dtype=np.uint8, offset=24 + 4 * n))
        assert pays[-1].size == int(lens[-1].sum())
    return np.concatenate(pays), np.concatenate(lens), conts


def oracle_batch(mi, orc, case, frames=FRAMES):
    return cached((case.name, "batch", frames), lambda: oracle_pack(mi, orc, case, frames_of(case, frames)))


def rectangles(case):
    """(an unaligned rectangle that crosses tile borders, with rw odd -- rw * c odd for an odd c --; one that is exactly its tiles)"""
    w, h, tw, th = case.w, case.h, min(case.tw, case.w), min(case.th, case.h)
    rw, rh = 7, 5
    x, y = min(max(1, tw - 3), w - rw), min(max(1, th - 2), h - rh)
    ax, ay = (tw if w > tw else 0), (th if h > th else 0)
    return (x, y, rw, rh), (ax, ay, min(tw, w - ax), min(2 * th, h - ay))


def status_of(codec, a):
    return codec.status(int(a.read("status", np.uint32)[0]))


def tables(a, n_slices, lens=None, name="slice_len"):
    """the naturally aligned buffers of a call: the slice table (loaded when `lens` is given), and -- once -- total and status"""
    a.carve(name, 4 * n_slices)
    if lens is not None:
        a.load(name, lens.astype("<u4"))
    if "status" not in a:
        # (both are left holding the arena's pattern, which is not zero, and are never cleared between calls on purpose: every entry
        # point has to set d_status itself, also when it has nothing to report)
        a.carve("total", 8)
        a.carve("status", 4)
    return a.ptr(name)


# ---- encode ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("triple", TRIPLES, ids=TRIPLE_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_encode(mi, orc, set_hooks, case, triple):
    imgs = frames_of(case)
    want_pay, want_lens, _ = oracle_batch(mi, orc, case)
    total, n = int(want_pay.size), int(want_lens.size)
    set_hooks(case.hooks)
    k = case.codec(mi)
    try:
        assert k.n_slices == n
        a = Arena(Arena.room(imgs.size, total, 4 * n, 8, 4), device="cuda")
        a.carve("px", imgs.size, skew=triple[0])
        a.load("px", imgs)
        a.carve("payload", total, skew=triple[1])  # payload_cap = the oracle's total, exactly
        tables(a, n)
        k.encode(a.ptr("px"), a.ptr("payload"), total, a.ptr("slice_len"), a.ptr("total"), a.ptr("status"), stream())
        sync()
        assert status_of(k, a) == mi.OK
        assert np.array_equal(a.read("slice_len", np.uint32), want_lens)
        assert int(a.read("total", np.uint64)[0]) == total
        assert np.array_equal(a.read("payload"), want_pay)
        a.unchanged("px")
        a.check()
        # one byte short: OVERFLOW, and nothing at or behind the capacity is written
        for name in ("payload", "slice_len", "total", "status"):
            a.reset(name)
        k.encode(a.ptr("px"), a.ptr("payload"), total - 1, a.ptr("slice_len"), a.ptr("total"), a.ptr("status"), stream())
        sync()
        assert status_of(k, a) == mi.OUTPUT_OVERFLOW
        assert np.array_equal(a.read("slice_len", np.uint32), want_lens) and int(a.read("total", np.uint64)[0]) == total
        last = total - int(want_lens[-1])  # the last slice does not fit and is not written; the ones in front of it are
        assert np.array_equal(a.read("payload")[:last], want_pay[:last])
        a.untouched("payload", first=last)
        a.unchanged("px")
        a.check()
    finally:
        k.close()


# ---- decode ----------------------------------------------------------------------------------------------------------------------

def load_batch(a, triple, pay, lens):
    a.carve("payload", pay.size, skew=triple[1])  # payload_bytes exact: the byte behind the payload is a red-zone byte
    a.load("payload", pay)
    tables(a, lens.size, lens)


def inputs_unchanged(a):
    a.unchanged("payload")
    a.unchanged("slice_len")
    a.check()


@pytest.mark.parametrize("triple", TRIPLES, ids=TRIPLE_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_decode(mi, orc, set_hooks, case, triple):
    imgs = frames_of(case)
    pay, lens, _ = oracle_batch(mi, orc, case)
    set_hooks(case.hooks)
    k = case.codec(mi)
    try:
        a = Arena(Arena.room(pay.size, 4 * lens.size, 8, 4, imgs.size), device="cuda")
        load_batch(a, triple, pay, lens)
        a.carve("out", imgs.size, skew=triple[2])
        k.decode(a.ptr("payload"), pay.size, a.ptr("slice_len"), a.ptr("out"), a.ptr("status"), stream())
        sync()
        assert status_of(k, a) == mi.OK
        assert np.array_equal(a.read("out").reshape(imgs.shape), imgs)
        inputs_unchanged(a)
    finally:
        k.close()


# ---- decode_region and decode_regions --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("triple", TRIPLES, ids=TRIPLE_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_decode_region_and_regions(mi, orc, set_hooks, case, triple):
    imgs = frames_of(case)
    pay, lens, _ = oracle_batch(mi, orc, case)
    set_hooks(case.hooks)
    k = case.codec(mi)
    try:
        rects = rectangles(case)
        a = Arena(Arena.room(pay.size, 4 * lens.size, 8, 4, *[FRAMES * rw * rh * case.c for (_, _, rw, rh) in rects] * 2), device="cuda")
        load_batch(a, triple, pay, lens)
        for i, (x, y, rw, rh) in enumerate(rects):
            out = f"region{i}"
            a.carve(out, FRAMES * rh * rw * case.c, skew=triple[2])  # exactly frames * rh * rw * c bytes
            k.decode_region(a.ptr("payload"), pay.size, a.ptr("slice_len"), x, y, rw, rh, a.ptr(out), a.ptr("status"), stream())
            sync()
            assert status_of(k, a) == mi.OK, (x, y, rw, rh)
            assert np.array_equal(a.read(out).reshape(FRAMES, rh, rw, case.c), imgs[:, y:y + rh, x:x + rw]), (x, y, rw, rh)
            inputs_unchanged(a)
            # a rectangle of this size at an offset of its own in every frame
            xy = [(x, y), (0, 0), (case.w - rw, case.h - rh)]
            out = f"regions{i}"
            a.carve(out, FRAMES * rh * rw * case.c, skew=triple[2])
            k.decode_regions(a.ptr("payload"), pay.size, a.ptr("slice_len"), xy, rw, rh, a.ptr(out), a.ptr("status"), stream())
            sync()
            assert status_of(k, a) == mi.OK, xy
            want = np.stack([imgs[f, yy:yy + rh, xx:xx + rw] for f, (xx, yy) in enumerate(xy)])
            assert np.array_equal(a.read(out).reshape(want.shape), want), xy
            inputs_unchanged(a)
    finally:
        k.close()


# ---- encode_region and update_region ---------------------------------------------------------------------------------------------

def update_expected(mi, orc, case, which):
    """(rectangle, new pixels of it, the oracle's batch of the modified frames, the oracle's batch of the covered box alone)"""
    def make():
        imgs = frames_of(case)
        x, y, rw, rh = rectangles(case)[which]
        rng = np.random.default_rng(zlib.crc32(case.name.encode()) + 1 + which)
        patch = rng.integers(0, 256, size=(FRAMES, rh, rw, case.c), dtype=np.uint8)
        patch[:, : rh // 2] = imgs[:, y:y + rh // 2, x:x + rw] ^ 1  # the upper half a near copy of what was there
        new = np.array(imgs)
        new[:, y:y + rh, x:x + rw] = patch
        full_pay, full_lens, _ = oracle_pack(mi, orc, case, new)
        tx0, ty0, tx1, ty1 = x // case.tw, y // case.th, -(-(x + rw) // case.tw), -(-(y + rh) // case.th)  # the tiles the rectangle touches
        n = (tx1 - tx0) * (ty1 - ty0) * (case.c if case.planar else 1)
        box = new[:, ty0 * case.th:min(ty1 * case.th, case.h), tx0 * case.tw:min(tx1 * case.tw, case.w)]
        sub_pay, sub_lens, _ = oracle_pack(mi, orc, case, box)
        assert sub_lens.size == FRAMES * n
        return (x, y, rw, rh), patch, full_pay, full_lens, sub_pay, sub_lens

    return cached((case.name, "update", which), make)


@pytest.mark.parametrize("triple", TRIPLES, ids=TRIPLE_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_encode_region_and_update_region(mi, orc, set_hooks, case, triple):
    pay, lens, _ = oracle_batch(mi, orc, case)
    set_hooks(case.hooks)
    k = case.codec(mi)
    try:
        for which in (0, 1):  # unaligned (the box is decoded and pasted into), aligned (the encoder reads d_rect itself)
            (x, y, rw, rh), patch, full_pay, full_lens, sub_pay, sub_lens = update_expected(mi, orc, case, which)
            a = Arena(Arena.room(pay.size, 4 * lens.size, 8, 4, patch.size, full_pay.size, 4 * lens.size, sub_pay.size, 4 * sub_lens.size), device="cuda")
            load_batch(a, triple, pay, lens)
            a.carve("rect", patch.size, skew=triple[0])
            a.load("rect", patch)
            a.carve("new_payload", full_pay.size, skew=triple[2])  # payload_cap exact
            a.carve("new_len", 4 * lens.size)
            a.carve("sub_payload", sub_pay.size, skew=triple[2])
            a.carve("sub_len", 4 * sub_lens.size)

            def unchanged():
                a.unchanged("rect")
                inputs_unchanged(a)

            k.update_region(a.ptr("payload"), pay.size, a.ptr("slice_len"), x, y, rw, rh, a.ptr("rect"), a.ptr("new_payload"), full_pay.size,
                            a.ptr("new_len"), a.ptr("total"), a.ptr("status"), stream())
            sync()
            assert status_of(k, a) == mi.OK, (x, y, rw, rh)
            assert int(a.read("total", np.uint64)[0]) == full_pay.size
            assert np.array_equal(a.read("new_len", np.uint32), full_lens), (x, y, rw, rh)
            assert np.array_equal(a.read("new_payload"), full_pay), (x, y, rw, rh)
            unchanged()
            a.untouched("sub_payload")
            k.encode_region(a.ptr("payload"), pay.size, a.ptr("slice_len"), x, y, rw, rh, a.ptr("rect"), a.ptr("sub_payload"), sub_pay.size,
                            a.ptr("sub_len"), a.ptr("total"), a.ptr("status"), stream())
            sync()
            assert status_of(k, a) == mi.OK, (x, y, rw, rh)
            assert int(a.read("total", np.uint64)[0]) == sub_pay.size
            assert np.array_equal(a.read("sub_len", np.uint32), sub_lens), (x, y, rw, rh)
            assert np.array_equal(a.read("sub_payload"), sub_pay), (x, y, rw, rh)
            assert np.array_equal(a.read("new_payload"), full_pay)
            unchanged()
    finally:
        k.close()


# ---- decode_resized_regions: u8 output, c = 1 and 3 (the float formats and c = 4 are covered by test_gpu_resized_output.py) ------------

RESIZED = ["rows_planar_c1", "rows_planar_c3", "small_tables_8x8_c3p"]


@pytest.mark.parametrize("out_skew", [1, 3])
@pytest.mark.parametrize("name", RESIZED)
def test_decode_resized_regions(mi, orc, set_hooks, name, out_skew):
    case = BY_NAME[name]
    frames, ow, oh = 2, 15, 9  # ow * c is odd
    imgs = frames_of(case, frames)
    pay, lens, _ = oracle_batch(mi, orc, case, frames)
    rects = [(3, 2, 41, 17), (case.w - 30, 0, 29, case.h - 1)]  # two frames, two rectangles of different sizes
    want = cached((name, "resized"), lambda: np.stack([resize(mi, imgs[f, y:y + rh, x:x + rw], ow, oh) for f, (x, y, rw, rh) in enumerate(rects)]))
    set_hooks(case.hooks)
    k = case.codec(mi, frames)
    try:
        a = Arena(Arena.room(pay.size, 4 * lens.size, 8, 4, want.size), device="cuda")
        load_batch(a, (0, 7, out_skew), pay, lens)
        a.carve("out", want.size, skew=out_skew)
        k.decode_resized_regions(a.ptr("payload"), pay.size, a.ptr("slice_len"), rects, ow, oh, a.ptr("out"), a.ptr("status"), stream=stream())
        sync()
        assert status_of(k, a) == mi.OK
        assert np.array_equal(a.read("out").reshape(want.shape), want)
        inputs_unchanged(a)
    finally:
        k.close()


# ---- the contract: tables and result words need their natural alignment -------------------------------------------------------------

@pytest.mark.parametrize("which", ["slice_len", "total", "status"])
def test_misaligned_table_is_refused_and_nothing_is_written(mi, orc, which):
    case = BY_NAME["rows_planar_c3"]
    imgs = frames_of(case)
    pay, lens, _ = oracle_batch(mi, orc, case)
    k = case.codec(mi)
    try:
        a = Arena(Arena.room(imgs.size, pay.size, 4 * lens.size + 8, 16, 8, pay.size, imgs.size), device="cuda")
        a.carve("px", imgs.size, skew=1)
        a.load("px", imgs)
        a.carve("payload", pay.size, skew=7)
        a.carve("slice_len", 4 * lens.size + 8)  # (room for the table 2 bytes in)
        a.carve("total", 16)
        a.carve("status", 8)
        a.carve("old_payload", pay.size, skew=5)
        a.load("old_payload", pay)
        a.carve("out", imgs.size, skew=3)
        off = {"slice_len": 0, "total": 0, "status": 0}
        off[which] = {"slice_len": 2, "total": 4, "status": 2}[which]  # (d_total: a multiple of 4 that is no multiple of 8)
        with pytest.raises(mi.LlcompError) as e:
            k.encode(a.ptr("px"), a.ptr("payload"), pay.size, a.ptr("slice_len") + off["slice_len"], a.ptr("total") + off["total"],
                     a.ptr("status") + off["status"], stream())
        assert e.value.status == mi.BAD_ARGS
        if which != "total":  # (a decode has no d_total)
            with pytest.raises(mi.LlcompError) as e:
                k.decode(a.ptr("old_payload"), pay.size, a.ptr("slice_len") + off["slice_len"], a.ptr("out"), a.ptr("status") + off["status"], stream())
            assert e.value.status == mi.BAD_ARGS
            with pytest.raises(mi.LlcompError) as e:
                k.decode_region(a.ptr("old_payload"), pay.size, a.ptr("slice_len") + off["slice_len"], 1, 1, 7, 5, a.ptr("out"),
                                a.ptr("status") + off["status"], stream())
            assert e.value.status == mi.BAD_ARGS
        with pytest.raises(mi.LlcompError) as e:
            k.update_region(a.ptr("old_payload"), pay.size, a.ptr("slice_len") + off["slice_len"], 1, 1, 7, 5, a.ptr("px"), a.ptr("payload"), pay.size,
                            a.ptr("slice_len") + off["slice_len"], a.ptr("total") + off["total"], a.ptr("status") + off["status"], stream())
        assert e.value.status == mi.BAD_ARGS
        with pytest.raises(mi.LlcompError) as e:
            k.encode_region(a.ptr("old_payload"), pay.size, a.ptr("slice_len") + off["slice_len"], 1, 1, 7, 5, a.ptr("px"), a.ptr("payload"), pay.size,
                            a.ptr("slice_len") + off["slice_len"], a.ptr("total") + off["total"], a.ptr("status") + off["status"], stream())
        assert e.value.status == mi.BAD_ARGS
        if which != "total":
            xy = [(1, 1), (0, 0), (5, 3)]
            with pytest.raises(mi.LlcompError) as e:
                k.decode_regions(a.ptr("old_payload"), pay.size, a.ptr("slice_len") + off["slice_len"], xy, 7, 5, a.ptr("out"),
                                 a.ptr("status") + off["status"], stream())
            assert e.value.status == mi.BAD_ARGS
            with pytest.raises(mi.LlcompError) as e:
                k.decode_resized_regions(a.ptr("old_payload"), pay.size, a.ptr("slice_len") + off["slice_len"], [(1, 1, 7, 5)] * FRAMES, 5, 3,
                                         a.ptr("out"), a.ptr("status") + off["status"], stream=stream())
            assert e.value.status == mi.BAD_ARGS
        if which == "status":  # the calls on host containers have no device table: their status word alone
            conts = oracle_batch(mi, orc, case)[2]
            with pytest.raises(mi.LlcompError) as e:
                k.decode_regions_host(conts, [(1, 1), (0, 0), (5, 3)], 7, 5, a.ptr("out"), a.ptr("status") + 2, stream())
            assert e.value.status == mi.BAD_ARGS
            with pytest.raises(mi.LlcompError) as e:
                k.decode_resized_regions_host(conts, [(1, 1, 7, 5)] * FRAMES, 5, 3, a.ptr("out"), a.ptr("status") + 2, stream=stream())
            assert e.value.status == mi.BAD_ARGS
        if which == "slice_len":  # d_sym of the stage-A call is a u32 array like the slice table
            with pytest.raises(mi.LlcompError) as e:
                k.model(a.ptr("px"), a.ptr("slice_len") + 2, stream())
            assert e.value.status == mi.BAD_ARGS
        sync()
        a.all_untouched()  # before anything is launched or written: not a byte of the arena has changed
    finally:
        k.close()


@pytest.mark.parametrize("which", ["vals", "start", "count", "out"])
def test_range_sums_misaligned_table_is_refused(mi, which):
    """llcomp_mi_device_range_sums: a u32 table, three u64 tables; the aligned call is compared with numpy first"""
    from llcomp_amd import _lib

    L = _lib.load()
    vals = np.arange(1, 41, dtype=np.uint32) * 1000
    start, count = np.array([0, 7, 39], np.uint64), np.array([7, 30, 1], np.uint64)
    a = Arena(Arena.room(4 * 42, 32, 32, 32), device="cuda")
    for name, data in (("vals", vals), ("start", start), ("count", count)):
        a.carve(name, data.nbytes + 8)
        a.load(name, np.concatenate([data.view(np.uint8), np.zeros(8, np.uint8)]))
    a.carve("out", 24)
    ptr = {name: a.ptr(name) for name in ("vals", "start", "count", "out")}
    assert L.llcomp_mi_device_range_sums(ptr["vals"], ptr["start"], ptr["count"], ptr["out"], 3, 25000, stream()) == mi.OK
    sync()
    want = [int(np.minimum(vals[int(s):int(s + n)], 25000).sum()) for s, n in zip(start, count)]
    assert a.read("out", np.uint64).tolist() == want
    a.check()
    a.reset("out")
    ptr[which] += 2 if which == "vals" else 4
    assert L.llcomp_mi_device_range_sums(ptr["vals"], ptr["start"], ptr["count"], ptr["out"], 2, 25000, stream()) == mi.BAD_ARGS
    sync()
    a.all_untouched()


# ---- the host calls: source and destination at odd addresses in host memory, at exact capacity ------------------------------------------

HOST_CASES = ["rows_planar_c3", "tables_8x8_c4i_shift3"]


def host_buffers(sizes_and_data):
    """a CPU arena with one buffer per (name, size, skew, data or None) -> (arena, {name: numpy view of the buffer})"""
    a = Arena(Arena.room(*[s for _, s, _, _ in sizes_and_data]), device="cpu")
    views = {}
    for name, size, skew, data in sizes_and_data:
        a.carve(name, size, skew=skew)
        if data is not None:
            a.load(name, data)
        views[name] = a.view(name).numpy()
        assert views[name].ctypes.data == a.ptr(name) and a.ptr(name) % 256 == skew
    return a, views


@pytest.mark.parametrize("name", HOST_CASES)
def test_host_calls(mi, orc, set_hooks, name):
    case = BY_NAME[name]
    w, h, c, tw, th, planar = case.w, case.h, case.c, case.tw, case.th, case.planar
    img = frames_of(case)[1]
    cont = oracle_batch(mi, orc, case)[2][1]
    (x, y, rw, rh), patch = update_expected(mi, orc, case, 0)[:2]
    patch = patch[1]
    new = np.array(img)
    new[y:y + rh, x:x + rw] = patch
    new_cont = orc.compress_sliced(new, tw, th, planar)
    set_hooks(case.hooks)
    a, v = host_buffers([("px", img.size, 1, img), ("cont", len(cont), 3, None),                   # encode_into: pixels at 1 -> container at 3
                         ("old", len(cont), 1, np.frombuffer(cont, np.uint8)), ("out", img.size, 3, None),  # decode_into
                         ("crop", rw * rh * c, 3, None),                                           # decode_region_into
                         ("patch", patch.size, 3, patch), ("new", len(new_cont), 1, None)])        # update_region_into
    n = mi.compress_image_into(v["px"], w, h, c, v["cont"], format=mi.FORMAT_SLICED, tile_w=tw, tile_h=th, planar=planar, device=0)
    assert n == len(cont) and v["cont"].tobytes() == cont
    assert mi.decompress_image_into(v["old"], v["out"], device=0) == (w, h, c)
    assert np.array_equal(v["out"].reshape(img.shape), img)
    assert mi.decompress_region_into(v["old"], v["crop"], x, y, rw, rh, device=0) == c
    assert np.array_equal(v["crop"].reshape(rh, rw, c), img[y:y + rh, x:x + rw])
    assert mi.update_region_into(v["old"], v["new"], x, y, v["patch"].reshape(rh, rw, c), device=0) == len(new_cont)
    assert v["new"].tobytes() == new_cont
    for inp in ("px", "old", "patch"):
        a.unchanged(inp)
    a.check()
    # one byte short: OUTPUT_OVERFLOW, and the destination stays as it was
    a.reset("cont")
    with pytest.raises(mi.LlcompError) as e:
        mi.compress_image_into(v["px"], w, h, c, v["cont"][:-1], format=mi.FORMAT_SLICED, tile_w=tw, tile_h=th, planar=planar, device=0)
    assert e.value.status == mi.OUTPUT_OVERFLOW and e.value.needed == len(cont)
    a.untouched("cont")
    a.check()


@pytest.mark.parametrize("name", HOST_CASES)
def test_decode_regions_host(mi, orc, set_hooks, name):
    case = BY_NAME[name]
    imgs = frames_of(case)
    conts = oracle_batch(mi, orc, case)[2]
    (x, y, rw, rh) = rectangles(case)[0]
    xy = [(x, y), (0, 0), (case.w - rw, case.h - rh)]
    want = np.stack([imgs[f, yy:yy + rh, xx:xx + rw] for f, (xx, yy) in enumerate(xy)])
    set_hooks(case.hooks)
    ha, hv = host_buffers([(f"cont{f}", len(d), (1, 3, 2)[f], np.frombuffer(d, np.uint8)) for f, d in enumerate(conts)])
    k = case.codec(mi)
    try:
        a = Arena(Arena.room(want.size, 4), device="cuda")
        a.carve("out", want.size, skew=3)
        a.carve("status", 4)
        k.decode_regions_host([hv[f"cont{f}"] for f in range(FRAMES)], xy, rw, rh, a.ptr("out"), a.ptr("status"), stream())
        sync()
        assert status_of(k, a) == mi.OK
        assert np.array_equal(a.read("out").reshape(want.shape), want)
        a.check()
        ha.all_untouched()
    finally:
        k.close()


# ---- llcomp_mi_device_copy_segments against numpy ------------------------------------------------------------------------------------

PIECE = 16384  # bytes one workgroup moves per step (kSegPieceDwords dwords)
LENGTHS = list(range(10)) + [15, 16, 17] + [PIECE * k + d for k in (1, 2) for d in (-1, 0, 1, 5)]


def copy_segments(mi, a, src_off, dst_off, lens, max_len, n_seg=None):
    """one call on the arena's "src" and "dst" with the three u64 tables loaded into naturally aligned buffers -> the status"""
    from llcomp_amd import _lib

    for name, vals in (("src_off", src_off), ("dst_off", dst_off), ("len", lens)):
        if name not in a:
            a.carve(name, 8 * len(vals))
        a.load(name, np.asarray(vals, dtype="<u8"))
    rc = _lib.load().llcomp_mi_device_copy_segments(a.ptr("src"), a.ptr("dst"), a.ptr("src_off"), a.ptr("dst_off"), a.ptr("len"),
                                                    len(lens) if n_seg is None else n_seg, max_len, stream())
    sync()
    return rc


def check_copy(a, src, src_off, dst_off, lens):
    """the destination holds the pattern with every range copied into it, the source and the tables are unchanged, the zones intact"""
    from arena import pattern

    want = pattern(a.ptr("dst") - a.base, a.size("dst"))
    for s, d, n in zip(src_off, dst_off, lens):
        want[d:d + n] = src[s:s + n]
    got = a.read("dst")
    bad = np.nonzero(got != want)[0]
    assert not bad.size, f"destination differs from numpy's at offset {int(bad[0])} ({bad.size} bytes)"
    for name in ("src", "src_off", "dst_off", "len"):
        a.unchanged(name)
    a.check()


def hint(which, lens):
    return {"max": max(lens) if len(lens) else 0, "one": 1, "zero": 0}[which]


@pytest.mark.parametrize("max_len", ["max", "one", "zero"])
@pytest.mark.parametrize("skews", [(s, d) for s in range(4) for d in range(4)], ids=lambda sd: f"src{sd[0]}_dst{sd[1]}")
def test_copy_segments_alignment_and_length_matrix(mi, skews, max_len):
    """every length at the source offset `s` and the destination offset `d` modulo 4, independently; a gap of up to three bytes of
    pattern lies between two ranges, and the comparison with numpy covers it"""
    s_mod, d_mod = skews
    lens = LENGTHS + [3 * PIECE + 7]
    rng = np.random.default_rng(4 * s_mod + d_mod)
    src_off, dst_off, s_at, d_at = [], [], 0, 0
    for n in lens:
        s_at += (s_mod - s_at) % 4
        d_at += (d_mod - d_at) % 4
        src_off.append(s_at)
        dst_off.append(d_at)
        s_at += n
        d_at += n
    src = rng.integers(0, 256, size=s_at, dtype=np.uint8)
    a = Arena(Arena.room(s_at, d_at, *[8 * len(lens)] * 3), device="cuda")
    a.carve("src", s_at)  # (256-byte aligned: an offset's residue modulo 4 is its address's)
    a.load("src", src)
    a.carve("dst", d_at)
    order = rng.permutation(len(lens))  # (the order of the segments in the tables is not the order in memory)
    src_off, dst_off, lens = [src_off[i] for i in order], [dst_off[i] for i in order], [lens[i] for i in order]
    assert copy_segments(mi, a, src_off, dst_off, lens, hint(max_len, lens)) == mi.OK
    check_copy(a, src, src_off, dst_off, lens)


@pytest.mark.parametrize("max_len", ["max", "one", "zero"])
def test_copy_segments_adjacent_ranges(mi, max_len):
    """destination ranges packed back to back in shuffled order: every segment's neighbours are its red zones (a byte too many at
    either end lands in a neighbour and differs from numpy's), the arena's own zones lie around the whole buffer"""
    rng = np.random.default_rng(77)
    lens = [n for n in LENGTHS + [3 * PIECE + 7] for _ in range(2)] + [int(v) for v in rng.integers(1, 40, size=60)]
    lens = [lens[i] for i in rng.permutation(len(lens))]
    total = sum(lens)
    src = rng.integers(0, 256, size=total + 3, dtype=np.uint8)
    # sources back to back as well, in another order, one byte into the buffer (an odd address)
    s_order = rng.permutation(len(lens))
    src_off = np.zeros(len(lens), np.int64)
    src_off[s_order] = 1 + np.concatenate([[0], np.cumsum([lens[i] for i in s_order])[:-1]])
    dst_off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    a = Arena(Arena.room(src.size, total, *[8 * len(lens)] * 3), device="cuda")
    a.carve("src", src.size, skew=2)
    a.load("src", src)
    a.carve("dst", total, skew=5)  # exactly the bytes the call may write
    table_order = rng.permutation(len(lens))
    src_off, dst_off, lens = [int(src_off[i]) for i in table_order], [int(dst_off[i]) for i in table_order], [lens[i] for i in table_order]
    assert copy_segments(mi, a, src_off, dst_off, lens, hint(max_len, lens)) == mi.OK
    check_copy(a, src, src_off, dst_off, lens)
    assert np.array_equal(np.sort(np.concatenate([np.arange(d, d + n) for d, n in zip(dst_off, lens)])), np.arange(total))  # (every byte once)


def test_copy_segments_counts(mi):
    rng = np.random.default_rng(5)
    n_max = 65535
    lens = [int(v) for v in rng.integers(0, 4, size=n_max)]
    dst_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
    total = sum(lens)
    src = rng.integers(0, 256, size=total + 8, dtype=np.uint8)
    src_off = [int(v) for v in rng.integers(0, total + 8 - 3, size=n_max)]
    a = Arena(Arena.room(src.size, total, *[8 * (n_max + 1)] * 3), device="cuda")
    a.carve("src", src.size, skew=1)
    a.load("src", src)
    a.carve("dst", total, skew=3)
    for name in ("src_off", "dst_off", "len"):
        a.carve(name, 8 * (n_max + 1))
    tabs = (src_off + [0], dst_off + [0], lens + [1])  # (entry 65535: one byte to dst[0], which no call may copy)
    # no segment: nothing is written, whatever the tables say
    assert copy_segments(mi, a, *tabs, 3, n_seg=0) == mi.OK
    a.untouched("dst")
    a.check()
    # one segment too many: refused (BAD_ARGS, before the launch that HIP would refuse with hipErrorInvalidValue), nothing is written
    assert copy_segments(mi, a, *tabs, 3, n_seg=n_max + 1) == mi.BAD_ARGS
    a.untouched("dst")
    a.check()
    # the most segments of one call, of 0 to 3 bytes each
    assert copy_segments(mi, a, *tabs, 3, n_seg=n_max) == mi.OK
    check_copy(a, src, src_off, dst_off, lens)
    # a misaligned u64 table is refused like a misaligned slice table
    from llcomp_amd import _lib

    a.reset("dst")
    rc = _lib.load().llcomp_mi_device_copy_segments(a.ptr("src"), a.ptr("dst"), a.ptr("src_off"), a.ptr("dst_off") + 4, a.ptr("len"), 8, 3, stream())
    sync()
    assert rc == mi.BAD_ARGS
    a.untouched("dst")
    a.check()
