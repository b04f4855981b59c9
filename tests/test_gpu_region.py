"""Region decode on the GPU (llcomp_mi_decode_region, llcomp_mi_codec_decode_region, llcompd --region): the rectangle of the picture,
bit for bit, from the covered slices alone.  Containers come from the oracle, so none of this depends on the HIP encoder; the
expected output is img[y:y+rh, x:x+rw]."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, make_image

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


@pytest.fixture
def set_hook(mi, monkeypatch):
    """the library reads its LLCOMP_MI_* hooks once per process: a test that changes one has them read again"""
    def _set(name, value):
        monkeypatch.setenv(name, value)
        mi.reload_tuning()

    yield _set
    monkeypatch.undo()
    mi.reload_tuning()


def rects(w, h, tw, th):
    """rectangles that touch every edge, one pixel, the whole picture, one tile, the partial last tile column / row only"""
    tw = w if tw == 0 else min(tw, w)
    th = h if th == 0 else min(th, h)
    lx, ly = (w - 1) // tw * tw, (h - 1) // th * th
    return [(0, 0, w, h), (w // 3, h // 4, max(1, w // 2), max(1, h // 2)), (0, 0, 1, 1), (w - 1, h - 1, 1, 1),
            (min(tw, w - 1), 0, w - min(tw, w - 1), max(1, h // 3)), (0, h - max(1, h // 5), max(1, w // 4), max(1, h // 5)),
            (lx, ly, w - lx, h - ly), (0, ly, w, h - ly), (lx, 0, w - lx, h), (0, 0, min(tw, w), min(th, h))]


def check_regions(mi, data, img, rs, small_model=False):
    for (x, y, rw, rh) in rs:
        got = mi.decompress_region(data, x, y, rw, rh, device=0, small_model=small_model)
        assert (got.width, got.height, got.channels) == (rw, rh, img.shape[2])
        assert np.array_equal(got.pixels, img[y:y + rh, x:x + rw]), (x, y, rw, rh)


def region_family(mi, img, tw, th, planar, rect, small_model=False):
    h, w, c = img.shape
    k = mi.Codec(1, w, h, c, tw, th, planar, device=0, small_model=small_model)
    try:
        return k.family, k.region_family(*rect)
    finally:
        k.close()


# (name, w, h, c, tile_w, tile_h, planar, generator, rectangle whose family is asserted, key that must be set in its family)
FAMILIES = [
    ("rows_fused_480x1p", 1100, 24, 3, 480, 1, True, "nat", (100, 5, 700, 11), "rows"),
    ("rows_interleaved_32x1i", 200, 30, 3, 32, 1, False, "mid", (5, 3, 150, 20), "rows"),
    ("lds_table_256x256p", 600, 520, 3, 256, 256, True, "nat", (300, 10, 100, 100), "lds_table"),
    ("lds_table_64x64i_few", 200, 150, 3, 64, 64, False, "mid", (70, 10, 60, 100), "lds_table"),
    ("hbm_bank_cache_32x32i", 800, 420, 3, 32, 32, False, "nat", (33, 17, 700, 380), "bank_cache"),
    ("c1_planar_tiles", 300, 200, 1, 40, 24, True, "g3", (13, 7, 250, 150), None),
    ("c4_interleaved_tiles", 300, 200, 4, 48, 16, False, "mid", (13, 7, 250, 150), None),
    ("c5_interleaved_tiles", 160, 90, 5, 32, 16, False, "g1", (13, 7, 100, 50), None),
    ("c5_planar_rows", 160, 30, 5, 40, 1, True, "g1", (13, 7, 100, 20), None),
    ("odd_19x13_on_100x37", 100, 37, 3, 19, 13, True, "checker", (17, 12, 70, 25), None),
]


@pytest.mark.parametrize("case", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_region_equals_crop_per_family(mi, orc, case):
    name, w, h, c, tw, th, planar, gen, rect, key = case
    img = make_image(gen, w, h, c)
    data = orc.compress_sliced(img, tw, th, planar)
    _, fam = region_family(mi, img, tw, th, planar, rect)
    if key:
        assert fam[key], (name, fam)
    check_regions(mi, data, img, rects(w, h, tw, th) + [rect])


def test_region_without_bank_cache(mi, orc, set_hook):
    set_hook("LLCOMP_MI_NOCACHE", "1")
    img = make_image("nat", 800, 420, 3)
    data = orc.compress_sliced(img, 32, 32, False)
    _, fam = region_family(mi, img, 32, 32, False, (33, 17, 700, 380))
    assert not fam["bank_cache"] and not fam["lds_table"] and not fam["rows"], fam
    check_regions(mi, data, img, [(33, 17, 700, 380), (400, 200, 1, 1), (0, 0, 800, 420)])


def test_region_forced_replay(mi, orc, set_hook):
    set_hook("LLCOMP_MI_FORCE_REPLAY", "1")
    for (w, h, tw, th, planar) in ((300, 120, 32, 32, False), (600, 20, 120, 1, True)):
        img = make_image("g3", w, h, 3)
        data = orc.compress_sliced(img, tw, th, planar)
        check_regions(mi, data, img, rects(w, h, tw, th)[:4])


def test_region_small_model(mi, orc):
    img = make_image("mid", 300, 100, 3)
    orc.set_small_model(True)
    try:
        sliced = orc.compress_sliced(img, 40, 16, True)
        legacy = orc.compress_image(img)
    finally:
        orc.set_small_model(False)
    check_regions(mi, sliced, img, rects(300, 100, 40, 16)[:5])                     # the header says so
    check_regions(mi, legacy, img, [(10, 20, 200, 50), (299, 99, 1, 1)], small_model=True)  # the caller says so


def test_region_legacy_and_single_tile(mi, orc):
    img = make_image("nat", 257, 131, 3)
    legacy = orc.compress_image(img)
    check_regions(mi, legacy, img, rects(257, 131, 0, 0)[:6])
    one_tile = orc.compress_sliced(img, 0, 0, True)
    check_regions(mi, one_tile, img, rects(257, 131, 0, 0)[:6])


def test_region_clamped_tile_changes_family(mi, orc):
    """only the 1-row remainder of 2-row tiles is covered: the sub-geometry clamps tile_h to 1 and runs the row kernels"""
    w, h = 160, 41
    img = make_image("nat", w, h, 3)
    for planar in (True, False):
        data = orc.compress_sliced(img, 40, 2, planar)
        full, fam = region_family(mi, img, 40, 2, planar, (10, 40, 100, 1))
        assert not full["rows"] and fam["rows"], (full, fam)
        check_regions(mi, data, img, [(10, 40, 100, 1), (0, 40, 160, 1), (159, 40, 1, 1), (0, 39, 160, 2)])


def _slice_spans(data):
    info_n = int.from_bytes(data[20:24], "little")
    lens = np.frombuffer(data[24:24 + 4 * info_n], dtype="<u4").astype(np.int64)
    offs = 24 + 4 * info_n + np.concatenate([[0], np.cumsum(lens)])
    return lens, offs


def test_damage_outside_the_region_is_not_read(mi, orc):
    w, h, tw, th = 512, 256, 32, 32  # 16 x 8 tiles, interleaved: slice id = tile row * 16 + tile column
    img = make_image("nat", w, h, 3)
    data = bytearray(orc.compress_sliced(img, tw, th, False))
    x, y, rw, rh = 100, 70, 60, 50   # tile columns 3..4, tile rows 2..3
    (box, n) = mi.region_plan(w, h, 3, tw, th, False, x, y, rw, rh)
    assert box == (3, 2, 5, 4) and n == 4
    lens, offs = _slice_spans(data)
    covered = {ty * 16 + tx for ty in range(2, 4) for tx in range(3, 5)}
    for s in range(len(lens)):
        if s not in covered:  # other tile rows, and other columns of the same tile rows (inside the copied span)
            data[offs[s]:offs[s + 1]] = b"\xff" * int(lens[s])
    data = bytes(data)
    try:
        full = mi.decompress_image(data, device=0).pixels
        assert not np.array_equal(full, img), "the damage must be real"
    except mi.LlcompError:
        pass  # (a damaged slice may also be refused outright: just as real)
    got = mi.decompress_region(data, x, y, rw, rh, device=0)
    assert np.array_equal(got.pixels, img[y:y + rh, x:x + rw])


def test_truncation_inside_and_after_the_covered_slices(mi, orc):
    w, h, tw, th = 512, 256, 32, 32
    img = make_image("mid", w, h, 3)
    data = orc.compress_sliced(img, tw, th, False)
    lens, offs = _slice_spans(data)
    x, y, rw, rh = 100, 70, 60, 50
    last = 3 * 16 + 4  # the last covered slice
    assert lens[last] > 2
    with pytest.raises(mi.LlcompError) as e:
        mi.decompress_region(data[:offs[last] + lens[last] // 2], x, y, rw, rh, device=0)
    assert e.value.status == mi.TRUNCATED
    got = mi.decompress_region(data[:offs[last + 1]], x, y, rw, rh, device=0)
    assert np.array_equal(got.pixels, img[y:y + rh, x:x + rw])
    # a table or header cut short fails as probe does
    with pytest.raises(mi.LlcompError) as e:
        mi.decompress_region(data[:30], x, y, rw, rh, device=0)
    assert e.value.status == mi.TRUNCATED


def test_output_capacity(mi, orc):
    img = make_image("nat", 200, 100, 4)
    data = np.frombuffer(orc.compress_sliced(img, 32, 32, False), np.uint8).copy()
    out = np.full(30 * 20 * 4 - 1, 0xA5, np.uint8)
    with pytest.raises(mi.LlcompError) as e:
        mi.decompress_region_into(data, out, 10, 10, 30, 20, device=0)
    assert e.value.status == mi.OUTPUT_OVERFLOW and e.value.channels == 4
    assert (out == 0xA5).all()
    out = np.full(30 * 20 * 4 + 7, 0xA5, np.uint8)
    assert mi.decompress_region_into(data, out, 10, 10, 30, 20, device=0) == 4
    assert np.array_equal(out[:30 * 20 * 4].reshape(20, 30, 4), img[10:30, 10:40]) and (out[30 * 20 * 4:] == 0xA5).all()
    for bad in ((0, 0, 0, 1), (190, 0, 11, 1), (10, 0, 2**32 - 5, 1)):
        with pytest.raises(mi.LlcompError) as e:
            mi.decompress_region(bytes(data), *bad, device=0)
        assert e.value.status == mi.BAD_ARGS


class Batch:
    """a batch of per-frame content in HBM as the codec takes it: the oracle's containers' tables and payloads back to back"""

    def __init__(self, orc, frames, w, h, c, tw, th, planar, gens):
        import torch

        self.imgs = np.stack([make_image(gens[i % len(gens)], w, h, c) for i in range(frames)])
        for i in range(frames):
            self.imgs[i] = np.roll(self.imgs[i], i * 7, axis=1)
        lens, pays = [], []
        for f in range(frames):
            d = orc.compress_sliced(self.imgs[f], tw, th, planar)
            n = int.from_bytes(d[20:24], "little")
            lens.append(np.frombuffer(d[24:24 + 4 * n], dtype="<u4"))
            pays.append(d[24 + 4 * n:])
        pay = b"".join(pays)
        self.total = len(pay)
        self.d_pay = torch.from_numpy(np.frombuffer(pay + bytes(16), np.uint8).copy()).cuda()
        self.d_len = torch.from_numpy(np.concatenate(lens).view(np.int32).copy()).cuda()
        self.d_st = torch.zeros(1, dtype=torch.int32, device="cuda")


GUARD = 4096


def decode_region_checked(codec, b, x, y, rw, rh):
    """codec.decode_region into a buffer with sentinel guard bytes on both sides: the rectangle comes out exact, nothing else is written"""
    import torch

    frames, c = b.imgs.shape[0], b.imgs.shape[3]
    n = frames * rh * rw * c
    buf = torch.full((n + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    codec.decode_region(b.d_pay.data_ptr(), b.total, b.d_len.data_ptr(), x, y, rw, rh, buf.data_ptr() + GUARD, b.d_st.data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(b.d_st.item()) == 0
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 0x5A).all() and (host[GUARD + n:] == 0x5A).all(), "a byte outside the output was written"
    assert np.array_equal(host[GUARD:GUARD + n].reshape(frames, rh, rw, c), b.imgs[:, y:y + rh, x:x + rw]), (x, y, rw, rh)


@pytest.mark.parametrize("shape", [(100, 37, 3, 32, 16, True), (100, 37, 4, 19, 13, False), (300, 12, 3, 64, 1, True), (90, 40, 5, 32, 8, False)],
                         ids=["planar_tiles", "odd_tiles_c4", "rows", "c5"])
def test_codec_region_batch(mi, orc, set_hook, shape):
    import torch  # noqa: F401

    w, h, c, tw, th, planar = shape
    b = Batch(orc, 5, w, h, c, tw, th, planar, ["g1", "g3", "mid", "checker", "nat"])
    codec = mi.Codec(5, w, h, c, tw, th, planar, device=0)
    for r in rects(w, h, tw, th):
        decode_region_checked(codec, b, *r)
    codec.close()
    set_hook("LLCOMP_MI_LPW", "4")  # fewer slices per wavefront: the same pixels
    codec = mi.Codec(5, w, h, c, tw, th, planar, device=0)
    for r in rects(w, h, tw, th)[:4]:
        decode_region_checked(codec, b, *r)
    codec.close()


def test_state_tables_across_generation_wraps(mi, orc):
    """one codec with state tables in HBM, ~600 calls alternating full decodes with region decodes of three rectangle shapes (another
    lane-group mapping each): the generation-tagged tables are shared safely, every output is exact"""
    import torch

    w, h, c, tw, th = 640, 320, 3, 32, 32
    b = Batch(orc, 4, w, h, c, tw, th, False, ["nat", "mid", "g3", "g1"])
    codec = mi.Codec(4, w, h, c, tw, th, False, device=0)
    assert not codec.family["rows"] and not codec.family["lds_table"]
    codec.prepare(encode=False, decode=True, region=True)
    st = torch.cuda.current_stream().cuda_stream
    want_full = torch.from_numpy(b.imgs).cuda()
    shapes = [(40, 20, 400, 200), (0, 96, 640, 128), (130, 0, 300, 320)]
    fams = [codec.region_family(*r) for r in shapes]
    assert all(not f["rows"] and not f["lds_table"] for f in fams) and len({f["lane_shift"] for f in fams} | {codec.family["lane_shift"]}) >= 2
    outs = [torch.empty((4, rh, rw, c), dtype=torch.uint8, device="cuda") for (_, _, rw, rh) in shapes]
    wants = [torch.from_numpy(np.ascontiguousarray(b.imgs[:, y:y + rh, x:x + rw])).cuda() for (x, y, rw, rh) in shapes]
    full = torch.empty_like(want_full)
    codec.counters(reset=True)
    for i in range(600):
        if i % 2 == 0:
            full.fill_(0)
            codec.decode(b.d_pay.data_ptr(), b.total, b.d_len.data_ptr(), full.data_ptr(), b.d_st.data_ptr(), st)
            ok = torch.equal(full, want_full)
        else:
            k = (i // 2) % 3
            outs[k].fill_(0)
            x, y, rw, rh = shapes[k]
            codec.decode_region(b.d_pay.data_ptr(), b.total, b.d_len.data_ptr(), x, y, rw, rh, outs[k].data_ptr(), b.d_st.data_ptr(), st)
            ok = torch.equal(outs[k], wants[k])
        assert ok and int(b.d_st.item()) == 0, i
    assert codec.counters()["generation_wraps"] >= 2
    codec.close()


# ---- the C++ drop-in and the CLI ---------------------------------------------------------------------------------------------
def _png_reader():
    spec = importlib.util.spec_from_file_location("cli_image_io_tests", os.path.join(ROOT, "tests", "test_cli_image_io.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.decode_png_py


def test_llcompd_region(orc, tmp_path):
    exe = os.path.join(ROOT, "tools", "llcompd")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools")])
    decode_png = _png_reader()
    img = make_image("nat", 150, 90, 3)
    p = tmp_path / "pic.llcomp"
    p.write_bytes(orc.compress_sliced(img, 32, 16, True))
    r = subprocess.run([exe, str(p), "--region", "20,30,77,41"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got, _, _ = decode_png((tmp_path / "pic.llcomp.png").read_bytes())
    assert np.array_equal(got, img[30:71, 20:97])
    for bad in (["--region", "20,30,77"], ["--region", "1,2,3,x"], ["--region", "100,0,51,1"], ["--region", "0,0,0,1"], ["--region"],
                ["--region", "0,0,1,1", "--devices", "0"]):
        r = subprocess.run([exe, str(p)] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "Usage" in r.stderr, (bad, r.returncode, r.stderr)
