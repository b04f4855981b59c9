"""Every decoder family against the oracle on streams no 8-bit image produces (the oracle's orc_encode_residuals): exponents up to 31,
rebuilt samples that wrap int16, unary runs of 32 and more ones ("Invalid exponent"), and damaged payloads whose slice table still
fits.  The expected outcome is always orc.decompress of the same container: its pixels where it decodes, BAD_EXPONENT where it
reports one.  Contents are mixed slice by slice, so the lanes of a wavefront diverge."""
import numpy as np
import pytest

import orc as orc_mod

pytestmark = pytest.mark.gpu

RUNS = (32, 33, 40)


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


@pytest.fixture
def set_hook(mi, monkeypatch):
    """the library reads its LLCOMP_MI_* test hooks once per process: every change is followed by reload_tuning"""
    def _set(name, value):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
        mi.reload_tuning()

    yield _set
    monkeypatch.undo()
    mi.reload_tuning()


def _limit(c, tile_w, tile_h, planar):
    """longest table entry a decoder accepts (llcomp_mi.h, LLCOMP_MI_TRUNCATED)"""
    n = tile_w * tile_h * (1 if planar else c)
    return -(-(13 * n + 16) // 16) * 16


class Geo:
    def __init__(self, w, h, c, tw, th, planar):
        self.w, self.h, self.c, self.tw, self.th, self.planar = w, h, c, tw, th, planar
        self.rects = orc_mod.slice_rects(w, h, c, tw, th, planar)
        self.nch = 1 if planar else c
        self.limit = _limit(c, min(tw, w), min(th, h), planar)

    def payloads(self, orc, rng, small, kinds, bad=None):
        """one stream per slice; kinds[j % len(kinds)] of orc_mod.adversarial_residuals for slice j; bad = (slice, sample, run)"""
        out = []
        orc.set_small_model(small)
        try:
            for j, (_, _, sw, sh, _) in enumerate(self.rects):
                res = orc_mod.adversarial_residuals(rng, sh, sw, self.nch, kinds[(j * 7 + 3) % len(kinds)])
                run = {"run_at": bad[1](sh * sw * self.nch), "run_len": bad[2]} if bad and bad[0] == j else {}
                out.append(orc.encode_residuals(res, **run)[0])
        finally:
            orc.set_small_model(False)
        return out

    def container(self, payloads, small, lens=None, tail=b""):
        lens = [len(p) for p in payloads] if lens is None else lens
        assert max(lens) <= self.limit, "the case must stay within the container's length limit"
        return orc_mod.sliced_container(self.w, self.h, self.c, self.tw, self.th, self.planar, payloads, small, lens) + tail


def _decode_codec(mi, codec, data):
    """a container through Codec.decode -> (status, pixels)"""
    import torch

    n = int.from_bytes(data[20:24], "little")
    lens = np.frombuffer(data[24:24 + 4 * n], dtype="<u4").copy()
    pay = data[24 + 4 * n:]
    d_pay = torch.from_numpy(np.frombuffer(pay + bytes(16), dtype=np.uint8).copy()).cuda()
    d_len = torch.from_numpy(lens.view(np.int32)).cuda()
    d_out = torch.zeros((1, codec.h, codec.w, codec.c), dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    codec.decode(d_pay.data_ptr(), len(pay), d_len.data_ptr(), d_out.data_ptr(), d_st.data_ptr(), st)
    torch.cuda.synchronize()
    return codec.status(int(d_st.item()) & 0xFFFFFFFF), d_out.cpu().numpy()[0]


def _same_as_oracle(orc, status, px, data, what):
    rc, want = orc.decompress(data)
    assert rc in (orc_mod.OK, orc_mod.BAD_EXPONENT), (what, rc)
    assert status == rc, (what, status, rc)
    if rc == orc_mod.OK:
        assert np.array_equal(px, want), what
    return rc


def _cases(orc, geo, rng, small, group_width):
    """(name, container) of every content case for one geometry"""
    n = len(geo.rects)
    mix = ["small", "sparse", "wrap", "sparse", "small", "ex31"]
    yield "mixed", geo.container(geo.payloads(orc, rng, small, mix), small)
    yield "ex31_first", geo.container(geo.payloads(orc, rng, small, ["ex31"]), small)
    gw = min(group_width, n)
    for ji, j in enumerate((0, gw // 2, gw - 1)):
        for ki, at in enumerate((lambda m: 0, lambda m: m // 2, lambda m: m - 1)):
            run = RUNS[(ji + ki) % 3]
            yield "run%d_slice%d_at%d" % (run, j, ki), geo.container(geo.payloads(orc, rng, small, mix, bad=(j, at, run)), small)
    base = geo.payloads(orc, rng, small, mix)
    j = n // 2
    p = list(base)
    b = bytearray(p[j])
    lo = len(b) // 3
    b[lo:lo + max(1, len(b) // 3)] = rng.integers(0, 256, size=len(b[lo:lo + max(1, len(b) // 3)]), dtype=np.uint8).tobytes()
    p[j] = bytes(b)
    yield "random_bytes", geo.container(p, small)
    for fill in (0x00, 0xFF):
        p = list(base)
        b = bytearray(p[j])
        b[2:] = bytes([fill]) * (len(b) - 2)
        p[j] = bytes(b)
        yield "run_of_%02x" % fill, geo.container(p, small)
    if n > 1:
        lens = [len(x) for x in base]
        k = min(n - 2, j)
        d = min(5, lens[k + 1])
        lens[k] += d
        lens[k + 1] -= d
        yield "moved_bytes", geo.container(base, small, lens=lens)
    yield "trailing_bytes", geo.container(base, small, tail=rng.integers(0, 256, size=97, dtype=np.uint8).tobytes())


# name, (w, h, c, tile_w, tile_h, planar), hooks, what Codec.family must say
FAMILIES = [
    *[("rows_c%d%s" % (c, "p" if p else "i"), (72, 20, c, 36 if c % 2 else 72, 1, p), {}, {"rows": True}) for c in (1, 2, 3, 4) for p in (False, True)],
    ("hbm_cache_s6", (96, 64, 3, 8, 8, False), {"LLCOMP_MI_LANE_SHIFT": "6"}, {"rows": False, "lds_table": False, "bank_cache": True, "lane_shift": 6}),
    ("hbm_cache_s3", (96, 64, 2, 8, 8, True), {"LLCOMP_MI_LANE_SHIFT": "3"}, {"rows": False, "lds_table": False, "bank_cache": True, "lane_shift": 3}),
    ("hbm_plain_s6", (96, 64, 4, 8, 8, False), {"LLCOMP_MI_LANE_SHIFT": "6", "LLCOMP_MI_NOCACHE": "1"},
     {"rows": False, "lds_table": False, "bank_cache": False, "lane_shift": 6}),
    ("hbm_plain_s3", (96, 64, 1, 8, 8, False), {"LLCOMP_MI_LANE_SHIFT": "3", "LLCOMP_MI_NOCACHE": "1"},
     {"rows": False, "lds_table": False, "bank_cache": False, "lane_shift": 3}),
    ("lds_table", (160, 48, 3, 80, 24, False), {}, {"rows": False, "lds_table": True}),
    ("lds_table_off", (160, 48, 3, 80, 24, False), {"LLCOMP_MI_NOLDSTAB": "1"}, {"rows": False, "lds_table": False}),
    ("generic_c5", (64, 40, 5, 8, 8, False), {"LLCOMP_MI_LANE_SHIFT": "6"}, {"rows": False, "lds_table": False, "bank_cache": False}),
    ("generic_c7", (48, 24, 7, 8, 6, False), {"LLCOMP_MI_LANE_SHIFT": "3"}, {"rows": False, "lds_table": False, "bank_cache": False}),
]
HOOKS = ("LLCOMP_MI_LANE_SHIFT", "LLCOMP_MI_NOCACHE", "LLCOMP_MI_NOLDSTAB", "LLCOMP_MI_FORCE_REPLAY")


@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f[0])
def test_every_family_decodes_like_the_oracle(mi, orc, set_hook, fam):
    import zlib

    name, shape, hooks, expect = fam
    geo = Geo(*shape)
    seen = {}
    for small in (False, True):
        for force in ("0", "1"):
            for h in HOOKS:
                set_hook(h, hooks.get(h))
            set_hook("LLCOMP_MI_FORCE_REPLAY", force)
            rng = np.random.default_rng(zlib.crc32(name.encode()) + 2 * small)
            codec = mi.Codec(1, geo.w, geo.h, geo.c, geo.tw, geo.th, geo.planar, small_model=small)
            try:
                for key, val in expect.items():
                    assert codec.family[key] == val, (name, key, codec.family)
                codec.counters(reset=True)
                for case, data in _cases(orc, geo, rng, small, 1 << codec.family["lane_shift"]):
                    status, px = _decode_codec(mi, codec, data)
                    rc = _same_as_oracle(orc, status, px, data, (name, case, small, force))
                    seen[rc] = seen.get(rc, 0) + 1
                    if case in ("mixed", "ex31_first") and force == "0":
                        assert codec.counters()["dec_replays"] > 0, (name, case, "exponent-heavy content must go through the checked replay")
            finally:
                codec.close()
    assert seen.get(orc_mod.OK) and seen.get(orc_mod.BAD_EXPONENT), seen


@pytest.mark.parametrize("noldstab", ["0", "1"])
def test_legacy_adversarial_streams_decode_like_the_oracle(mi, orc, set_hook, noldstab):
    set_hook("LLCOMP_MI_NOLDSTAB", noldstab)
    rng = np.random.default_rng(31 + int(noldstab))
    for force in ("0", "1"):
        set_hook("LLCOMP_MI_FORCE_REPLAY", force)
        for small in (False, True):
            for i, kind in enumerate(("sparse", "wrap", "ex31", "sparse")):
                c = (1, 3, 4, 5)[i]
                w, h = int(rng.integers(8, 60)), int(rng.integers(2, 30))
                fam = mi.Codec(1, w, h, c, w, h, False, small_model=small).family
                assert fam["lds_table"] == (noldstab == "0"), fam
                run = {"run_at": int(rng.integers(0, w * h * c)), "run_len": RUNS[i % 3]} if i == 3 else {}
                orc.set_small_model(small)
                try:
                    stream, _ = orc.encode_residuals(orc_mod.adversarial_residuals(rng, h, w, c, kind), **run)
                    data = orc_mod.legacy_stream(w, h, c, stream)
                    rc, want = orc.decompress(data)
                finally:
                    orc.set_small_model(False)
                if rc == orc_mod.OK:
                    assert np.array_equal(mi.decompress_image(data, small_model=small).pixels, want)
                else:
                    assert rc == orc_mod.BAD_EXPONENT
                    with pytest.raises(mi.LlcompError) as e:
                        mi.decompress_image(data, small_model=small)
                    assert e.value.status == mi.BAD_EXPONENT


@pytest.mark.parametrize("shape", [(1, 1, 3), (2, 2, 3), (5, 3, 4)])
def test_legacy_streams_with_trailing_bytes_decode_exactly(mi, orc, shape, tmp_path):
    """A LEGACY stream is whatever follows its header: the reference reads what the samples need and ignores the rest"""
    import os
    import subprocess

    w, h, c = shape
    rng = np.random.default_rng(w * h)
    img = rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)
    good = orc.compress_image(img)
    over_limit = False
    for tail in (bytes(300), b"\xff" * 300, rng.integers(0, 256, size=400, dtype=np.uint8).tobytes(), b"\xff" * (65 * w * h * c + 40)):
        data = good + tail
        over_limit |= len(data) - 6 > _limit(c, w, h, False)
        rc, want = orc.decompress(data)
        assert rc == orc_mod.OK
        if not any(tail):  # (zeros are what a decoder reads past the end; other bytes may change the last samples, in the reference too)
            assert np.array_equal(want, img)
        assert np.array_equal(mi.decompress_image(data).pixels, want)
        assert np.array_equal(mi.decompress_image(data, devices=[0, 0, 0]).pixels, want)
        assert np.array_equal(mi.decompress_region(data, 0, 0, w, h).pixels, want)
        if w > 1:
            assert np.array_equal(mi.decompress_region(data, 1, 0, w - 1, h).pixels, want[:, 1:])
    assert over_limit, "some stream must be longer than a sliced entry may be"
    # the CLI: the padded stream gives the same picture file as the stream alone
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    llcompd = os.path.join(root, "tools", "llcompd")
    if not os.path.exists(llcompd):
        subprocess.check_call(["make", "-C", os.path.join(root, "tools")])
    pics = []
    for name, data in (("plain", good), ("padded", good + bytes(300))):
        src = tmp_path / (name + ".llcomp")
        src.write_bytes(data)
        assert subprocess.run([llcompd, str(src)], timeout=120).returncode == 0
        pics.append((tmp_path / (name + ".llcomp.png")).read_bytes())
    assert pics[0] == pics[1]


def test_sliced_entries_at_the_limit_decode_and_beyond_it_are_truncated(mi, orc):
    geo = Geo(48, 24, 3, 8, 8, False)
    rng = np.random.default_rng(5)
    pays = geo.payloads(orc, rng, False, ["sparse", "small"])
    j = 7  # a full interior tile
    lim = geo.limit
    at = list(pays)
    at[j] = at[j] + bytes(lim - len(at[j]))  # zero padding behind a stream is never read
    data = geo.container(at, False)
    rc, want = orc.decompress(data)
    assert rc == orc_mod.OK
    assert np.array_equal(mi.decompress_image(data).pixels, want)
    over = list(at)
    over[j] = over[j] + b"\0"
    data = orc_mod.sliced_container(geo.w, geo.h, geo.c, geo.tw, geo.th, geo.planar, over)
    assert orc.decompress(data)[0] == orc_mod.OK  # (the oracle has no such rule: the container is this project's own)
    with pytest.raises(mi.LlcompError) as e:
        mi.decompress_image(data)
    assert e.value.status == mi.TRUNCATED


def _crop_from_covered(orc, geo, data, x, y, rw, rh):
    """the oracle's pixels of a rectangle from the slices of the tiles it covers alone"""
    n = len(geo.rects)
    lens = np.frombuffer(data[24:24 + 4 * n], dtype="<u4").astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]) + 24 + 4 * n
    s = np.zeros((geo.h, geo.w, geo.c), np.int16)
    for j, (x0, y0, sw, sh, k) in enumerate(geo.rects):
        if x0 + sw <= x or x0 >= x + rw or y0 + sh <= y or y0 >= y + rh:
            continue
        rc, part = orc.decode_samples(data[offs[j]:offs[j + 1]], sw, sh, geo.nch)
        assert rc == orc_mod.OK
        if k is None:
            s[y0:y0 + sh, x0:x0 + sw] = part
        else:
            s[y0:y0 + sh, x0:x0 + sw, k] = part[:, :, 0]
    return orc.inverse_rct(np.ascontiguousarray(s[y:y + rh, x:x + rw]))


def test_region_decode_of_adversarial_containers(mi, orc):
    geo = Geo(96, 48, 3, 16, 8, True)
    rng = np.random.default_rng(9)
    mix = ["small", "sparse", "wrap", "ex31"]
    x, y, rw, rh = 20, 10, 30, 12  # tiles 1..3 x 1..2
    bad_out = [i for i, r in enumerate(geo.rects) if r[0] >= 64 and r[1] >= 24][0]
    bad_in = [i for i, r in enumerate(geo.rects) if r[0] == 32 and r[1] == 8][0]
    for j, want_rc in ((bad_out, mi.OK), (bad_in, mi.BAD_EXPONENT)):
        data = geo.container(geo.payloads(orc, rng, False, mix, bad=(j, lambda m: m // 2, 33)), False)
        assert orc.decompress(data)[0] == orc_mod.BAD_EXPONENT
        if want_rc == mi.OK:
            got = mi.decompress_region(data, x, y, rw, rh).pixels
            assert np.array_equal(got, _crop_from_covered(orc, geo, data, x, y, rw, rh))
        else:
            with pytest.raises(mi.LlcompError) as e:
                mi.decompress_region(data, x, y, rw, rh)
            assert e.value.status == mi.BAD_EXPONENT


def test_batch_decode_of_forged_frames(mi, orc):
    import torch

    geo = Geo(64, 32, 3, 8, 8, False)
    rng = np.random.default_rng(11)
    mix = ["small", "sparse", "wrap", "ex31"]
    frames = [geo.container(geo.payloads(orc, rng, False, mix), False) for _ in range(3)]
    bad = geo.container(geo.payloads(orc, rng, False, mix, bad=(5, lambda m: m - 1, 32)), False)
    codec = mi.Codec(3, geo.w, geo.h, geo.c, geo.tw, geo.th, geo.planar)
    n = len(geo.rects)
    st = torch.cuda.current_stream().cuda_stream
    try:
        for batch, ok in ((frames, True), ([frames[0], bad, frames[2]], False)):
            lens = np.concatenate([np.frombuffer(f[24:24 + 4 * n], dtype="<u4") for f in batch])
            pay = b"".join(f[24 + 4 * n:] for f in batch)
            d_pay = torch.from_numpy(np.frombuffer(pay + bytes(16), dtype=np.uint8).copy()).cuda()
            d_len = torch.from_numpy(lens.view(np.int32).copy()).cuda()
            d_out = torch.zeros((3, geo.h, geo.w, geo.c), dtype=torch.uint8, device="cuda")
            d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
            codec.decode(d_pay.data_ptr(), len(pay), d_len.data_ptr(), d_out.data_ptr(), d_st.data_ptr(), st)
            torch.cuda.synchronize()
            status = codec.status(int(d_st.item()) & 0xFFFFFFFF)
            if ok:
                assert status == mi.OK
                out = d_out.cpu().numpy()
                for f in range(3):
                    rc, want = orc.decompress(batch[f])
                    assert rc == orc_mod.OK and np.array_equal(out[f], want)
            else:
                assert status == mi.BAD_EXPONENT
    finally:
        codec.close()


def test_device_list_decode_of_forged_containers(mi, orc):
    geo = Geo(64, 48, 3, 16, 4, True)
    rng = np.random.default_rng(13)
    mix = ["small", "sparse", "wrap", "ex31"]
    data = geo.container(geo.payloads(orc, rng, False, mix), False)
    rc, want = orc.decompress(data)
    assert rc == orc_mod.OK
    assert np.array_equal(mi.decompress_image(data, devices=[0, 0, 0]).pixels, want)
    bad = geo.container(geo.payloads(orc, rng, False, mix, bad=(len(geo.rects) - 2, lambda m: m // 2, 40)), False)
    assert orc.decompress(bad)[0] == orc_mod.BAD_EXPONENT
    out = np.full(geo.w * geo.h * geo.c, 0xA5, dtype=np.uint8)
    with pytest.raises(mi.LlcompError) as e:
        mi.decompress_image_into(np.frombuffer(bad, dtype=np.uint8).copy(), out, devices=[0, 0, 0])
    assert e.value.status == mi.BAD_EXPONENT
    assert (out == 0xA5).all(), "a failed device-list decode writes nothing"


def test_stream_pipeline_reports_a_bad_job_and_decodes_the_next(mi, orc):
    geo = Geo(64, 16, 3, 64, 1, True)
    rng = np.random.default_rng(17)
    mix = ["small", "sparse", "wrap", "ex31"]
    bad = geo.container(geo.payloads(orc, rng, False, mix, bad=(3, lambda m: 0, 32)), False)
    good = geo.container(geo.payloads(orc, rng, False, mix), False)
    rc, want = orc.decompress(good)
    assert rc == orc_mod.OK and orc.decompress(bad)[0] == orc_mod.BAD_EXPONENT
    st = mi.Stream(geo.w, geo.h, geo.c, geo.tw, geo.th, geo.planar, depth=2, device=0)
    try:
        for data, want_status in ((bad, mi.BAD_EXPONENT), (good, mi.OK)):
            buf = np.frombuffer(data, dtype=np.uint8).copy()
            assert st.submit_decode(buf)
            job = st.wait()
            assert job.status == want_status
            if want_status == mi.OK:
                assert np.array_equal(job.data, want)
            st.release(job)
    finally:
        st.close()
