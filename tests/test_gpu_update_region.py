"""Region update on the GPU (llcomp_mi_update_region, llcomp_mi_codec_encode_region / _update_region, llcomp::updateRegion,
llcompc --update): a rectangle of a container is replaced and only the slices of the tiles it touches are coded again.  The acceptance
rule is one identity: the result is BYTE FOR BYTE the oracle's container of the modified picture.  Old containers come from the oracle,
so nothing here depends on the HIP encoder for its inputs."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, make_image
from test_gpu_region import FAMILIES, Batch, rects

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


def patch_for(img, x, y, rw, rh, seed):
    """new pixels for the rectangle: the upper half a near copy of what was there, the lower half noise"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 256, size=(rh, rw, img.shape[2]), dtype=np.uint8)
    p[: rh // 2] = (img[y:y + rh // 2, x:x + rw].astype(np.int32) + 5).clip(0, 255).astype(np.uint8)
    return p


def pasted(img, x, y, p):
    new = img.copy()
    new[y:y + p.shape[0], x:x + p.shape[1]] = p
    return new


def random_rects(w, h, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        out.append((x, y, int(rng.integers(1, w - x + 1)), int(rng.integers(1, h - y + 1))))
    return out


def check_updates(mi, orc, img, tw, th, planar, rs, small_model=False, verify_decode=True):
    old = orc.compress_sliced(img, tw, th, planar)
    for i, (x, y, rw, rh) in enumerate(rs):
        p = patch_for(img, x, y, rw, rh, seed=i)
        new_img = pasted(img, x, y, p)
        got = mi.update_region(old, x, y, p, device=0)
        assert got == orc.compress_sliced(new_img, tw, th, planar), (x, y, rw, rh)
        if verify_decode:
            assert np.array_equal(mi.decompress_image(got, device=0).pixels, new_img), (x, y, rw, rh)


@pytest.mark.parametrize("case", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_update_equals_full_encode_per_family(mi, orc, case):
    name, w, h, c, tw, th, planar, gen, rect, key = case
    img = make_image(gen, w, h, c)
    k = mi.Codec(1, w, h, c, tw, th, planar, device=0)
    try:
        fam = k.region_family(*rect)
    finally:
        k.close()
    if key:
        assert fam[key], (name, fam)
    check_updates(mi, orc, img, tw, th, planar, rects(w, h, tw, th) + [rect] + random_rects(w, h, 4, seed=w * 7 + h))


# enough tiles in one frame (more than 512 slices above 4096 samples) that the codec itself is on the chunked snapshot pass
CHUNKED = [("chunked_64x64i", 1600, 1408, 3, 64, 64, False, "nat"), ("chunked_128x128p", 2048, 1536, 3, 128, 128, True, "mid")]


@pytest.mark.parametrize("case", CHUNKED, ids=[c[0] for c in CHUNKED])
def test_update_on_the_chunked_snapshot_pass(mi, orc, case):
    name, w, h, c, tw, th, planar, gen = case
    img = make_image(gen, w, h, c)
    k = mi.Codec(1, w, h, c, tw, th, planar, device=0)
    try:
        assert k.family["snapshot"] and tw * th * (1 if planar else c) > 4096 and k.n_slices > 512, k.family
        whole, inner = k.region_family(0, 0, w, h), k.region_family(1, 1, w - 2, h - 2)
        assert whole["snapshot"] and inner["snapshot"], (whole, inner)  # the box is every tile: the codec's own family, chunks and all
        small = k.region_family(w // 3, h // 4, w // 2, h // 2)
    finally:
        k.close()
    assert small["lds_table"], small  # at most 512 big slices: one per wavefront, another family than the codec's
    rs = [(0, 0, w, h), (1, 1, w - 2, h - 2), (w // 3, h // 4, w // 2, h // 2), (tw, th, 3 * tw, 2 * th), (w - 1, h - 1, 1, 1)]
    check_updates(mi, orc, img, tw, th, planar, rs + random_rects(w, h, 2, seed=w))


def test_update_where_the_sub_geometry_switches_family(mi, orc):
    """only the 1-row remainder of 2-row tiles is covered: the sub-geometry clamps tile_h to 1 and the ROW encoder codes it"""
    w, h = 160, 41
    img = make_image("nat", w, h, 3)
    for planar in (True, False):
        k = mi.Codec(1, w, h, 3, 40, 2, planar, device=0)
        try:
            full, fam = k.family, k.region_family(10, 40, 100, 1)
        finally:
            k.close()
        assert not full["rows"] and fam["rows"], (full, fam)
        check_updates(mi, orc, img, 40, 2, planar, [(10, 40, 100, 1), (0, 40, 160, 1), (159, 40, 1, 1), (0, 39, 160, 2)])


def _spans(data):
    n = int.from_bytes(data[20:24], "little")
    lens = np.frombuffer(data[24:24 + 4 * n], dtype="<u4").astype(np.int64)
    return lens, 24 + 4 * n + np.concatenate([[0], np.cumsum(lens)])


def test_aligned_rectangle_never_reads_the_old_slices(mi, orc):
    w, h, tw, th = 512, 256, 32, 32  # 16 x 8 tiles, interleaved: slice id = tile row * 16 + tile column
    img = make_image("nat", w, h, 3)
    good = orc.compress_sliced(img, tw, th, False)
    lens, offs = _spans(good)
    x, y, rw, rh = 96, 64, 64, 64    # tile columns 3..4, tile rows 2..3, exactly
    covered = [ty * 16 + tx for ty in range(2, 4) for tx in range(3, 5)]
    # garbage where the old covered slices were: all ones, and for the first of them a stream with a unary run of 33 ones, which every
    # decoder refuses ("Invalid exponent") -- so the verdict of decoding the box is known, not hoped for
    bad_stream, _ = orc.encode_residuals(np.ones((th, tw, 3), np.int64), run_at=100, run_len=33)
    pieces = [bad_stream if s == covered[0] else b"\xff" * int(lens[s]) if s in covered else good[offs[s]:offs[s + 1]] for s in range(len(lens))]
    old = good[:24] + np.array([len(q) for q in pieces], dtype="<u4").tobytes() + b"".join(pieces)
    assert orc.decompress(old)[0] != 0
    p = patch_for(img, x, y, rw, rh, seed=1)
    got = mi.update_region(old, x, y, p, device=0)
    assert got == orc.compress_sliced(pasted(img, x, y, p), tw, th, False)
    # the same garbage under an unaligned rectangle: the verdict a region decode of the box gives, and the output untouched
    with pytest.raises(mi.LlcompError) as want:
        mi.decompress_region(old, x, y, rw, rh, device=0)
    assert want.value.status in (mi.BAD_EXPONENT, mi.TRUNCATED)
    out = np.full(len(old) + 4096, 0xA5, np.uint8)
    with pytest.raises(mi.LlcompError) as e:
        mi.update_region_into(np.frombuffer(old, np.uint8), out, x + 1, y + 1, p[:-2, :-2], device=0)
    assert e.value.status == want.value.status
    assert (out == 0xA5).all()
    # through a Codec: the decode count does not move for the aligned rectangle, and does for the unaligned one
    import torch

    b = Batch(orc, 2, w, h, 3, tw, th, False, ["nat", "mid"])
    codec = mi.Codec(2, w, h, 3, tw, th, False, device=0)
    st = torch.cuda.current_stream().cuda_stream
    d_rect = torch.from_numpy(np.stack([p, p])).cuda()
    cap = codec.max_payload_bytes
    d_out, d_len = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda"), torch.zeros(codec.n_slices, dtype=torch.int32, device="cuda")
    d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
    codec.get_profile()
    codec.update_region(b.d_pay.data_ptr(), b.total, b.d_len.data_ptr(), x, y, rw, rh, d_rect.data_ptr(), d_out.data_ptr(), cap, d_len.data_ptr(),
                        d_total.data_ptr(), b.d_st.data_ptr(), st)
    torch.cuda.synchronize()
    _, n_enc, n_dec = codec.get_profile()
    assert (n_enc, n_dec) == (1, 0) and int(b.d_st.item()) == 0
    d_small = torch.from_numpy(np.ascontiguousarray(np.stack([p, p])[:, :-2, :-2])).cuda()
    codec.update_region(b.d_pay.data_ptr(), b.total, b.d_len.data_ptr(), x + 1, y + 1, rw - 2, rh - 2, d_small.data_ptr(), d_out.data_ptr(), cap,
                        d_len.data_ptr(), d_total.data_ptr(), b.d_st.data_ptr(), st)
    torch.cuda.synchronize()
    _, n_enc, n_dec = codec.get_profile()
    assert (n_enc, n_dec) == (1, 1) and int(b.d_st.item()) == 0
    codec.close()


def test_damage_outside_the_box_is_carried_over(mi, orc):
    w, h, tw, th = 512, 256, 32, 32
    img = make_image("nat", w, h, 3)
    old = bytearray(orc.compress_sliced(img, tw, th, False))
    lens, offs = _spans(old)
    covered = {ty * 16 + tx for ty in range(2, 4) for tx in range(3, 5)}
    for s in range(len(lens)):
        if s not in covered:
            old[offs[s]:offs[s + 1]] = bytes((s * 7 + i) & 0xFF for i in range(int(lens[s])))
    old = bytes(old)
    x, y, rw, rh = 100, 70, 60, 50  # inside tile columns 3..4, tile rows 2..3: the box is decoded, the damage around it is not
    p = patch_for(img, x, y, rw, rh, seed=2)
    got = mi.update_region(old, x, y, p, device=0)
    want = orc.compress_sliced(pasted(img, x, y, p), tw, th, False)
    nlens, noffs = _spans(got)
    wlens, woffs = _spans(want)
    assert len(nlens) == len(lens)
    for s in range(len(lens)):
        if s in covered:
            assert got[noffs[s]:noffs[s + 1]] == want[woffs[s]:woffs[s + 1]], s
        else:
            assert got[noffs[s]:noffs[s + 1]] == old[offs[s]:offs[s + 1]], s
    assert len(got) == noffs[-1]


def _packed(mi, orc, imgs, tw, th, planar):
    return mi.pack_batch([orc.compress_sliced(f, tw, th, planar) for f in imgs])


@pytest.mark.parametrize("shape", [(100, 37, 3, 32, 16, True), (100, 37, 4, 19, 13, False), (300, 12, 3, 64, 1, True), (90, 40, 5, 32, 8, False),
                                   (320, 160, 3, 64, 64, False)],
                         ids=["planar_tiles", "odd_tiles_c4", "rows", "c5", "tiles_64x64i"])
def test_codec_update_region_batch(mi, orc, shape):
    import torch

    w, h, c, tw, th, planar = shape
    frames, guard = 5, 4096
    b = Batch(orc, frames, w, h, c, tw, th, planar, ["g1", "g3", "mid", "checker", "nat"])
    codec = mi.Codec(frames, w, h, c, tw, th, planar, device=0)
    codec.prepare(update=True)
    st = torch.cuda.current_stream().cuda_stream
    for i, (x, y, rw, rh) in enumerate(rects(w, h, tw, th)[:8] + random_rects(w, h, 3, seed=w + h)):
        ps = np.stack([patch_for(b.imgs[f], x, y, rw, rh, seed=10 * i + f) for f in range(frames)])
        new = np.stack([pasted(b.imgs[f], x, y, ps[f]) for f in range(frames)])
        want_pay, want_len = _packed(mi, orc, new, tw, th, planar)
        d_rect = torch.from_numpy(ps).cuda()
        cap = int(want_pay.size)
        d_out = torch.full((cap + guard,), 0x5A, dtype=torch.uint8, device="cuda")
        d_len = torch.zeros(codec.n_slices, dtype=torch.int32, device="cuda")
        d_total = torch.zeros(1, dtype=torch.int64, device="cuda")
        codec.update_region(b.d_pay.data_ptr(), b.total, b.d_len.data_ptr(), x, y, rw, rh, d_rect.data_ptr(), d_out.data_ptr(), cap,
                            d_len.data_ptr(), d_total.data_ptr(), b.d_st.data_ptr(), st)
        torch.cuda.synchronize()
        assert int(b.d_st.item()) == 0, (x, y, rw, rh)
        host = d_out.cpu().numpy()
        assert int(d_total.item()) == cap and np.array_equal(d_len.cpu().numpy().view(np.uint32), want_len), (x, y, rw, rh)
        assert np.array_equal(host[:cap], want_pay), (x, y, rw, rh)
        assert (host[cap:] == 0x5A).all(), "a byte past the payload was written"
        # one byte short: OVERFLOW, and nothing past the capacity
        d_out.fill_(0x5A)
        codec.update_region(b.d_pay.data_ptr(), b.total, b.d_len.data_ptr(), x, y, rw, rh, d_rect.data_ptr(), d_out.data_ptr(), cap - 1,
                            d_len.data_ptr(), d_total.data_ptr(), b.d_st.data_ptr(), st)
        torch.cuda.synchronize()
        assert codec.status(b.d_st.item()) == mi.OUTPUT_OVERFLOW
        assert (d_out.cpu().numpy()[cap - 1:] == 0x5A).all(), "a byte past the capacity was written"
        # encode_region alone: the sub-containers' slices, frame after frame
        (tx0, ty0, tx1, ty1), n = mi.region_plan(w, h, c, tw, th, planar, x, y, rw, rh)
        box_px = new[:, ty0 * th:min(ty1 * th, h), tx0 * tw:min(tx1 * tw, w)]
        sub_pay, sub_len = _packed(mi, orc, box_px, tw, th, planar)
        scap = int(sub_pay.size)
        d_sub = torch.full((scap + guard,), 0x5A, dtype=torch.uint8, device="cuda")
        d_sub_len = torch.zeros(frames * n, dtype=torch.int32, device="cuda")
        codec.encode_region(b.d_pay.data_ptr(), b.total, b.d_len.data_ptr(), x, y, rw, rh, d_rect.data_ptr(), d_sub.data_ptr(), scap,
                            d_sub_len.data_ptr(), d_total.data_ptr(), b.d_st.data_ptr(), st)
        torch.cuda.synchronize()
        assert int(b.d_st.item()) == 0 and int(d_total.item()) == scap
        host = d_sub.cpu().numpy()
        assert np.array_equal(d_sub_len.cpu().numpy().view(np.uint32), sub_len) and np.array_equal(host[:scap], sub_pay), (x, y, rw, rh)
        assert (host[scap:] == 0x5A).all()
    assert codec.allocated_bytes() <= codec.workspace_bytes
    # a rectangle outside the image: BAD_ARGS before anything is launched or written
    d_out.fill_(0x5A)
    b.d_st.fill_(77)
    with pytest.raises(mi.LlcompError) as e:
        codec.update_region(b.d_pay.data_ptr(), b.total, b.d_len.data_ptr(), w - 1, 0, 2, 1, d_rect.data_ptr(), d_out.data_ptr(), cap,
                            d_len.data_ptr(), d_total.data_ptr(), b.d_st.data_ptr(), st)
    torch.cuda.synchronize()
    assert e.value.status == mi.BAD_ARGS and int(b.d_st.item()) == 77 and (d_out.cpu().numpy() == 0x5A).all()
    # an uncovered slice whose table entry runs past the old payload (the last one, with the payload one byte short): TRUNCATED, and
    # nothing is read or written past either payload
    d_rect = torch.from_numpy(np.ascontiguousarray(ps[:, :1, :1])).cuda()
    codec.update_region(b.d_pay.data_ptr(), b.total - 1, b.d_len.data_ptr(), 0, 0, 1, 1, d_rect.data_ptr(), d_out.data_ptr(), cap + guard,
                        d_len.data_ptr(), d_total.data_ptr(), b.d_st.data_ptr(), st)
    torch.cuda.synchronize()
    assert codec.status(b.d_st.item()) == mi.TRUNCATED
    codec.close()


@pytest.mark.parametrize("hook", [("LLCOMP_MI_NOSNAP", "1"), ("LLCOMP_MI_NOROWS", "1"), ("LLCOMP_MI_OVERLAP", "0"), ("LLCOMP_MI_LANE_SHIFT", "2")],
                         ids=["nosnap", "norows", "overlap0", "lane_shift2"])
def test_hooks_change_no_byte(mi, orc, set_hook, hook):
    set_hook(*hook)
    for (w, h, c, tw, th, planar, gen) in ((800, 420, 3, 32, 32, False, "nat"), (1100, 24, 3, 480, 1, True, "nat"), (1600, 1408, 3, 64, 64, False, "mid")):
        img = make_image(gen, w, h, c)
        rs = [(w // 3, h // 4, w // 2, h // 2), (0, 0, w, h), (1, 1, w - 2, h - 2)]
        check_updates(mi, orc, img, tw, th, planar, rs, verify_decode=False)


def test_small_model_and_legacy(mi, orc):
    img = make_image("mid", 300, 100, 3)
    p = patch_for(img, 10, 20, 200, 50, seed=3)
    new = pasted(img, 10, 20, p)
    other = make_image("g3", 300, 100, 3)
    orc.set_small_model(True)
    try:
        sliced, legacy = orc.compress_sliced(img, 40, 16, True), orc.compress_image(img)
        want_sliced, want_legacy, want_whole = orc.compress_sliced(new, 40, 16, True), orc.compress_image(new), orc.compress_image(other)
    finally:
        orc.set_small_model(False)
    assert mi.update_region(sliced, 10, 20, p, device=0) == want_sliced                       # the header says so
    assert mi.update_region(legacy, 10, 20, p, device=0, small_model=True) == want_legacy     # the caller says so
    assert mi.update_region(legacy, 0, 0, other, device=0, small_model=True) == want_whole    # the whole picture: nothing is decoded
    # a LEGACY stream of the large model: decoded whole, pasted into, encoded whole, a LEGACY stream again
    img2 = make_image("nat", 257, 131, 3)
    legacy2 = orc.compress_image(img2)
    for (x, y, rw, rh) in rects(257, 131, 0, 0)[:6]:
        p2 = patch_for(img2, x, y, rw, rh, seed=x + y)
        got = mi.update_region(legacy2, x, y, p2, device=0)
        assert got == orc.compress_image(pasted(img2, x, y, p2)), (x, y, rw, rh)


def test_update_errors(mi, orc):
    img = make_image("nat", 200, 100, 4)
    old = orc.compress_sliced(img, 32, 32, False)
    p = patch_for(img, 0, 0, 30, 20, seed=4)
    for bad in ((190, 0), (0, 90), (2**32 - 5, 0)):
        with pytest.raises(mi.LlcompError) as e:
            mi.update_region(old, bad[0], bad[1], p, device=0)
        assert e.value.status == mi.BAD_ARGS
    with pytest.raises(mi.LlcompError) as e:
        mi.update_region(old, 0, 0, p[:, :, :3], device=0)  # the patch's channel count is not the container's
    assert e.value.status == mi.BAD_ARGS
    with pytest.raises(mi.LlcompError) as e:
        mi.update_region(old[:30], 0, 0, p, device=0)
    assert e.value.status == mi.TRUNCATED
    want = orc.compress_sliced(pasted(img, 10, 10, p), 32, 32, False)
    out = np.full(len(want) - 1, 0xA5, np.uint8)
    with pytest.raises(mi.LlcompError) as e:
        mi.update_region_into(np.frombuffer(old, np.uint8), out, 10, 10, p, device=0)
    assert e.value.status == mi.OUTPUT_OVERFLOW and e.value.needed == len(want) and (out == 0xA5).all()
    out = np.full(len(want) + 7, 0xA5, np.uint8)
    assert mi.update_region_into(np.frombuffer(old, np.uint8), out, 10, 10, p, device=0) == len(want)
    assert out[:len(want)].tobytes() == want and (out[len(want):] == 0xA5).all()


def test_4k_rgb_in_480x1_planes(mi, orc):
    w, h = 3840, 2160
    img = make_image("nat", w, h, 3)
    old = orc.compress_sliced(img, 480, 1, True)
    for (x, y, rw, rh) in ((1000, 700, 224, 224), (960, 540, 1920, 1080)):
        p = patch_for(img, x, y, rw, rh, seed=rw)
        got = mi.update_region(old, x, y, p, device=0)
        assert got == orc.compress_sliced(pasted(img, x, y, p), 480, 1, True), (x, y, rw, rh)


def _write_ppm(path, px):
    h, w, c = px.shape
    assert c == 3
    path.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + px.tobytes())


def test_llcompc_update(orc, tmp_path):
    """llcompc <patch> --update <container> --at X,Y (llcomp::updateRegion): the rewritten file is the oracle's container"""
    exe = os.path.join(ROOT, "tools", "llcompc")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools")])
    img = make_image("nat", 150, 90, 3)
    p = patch_for(img, 20, 30, 77, 41, seed=5)
    for name, old, want in (("pic.llcomp", orc.compress_sliced(img, 32, 16, True), orc.compress_sliced(pasted(img, 20, 30, p), 32, 16, True)),
                            ("leg.llcomp", orc.compress_image(img), orc.compress_image(pasted(img, 20, 30, p)))):
        f = tmp_path / name
        f.write_bytes(old)
        _write_ppm(tmp_path / "patch.ppm", p)
        r = subprocess.run([exe, str(tmp_path / "patch.ppm"), "--update", str(f), "--at", "20,30"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert f.read_bytes() == want
        assert not (tmp_path / (name + ".tmp")).exists()
    f = tmp_path / "pic.llcomp"
    before = f.read_bytes()
    for bad in (["--update", str(f)], ["--at", "1,2"], ["--update", str(f), "--at", "1"], ["--update", str(f), "--at", "1,2,3"],
                ["--update", str(f), "--at", "1,2", "--sliced", "32x16"], ["--update"]):
        r = subprocess.run([exe, str(tmp_path / "patch.ppm")] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "Usage" in r.stderr, (bad, r.returncode, r.stderr)
    r = subprocess.run([exe, str(tmp_path / "patch.ppm"), "--update", str(f), "--at", "100,60"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Error updating container" in r.stderr  # the rectangle leaves the picture
    _write_ppm(tmp_path / "patch.ppm", p)
    assert f.read_bytes() == before
