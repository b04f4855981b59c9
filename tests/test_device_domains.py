"""The inputs of the whole-domain GPU tests checked without a GPU (tests/device_domains.py, tests/warp_families.py): the sweeps of
test_gpu_photo_domains.py, test_gpu_warp_families.py and test_gpu_mix_domains.py prove something only if their inputs hold what a
named mistake of the device compilation would change.  So: contraction witnesses exist and sit in F and in the frames; the hue factors
give their shift bytes; the ramp views hold all values and their means spread; the white frame's sum of L passes 2^32; the blur's
threshold radii step the box radius and change bytes; the map families are mostly not fill, lie within the limits and hold the
committed contraction vectors; the blend's batches hold a pair that a fused multiply-add changes, a subnormal product and ties.

What the rules themselves make impossible is asserted as such: BRIGHTNESS has no contraction witness (0 + a * v rounds once either
way), no hue factor gives the shift byte 128, no radius within the limit of 32 steps the box radius to 32, and a view of 4096 x 4096
cannot sum L past 2^32 (the white frame is 4352 wide)."""
import numpy as np
import pytest

import device_domains as dd
import photo_spec
import warp_families as wf

F32 = np.float32


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


def test_contraction_witnesses_exist_and_lead_f():
    ws = dd.witnesses()
    assert len(ws) >= 1
    for a, d, v, byte, fused in ws:
        assert int(photo_spec.blend(d, v, a)) == byte != fused == int(dd.blend_fused(d, v, a))
        assert d in dd.CONTRAST_MEANS and 0.0 <= a <= 256.0 and float(F32(a)) == a
        r, g, b = px = dd.colour_of(d, v)
        assert int(photo_spec.luma(np.array([[px]], np.uint8))[0, 0]) == d and v in px
        i = (r << 16) | (g << 8) | b  # ... which the frame of every colour holds at pixel i
        assert tuple(dd.all_colours()[i >> 12, i & 4095]) == px
    assert dd.factors()[:len(ws)] == [w[0] for w in ws]
    # d = 0: the sum 0 + a * v is exact, so the fused and the separate evaluation round the same product once
    assert dd.brightness_has_none()


def test_factor_set():
    f = dd.factors()
    n = len(dd.witnesses())
    assert len(f) == n + 13 + 40 and all(float(F32(a)) == a and 0.0 <= a <= 256.0 for a in f)
    fixed = f[n:n + 13]
    assert fixed[:2] == [0.0, 1.0] and fixed[2] < 1.0 < fixed[3] and fixed[3] - fixed[2] == 2.0 ** -24 + 2.0 ** -23
    assert fixed[4:9] == [0.5, 0.25, 1.5, 2.0, 255 / 256] and fixed[9] == float(F32(1e-8)) and fixed[12] == 256.0
    assert 0.0 < fixed[10] < float(np.finfo(F32).tiny) and fixed[11] == float(F32(100.3))  # 1e-40: a binary32 subnormal
    seeded = f[n + 13:]
    assert all(0.0 <= a <= 2.0 for a in seeded[:20]) and all(2.0 ** -30 <= a <= 256.0 for a in seeded[20:]) and min(seeded[20:]) < 1e-6
    more = dd.more_factors()
    assert len(more) == 512 and len(set(more)) > 500 and all(float(F32(a)) == a and 0.0 <= a <= 256.0 for a in more)


def test_hue_factors_give_their_shift_bytes():
    assert len(dd.SHIFTS) == 255
    for s in dd.SHIFTS:
        f = dd.hue_factor(s)
        assert -0.5 <= f <= 0.5 and float(F32(f)) == f and photo_spec.hue_shift(f) == s
    # the ends of the range truncate to +-127: the byte 128 is no factor's
    assert photo_spec.hue_shift(0.5) == 127 and photo_spec.hue_shift(-0.5) == 129


def test_frames_of_the_pixel_ops():
    assert dd.pair_classes(dd.pairs_frame()).sum() == 256 * 257 // 2  # every (max - min, max) with max - min <= max
    rgb = dd.all_colours()
    assert rgb.shape == (4096, 4096, 3) and tuple(rgb[0x123, 0x456]) == (0x12, 0x34, 0x56)
    # a 512 x 512 rectangle of that frame spans 32 reds: far from every pair
    assert dd.pair_classes(rgb[:512, :512]).sum() < 256 * 257 // 4
    one = dd.all_levels()
    assert one.shape == (4096, 4096, 1) and len(np.unique(one[1024:1040, 2048:2064])) == 256
    assert sorted(dd.tiles()) == sorted((x, y, 1024, 1024) for x in range(0, 4096, 1024) for y in range(0, 4096, 1024))


@pytest.mark.parametrize("c", [1, 3])
def test_ramp_views_and_the_spread_of_their_means(c):
    frame = dd.ramp_frame(c)
    for k in (0, 100, 255):
        assert all(len(np.unique(frame[16 * k:16 * k + 16, :16, ch])) == 256 for ch in range(c))
    means = dd.band_means(c)
    assert min(means) <= 64 and max(means) >= 191 and set(means) >= set(dd.CONTRAST_MEANS)
    todo = dd.contrast_views(c)
    for a in dd.factors():
        assert len({means[k] for k, b in todo if b == a}) >= 4, a
    for (k, a), (wa, d, v, byte, fused) in zip(todo, dd.witnesses()):
        view = frame[16 * k:16 * k + 16]
        out = photo_spec.apply(view, [("contrast", a)])
        assert a == wa and means[k] == d and (view == v).any() and (out[view == v] == byte).all() and byte != fused


@pytest.mark.parametrize("c", [1, 3])
def test_white_frame_sums_past_32_bits(c):
    frame = dd.white_heavy(c)
    total = int(photo_spec.luma(frame).sum())
    assert total > 1 << 32 > 4096 * 4096 * 255
    for ch in range(c):
        hist = np.bincount(frame[..., ch].reshape(-1), minlength=256)
        # autocontrast and equalize have work to do, and the lowest value present is one pixel's
        assert hist[16] == 1 and not hist[:16].any() and (hist > 0).sum() > 200 and (int(hist.sum()) - int(hist[255])) // 255 > 0
        for op in ("autocontrast", "equalize"):
            part = frame[:64, :, ch:ch + 1]
            assert not np.array_equal(photo_spec.apply(part, [op]), part)


def test_blur_thresholds_step_the_box_radius_and_change_bytes():
    th = dd.blur_thresholds()
    assert dd.TOP_R == 31 == len(th) and photo_spec.blur_weights(32.0)[1] == 31  # (no radius within the limit gives 32)
    view = dd.block_frames(1)[0, :24, :24]
    assert set(np.unique(view)) == {0, 255}
    for r, t in zip(range(1, 32), th):
        below = float(np.nextafter(F32(t), F32(0)))
        assert photo_spec.blur_weights(t)[1] == r and photo_spec.blur_weights(below)[1] == r - 1 and 0.0 < below < t <= 32.0
        # adjacent thresholds give different bytes.  (Across one threshold the box is continuous: the two samples at r + 1 fade out
        # as the radius r comes in, so the bytes just below and at a threshold are alike and only the weights' own rounding shows)
        at, before = photo_spec.apply(view, [("gaussian_blur", t)]), photo_spec.apply(view, [("gaussian_blur", th[r - 2] if r > 1 else 0.0)])
        assert (at != before).mean() > 0.1, r
    radii = dd.blur_radii()
    assert len(radii) == 5 * 31 + 64 and all(0.0 <= x <= 32.0 and float(F32(x)) == x for x in radii)


@pytest.mark.parametrize("c", [1, 3, 4])
def test_map_families(mi, orc, c):
    import test_gpu_perspective_views as persp
    import test_gpu_warped_views as warped

    ks, refused = wf.keystones(mi)
    assert len(wf.affine()) == len(ks) == wf.N == 300 and refused == 0  # (a refused draw would have been replaced and counted)
    for members in (wf.affine(), ks):
        sizes = [len(ms) for _, ms in wf.groups(members)]
        assert len(sizes) <= 8 and min(sizes) >= 24
    aff = wf.affine()
    assert all(m[2][:2] == (1.0, 0.0) and m[2][2] == round(m[2][2]) and m[2][5] == round(m[2][5]) for m in aff[::7])
    assert all(m[2][1] == 0.0 == m[2][3] for m in aff[::5]) and any(m[2][0] < 0 for m in aff[::5]) and any(m[3] for m in aff)
    for mod, members, is_persp in ((warped, aff, False), (persp, ks, True)):
        imgs, _ = mod.batch(orc, c, 16, 16, False)
        assert imgs.shape == (wf.FRAMES, wf.H, wf.W, c)
        for name in wf.FILTERS:  # (the keystones' limits: every reference call below would raise outside them)
            assert wf.fill_share(mi, imgs, members, name, is_persp) <= 0.25, (is_persp, name)
        member, name, (x, y), byte, fused = wf.witness(is_persp)
        out = wf.reference(mi, imgs, [member], name, is_persp)
        assert (out[0, y, x] == byte).all() and byte != fused


def test_blend_batches_hold_what_named_mistakes_change():
    import test_gpu_mix_batch

    assert dd.LAM == test_gpu_mix_batch.LAM and dd.LAMBDAS[:5] == [dd.LAM, 0.5, 0.0, 1.0, 2.0 ** -20] and 0.0 < dd.LAMBDAS[5] < 1.0
    for dtype in dd.PARTNERS:
        bits = dd.mix_batch_bits(dtype)
        assert len(dd.PARTNERS[dtype]) == 16 and bits.shape[0] == 32 and (bits[1::2] == bits[1::2, :, :1, :1]).all()
        assert len(np.unique(bits[0])) == (65536 if dtype != "float32" else 256 * 2 * 32)
        nan = dd.is_nan_bits(np.array(dd.PARTNERS[dtype], np.uint32), dtype)
        assert nan.tolist() == [False] * 8 + [True, True] + [False] * 6
    assert dd.widen(np.array(dd.PARTNERS["float16"], np.uint32), "float16")[[2, 4, 10, 11, 12, 13, 14]].tolist() == [
        1.0, 65504.0, 2.0 ** -24, 2.0 ** -14, 1.5 * 2.0 ** -14, 2.0 ** -10, -2.5]
    for dtype in ("bfloat16", "float32"):
        fi = np.finfo(F32)
        top = float(fi.max) if dtype == "float32" else float(np.array([0x7F7F0000], np.uint32).view(F32)[0])
        sub = 2.0 ** -149 if dtype == "float32" else 2.0 ** -133
        assert dd.widen(np.array(dd.PARTNERS[dtype], np.uint32), dtype)[[2, 4, 10, 11, 12, 14]].tolist() == [
            1.0, top, sub, 2.0 ** -126, 1.5 * 2.0 ** -126, -2.5]
    with np.errstate(all="ignore"):
        # float32: a pair whose blend a fused multiply-add changes -- own * w_own + rd(partner * w_partner) rounded once
        own, w_own, a, b = dd.blend_parts("float32", dd.LAM, 15)
        fused, separate = (own * w_own + b).astype(F32), (a + b).astype(F32)
        assert (np.isfinite(separate) & (fused != separate)).sum() > 100
        # float16: a product that is a subnormal and would be flushed, against the partner +0
        own, w_own, a, b = dd.blend_parts("float16", 0.5, 0)
        assert b == 0.0 and ((a != 0) & (np.abs(a) < 2.0 ** -14)).sum() > 1000
        # ties: sums of the two rounded products that lie halfway between two values of the dtype (lam 0.5, partner 1)
        for dtype, low, half in (("float16", 0x1FFF, 0x1000), ("bfloat16", 0xFFFF, 0x8000)):
            own, w_own, a, b = dd.blend_parts(dtype, 0.5, 2)
            s = (a + b).astype(F32)
            exact = np.isfinite(s) & (s.astype(np.float64) == a + b) & (np.abs(s) >= 2.0 ** -14) & (np.abs(s) < 65504.0)
            ties = exact & ((s.view(np.uint32) & low) == half)
            assert ties.sum() > 10, dtype
            up = dd.narrow(s[ties].astype(np.float64), dtype)
            assert ((up > s[ties]).any() and (up < s[ties]).any())  # to even: some up, some down
