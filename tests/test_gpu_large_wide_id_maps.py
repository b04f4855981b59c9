"""The calls on id maps of 3 and 4 bytes per pixel (include/llcomp_mi.h: "Wide id maps") on batches and samples past 2^31 pixels and
2^32 bytes: paste_batch32, label_boxes32 and label_targets32, with the machinery and the rules of tests/test_gpu_large_batches.py.  A
3-byte map passes 2^32 bytes at 1.43 G pixels, a 4-byte map at 1.07 G, and 2^33 bytes inside one sample; a sample of 517 x 389 3-byte
pixels is 603339 bytes, odd, so the samples of a batch start at every residue modulo 16 and a pixel may straddle byte 2^31 or 2^32.

Nothing expected comes from the library: the numpy specs of the small wide tests (boxes_spec, wide_maps, ids_of, index_spec, value_spec,
apply32) on bank entries and on the active samples, closed forms, and the torch formulations of tests/large_wide_formulations.py, which
tests/test_large_wide_formulations.py checks against those specs on the CPU.  Every byte is compared, guards of 256 bytes of 0x5A
included, and every input against a clone from before the call.  3-byte maps lie 3 bytes past a 256-byte boundary, 4-byte maps 4 or 12.

Leg A: many samples, the batch past 2^32 bytes.  Leg B: one sample whose inner offsets pass the marks -- 46342 x 46343 pixels (more
than 2^31; 6.4 GB and 8.6 GB), 65537 x 65535 3-byte pixels (2^32 - 1; two samples of 12.9 GB) and 38000 x 38000 x 3 bytes under maps of
both widths.  profiles/large_batches.txt keeps a run's lines and what a truncated offset would trip in each wide code path."""
import numpy as np
import pytest

import large_wide_formulations as F
from test_gpu_large_batches import (DEV, IH, IW, LH, LW, M31, M32, OH, OW, PIECE, Held, _stream, _sync, active_set, assert_banked, assert_same, bank_lists,
                                    banked, body_of, closed_form, get_samples, localise, mi, past, pieces_between, put_samples, records, run_leg,  # noqa: F401
                                    straddlers, to_dev)
from test_wide_id_maps_rule import HIGH_BYTES, TOP, blobs, boxes_spec, ids_of, wide_maps

pytestmark = pytest.mark.gpu

M33, M34 = 1 << 33, 1 << 34
LP = LH * LW
STRADDLING = {3: (3559, 7118), 4: (2669, 5338)}  # the samples of LP pixels that hold bytes 2^31 and 2^32 of a batch
ONE_PIXEL = (0x123456, 0x123457, 0x563412, 0x000100)  # ids of one pixel, at the corners of bank entries 2 and 5


def bank_of(rng, mb):
    """7 maps of LH x LW ids of HIGH_BYTES[mb] -- ids that differ in the high byte only, 0 and the top id -- with one-pixel ids at the
    corners, and per entry a list of ids: some the map has, some it has not, of several lengths, entry 3 empty"""
    bank = blobs(rng, 7, LH, LW, HIGH_BYTES[mb])
    bank[2, 0, 0], bank[2, LH - 1, LW - 1], bank[5, LH - 1, 0], bank[5, 0, LW - 1] = ONE_PIXEL
    bank[6, 5:9, 7:30] = TOP[mb]
    lists = bank_lists(rng, bank, TOP[mb] + 1)
    lists[2], lists[5] = sorted(set(lists[2]) | set(ONE_PIXEL[:2])), sorted(set(lists[5]) | set(ONE_PIXEL[2:]))
    lists[6] = sorted(set(lists[6]) | {0, TOP[mb]})  # (the top id is listed and has pixels)
    assert len({len(l) for l in lists}) > 3 and lists[3] == [] and max(max(l) for l in lists if l) == TOP[mb]
    return bank, lists


def many_maps(mb, n, bank, offset):
    """n maps of mb bytes per pixel in device memory, map i bank entry i % 7 -> (held, its clone)"""
    S = LP * mb
    assert straddlers(n, S) == STRADDLING[mb] and all(b % 7 for b in STRADDLING[mb])  # (a straddling sample is not bank entry 0 again)
    maps = Held(n * S, offset, value=0)
    banked(maps, to_dev(wide_maps(bank, mb)), n, S)
    return maps, maps.buf.clone()


# ---- leg A: many samples, the batch past 2^32 bytes ------------------------------------------------------------------------------
def boxes32_many(mi, codec, mb, offset):
    S = LP * mb
    n = past(S)
    rng = np.random.default_rng(70 + mb)
    bank, lists = bank_of(rng, mb)
    maps, before = many_maps(mb, n, bank, offset)
    tables = [boxes_spec(bank[k:k + 1], lists[k:k + 1]) for k in range(7)]
    assert all(t[:, 0].any() for t in tables if len(t)), "every list names an id that has pixels"
    assert all((tables[k][[lists[k].index(m) for m in ONE_PIXEL[j:j + 2]], 0] == 1).all() for k, j in ((2, 0), (5, 2))), "the ids of one pixel"
    per = [records(t).reshape(-1) for t in tables]
    want = np.concatenate([per[i % 7] for i in range(n)])
    out = Held(want.size, 12)
    codec.label_boxes32(maps.ptr, mb, n, LW, LH, [lists[i % 7] for i in range(n)], out.ptr, stream=_stream())
    _sync()
    got = out.buf.cpu().numpy()
    assert (got[:out.lo] == 0x5A).all() and (got[out.lo + want.size:] == 0x5A).all(), f"label_boxes32 mb {mb}: a guard byte was written"
    bad = np.flatnonzero(got[out.lo:out.lo + want.size] != want)
    assert not bad.size, f"label_boxes32 mb {mb}: record {bad[0] // 20} differs"
    assert_same(maps.buf, before, maps, f"label_boxes32 mb {mb}, maps", S)
    assert codec.allocated_bytes() <= codec.label_boxes32_workspace_bytes(n, want.size // 20)


def test_a_label_boxes32_3_bytes(mi):
    run_leg(mi, "A_boxes32_mb3", 2 * past(LP * 3) * LP * 3 + (1 << 26), lambda codec, leg: boxes32_many(mi, codec, 3, 3))


def test_a_label_boxes32_4_bytes(mi):
    run_leg(mi, "A_boxes32_mb4", 2 * past(LP * 4) * LP * 4 + (1 << 26), lambda codec, leg: boxes32_many(mi, codec, 4, 12))


def index32_many(mi, codec, mb, dtype, n, offset):
    from test_label_targets import index_spec

    es = np.dtype(dtype).itemsize
    Sm, So = LP * mb, LP * es
    if es == 8:  # maps and output pass 2^32 bytes, the output 2^33 and 2^34 too
        assert n * So > M34 and all((m // So) % 7 for m in (M31, M32, M33, M34)) and straddlers(n, So)
    else:  # the maps alone: the leg isolates the map addresses
        assert n * Sm > M32 and n * So < M31
    rng = np.random.default_rng(80 + mb)
    bank, lists = bank_of(rng, mb)
    values = [rng.integers(0, 255, size=len(l)).tolist() if es == 1 else rng.integers(-100, 1 << 20, size=len(l)).tolist() for l in lists]
    default = 255 if es == 1 else -100
    want = index_spec(bank, lists, values, default, dtype)
    assert all((want[k] != default).any() for k in range(7) if lists[k])
    maps, before = many_maps(mb, n, bank, offset)
    out = Held(n * So, 3 * es)
    codec.label_targets32(maps.ptr, mb, n, LW, LH, [lists[i % 7] for i in range(n)], [values[i % 7] for i in range(n)], out.ptr, dtype=dtype, default=default,
                          stream=_stream())
    _sync()
    assert_banked(out, to_dev(want), n, So, f"label_targets32 mb {mb} index {dtype}")
    assert_same(maps.buf, before, maps, f"label_targets32 mb {mb}, maps", Sm)
    assert codec.allocated_bytes() <= codec.label_targets32_workspace_bytes(n, sum(len(lists[i % 7]) for i in range(n)))


def test_a_label_targets32_index_3_bytes_to_int64(mi):
    """maps past 2^32 bytes and an int64 output past 2^34: past(LP * 3) = 7143 samples write 11.5 GB, which passes 2^33 only, so the
    leg takes the 10702 samples at which the output passes 2^34 (the maps: 6.5 GB)"""
    n = M34 // (LP * 8) + 25
    assert n == 10702 > past(LP * 3)
    run_leg(mi, "A_targets32_index_mb3_i64", n * LP * (3 + 3 + 8), lambda codec, leg: index32_many(mi, codec, 3, "int64", n, 3))


def test_a_label_targets32_index_4_bytes_to_uint8(mi):
    n = past(LP * 4)
    run_leg(mi, "A_targets32_index_mb4_u8", n * LP * (4 + 4 + 1), lambda codec, leg: index32_many(mi, codec, 4, "uint8", n, 4))


ON_OFF = {"on": 0.9, "off": 0.05, "bits": (0x3B33, 0x2A66)}  # float16 patterns that differ in both bytes


def planes32_many(mi, codec, oh, ow, n, planes):
    import torch

    from test_label_targets import value_spec

    P, es = oh * ow, 2
    assert n * planes * P * es > M33 and planes == mi.label_targets_max_planes()
    assert np.array_equal(np.array([ON_OFF["on"], ON_OFF["off"]], np.float16).view(np.uint16), ON_OFF["bits"])
    rng = np.random.default_rng(87)
    extra = np.setdiff1d(np.unique(rng.integers(0, TOP[3] + 1, size=80)), HIGH_BYTES[3])[:60 - len(HIGH_BYTES[3])]
    pool = np.array(sorted(set(HIGH_BYTES[3]) | set(extra.tolist())), np.int64)
    assert len(pool) == 60 and pool[-1] == TOP[3]
    ids = pool[rng.integers(0, 60, size=(n, oh, ow))]  # every id in every map, pixel by pixel
    lists = [pool[0:50].tolist(), pool[5:60].tolist(), pool[0:60:2].tolist()][:n]
    values = [rng.integers(-1, planes + 2, size=len(l)).tolist() for l in lists]
    marked = []
    for m in (M31, M32, M33):  # the planes around the marks of the output take pixels
        i, k = divmod(m // (P * es), planes)
        assert i < n and 0 < k < planes - 1
        for d in (-1, 0, 1):
            values[i][(k + d) % len(values[i])] = k + d
            marked.append((i, k + d))
    default = planes // 2
    vh = value_spec(ids, lists, values, default)
    assert all((vh[i] == k).any() for i, k in marked)
    vm = torch.from_numpy(vh.reshape(n, P)).to(DEV)
    maps, out = Held(n * P * 3, 3, value=0), Held(n * planes * P * es, 3 * es)
    put_samples(maps.buf, maps, range(n), P * 3, wide_maps(ids, 3))
    before = maps.buf.clone()
    codec.label_targets32(maps.ptr, 3, n, ow, oh, lists, values, out.ptr, kind="planes", dtype="float16", default=default, planes=planes, on=ON_OFF["on"],
                          off=ON_OFF["off"], stream=_stream())
    _sync()
    ov = out.body.view(torch.int16).view(n, planes, P)
    on, off = (torch.tensor(b, dtype=torch.int16, device=DEV) for b in ON_OFF["bits"])
    step = max(1, PIECE // (2 * P))
    ons = 0
    for i in range(n):
        for a in range(0, planes, step):
            b = min(planes, a + step)
            hit = vm[i][None] == torch.arange(a, b, device=DEV)[:, None]
            ons += int(hit.sum())
            assert torch.equal(ov[i, a:b], torch.where(hit, on, off)), f"label_targets32 planes: sample {i}, planes {a}..{b - 1}"
    assert ons > n * P // 2
    assert bool((out.buf[:out.lo] == 0x5A).all()) and bool((out.buf[out.lo + out.nbytes:] == 0x5A).all()), "label_targets32 planes: a guard byte was written"
    assert_same(maps.buf, before, maps, "label_targets32 planes, maps", P * 3)
    assert codec.allocated_bytes() <= codec.label_targets32_workspace_bytes(n, sum(len(l) for l in lists))


def test_a_label_targets32_planes_3_bytes_float16(mi):
    run_leg(mi, "A_targets32_planes_mb3", 3 * 4096 * 800 * 450 * 2 + (1 << 30), lambda codec, leg: planes32_many(mi, codec, 450, 800, 3, 4096))


def paste_pool(mb):
    """ids inside and beside the windows of paste_windows"""
    top = TOP[mb]
    pool = [0, 1, 5, 255, 256, 0x00FF00, 0x00FF80, 0x00FFFF, 0x010000, 0xFF0001, 0xFF0100, 0xFF0101, top - 101, top - 100, top - 1, top, 0x010001, 0x123456]
    return np.array(pool + ([0x7FFFFFFF, 0x80000000, 0x80000005, 0x800000FF, 0x80000100, 0x01000001] if mb == 4 else []), np.int64)


def paste_windows(rng, mb):
    """windows at bases 0, 0x00FF00, 0xFF0001 and TOP - 100, which passes the top id; for 4 bytes one at a base above 2^31 - 1"""
    from test_wide_id_paste_rule import Window, select

    wins = [Window(b, rng.integers(0, 3, size=256) > 0) for b in [0, 0x00FF00, 0xFF0001, TOP[mb] - 100] + ([0x80000000] if mb == 4 else [])]
    pool = paste_pool(mb)
    assert all(0 < select(pool, w).sum() < len(pool) for w in wins) and wins[3].base + 255 > TOP[mb]
    return wins


def paste32_many(mi, codec, mb):
    from batch_support import bits_of
    from test_wide_id_paste_rule import apply32, window_array

    dtype, layout, c, es, np_t = ("uint8", "hwc", 3, 1, np.uint8) if mb == 3 else ("float16", "chw", 1, 2, np.float16)
    own_mask = mb == 4
    Ss, Sd, Sm = IH * IW * c * es, OH * OW * c * es, IH * IW * mb
    s_shape, d_shape = ((c, IH, IW), (c, OH, OW)) if layout == "chw" else ((IH, IW, c), (OH, OW, c))
    m_np, m_shape = (np.uint8, (IH, IW, 3)) if mb == 3 else (np.uint32, (IH, IW))
    n_src, n_dst = past(Ss), past(Sd)
    act_d = active_set(n_dst, *straddlers(n_dst, Sd))
    rounds = [active_set(n_src, *straddlers(n_src, Ss))]
    src, dst = Held(n_src * Ss, 3 if mb == 3 else 6, seed=91), Held(n_dst * Sd, 5 * es, seed=92)
    if own_mask:  # the map batch is twice the src batch: the samples at its bytes 2^31 and 2^32 get a call of their own
        mask = Held(n_src * Sm, 12, seed=93)
        rounds.append(active_set(n_src, *straddlers(n_src, Sm)))
        assert n_src * Sm > M33 and M33 // Sm == rounds[0][5]  # (byte 2^33 of the maps lies in the sample that holds byte 2^32 of src)
    else:
        mask = src
        assert Sm == Ss
    rng = np.random.default_rng(94)
    wins = paste_windows(rng, mb)
    every = sorted(set(sum(rounds, [])))  # the active src samples alone hold ids of the pool, the others noise
    pool = paste_pool(mb)
    put_samples(mask.buf, mask, every, Sm, wide_maps(pool[rng.integers(0, len(pool), size=(len(every), IH, IW))], mb))
    src_before, mask_before, want = src.buf.clone(), (mask.buf.clone() if own_mask else None), dst.buf.clone()
    for r, act_s in enumerate(rounds):
        pieces = [p + (wins[(k + r) % len(wins)],) for k, p in enumerate(pieces_between(act_s, act_d, IW, IH, OW, OH))]
        pieces.append((act_d[6], act_s[1], 40, 50, 30, 20, 90, 70, wins[2], 0xC7 if es == 1 else 0xFC01))  # a VALUE piece
        if mb == 3:  # VALUE_PIXEL pieces, on dst samples b32 + 1 and n - 1
            pieces.append((act_d[6], act_s[2], 100, 120, 50, 60, 80, 60, wins[0], 0xC0B0A1, True))
            pieces.append((act_d[7], act_s[6], 3, OH - 61, 5, IH - 61, 120, 61, wins[3], 0x0102FE, True))
        arr = window_array(mi, pieces)
        codec.paste_batch32(src.ptr, mask.ptr, mb, n_src, IW, IH, dst.ptr, n_dst, OW, OH, arr, dtype=dtype, layout=layout, stream=_stream())
        _sync()
        s_sub, d_sub = get_samples(src_before, src, act_s, Ss, np_t, s_shape), get_samples(want, dst, act_d, Sd, np_t, d_shape)
        i_sub = ids_of(get_samples(mask_before if own_mask else src_before, mask, act_s, Sm, m_np, m_shape))
        assert np.isin(i_sub, pool).all()
        exp = apply32(s_sub, i_sub, d_sub, localise(pieces, act_s, act_d), layout)
        assert all(not np.array_equal(bits_of(exp[k]), bits_of(d_sub[k])) for k in range(8))
        put_samples(want, dst, act_d, Sd, exp)
        assert_same(dst.buf, want, dst, f"paste_batch32 mb {mb} call {r}, dst", Sd)
        assert_same(src.buf, src_before, src, f"paste_batch32 mb {mb} call {r}, src", Ss)
        if own_mask:
            assert_same(mask.buf, mask_before, mask, f"paste_batch32 mb {mb} call {r}, mask", Sm)
        assert codec.allocated_bytes() <= codec.paste32_workspace_bytes(n_dst, len(arr))


def test_a_paste_batch32_3_bytes_uint8_hwc_maps_are_src(mi):
    run_leg(mi, "A_paste32_mb3_u8_hwc_c3_maps_are_src", 4 * (M32 + (1 << 25)), lambda codec, leg: paste32_many(mi, codec, 3), c=3)


def test_a_paste_batch32_4_bytes_float16_chw_own_maps(mi):
    run_leg(mi, "A_paste32_mb4_f16_chw_c1", 8 * (M32 + (1 << 25)), lambda codec, leg: paste32_many(mi, codec, 4), c=1)


# ---- leg B: one sample, the offsets inside it past the marks ---------------------------------------------------------------------
def signed32(m):
    return m - ((m >> 31) << 32)


def map_view(maps, mb, shape):
    """the map batch in held `maps` as torch sees it: uint8 [*shape, 3] or int32 [*shape]"""
    import torch

    return maps.body.view(shape + (3,)) if mb == 3 else maps.body.view(torch.int32).view(shape)


def put_id(v, mb, m):
    """id m into every pixel of the view v of a map (a sample, or a rectangle of one)"""
    if mb == 4:
        v.fill_(signed32(m))
    else:
        for b in range(3):
            v[..., b].fill_((m >> (8 * b)) & 0xFF)


def box_rows(host, out, n_rec):
    assert (host[:out.lo] == 0x5A).all() and (host[out.lo + out.nbytes:] == 0x5A).all(), "a guard byte of the boxes was written"
    return host[out.lo:out.lo + out.nbytes].copy().view("<u4").reshape(n_rec, 5).astype(np.int64)


def label32_one_sample(mi, codec, mb, ow, oh):
    import torch

    P, top = ow * oh, TOP[mb]
    assert P > M31 and mb * P > M32
    y31, x31 = divmod(M31, ow)  # pixel 2^31
    p32 = M32 // mb             # the pixel that holds byte 2^32 of the sample
    y32, x32 = divmod(p32, ow)
    if mb == 3:
        assert 3 * p32 < M32 < 3 * p32 + 3, "the pixel straddles byte 2^32"
    else:
        assert mb * P > M33 and 4 * M31 == M33  # (pixel 2^31 of a 4-byte map holds byte 2^33: its rectangle is the one around that mark)
    assert 45 < y32 < y31 - 45 and y31 + 1 < oh - 1
    w1 = min(20000, ow // 3)

    def around(x):
        x1 = min(max(0, x - w1 // 2), ow - 1 - w1)
        assert x1 <= x < x1 + w1 <= ow - 1  # (the last column stays the background's, but for one pixel)
        return x1

    back, id31 = 0x010100, 0x80010101 if mb == 4 else 0x010101
    rects = {0x000001: [(0, 0, min(1000, ow - 1), 2)], id31: [(around(x31), y31 - 1, w1, 3)],  # rows on both sides of pixel 2^31
             top: [(around(x32), y32 - 1, w1, 3)],                                # ... and of the pixel of byte 2^32
             0xFF0001: [(ow // 2, oh - 1, 1, 1)], 0xFF0002: [(ow - 1, 7, 1, 1)],  # one pixel in the last row, one in the last column
             0x020001: [(3, y31 - 40, min(5000, ow - 4), 2)]}                                # (not listed)
    maps = Held(mb * P, mb, value=0)
    mv = map_view(maps, mb, (oh, ow))
    put_id(mv, mb, back)
    for m, rs in rects.items():
        for x, y, w, h in rs:
            put_id(mv[y:y + h, x:x + w], mb, m)
    before = maps.buf.clone()
    listed = sorted([0x000001, back, id31, 700, top, 0xFF0001, 0xFF0002])
    assert max(listed) == top and (mb == 3 or id31 >> 31) and back > 0xFFFF
    # label_boxes32: closed form
    form = closed_form(rects, ow, oh, P, back)
    assert form[back][0] > M31
    want = np.array([form.get(m, (0, ow, oh, 0, 0)) for m in listed], np.int64)
    out = Held(len(listed) * 20, 12)
    codec.label_boxes32(maps.ptr, mb, 1, ow, oh, [listed], out.ptr, stream=_stream())
    _sync()
    got = box_rows(out.buf.cpu().numpy(), out, len(listed))
    assert np.array_equal(got, want), [(hex(listed[j]), got[j].tolist(), want[j].tolist()) for j in np.flatnonzero((got != want).any(1))]
    del out
    # label_targets32: the default, then out[m == id] = value per listed id, in row bands
    step = max(1, PIECE // (8 * ow))
    values = [3, -7, 1 << 20, 5, -(1 << 31), 77, -1]
    out = Held(4 * P, 12)
    assert out.nbytes > M33
    codec.label_targets32(maps.ptr, mb, 1, ow, oh, [listed], [values], out.ptr, dtype="int32", default=-100, stream=_stream())
    _sync()
    ov = out.body.view(torch.int32).view(oh, ow)
    for r0 in range(0, oh, step):
        r1 = min(oh, r0 + step)
        m = F.ids_of_maps(mv[r0:r1], mb)
        assert torch.equal(ov[r0:r1], F.index_of(m, listed, values, -100, torch.int32)), f"label_targets32 mb {mb} index: rows {r0}..{r1 - 1} differ"
    assert bool((out.buf[:out.lo] == 0x5A).all()) and bool((out.buf[out.lo + out.nbytes:] == 0x5A).all()), "label_targets32 index: a guard byte was written"
    del out, ov
    values = [1, 0, 1, 0, 2, 0, 1]  # (a value of 2 has no plane, 0x020001 takes the default: none either)
    out = Held(2 * P, 3)
    codec.label_targets32(maps.ptr, mb, 1, ow, oh, [listed], [values], out.ptr, kind="planes", dtype="uint8", default=-1, planes=2, on=255, off=7, stream=_stream())
    _sync()
    ov = out.body.view(2, oh, ow)
    for r0 in range(0, oh, step):
        r1 = min(oh, r0 + step)
        m = F.ids_of_maps(mv[r0:r1], mb)
        assert torch.equal(ov[:, r0:r1], F.planes_of(m, listed, values, -1, 2, 255, 7, torch.uint8)), f"label_targets32 mb {mb} planes: rows {r0}..{r1 - 1} differ"
    assert bool((out.buf[:out.lo] == 0x5A).all()) and bool((out.buf[out.lo + out.nbytes:] == 0x5A).all()), "label_targets32 planes: a guard byte was written"
    assert_same(maps.buf, before, maps, f"label32 mb {mb} one sample, maps")


@pytest.mark.parametrize("mb", (3, 4))
def test_b_label_boxes32_and_targets32_one_sample_past_2_31_pixels(mi, mb):
    ow, oh = 46342, 46343
    assert ow * oh == 2147627306
    run_leg(mi, f"B_label32_mb{mb}_46342x46343", (2 * mb + 4) * ow * oh + (1 << 30), lambda codec, leg: label32_one_sample(mi, codec, mb, ow, oh))


def largest_sample3(mi, codec, ow, oh):
    """two samples of 2^32 - 1 3-byte pixels: bytes 2^32 and 2^33 of the batch lie in sample 0, every byte of sample 1 past them"""
    P = ow * oh
    assert P == M32 - 1
    S = 3 * P
    assert M33 < S < M34 < 2 * S
    back = (0x010011, 0xFF00C8)
    at = lambda p: [(p % ow, p // ow, 1, 1)]  # noqa: E731
    p32, p33 = M32 // 3, M33 // 3
    assert 3 * p32 < M32 < 3 * p32 + 3 and 3 * p33 < M33 < 3 * p33 + 3  # (both pixels straddle their mark)
    special = [{0x000101: at(p32), 0x010101: at(p33)},  # sample 0: the pixels that hold bytes 2^32 and 2^33 of the batch
               {0x000001: at(0), 0x010001: at(ow - 1), 0xFF0001: at(P - ow), TOP[3]: at(P - 1), 0x000002: at(M31), 0x010002: at(p32), 0xFF0002: at(p33),
                0x000003: at((M34 - S) // 3),  # (the pixel that holds byte 2^34 of the batch)
                0x000009: at(7 * ow + 5)}]     # sample 1: the corners, pixel 2^31, bytes 2^32 and 2^33 of the sample
    assert len({tuple(r[0][:2]) for r in special[1].values()}) == 9
    maps = Held(2 * S, 3, value=0)
    mv = map_view(maps, 3, (2, oh, ow))
    for i in range(2):
        put_id(mv[i], 3, back[i])
        for m, rs in special[i].items():
            for x, y, w, h in rs:
                put_id(mv[i, y:y + h, x:x + w], 3, m)
    before = maps.buf.clone()
    lists = [sorted([back[i], 12345] + list(special[i])) for i in range(2)]
    forms = [closed_form(special[i], ow, oh, P, back[i]) for i in range(2)]
    assert forms[1][back[1]][0] == M32 - 10 and forms[0][back[0]][0] == M32 - 3
    want = np.array([forms[i].get(m, (0, ow, oh, 0, 0)) for i in range(2) for m in lists[i]], np.int64)
    out = Held(len(want) * 20, 12)
    codec.label_boxes32(maps.ptr, 3, 2, ow, oh, lists, out.ptr, stream=_stream())
    _sync()
    got = box_rows(out.buf.cpu().numpy(), out, len(want))
    assert np.array_equal(got, want), [(j, got[j].tolist(), want[j].tolist()) for j in np.flatnonzero((got != want).any(1))]
    del out
    # INDEX uint8 by a closed form: the value of the background id in every pixel but the special ones
    values = [[10 + j for j in range(len(l))] for l in lists]
    out = Held(2 * P, 3)
    want = out.buf.clone()
    wv = body_of(want, out, want.dtype, (2, oh, ow))
    for i in range(2):
        wv[i].fill_(values[i][lists[i].index(back[i])])
        for m, rs in special[i].items():
            for x, y, w, h in rs:
                wv[i, y, x] = values[i][lists[i].index(m)]
    codec.label_targets32(maps.ptr, 3, 2, ow, oh, lists, values, out.ptr, dtype="uint8", default=255, stream=_stream())
    _sync()
    assert_same(out.buf, want, out, "label_targets32 index uint8, 2^32 - 1 pixels", P)
    assert_same(maps.buf, before, maps, "label32 largest sample, maps", S)


def test_b_label_boxes32_and_targets32_largest_sample_3_bytes(mi):
    ow, oh = 65537, 65535
    run_leg(mi, "B_label32_mb3_65537x65535", 16 * ow * oh + (1 << 30), lambda codec, leg: largest_sample3(mi, codec, ow, oh))


def paste32_one_sample(mi, codec, mb, side):
    import torch

    from test_wide_id_paste_rule import window_array

    c = 3
    S, Sm = c * side * side, mb * side * side
    assert S > M32
    y32, y32m = M32 // (side * c), M32 // (side * mb)  # the rows that hold byte 2^32 of src and dst, and of the maps
    assert 40 < y32m <= y32 < side - 40 and (mb == 3 or y32 - y32m > 100)
    rng = np.random.default_rng(95)
    wins, pool = paste_windows(rng, mb), paste_pool(mb)
    own_mask = mb == 4
    src, dst = Held(S, 3, seed=None if mb == 3 else 96, value=0), Held(S, 5, seed=97)
    mask = Held(Sm, 12, value=0) if own_mask else src
    flat = mask.body.view(-1, 3) if mb == 3 else mask.body.view(torch.int32)
    bank = torch.from_numpy(wide_maps(pool, 3) if mb == 3 else wide_maps(pool, 4).view(np.int32)).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(98)
    for a in range(0, side * side, PIECE // 8):  # ids of the pool, pixel by pixel
        b = min(side * side, a + PIECE // 8)
        flat[a:b] = bank[torch.randint(0, len(pool), (b - a,), device=DEV, generator=g)]
    src_before, want = src.buf.clone(), dst.buf.clone()
    mask_before = mask.buf.clone() if own_mask else src_before
    sv, wv = body_of(src_before, src, torch.uint8, (side, side, c)), body_of(want, dst, torch.uint8, (side, side, c))
    mv = body_of(mask_before, mask, torch.uint8, (side, side, 3)) if mb == 3 else body_of(mask_before, mask, torch.int32, (side, side))
    # (dx, dy, sx, sy, w, h): src rows below byte 2^32 to dst rows across it; src rows across it to dst rows below; the last pixel of both
    ps = [(100, y32 - 3, 7, 11, side // 2, 10), (9, 20, side // 3, y32 - 5, side // 2, 10), (side - 64, side - 32, side - 64, side - 32, 64, 32),
          (side // 2, y32 - 1, 1, y32 + 2, side // 3, 7)]
    if own_mask:  # the same around the row that holds byte 2^32 of the maps
        ps += [(50, 300, 11, y32m - 4, side // 2, 9), (side // 4, y32m - 2, 5, y32m + 1, side // 3, 6)]
    recs = [(0, 0) + p + (wins[k % len(wins)],) for k, p in enumerate(ps)]
    recs.append((0, 0, side // 5, y32 - 2, 3, 100, side // 4, 5, wins[0], 0xC0B0A1, True))  # VALUE_PIXEL across the row of byte 2^32 of dst
    recs.append((0, 0, 3, 5, side - 300, y32m - 1, 200, 3, wins[1], 0x3D))                    # VALUE
    codec.paste_batch32(src.ptr, mask.ptr, mb, 1, side, side, dst.ptr, 1, side, side, window_array(mi, recs), dtype="uint8", layout="hwc", stream=_stream())
    _sync()
    for r in recs:
        sy, h = r[5], r[7]
        taken = F.paste_piece32(wv, sv, (F.ids_of_maps(mv[sy:sy + h], mb), sy), r[2:8], r[8], *r[9:])
        assert taken > 0, f"piece {r[2:8]} selects pixels"
    assert_same(dst.buf, want, dst, f"paste_batch32 mb {mb} one sample, dst")
    assert_same(src.buf, src_before, src, f"paste_batch32 mb {mb} one sample, src")
    if own_mask:
        assert_same(mask.buf, mask_before, mask, f"paste_batch32 mb {mb} one sample, mask")


@pytest.mark.parametrize("mb", (3, 4))
def test_b_paste_batch32_one_sample_past_2_32(mi, mb):
    side = 38000
    run_leg(mi, f"B_paste32_mb{mb}_u8_hwc_38000", (4 * 3 + (2 * mb if mb == 4 else 0)) * side * side, lambda codec, leg: paste32_one_sample(mi, codec, mb, side))
