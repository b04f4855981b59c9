"""The batch calls on batches and samples past 2^31 and 2^32 bytes (include/llcomp_mi.h: "Batch mixing" to "Label targets"): mix_batch,
orient_batch, compose_batch, paste_batch, paste_batch16, label_boxes, label_boxes16 and label_targets, where an offset held in 32 bits
lands on another byte.  tests/test_gpu_large.py does the same for the codec itself.

Nothing expected comes from the library: the active samples of a many-samples leg -- {0, b31 - 1, b31, b31 + 1, b32 - 1, b32, b32 + 1,
n - 1}, b31 and b32 the samples that hold byte 2^31 and 2^32 of the batch -- are brought to the host and compared bit for bit with the
numpy specs the small tests use; where a call moves data in every sample, the expectation is torch indexing on the GPU (slicing, flip,
transpose, roll, ==, a table gather), each formulation checked first at a few samples against the numpy spec.  Every byte is compared:
a batch the call may write against a copy from before the call with the expected samples put in, guards of 256 bytes included; every
input against its copy.  Batches start 3 elements past a 256-byte boundary, samples are no powers of two.

Leg A: many samples, the batch past 2^32 bytes -- every call.  Leg B: one sample past 2^32 bytes (uint8 38000 x 38000 x 3; label
maps of 2^32 - 1 pixels and of more than 2^31 16-bit pixels), where the offsets INSIDE a sample pass the marks; expected by torch
slicing, closed forms and a table gather.  Leg C: one group of views past 2^32 bytes through each of the three stores of a formatted
output (the vertical resample pass, the warped views' gather, the last step of a photometric chain): view v is one of 30 classes,
computed by the numpy specs (PIL's transform for the warped views); and past 2^32 ELEMENTS as uint8 CHW, since the stores index
elements.  profiles/large_batches.txt keeps a run's lines and what a truncated offset would trip.

Every test frees what it holds, skips (stating both numbers) only when the device has less free memory than it needs, and prints one
"LARGE" line: the bytes it holds, the least free device memory seen, wall time."""
import numpy as np
import pytest

from test_gpu_large import Leg, _release

pytestmark = pytest.mark.gpu

DEV = "cuda"
M31, M32 = 1 << 31, 1 << 32
GUARD = 256
PIECE = 1 << 28  # bytes filled or compared per step
LAM = 0.3712345678901234


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream if DEV == "cuda" else 0


def _sync():
    import torch

    if DEV == "cuda":
        torch.cuda.synchronize()


class BatchLeg(Leg):
    """Leg for a test whose memory is its own buffers: need() skips when they do not fit, the report line states them"""

    def need(self, nbytes):
        import torch

        free = torch.cuda.mem_get_info()[0]
        self.held = nbytes
        if free < nbytes + (1 << 30):
            pytest.skip(f"{self.name}: needs {nbytes + (1 << 30)} bytes; {free} bytes free")

    def report(self):
        import time

        self.seen()
        print(f"\nLARGE {self.name}: held_bytes={self.held} min_free_bytes={self.min_free} wall_s={time.time() - self.t0:.1f}")


def run_leg(mi, name, need, body, c=3):
    """one test: the memory check, a codec of c channels (it supplies nothing else), the body, the report, and everything freed"""
    leg = BatchLeg(mi, name)
    leg.need(need)
    codec = mi.Codec(1, 32, 16, c, 32, 16, False, device=0)
    try:
        body(codec, leg)
        leg.report()
    finally:
        codec.close()
        _release(mi)


class Held:
    """nbytes in device memory, `offset` bytes past a 256-byte boundary, between GUARD bytes of 0x5A: seeded noise (every bit pattern,
    NaNs among them) or one value"""

    def __init__(self, nbytes, offset, seed=None, value=0xA5):
        import torch

        self.lo, self.nbytes = GUARD + offset, nbytes
        self.buf = torch.empty(self.lo + nbytes + GUARD, dtype=torch.uint8, device=DEV)
        assert DEV != "cuda" or self.buf.data_ptr() % 256 == 0
        self.buf[:self.lo] = 0x5A
        self.buf[self.lo + nbytes:] = 0x5A
        if seed is None:
            self.body.fill_(value)
        else:
            g = torch.Generator(device=DEV).manual_seed(seed)
            for a in range(0, nbytes, PIECE):
                b = min(nbytes, a + PIECE)
                self.body[a:b] = torch.randint(0, 256, (b - a,), dtype=torch.uint8, device=DEV, generator=g)

    @property
    def body(self):
        return self.buf[self.lo:self.lo + self.nbytes]

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lo


def body_of(buf, held, tdtype, shape):
    """the batch inside `buf` -- held.buf or a clone of it -- as a tensor of the integer type tdtype and the shape"""
    return buf[held.lo:held.lo + held.nbytes].view(tdtype).view(shape)


def get_samples(buf, held, idx, sample_bytes, np_dtype, shape):
    """samples idx of the batch inside buf -> a numpy array [len(idx), *shape] on the host"""
    out = [buf[held.lo + i * sample_bytes:held.lo + (i + 1) * sample_bytes].cpu().numpy().view(np_dtype).reshape(shape) for i in idx]
    return np.stack(out)


def put_samples(buf, held, idx, sample_bytes, arr):
    import torch

    for k, i in enumerate(idx):
        raw = np.ascontiguousarray(arr[k]).reshape(-1).view(np.uint8)
        assert raw.size == sample_bytes
        buf[held.lo + i * sample_bytes:held.lo + (i + 1) * sample_bytes] = torch.from_numpy(raw.copy()).to(DEV)


def assert_same(got, want, held, what, sample_bytes=None):
    """two whole buffers (guards and all) hold the same bytes, compared piece by piece on the device"""
    import torch

    assert got.shape == want.shape and got.dtype == want.dtype == torch.uint8
    n = got.numel()
    for a in range(0, n, PIECE):
        b = min(n, a + PIECE)
        if not torch.equal(got[a:b], want[a:b]):
            at = a + int((got[a:b] != want[a:b]).to(torch.uint8).argmax()) - held.lo
            where = "a guard byte" if not 0 <= at < held.nbytes else f"byte {at} of the batch" + (
                f" (sample {at // sample_bytes}, its byte {at % sample_bytes})" if sample_bytes else "")
            raise AssertionError(f"{what}: {where} differs")


def straddlers(n, sample_bytes):
    """the preconditions of a many-samples leg -> (b31, b32), the samples that hold byte 2^31 and byte 2^32 of the batch"""
    assert n * sample_bytes > M32, "precondition: the batch passes 2^32 bytes"
    assert sample_bytes & (sample_bytes - 1), "precondition: the sample size is no power of two"
    b31, b32 = M31 // sample_bytes, M32 // sample_bytes
    for b, m in ((b31, M31), (b32, M32)):
        assert b * sample_bytes < m < (b + 1) * sample_bytes, "precondition: the sample straddles the mark"
    assert 0 < b31 - 1 and b31 + 1 < b32 - 1 and b32 + 1 < n - 1 <= 65534
    return b31, b32


def active_set(n, b31, b32):
    return [0, b31 - 1, b31, b31 + 1, b32 - 1, b32, b32 + 1, n - 1]


def past(sample_bytes, more=25):
    """the number of samples of a batch that passes 2^32 bytes by `more` samples"""
    return M32 // sample_bytes + more


# ---- the torch formulations of whole-batch data movement, and their checks against the numpy specs -------------------------------
def roll_box(v, box, layout):
    """CutMix with partner "roll" and the same box in every sample, in place on the integer view v [n, c, h, w] / [n, h, w, c]"""
    x, y, w, h = box
    region = v[:, :, y:y + h, x:x + w] if layout == "chw" else v[:, y:y + h, x:x + w, :]
    region.copy_(region.roll(1, 0))


def orient_classes(v, layout):
    """codes[i] = i % 8, in place on the integer view v of square samples"""
    ay, ax = (2, 3) if layout == "chw" else (1, 2)
    for code in range(1, 8):
        s = v[code::8]
        s.copy_({1: lambda t: t.flip(ax), 2: lambda t: t.flip(ay), 3: lambda t: t.flip(ax).transpose(ay, ax), 4: lambda t: t.flip(ay).flip(ax),
                 5: lambda t: t.transpose(ay, ax).flip(ax), 6: lambda t: t.transpose(ay, ax),
                 7: lambda t: t.transpose(ay, ax).flip(ay).flip(ax)}[code](s).contiguous())


def filled_with_one_piece_each(dv, sv, src_of, rect, fill_elems):
    """compose_batch without keep, CHW: every dst sample the fill, then the rectangle (dx, dy, sx, sy, w, h) from src sample src_of[i],
    in place on the integer view dv [n_dst, c, oh, ow]; sv [n_src, c, ih, iw]; fill_elems: c elements as integers"""
    import torch

    dx, dy, sx, sy, w, h = rect
    dv[:] = torch.as_tensor(fill_elems, dtype=dv.dtype, device=dv.device).view(1, -1, 1, 1)
    dv[:, :, dy:dy + h, dx:dx + w] = sv[:, :, sy:sy + h, sx:sx + w][torch.as_tensor(src_of, dtype=torch.long, device=dv.device)]


def test_the_torch_formulations_are_the_numpy_specs(mi):
    import torch

    import compose_spec
    import mix_spec
    import orient_spec
    from batch_support import bits_of
    from mix_batches import Case, to_layout

    t = mix_spec.gen_batch("float32", 5, 3, 9, 11, seed=1)
    box = (2, 3, 5, 4)
    for layout in ("chw", "hwc"):
        v = torch.from_numpy(bits_of(to_layout(t, layout)).view(np.int32).copy())
        roll_box(v, box, layout)
        assert np.array_equal(v.numpy().view(np.uint32), Case("roll", boxes=box).expected(t, layout)), layout
    for dtype, layout in (("float16", "hwc"), ("uint8", "chw")):
        batch = orient_spec.gen_batch(dtype, 13, 3, 7, 7, layout, seed=2)  # 13 samples: every code class, some with two members
        v = torch.from_numpy(bits_of(batch).view({1: np.uint8, 2: np.int16}[batch.itemsize]).copy())
        orient_classes(v, layout)
        want = bits_of(orient_spec.apply(batch, [i % 8 for i in range(13)], layout))
        assert np.array_equal(v.numpy().view(want.dtype), want), (dtype, layout)
    src, dst = compose_spec.gen_batch("bfloat16", 6, 3, 7, 9, "chw", 3), compose_spec.gen_batch("bfloat16", 5, 3, 8, 11, "chw", 4)
    rect, src_of, fill = (3, 2, 1, 4, 6, 3), [4, 0, 5, 5, 2], [0.5, -2.0, 3.25]
    dv, sv = torch.from_numpy(dst.view(np.int16).copy()), torch.from_numpy(src.view(np.int16).copy())
    filled_with_one_piece_each(dv, sv, src_of, rect, compose_spec.fill_bits(fill, 3, "bfloat16").view(np.int16).tolist())
    want = compose_spec.apply(src, dst, [(i, s) + rect for i, s in enumerate(src_of)], "chw", "bfloat16", fill=fill)
    assert np.array_equal(dv.numpy().view(np.uint16), want)


# ---- leg A: many samples, the batch past 2^32 bytes ------------------------------------------------------------------------------
def mix_many(mi, codec, layout, c, oh, ow, n, roll):
    import mix_spec
    from mix_batches import Case, to_layout

    es = 4
    S = c * oh * ow * es
    b31, b32 = straddlers(n, S)
    act = active_set(n, b31, b32)
    held = Held(n * S, 3 * es, seed=11)
    shape = (c, oh, ow) if layout == "chw" else (oh, ow, c)
    clean = mix_spec.gen_batch("float32", 8, c, oh, ow, seed=5)  # (the blends run on numbers: a NaN's payload is nobody's rule)
    put_samples(held.buf, held, act, S, to_layout(clean, layout))
    want = held.buf.clone()
    # one cycle through the active samples that crosses 2^31 and 2^32 upwards and downwards
    cycle = [0, b32, b31 - 1, n - 1, b31, b32 + 1, b31 + 1, b32 - 1]
    partner = list(range(n))
    for k, i in enumerate(cycle):
        partner[i] = cycle[(k + 1) % len(cycle)]
    lam = {0: LAM, b31 + 1: 0.25, b32: 0.8125, n - 1: LAM}  # (n - 1 and b31 + 1 blend with a partner that is erased)
    boxes = {b31 - 1: (ow - 40, oh - 30, 40, 30), b31 + 1: (3, 5, 100, 77), b32 - 1: (0, 0, ow, 1), b32 + 1: (17, 0, 31, oh)}
    erase = {b31: (10, 20, 200, 150), b32 - 1: (ow - 1, 0, 1, oh)}
    ev = [0.25, -1.5, 1e-6]
    samples = mi.mix_samples(n, partner, [lam.get(i) for i in range(n)], [boxes.get(i) for i in range(n)], [erase.get(i) for i in range(n)])
    codec.mix_batch(held.ptr, n, ow, oh, samples, dtype="float32", layout=layout, erase_value=ev, stream=_stream())
    _sync()
    local = {s: k for k, s in enumerate(act)}
    case = Case([local[partner[s]] for s in act], [lam.get(s) for s in act], [boxes.get(s) for s in act], [erase.get(s) for s in act], ev)
    exp = case.expected(clean, layout)
    before = mix_spec.bits(clean if layout == "chw" else clean.permute(0, 2, 3, 1))
    assert all(not np.array_equal(exp[k], before[k]) for k in range(8)), "every active sample changes"
    put_samples(want, held, act, S, exp)
    assert_same(held.buf, want, held, f"mix_batch {layout}, the active samples", S)
    assert codec.allocated_bytes() <= codec.mix_workspace_bytes(n, ow, oh, "float32")
    if roll:  # every sample takes a box of the sample before it
        import torch

        box = (101, 57, 97, 55)
        codec.mix_batch(held.ptr, n, ow, oh, mi.mix_samples(n, "roll", None, box, None), dtype="float32", layout=layout, stream=_stream())
        _sync()
        roll_box(body_of(want, held, torch.int32, (n,) + shape), box, layout)
        assert_same(held.buf, want, held, f"mix_batch {layout}, roll", S)
        assert codec.allocated_bytes() <= codec.mix_workspace_bytes(n, ow, oh, "float32")


def test_a_mix_batch_float32_chw(mi):
    c, oh, ow = 3, 333, 251
    assert c * oh * ow * 4 == 1002996 and 1002996 % 16
    run_leg(mi, "A_mix_f32_chw_4300", 3 * 4300 * 1002996, lambda codec, leg: mix_many(mi, codec, "chw", c, oh, ow, 4300, True))


def test_a_mix_batch_float32_hwc_vector_path(mi):
    c, oh, ow = 3, 332, 252
    assert c * oh * ow * 4 % 16 == 0
    run_leg(mi, "A_mix_f32_hwc_4300", 3 * 4300 * c * oh * ow * 4, lambda codec, leg: mix_many(mi, codec, "hwc", c, oh, ow, 4300, False))


def orient_many(mi, codec, dtype, layout, c, side, n, every):
    import torch

    import orient_spec
    from batch_support import bits_of

    es, np_t, t_t = {"float16": (2, np.float16, torch.int16), "uint8": (1, np.uint8, torch.uint8)}[dtype]
    S = c * side * side * es
    b31, b32 = straddlers(n, S)
    act = active_set(n, b31, b32)
    held = Held(n * S, 3 * es, seed=12)
    shape = (c, side, side) if layout == "chw" else (side, side, c)
    want = held.buf.clone()
    codes = [0] * n
    for k, s in enumerate(act):
        codes[s] = 1 + k % 7  # all seven, FLIP_LEFT_RIGHT twice
    codec.orient_batch(held.ptr, n, side, side, codes, dtype=dtype, layout=layout, stream=_stream())
    _sync()
    sub = get_samples(want, held, act, S, np_t, shape)
    exp = orient_spec.apply(sub, [codes[s] for s in act], layout)
    assert all(not np.array_equal(bits_of(exp[k]), bits_of(sub[k])) for k in range(8))
    put_samples(want, held, act, S, exp)
    assert_same(held.buf, want, held, f"orient_batch {dtype} {layout}, the active samples", S)
    if every:
        codec.orient_batch(held.ptr, n, side, side, [i % 8 for i in range(n)], dtype=dtype, layout=layout, stream=_stream())
        _sync()
        orient_classes(body_of(want, held, t_t, (n,) + shape), layout)
        assert_same(held.buf, want, held, f"orient_batch {dtype} {layout}, codes i % 8", S)
    assert codec.allocated_bytes() <= codec.orient_workspace_bytes(n)


def test_a_orient_batch_float16_hwc(mi):
    run_leg(mi, "A_orient_f16_hwc_8600", 3 * 8600 * 3 * 289 * 289 * 2, lambda codec, leg: orient_many(mi, codec, "float16", "hwc", 3, 289, 8600, True))


def test_a_orient_batch_uint8_chw(mi):
    run_leg(mi, "A_orient_u8_chw_17200", 3 * 17200 * 3 * 289 * 289, lambda codec, leg: orient_many(mi, codec, "uint8", "chw", 3, 289, 17200, False))


IH, IW, OH, OW = 301, 203, 333, 251  # the src and dst samples of the compose and paste legs


def pieces_between(act_s, act_d, iw, ih, ow, oh):
    """geometry of pieces between the active samples: dst k from src 7 - k (low to high and high to low), a second piece over the
    first, and one that ends in the last row and column of both -> (dst, src, dx, dy, sx, sy, w, h)"""
    out = []
    for k in range(8):
        w, h = 30 + 17 * k, 25 + 11 * k
        out.append((act_d[k], act_s[7 - k], 5 + 9 * k, 3 + 13 * k, 7 * k, 11 * k, w, h))
        out.append((act_d[k], act_s[k], 20 + 9 * k, 10 + 13 * k, 1 + k, 2 * k, 21, 19))
    out.append((act_d[3], act_s[5], ow - 50, oh - 40, iw - 50, ih - 40, 50, 40))
    out.append((act_d[5], act_s[2], 0, oh - 1, 0, ih - 1, iw, 1))
    return out


def localise(pieces, act_s, act_d):
    ls, ld = {s: k for k, s in enumerate(act_s)}, {d: k for k, d in enumerate(act_d)}
    return [(ld[p[0]], ls[p[1]]) + tuple(p[2:]) for p in pieces]


def compose_many(mi, codec):
    import torch

    import compose_spec

    c, es = 3, 2
    Ss, Sd = c * IH * IW * es, c * OH * OW * es
    n_src, n_dst = past(Ss), past(Sd)
    act_s, act_d = active_set(n_src, *straddlers(n_src, Ss)), active_set(n_dst, *straddlers(n_dst, Sd))
    src, dst = Held(n_src * Ss, 3 * es, seed=21), Held(n_dst * Sd, 5 * es, seed=22)
    src_before, want = src.buf.clone(), dst.buf.clone()
    pieces = pieces_between(act_s, act_d, IW, IH, OW, OH)
    codec.compose_batch(src.ptr, n_src, IW, IH, dst.ptr, n_dst, OW, OH, pieces, dtype="bfloat16", layout="chw", keep=True, stream=_stream())
    _sync()
    s_sub, d_sub = get_samples(src_before, src, act_s, Ss, np.uint16, (c, IH, IW)), get_samples(want, dst, act_d, Sd, np.uint16, (c, OH, OW))
    exp = compose_spec.apply(s_sub, d_sub, localise(pieces, act_s, act_d), "chw", "bfloat16", keep=True)
    assert all(not np.array_equal(exp[k], d_sub[k]) for k in range(8))
    put_samples(want, dst, act_d, Sd, exp)
    assert_same(dst.buf, want, dst, "compose_batch keep, dst", Sd)
    assert_same(src.buf, src_before, src, "compose_batch keep, src", Ss)
    # without keep: every dst sample the fill and one rectangle, the active dst samples from the active src samples
    rect, fill = (100, 200, 60, 150, 143, 133), [0.5, -2.0, 3.25]  # (it ends in the last row and the last column of src and of dst)
    assert rect[0] + rect[4] <= OW and rect[1] + rect[5] == OH and rect[2] + rect[4] == IW and rect[3] + rect[5] <= IH
    src_of = [(i * 7919 + 13) % n_src for i in range(n_dst)]
    for k, d in enumerate(act_d):
        src_of[d] = act_s[(k + 3) % 8]
    codec.compose_batch(src.ptr, n_src, IW, IH, dst.ptr, n_dst, OW, OH, [(i, s) + rect for i, s in enumerate(src_of)], dtype="bfloat16", layout="chw",
                        fill=fill, stream=_stream())
    _sync()
    filled_with_one_piece_each(body_of(want, dst, torch.int16, (n_dst, c, OH, OW)), body_of(src_before, src, torch.int16, (n_src, c, IH, IW)), src_of, rect,
                               compose_spec.fill_bits(fill, c, "bfloat16").view(np.int16).tolist())
    assert_same(dst.buf, want, dst, "compose_batch fill, dst", Sd)
    assert_same(src.buf, src_before, src, "compose_batch fill, src", Ss)
    assert codec.allocated_bytes() <= codec.compose_workspace_bytes(n_dst, n_dst)


def test_a_compose_batch_bfloat16_chw(mi):
    run_leg(mi, "A_compose_bf16_chw", 4 * (M32 + (1 << 25)), lambda codec, leg: compose_many(mi, codec))


def paste_many(mi, codec):
    import paste_spec

    c, es = 3, 4
    Ss, Sd, Sm = IH * IW * c * es, OH * OW * c * es, IH * IW
    n_src, n_dst = past(Ss), past(Sd)
    act_s, act_d = active_set(n_src, *straddlers(n_src, Ss)), active_set(n_dst, *straddlers(n_dst, Sd))
    src, dst, mask = Held(n_src * Ss, 3 * es, seed=31), Held(n_dst * Sd, 5 * es, seed=32), Held(n_src * Sm, 3, seed=33)
    src_before, mask_before, want = src.buf.clone(), mask.buf.clone(), dst.buf.clone()
    ids = [range(0, 128), "nonzero", range(1, 256, 2), [0, 7, 200, 255], range(64, 192)]
    pieces = [p + (ids[k % len(ids)],) for k, p in enumerate(pieces_between(act_s, act_d, IW, IH, OW, OH))]
    pieces.append((act_d[6], act_s[1], 40, 50, 30, 20, 90, 70, range(0, 256, 3), -7.25))  # a VALUE piece
    codec.paste_batch(src.ptr, mask.ptr, n_src, IW, IH, dst.ptr, n_dst, OW, OH, pieces, dtype="float32", layout="hwc", stream=_stream())
    _sync()
    s_sub, m_sub = get_samples(src_before, src, act_s, Ss, np.float32, (IH, IW, c)), get_samples(mask_before, mask, act_s, Sm, np.uint8, (IH, IW))
    d_sub = get_samples(want, dst, act_d, Sd, np.float32, (OH, OW, c))
    exp = paste_spec.apply(s_sub, m_sub, d_sub, localise(pieces, act_s, act_d), "hwc", "float32")
    assert all(not np.array_equal(exp[k].view(np.uint32), d_sub[k].view(np.uint32)) for k in range(8))
    put_samples(want, dst, act_d, Sd, exp)
    assert_same(dst.buf, want, dst, "paste_batch, dst", Sd)
    assert_same(src.buf, src_before, src, "paste_batch, src", Ss)
    assert_same(mask.buf, mask_before, mask, "paste_batch, mask", Sm)
    assert codec.allocated_bytes() <= codec.paste_workspace_bytes(n_dst, len(pieces))


def test_a_paste_batch_float32_hwc(mi):
    run_leg(mi, "A_paste_f32_hwc", 4 * (M32 + (1 << 25)) + 2 * past(IH * IW * 12) * IH * IW, lambda codec, leg: paste_many(mi, codec))


def paste16_many(mi, codec, dtype, layout, c, own_mask):
    import paste16_spec
    from batch_support import bits_of

    es, np_t = {"uint8": (1, np.uint8), "float16": (2, np.float16)}[dtype]
    Ss, Sd, Sm = IH * IW * c * es, OH * OW * c * es, IH * IW * 2
    s_shape, d_shape = ((c, IH, IW), (c, OH, OW)) if layout == "chw" else ((IH, IW, c), (OH, OW, c))
    n_src, n_dst = past(Ss), past(Sd)
    act_s, act_d = active_set(n_src, *straddlers(n_src, Ss)), active_set(n_dst, *straddlers(n_dst, Sd))
    src, dst = Held(n_src * Ss, 6, seed=41), Held(n_dst * Sd, 3 * es, seed=42)
    mask = Held(n_src * Sm, 10, seed=43) if own_mask else src
    assert Sm == Ss  # (either way the maps pass 2^32 bytes where the src batch does)
    m_sub = paste16_spec.gen_mask(np.random.default_rng(44), 8, IH, IW)  # the active maps hold ids of the pool, the others noise
    put_samples(mask.buf, mask, act_s, Sm, m_sub)
    src_before, mask_before, want = src.buf.clone(), (mask.buf.clone() if own_mask else None), dst.buf.clone()
    pool = paste16_spec.HIGH_BYTE
    ids = [pool[:4], pool[:6], pool[1::2], [0x0101, 0xFF00], pool[4:]]  # (sets of up to four windows of 256 ids: a piece per window)
    pieces = [p + (ids[k % len(ids)],) for k, p in enumerate(pieces_between(act_s, act_d, IW, IH, OW, OH))]
    pieces.append((act_d[6], act_s[1], 40, 50, 30, 20, 90, 70, pool[::3], 0xC7 if es == 1 else 0xFC01))  # a VALUE piece
    codec.paste_batch16(src.ptr, mask.ptr, n_src, IW, IH, dst.ptr, n_dst, OW, OH, pieces, dtype=dtype, layout=layout, stream=_stream())
    _sync()
    s_sub, d_sub = get_samples(src_before, src, act_s, Ss, np_t, s_shape), get_samples(want, dst, act_d, Sd, np_t, d_shape)
    exp = paste16_spec.apply(s_sub, m_sub, d_sub, localise(pieces, act_s, act_d), layout)
    assert all(not np.array_equal(bits_of(exp[k]), bits_of(d_sub[k])) for k in range(8))
    put_samples(want, dst, act_d, Sd, exp)
    assert_same(dst.buf, want, dst, f"paste_batch16 {dtype}, dst", Sd)
    assert_same(src.buf, src_before, src, f"paste_batch16 {dtype}, src", Ss)
    if own_mask:
        assert_same(mask.buf, mask_before, mask, f"paste_batch16 {dtype}, mask", Sm)
    assert codec.allocated_bytes() <= codec.paste16_workspace_bytes(n_dst, len(mi.paste_pieces16(pieces)))


def test_a_paste_batch16_uint8_hwc_maps_are_src(mi):
    run_leg(mi, "A_paste16_u8_hwc_c2", 4 * (M32 + (1 << 25)), lambda codec, leg: paste16_many(mi, codec, "uint8", "hwc", 2, False), c=2)


def test_a_paste_batch16_float16_chw_own_maps(mi):
    run_leg(mi, "A_paste16_f16_chw_c1", 6 * (M32 + (1 << 25)), lambda codec, leg: paste16_many(mi, codec, "float16", "chw", 1, True), c=1)


LH, LW = 517, 389  # the id maps of the label legs


def banked(held, bank, n, sample_bytes):
    """sample i of the batch in held = bank[i % len(bank)] (a uint8 tensor [K, sample_bytes] on the device), by a gather"""
    import torch

    v = held.body.view(n, sample_bytes)
    step = max(1, PIECE // sample_bytes)
    for a in range(0, n, step):
        b = min(n, a + step)
        v[a:b] = bank[torch.arange(a, b, device=DEV) % len(bank)]


def assert_banked(held, want_bank, n, sample_bytes, what):
    """sample i of the output in held is want_bank[i % K], compared on the device piece by piece"""
    import torch

    v = held.body.view(n, sample_bytes)
    step = max(1, PIECE // sample_bytes)
    for a in range(0, n, step):
        b = min(n, a + step)
        same = (v[a:b] == want_bank[torch.arange(a, b, device=DEV) % len(want_bank)]).all(1)
        if not bool(same.all()):
            i = a + int((~same).to(torch.uint8).argmax())
            raise AssertionError(f"{what}: sample {i} (bank entry {i % len(want_bank)}) differs")
    assert bool((held.buf[:held.lo] == 0x5A).all()) and bool((held.buf[held.lo + held.nbytes:] == 0x5A).all()), f"{what}: a guard byte was written"


def to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).reshape(len(a), -1).view(np.uint8).copy()).to(DEV)


def records(table):
    """[..., 5] of (count, x0, y0, x1, y1) -> the records' bytes [..., 20]"""
    return np.ascontiguousarray(table.astype("<u4")).view(np.uint8).reshape(table.shape[:-1] + (20,))


def label_boxes_many(mi, codec, n):
    from test_label_boxes import blobs, label_boxes_spec

    P = LH * LW
    b31, b32 = straddlers(n, P)
    assert b31 % 7 and b32 % 7  # (the straddling samples are not sample 0's map again)
    bank = blobs(np.random.default_rng(51), 7, LH, LW, 40)
    bank[3, 0, 0], bank[3, LH - 1, LW - 1], bank[5, LH - 1, 0] = 250, 251, 252  # ids of one pixel, at corners
    maps, out = Held(n * P, 3, value=0), Held(n * 256 * 20, 12)
    banked(maps, to_dev(bank), n, P)
    before = maps.buf.clone()
    codec.label_boxes(maps.ptr, n, LW, LH, out.ptr, stream=_stream())
    _sync()
    assert_banked(out, to_dev(records(label_boxes_spec(bank))), n, 256 * 20, "label_boxes")
    assert_same(maps.buf, before, maps, "label_boxes, maps", P)


def test_a_label_boxes_u8(mi):
    run_leg(mi, "A_label_boxes_u8_21400", 2 * 21400 * LH * LW + 21400 * 5120, lambda codec, leg: label_boxes_many(mi, codec, 21400))


def bank_lists(rng, bank, top):
    """per bank entry a list of ids: some the map has, some it has not, of different lengths; entry 3 lists nothing"""
    out = []
    for k in range(len(bank)):
        have = np.unique(bank[k])
        pick = set(rng.choice(have, size=min(len(have), 3 + 2 * k), replace=False).tolist()) | set(rng.integers(0, top, size=2 + k).tolist())
        out.append(sorted(int(m) for m in pick))
    out[3] = []
    return out


def label_boxes16_many(mi, codec, n):
    from test_label_boxes16 import HIGH_BYTE, blobs16, label_boxes16_spec

    P2 = LH * LW * 2
    b31, b32 = straddlers(n, P2)
    assert b31 % 7 and b32 % 7
    rng = np.random.default_rng(52)
    bank = blobs16(rng, 7, LH, LW, HIGH_BYTE + (700, 0x8000, 65535))
    lists = bank_lists(rng, bank, 65536)
    assert len({len(l) for l in lists}) > 3 and lists[3] == []
    maps = Held(n * P2, 6, value=0)
    banked(maps, to_dev(bank), n, P2)
    before = maps.buf.clone()
    tables = [label_boxes16_spec(bank[k:k + 1], lists[k:k + 1]) for k in range(7)]
    assert all(t[:, 0].any() for t in tables if len(t)), "every list names an id that has pixels"
    per = [records(t).reshape(-1) for t in tables]
    want = np.concatenate([per[i % 7] for i in range(n)])
    out = Held(want.size, 12)
    codec.label_boxes16(maps.ptr, n, LW, LH, [lists[i % 7] for i in range(n)], out.ptr, stream=_stream())
    _sync()
    got = out.buf.cpu().numpy()
    assert (got[:out.lo] == 0x5A).all() and (got[out.lo + want.size:] == 0x5A).all(), "label_boxes16: a guard byte was written"
    bad = np.flatnonzero(got[out.lo:out.lo + want.size] != want)
    assert not bad.size, f"label_boxes16: record {bad[0] // 20} differs"
    assert_same(maps.buf, before, maps, "label_boxes16, maps", P2)
    assert codec.allocated_bytes() <= codec.label_boxes16_workspace_bytes(n, want.size // 20)


def test_a_label_boxes16_u16(mi):
    run_leg(mi, "A_label_boxes16_u16_10700", 2 * 10700 * LH * LW * 2 + (1 << 26), lambda codec, leg: label_boxes16_many(mi, codec, 10700))


def label_index_many(mi, codec, n, map_dtype, dtype, maps_past):
    from test_label_boxes import blobs
    from test_label_boxes16 import HIGH_BYTE, blobs16
    from test_label_targets import index_spec

    ms, es = np.dtype(map_dtype).itemsize, np.dtype(dtype).itemsize
    Sm, So = LH * LW * ms, LH * LW * es
    b31, b32 = straddlers(n, So)  # the output passes 2^32 bytes
    assert b31 % 7 and b32 % 7
    if maps_past:
        straddlers(n, Sm)
    else:
        assert n * Sm < M31
    rng = np.random.default_rng(53 + es)
    bank = blobs(rng, 7, LH, LW, 40) if ms == 1 else blobs16(rng, 7, LH, LW, HIGH_BYTE + (700, 0x8000, 65535))
    lists = bank_lists(rng, bank, 256 if ms == 1 else 65536)
    values = [rng.integers(0, 255, size=len(l)).tolist() if es == 1 else rng.integers(-100, 1 << 20, size=len(l)).tolist() for l in lists]
    default = 255 if es == 1 else -100
    want = index_spec(bank, lists, values, default, dtype)
    assert all((want[k] != default).any() for k in range(7) if lists[k])
    maps, out = Held(n * Sm, 3 * ms, value=0), Held(n * So, 3 * es)
    banked(maps, to_dev(bank), n, Sm)
    before = maps.buf.clone()
    codec.label_targets(maps.ptr, n, LW, LH, [lists[i % 7] for i in range(n)], [values[i % 7] for i in range(n)], out.ptr, map_dtype=np.dtype(map_dtype).name,
                        dtype=dtype, default=default, stream=_stream())
    _sync()
    assert_banked(out, to_dev(want), n, So, f"label_targets index {dtype}")
    assert_same(maps.buf, before, maps, "label_targets, maps", Sm)
    assert codec.allocated_bytes() <= codec.label_targets_workspace_bytes(n, sum(len(lists[i % 7]) for i in range(n)))


def test_a_label_targets_index_u8_to_uint8(mi):
    run_leg(mi, "A_targets_index_u8_u8_21400", 3 * 21400 * LH * LW, lambda codec, leg: label_index_many(mi, codec, 21400, np.uint8, "uint8", True))


def test_a_label_targets_index_u16_to_int64(mi):
    run_leg(mi, "A_targets_index_u16_i64_2800", 2800 * LH * LW * 12, lambda codec, leg: label_index_many(mi, codec, 2800, np.uint16, "int64", False))


def label_planes_many(mi, codec, oh, ow, n, planes):
    import torch

    from test_label_boxes import blobs
    from test_label_targets import value_spec

    P = oh * ow
    assert n * planes * P > M32 and planes == mi.label_targets_max_planes()
    rng = np.random.default_rng(57)
    maps_h = blobs(rng, n, oh, ow, 60)
    lists = [list(range(0, 50)), list(range(5, 60)), list(range(0, 60, 2))][:n]
    values = [rng.integers(-1, planes + 2, size=len(l)).tolist() for l in lists]
    for m in (M31, M32):  # the planes around the marks take pixels
        i, k = divmod(m // P, planes)
        for d in (-1, 0, 1):
            values[i][(k + d) % len(values[i])] = k + d
    default = planes // 2
    vm = torch.from_numpy(value_spec(maps_h, lists, values, default).reshape(n, P)).to(DEV)
    maps, out = Held(n * P, 3, value=0), Held(n * planes * P, 3)
    put_samples(maps.buf, maps, range(n), P, maps_h)
    before = maps.buf.clone()
    codec.label_targets(maps.ptr, n, ow, oh, lists, values, out.ptr, kind="planes", dtype="uint8", default=default, planes=planes, on=255, off=7, stream=_stream())
    _sync()
    ov = out.body.view(n, planes, P)
    on, off = torch.tensor(255, dtype=torch.uint8, device=DEV), torch.tensor(7, dtype=torch.uint8, device=DEV)
    step = max(1, PIECE // P)
    ons = 0
    for i in range(n):
        for a in range(0, planes, step):
            b = min(planes, a + step)
            hit = vm[i][None] == torch.arange(a, b, device=DEV)[:, None]
            ons += int(hit.sum())
            assert torch.equal(ov[i, a:b], torch.where(hit, on, off)), f"label_targets planes: sample {i}, planes {a}..{b - 1}"
    assert ons > n * P // 2
    assert bool((out.buf[:out.lo] == 0x5A).all()) and bool((out.buf[out.lo + out.nbytes:] == 0x5A).all())
    assert_same(maps.buf, before, maps, "label_targets planes, maps", P)


def test_a_label_targets_planes_uint8(mi):
    run_leg(mi, "A_targets_planes_u8_3x4096", 3 * 4096 * 800 * 450 + (1 << 30), lambda codec, leg: label_planes_many(mi, codec, 450, 800, 3, 4096))


# ---- leg B: one sample past 2^32 bytes: the offsets inside a sample --------------------------------------------------------------
def erase_rect(v, rect, values, layout):
    """RandomErasing of one sample, in place on its uint8 view v [c, h, w] / [h, w, c]"""
    import torch

    x, y, w, h = rect
    val = torch.as_tensor(values, dtype=v.dtype, device=v.device)
    if layout == "chw":
        v[:, y:y + h, x:x + w] = val.view(-1, 1, 1)
    else:
        v[y:y + h, x:x + w, :] = val.view(1, 1, -1)


def swap_box(v, box, layout):
    """CutMix of two samples that are each other's partner with the same box, in place on v [2, ...]"""
    x, y, w, h = box
    r = v[:, :, y:y + h, x:x + w] if layout == "chw" else v[:, y:y + h, x:x + w, :]
    r.copy_(r.flip(0))


INVERSE = {1: 1, 2: 2, 3: 5, 4: 4, 5: 3, 6: 6, 7: 7}


def orient_band(o, code, r0, r1):
    """rows [r0, r1) of the square HWC sample o [s, s, c] under the code, from the rows or columns of o they come from"""
    s = o.shape[0]
    return {1: lambda: o[r0:r1].flip(1), 2: lambda: o[s - r1:s - r0].flip(0), 3: lambda: o[:, s - r1:s - r0].flip(1).transpose(0, 1),
            4: lambda: o[s - r1:s - r0].flip(0).flip(1), 5: lambda: o[:, r0:r1].transpose(0, 1).flip(1), 6: lambda: o[:, r0:r1].transpose(0, 1),
            7: lambda: o[:, s - r1:s - r0].transpose(0, 1).flip(0).flip(1)}[code]()


def copy_piece(dv, sv, p):
    """a compose piece (dx, dy, sx, sy, w, h) between two HWC samples, in place on dv"""
    dx, dy, sx, sy, w, h = p
    dv[dy:dy + h, dx:dx + w] = sv[sy:sy + h, sx:sx + w]


def paste_piece(dv, sv, mv, p, ids):
    """a paste piece between two HWC samples with the u8 id map mv [ih, iw] of the src sample, in place on dv"""
    import torch

    dx, dy, sx, sy, w, h = p
    lut = torch.zeros(256, dtype=torch.bool, device=dv.device)
    lut[torch.as_tensor(list(ids), dtype=torch.long, device=dv.device)] = True
    sel = lut[mv[sy:sy + h, sx:sx + w].long()]
    dv[dy:dy + h, dx:dx + w] = torch.where(sel[..., None], sv[sy:sy + h, sx:sx + w], dv[dy:dy + h, dx:dx + w])


def test_the_in_sample_formulations_are_the_numpy_specs(mi):
    import torch

    import compose_spec
    import mix_spec
    import orient_spec
    import paste_spec
    from mix_batches import Case, to_layout

    t = mix_spec.gen_batch("uint8", 5, 3, 9, 11, seed=6)
    rects, ev = [(2, 3, 5, 4), None, (0, 0, 11, 1), (10, 8, 1, 1), (0, 0, 11, 9)], [3.0, 0.0, 200.0]
    for layout in ("chw", "hwc"):
        v = torch.from_numpy(to_layout(t, layout).copy())
        for i, r in enumerate(rects):
            if r:
                erase_rect(v[i], r, [3, 0, 200], layout)
        assert np.array_equal(v.numpy(), Case(None, erase=rects, erase_value=ev).expected(t, layout)), layout
        v = torch.from_numpy(to_layout(t[:2], layout).copy())
        swap_box(v, (1, 4, 9, 5), layout)
        assert np.array_equal(v.numpy(), Case([1, 0], boxes=(1, 4, 9, 5)).expected(t[:2], layout)), layout
    o = orient_spec.gen_batch("uint8", 1, 3, 7, 7, "hwc", seed=7)
    for code in range(1, 8):
        want = orient_spec.apply(o, [code], "hwc")[0]
        got = torch.cat([orient_band(torch.from_numpy(o[0]), code, r0, min(7, r0 + 3)) for r0 in range(0, 7, 3)])
        assert np.array_equal(got.numpy(), want), code
        assert np.array_equal(orient_spec.apply(want[None], [INVERSE[code]], "hwc")[0], o[0]), code
    src, dst = compose_spec.gen_batch("uint8", 1, 3, 8, 9, "hwc", 8), compose_spec.gen_batch("uint8", 1, 3, 10, 11, "hwc", 9)
    mask = paste_spec.gen_mask(np.random.default_rng(10), 1, 8, 9)
    ps, ids = [(1, 2, 3, 0, 5, 6), (4, 7, 0, 5, 7, 3), (0, 0, 2, 2, 3, 3)], [[0, 3, 5], range(1, 8, 2), [7]]
    dv, sv = torch.from_numpy(dst[0].copy()), torch.from_numpy(src[0].copy())
    for p in ps:
        copy_piece(dv, sv, p)
    assert np.array_equal(dv.numpy(), compose_spec.apply(src, dst, [(0, 0) + p for p in ps], "hwc", "uint8", keep=True)[0])
    dv = torch.from_numpy(dst[0].copy())
    for p, m in zip(ps, ids):
        paste_piece(dv, sv, torch.from_numpy(mask[0]), p, m)
    assert np.array_equal(dv.numpy(), paste_spec.apply(src, mask, dst, [(0, 0) + p + (m,) for p, m in zip(ps, ids)], "hwc", "uint8")[0])


def mix_one_sample(mi, codec, layout, side, tail=400, wide=300):
    import torch

    c = 3
    S = c * side * side
    assert S > M32, "precondition: the sample passes 2^32 bytes"
    if layout == "hwc":
        y32, r = divmod(M32, side * c)
        x32 = r // c
    else:
        y32, x32 = divmod(M32 % (side * side), side)
    shape = (c, side, side) if layout == "chw" else (side, side, c)
    held = Held(2 * S, 3, seed=61)
    want = held.buf.clone()
    wv = body_of(want, held, torch.uint8, (2,) + shape)
    across = (min(max(0, x32 - wide // 2), side - wide), y32 - 2, wide, 5)
    assert across[0] <= x32 < across[0] + wide and across[1] <= y32 < across[1] + 5 <= side, "element 2^32 lies in an erased rectangle"
    for rect in ((5, 0, side - 9, 3), across, (side - wide - 1, side - wide // 2, wide + 1, wide // 2)):
        codec.mix_batch(held.ptr, 1, side, side, mi.mix_samples(1, None, None, None, rect), dtype="uint8", layout=layout, erase_value=[3.0, 0.0, 200.0],
                        stream=_stream())
        _sync()
        erase_rect(wv[0], rect, [3, 0, 200], layout)
        assert_same(held.buf, want, held, f"mix_batch {layout} {side}, erase {rect}", S)
    box = (0, side - tail, side, tail)  # (every element of it lies past element 2^32 in HWC; in CHW that of the last plane)
    codec.mix_batch(held.ptr, 2, side, side, mi.mix_samples(2, [1, 0], None, box, None), dtype="uint8", layout=layout, stream=_stream())
    _sync()
    swap_box(wv, box, layout)
    assert_same(held.buf, want, held, f"mix_batch {layout} {side}, two samples", S)
    assert codec.allocated_bytes() <= codec.mix_workspace_bytes(2, side, side, "uint8")


@pytest.mark.parametrize("side", (38000, 37999))
@pytest.mark.parametrize("layout", ("hwc", "chw"))
def test_b_mix_batch_one_sample_past_2_32(mi, layout, side):
    assert (3 * side * side % 16 == 0) == (side == 38000)
    run_leg(mi, f"B_mix_u8_{layout}_{side}", 4 * 3 * side * side, lambda codec, leg: mix_one_sample(mi, codec, layout, side))


def orient_one_sample(mi, codec, side, band=2048):
    import torch

    c = 3
    S = c * side * side
    assert S > M32
    held = Held(S, 3, seed=62)
    orig = held.buf.clone()
    gv, ov = body_of(held.buf, held, torch.uint8, (side, side, c)), body_of(orig, held, torch.uint8, (side, side, c))
    for code in range(1, 8):
        codec.orient_batch(held.ptr, 1, side, side, [code], dtype="uint8", layout="hwc", stream=_stream())
        _sync()
        for r0 in range(0, side, band):
            r1 = min(side, r0 + band)
            assert torch.equal(gv[r0:r1], orient_band(ov, code, r0, r1)), f"orient_batch code {code}: rows {r0}..{r1 - 1} differ"
        assert bool((held.buf[:held.lo] == 0x5A).all()) and bool((held.buf[held.lo + S:] == 0x5A).all()), f"orient_batch code {code}: a guard byte was written"
        codec.orient_batch(held.ptr, 1, side, side, [INVERSE[code]], dtype="uint8", layout="hwc", stream=_stream())
        _sync()
        assert_same(held.buf, orig, held, f"orient_batch code {code} and its inverse")
    assert codec.allocated_bytes() <= codec.orient_workspace_bytes(1)


def test_b_orient_batch_one_sample_past_2_32(mi):
    run_leg(mi, "B_orient_u8_hwc_38000", 3 * 3 * 38000 * 38000, lambda codec, leg: orient_one_sample(mi, codec, 38000))


def place_one_sample(mi, codec, side, paste):
    import torch

    c = 3
    S = c * side * side
    assert S > M32
    y32 = M32 // (side * c)  # the row that holds byte 2^32 of a sample
    assert 40 < y32 < side - 40
    src, dst = Held(S, 3, seed=63), Held(S, 5, seed=64)
    mask = Held(side * side, 7, seed=65) if paste else None
    src_before, want = src.buf.clone(), dst.buf.clone()
    mask_before = mask.buf.clone() if paste else None
    sv, wv = body_of(src_before, src, torch.uint8, (side, side, c)), body_of(want, dst, torch.uint8, (side, side, c))
    # (dx, dy, sx, sy, w, h): src rows below byte 2^32 to dst rows across it; src rows across it to dst rows below; the last pixel of both
    ps = [(100, y32 - 3, 7, 11, side // 2, 10), (9, 20, side // 3, y32 - 5, side // 2, 10), (side - 64, side - 32, side - 64, side - 32, 64, 32),
          (side // 2, y32 - 1, 1, y32 + 2, side // 3, 7)]
    ids = [range(0, 128), range(1, 256, 2), [0, 7, 200, 255] + list(range(30, 99)), range(64, 256)]
    if paste:
        codec.paste_batch(src.ptr, mask.ptr, 1, side, side, dst.ptr, 1, side, side, [(0, 0) + p + (m,) for p, m in zip(ps, ids)], dtype="uint8", layout="hwc",
                          stream=_stream())
    else:
        codec.compose_batch(src.ptr, 1, side, side, dst.ptr, 1, side, side, [(0, 0) + p for p in ps], dtype="uint8", layout="hwc", keep=True, stream=_stream())
    _sync()
    for p, m in zip(ps, ids):
        if paste:
            paste_piece(wv, sv, body_of(mask_before, mask, torch.uint8, (side, side)), p, m)
        else:
            copy_piece(wv, sv, p)
    what = "paste_batch" if paste else "compose_batch"
    assert_same(dst.buf, want, dst, f"{what} one sample, dst")
    assert_same(src.buf, src_before, src, f"{what} one sample, src")
    if paste:
        assert_same(mask.buf, mask_before, mask, f"{what} one sample, mask")


def test_b_compose_batch_one_sample_past_2_32(mi):
    run_leg(mi, "B_compose_u8_hwc_38000", 4 * 3 * 38000 * 38000, lambda codec, leg: place_one_sample(mi, codec, 38000, False))


def test_b_paste_batch_one_sample_past_2_32(mi):
    run_leg(mi, "B_paste_u8_hwc_38000", 5 * 3 * 38000 * 38000, lambda codec, leg: place_one_sample(mi, codec, 38000, True))


def closed_form(points_or_rects, ow, oh, P, background):
    """{id: [(x, y, w, h), ...]} of rectangles that do not overlap, over a background id that still reaches every edge
    -> {id: (count, x0, y0, x1, y1)}"""
    out, total = {}, 0
    for m, rs in points_or_rects.items():
        count = sum(w * h for _, _, w, h in rs)
        total += count
        out[m] = (count, min(r[0] for r in rs), min(r[1] for r in rs), max(r[0] + r[2] for r in rs), max(r[1] + r[3] for r in rs))
    out[background] = (P - total, 0, 0, ow, oh)
    return out


def label_boxes_one_sample(mi, codec, ow, oh):
    P = ow * oh
    assert M31 < P < M32
    maps = Held(2 * P, 3, value=17)  # sample 0: id 17 everywhere; every byte of sample 1 lies past byte 2^32 - 1 of the batch
    mv = maps.body.view(2, oh, ow)
    mv[1].fill_(200)
    y31, x31 = divmod(M31, ow)
    special = {1: [(0, 0, 1, 1)], 2: [(ow - 1, 0, 1, 1)], 3: [(0, oh - 1, 1, 1)], 4: [(ow - 1, oh - 1, 1, 1)], 5: [(ow // 2, oh - 1, 1, 1)],
               6: [(1, 0, 1, 1)],  # (byte 2^32 of the batch, where P is 2^32 - 1)
               7: [(x31, y31, 1, 1)], 9: [(5, 7, 1, 1), (ow - 3, oh - 2, 1, 1)]}
    for m, rs in special.items():
        for x, y, w, h in rs:
            mv[1, y:y + h, x:x + w] = m
    before = maps.buf.clone()
    out = Held(2 * 256 * 20, 12)
    codec.label_boxes(maps.ptr, 2, ow, oh, out.ptr, stream=_stream())
    _sync()
    want = np.zeros((2, 256, 5), np.int64)
    want[:] = (0, ow, oh, 0, 0)
    want[0, 17] = (P, 0, 0, ow, oh)
    for m, rec in closed_form(special, ow, oh, P, 200).items():
        want[1, m] = rec
    assert want[1, 200, 0] == P - 9 and (P < 1 << 31 or want[1, 200, 0] >= 1 << 31)
    host = out.buf.cpu().numpy()
    assert (host[:out.lo] == 0x5A).all() and (host[out.lo + out.nbytes:] == 0x5A).all()
    got = host[out.lo:out.lo + out.nbytes].copy().view("<u4").reshape(2, 256, 5).astype(np.int64)
    assert np.array_equal(got, want), np.argwhere(got != want)[:6].tolist()
    assert_same(maps.buf, before, maps, "label_boxes one sample, maps", P)


def test_b_label_boxes_largest_sample(mi):
    ow, oh = 65537, 65535
    assert ow * oh == M32 - 1
    run_leg(mi, "B_label_boxes_u8_65537x65535", 4 * ow * oh, lambda codec, leg: label_boxes_one_sample(mi, codec, ow, oh))


def label16_one_sample(mi, codec, ow, oh):
    import torch

    P = ow * oh
    assert P > M31 and 2 * P > M32
    y31 = M31 // ow  # the row that holds pixel 2^31
    assert 45 < y31 < oh - 3
    back = 0x0100
    x31, w1 = M31 % ow, min(20000, ow - 200)
    x1 = min(max(0, x31 - w1 // 2), ow - w1)
    assert x1 <= x31 < x1 + w1  # pixel 2^31 lies in the rectangle of 0x0101, which has rows on both sides of it
    rects = {0x0001: [(0, 0, min(1000, ow - 1), 2)], 0x0101: [(x1, y31 - 1, w1, 3)], 0xFF01: [(ow - 300, oh - 1, 300, 1), (7, oh - 2, 5, 1)],
             0x0201: [(3, y31 - 40, min(5000, ow - 3), 2)]}  # (0x0201 is not listed)
    maps = Held(2 * P, 6, value=0)
    mv = maps.body.view(torch.int16).view(oh, ow)
    mv.fill_(back)
    for m, rs in rects.items():
        for x, y, w, h in rs:
            mv[y:y + h, x:x + w] = m - (m >> 15 << 16)
    before = maps.buf.clone()
    listed = [0x0001, back, 0x0101, 700, 0xFF01]
    # label_boxes16: closed form
    form = closed_form(rects, ow, oh, P, back)
    assert form[back][0] > M31
    want = np.array([form.get(m, (0, ow, oh, 0, 0)) for m in listed], np.int64)
    out = Held(len(listed) * 20, 12)
    codec.label_boxes16(maps.ptr, 1, ow, oh, [listed], out.ptr, stream=_stream())
    _sync()
    host = out.buf.cpu().numpy()
    assert (host[:out.lo] == 0x5A).all() and (host[out.lo + out.nbytes:] == 0x5A).all()
    got = host[out.lo:out.lo + out.nbytes].copy().view("<u4").reshape(-1, 5).astype(np.int64)
    assert np.array_equal(got, want), [(listed[j], got[j].tolist(), want[j].tolist()) for j in np.flatnonzero((got != want).any(1))]
    del out
    # label_targets: a table gather on the device
    step = max(1, PIECE // (8 * ow))

    def lut_of(values, default):
        lut = torch.full((65536,), default, dtype=torch.int32, device=DEV)
        lut[torch.as_tensor(listed, dtype=torch.long, device=DEV)] = torch.as_tensor(values, dtype=torch.int32, device=DEV)
        return lut

    values = [3, -7, 1 << 20, 5, -(1 << 31)]
    out = Held(4 * P, 12)
    assert out.nbytes > 1 << 33 or M32 < 1 << 32
    codec.label_targets(maps.ptr, 1, ow, oh, [listed], [values], out.ptr, map_dtype="uint16", dtype="int32", default=-100, stream=_stream())
    _sync()
    lut, ov = lut_of(values, -100), out.body.view(torch.int32).view(oh, ow)
    for r0 in range(0, oh, step):
        r1 = min(oh, r0 + step)
        assert torch.equal(ov[r0:r1], lut[mv[r0:r1].long() & 0xFFFF]), f"label_targets index: rows {r0}..{r1 - 1} differ"
    assert bool((out.buf[:out.lo] == 0x5A).all()) and bool((out.buf[out.lo + out.nbytes:] == 0x5A).all())
    del out, ov
    values = [1, 0, 1, 0, 2]  # (0xFF01 has no plane, 0x0201 takes the default: none either)
    out = Held(2 * P, 3)
    codec.label_targets(maps.ptr, 1, ow, oh, [listed], [values], out.ptr, map_dtype="uint16", kind="planes", dtype="uint8", default=-1, planes=2, on=255, off=7,
                        stream=_stream())
    _sync()
    lut, ov = lut_of(values, -1), out.body.view(2, oh, ow)
    on, off = torch.tensor(255, dtype=torch.uint8, device=DEV), torch.tensor(7, dtype=torch.uint8, device=DEV)
    for r0 in range(0, oh, step):
        r1 = min(oh, r0 + step)
        v = lut[mv[r0:r1].long() & 0xFFFF]
        for k in range(2):
            assert torch.equal(ov[k, r0:r1], torch.where(v == k, on, off)), f"label_targets planes: plane {k}, rows {r0}..{r1 - 1} differ"
    assert bool((out.buf[:out.lo] == 0x5A).all()) and bool((out.buf[out.lo + out.nbytes:] == 0x5A).all())
    assert_same(maps.buf, before, maps, "label16 one sample, maps")


def test_b_label_boxes16_and_targets_one_sample_past_2_31_pixels(mi):
    ow, oh = 46342, 46343
    run_leg(mi, "B_label16_u16_46342x46343", 8 * ow * oh, lambda codec, leg: label16_one_sample(mi, codec, ow, oh))


# ---- leg C: formatted view outputs past 2^32 bytes -------------------------------------------------------------------------------
VW, VH, VC, VOUT = 241, 229, 3, 224  # three frames in planar 8 x 8 tiles; the views' side (no larger than a frame: the workspace bounds hold)
VRECTS = [(0, 0, 241, 229), (10, 5, 200, 180), (33, 20, 57, 91), (233, 223, 8, 6), (1, 1, 239, 227)]
BLUR_INVERT = [("gaussian_blur", 1.5), "invert"]  # an area op, then the point op that stores the formatted output
VES = {"float32": 4, "float16": 2, "uint8": 1}


def view_matrices():
    from test_gpu_warped_views import rot

    return [rot(30, 120, 115, 111.5, 111.5, 0.9), [1.0, 0.35, -3.0, 0.15, 0.9, 2.0], rot(-50, 100, 110, 111.5, 111.5, 0.5), [0.75, 0.0, 5.25, 0.0, 1.0, -2.5],
            rot(12, 200, 190, 100.0, 90.0, 1.1)]  # (the last reads past the frame: the fill)


def view_list(kind, n, filt):
    """view v: frame v % 3, rectangle or matrix v % 5, mirrored by v % 2 -- 30 classes, view v in class v % 30"""
    per = VRECTS if kind != "warp" else view_matrices()
    return [(v % 3, *per[v % 5], (filt << 4) | (v % 2)) for v in range(n)]


def view_classes(mi, imgs, kind, filt, dtype, layout):
    """the 30 distinct outputs [30, ...] in the format, from the numpy resize spec (PIL's transform for the warped views), the numpy
    photo spec and the output table"""
    import photo_spec
    from test_gpu_resized_output import norm, place
    from test_gpu_views import G

    views = view_list(kind, 30, filt)
    if kind == "warp":
        from PIL import Image

        from test_gpu_warped_views import WG, pil_one

        return WG(views, VOUT, VOUT, dtype, layout).expected(mi, imgs, pil_one(Image))
    if kind == "views":
        return G(views, VOUT, VOUT, dtype, layout).expected(mi, imgs)
    u8 = G(views, VOUT, VOUT).expected(mi, imgs)
    u8 = np.stack([photo_spec.apply(v, BLUR_INVERT) for v in u8])
    return place(mi.output_table(VC, dtype, **norm(VC, dtype)), u8, layout)


def views_many(mi, orc, name, kind, n, dtype, layout, filt):
    import torch

    from test_gpu_regions_host import make_batch
    from test_gpu_resized_output import norm
    from test_gpu_resized_regions import packed

    vb = VOUT * VOUT * VC * VES[dtype]
    b31, b32 = straddlers(n, vb)
    assert b31 % 30 and b32 % 30
    leg = BatchLeg(mi, name)
    leg.need(n * vb + (4 << 30))
    imgs, conts = make_batch(orc, 3, VW, VH, VC, 8, 8, True)
    want = view_classes(mi, imgs, kind, filt, dtype, layout)
    assert len({want[k].tobytes() for k in range(30)}) == 30, "30 distinct outputs"
    codec = mi.Codec(3, VW, VH, VC, 8, 8, True, device=0)
    try:
        d_pay, n_pay, d_len = packed(mi, conts)
        pay_before, len_before = d_pay.clone(), d_len.clone()
        out = Held(n * vb, 4)
        st = torch.full((1,), 0x5A5A, dtype=torch.int32, device=DEV)
        views = view_list(kind, n, filt)
        fmt = dict(dtype=dtype, layout=layout, **norm(VC, dtype))
        if kind == "warp":
            codec.decode_warped_views(d_pay.data_ptr(), n_pay, d_len.data_ptr(), [mi.WarpGroup(views, VOUT, VOUT, out.ptr, **fmt)], st.data_ptr(), _stream())
        else:
            group = mi.ViewGroup(views, VOUT, VOUT, out.ptr, photo=BLUR_INVERT if kind == "photo" else None, **fmt)
            codec.decode_views(d_pay.data_ptr(), n_pay, d_len.data_ptr(), [group], st.data_ptr(), _stream())
        _sync()
        assert int(st.item()) == 0, f"status {int(st.item()):#x}"
        assert_banked(out, to_dev(want), n, vb, name)
        assert torch.equal(d_pay, pay_before) and torch.equal(d_len, len_before), f"{name}: the payload or the slice lengths were written"
        bound = {"views": codec.views_workspace_bytes, "warp": codec.warp_workspace_bytes, "photo": codec.photo_workspace_bytes}[kind](n)
        assert codec.allocated_bytes() <= bound, (codec.allocated_bytes(), bound)
        leg.report()
        del out
    finally:
        codec.close()
        _release(mi)


def test_c_decode_views_float32_chw_bilinear(mi, orc):
    views_many(mi, orc, "C_views_f32_chw_7200", "views", 7200, "float32", "chw", 0)


def test_c_decode_views_float32_chw_lanczos(mi, orc):
    import resize_filters_spec as spec

    views_many(mi, orc, "C_views_lanczos_f32_chw_7200", "views", 7200, "float32", "chw", spec.LANCZOS)


def test_c_decode_views_float16_hwc(mi, orc):
    views_many(mi, orc, "C_views_f16_hwc_14400", "views", 14400, "float16", "hwc", 0)


def test_c_decode_warped_views_float32_chw_bilinear(mi, orc):
    import resize_filters_spec as spec

    views_many(mi, orc, "C_warped_f32_chw_7200", "warp", 7200, "float32", "chw", spec.BILINEAR)


def test_c_decode_views_photo_chain_float32_chw(mi, orc):
    views_many(mi, orc, "C_photo_f32_chw_7200", "photo", 7200, "float32", "chw", 0)


# The three stores index ELEMENTS -- (v * c + ch) * plane + px -- and scale to bytes in the pointer: 7200 float32 views pass 2^32 bytes
# at 1.1 * 10^9 elements.  28560 uint8 CHW views pass 2^32 elements (and so do the u8 intermediates of the resample and of the chains).
@pytest.mark.parametrize("kind", ("views", "warp", "photo"))
def test_c_uint8_chw_past_2_32_elements(mi, orc, kind):
    assert 28560 * VOUT * VOUT * VC > M32
    views_many(mi, orc, f"C_{kind}_u8_chw_28560", kind, 28560, "uint8", "chw", 0)
