"""Resized regions decode in an output format (llcomp_mi_codec_decode_resized_regions_ex, ..._host_ex,
llcomp_mi_stream_submit_decode_resized_regions_ex): the u8 call's value of every output element, looked up in llcomp_mi_output_table and
placed in the layout.  The expected output is output_table[ch][u8] over the numpy statement of the resampling rule (tests/resize_spec.py),
bit for bit; for f32 CHW with ImageNet values it is also torch's ToTensor() + Normalize() chain over the u8 call's own bytes."""
import zlib

import numpy as np
import pytest

import orc as orc_mod
from conftest import make_image
from resize_spec import random_resized_crop
from test_gpu_regions_host import GUARD, Out, make_batch, stream
from test_gpu_resized_regions import CROPS, FAMILIES, _batch_rects, expected, packed

pytestmark = pytest.mark.gpu

IMAGENET_MEAN = [0.485, 0.456, 0.406]
IMAGENET_STD = [0.229, 0.224, 0.225]
ESIZE = {"uint8": 1, "float32": 4, "float16": 2, "bfloat16": 2}
NP = {"uint8": np.uint8, "float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


def norm(c, dtype):
    """the format's keyword arguments: ImageNet-like mean / std for every float dtype (c values), nothing for uint8"""
    if dtype == "uint8":
        return {}
    return dict(scale=True, mean=[IMAGENET_MEAN[i % 3] + 0.01 * (i // 3) for i in range(c)],
                std=[IMAGENET_STD[i % 3] + 0.02 * (i // 3) for i in range(c)])


def place(table, u8, layout):
    """u8 [F, oh, ow, c] -> table[ch][u8] in the layout: [F, oh, ow, c] (hwc) or [F, c, oh, ow] (chw)"""
    c = u8.shape[-1]
    v = np.stack([table[ch][u8[..., ch]] for ch in range(c)], axis=-1)
    return np.ascontiguousarray(v.transpose(0, 3, 1, 2) if layout == "chw" else v)


class TOut:
    """an output of `frames` elements of `dtype` in a layout, `offset` bytes past a GUARD boundary, guard bytes on both sides, a status"""

    def __init__(self, frames, ow, oh, c, dtype, layout, offset=0, status=0):
        import torch

        self.nbytes = frames * oh * ow * c * ESIZE[dtype]
        self.dtype, self.offset = dtype, offset
        self.shape = (frames, c, oh, ow) if layout == "chw" else (frames, oh, ow, c)
        self.buf = torch.full((self.nbytes + 2 * GUARD + offset,), 0x5A, dtype=torch.uint8, device="cuda")
        self.st = torch.full((1,), status, dtype=torch.int32, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD + offset

    def read(self):
        import torch

        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        lo, hi = GUARD + self.offset, GUARD + self.offset + self.nbytes
        assert (host[:lo] == 0x5A).all() and (host[hi:] == 0x5A).all(), "a byte outside the output was written"
        return int(self.st.item()) & 0xFFFFFFFF, host[lo:hi].copy().view(NP[self.dtype]).reshape(self.shape)


def run_dev(codec, dev, rects, ow, oh, c, dtype, layout, flags=None, offset=0, **kw):
    d_pay, n, d_len = dev
    o = TOut(len(rects), ow, oh, c, dtype, layout, offset)
    codec.decode_resized_regions(d_pay.data_ptr(), n, d_len.data_ptr(), rects, ow, oh, o.ptr, o.st.data_ptr(), flags=flags, stream=stream(),
                                 dtype=dtype, layout=layout, **kw)
    return o.read()


def run_host(codec, conts, rects, ow, oh, c, dtype, layout, flags=None, offset=0, **kw):
    o = TOut(len(rects), ow, oh, c, dtype, layout, offset)
    codec.decode_resized_regions_host(conts, rects, ow, oh, o.ptr, o.st.data_ptr(), flags=flags, stream=stream(), dtype=dtype, layout=layout, **kw)
    return o.read()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


FORMATS = [(d, lay) for d in ("uint8", "float32", "float16", "bfloat16") for lay in ("hwc", "chw")]


@pytest.mark.parametrize("case", CROPS, ids=[c[0] for c in CROPS])
def test_every_format_is_the_table_over_the_u8_output(mi, orc, case):
    name, w, h, c, tw, th, planar, frames, kind, (ow, oh), _ = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    imgs, conts = make_batch(orc, frames, w, h, c, tw, th, planar)
    rects = _batch_rects(rng, w, h, frames, kind)
    flags = np.array([f % 2 for f in range(frames)], np.uint8)
    codec = mi.Codec(frames, w, h, c, tw, th, planar, device=0)
    try:
        dev = packed(mi, conts)
        u8 = {True: expected(mi, imgs, rects, ow, oh, flags), False: expected(mi, imgs, rects, ow, oh)}
        for dtype, layout in FORMATS:
            kw = norm(c, dtype)
            table = mi.output_table(c, dtype, **kw)
            for mirrored in (True, False):
                want = place(table, u8[mirrored], layout)
                fl = flags if mirrored else None
                for host in (False, True):
                    run = run_host if host else run_dev
                    st, out = run(codec, conts if host else dev, rects, ow, oh, c, dtype, layout, fl, **kw)
                    assert st == 0 and same_bits(out, want), (dtype, layout, mirrored, host)
    finally:
        codec.close()


@pytest.mark.parametrize("case", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_f32_chw_imagenet_is_the_torch_chain(mi, orc, case):
    """f32 CHW with ImageNet's mean and std: torch.equal to ToTensor() + Normalize() (torch's CPU ops) over the u8 call's own output"""
    import torch

    name, frames, w, h, c, tw, th, planar, small, rw, rh, xy = case
    imgs, conts = make_batch(orc, frames, w, h, c, tw, th, planar, small_model=small)
    codec = mi.Codec(frames, w, h, c, tw, th, planar, device=0, small_model=small)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    rects = [random_resized_crop(rng, w, h) for _ in range(frames)]
    flags = np.array([1 - f % 2 for f in range(frames)], np.uint8)
    try:
        dev = packed(mi, conts)
        ref = Out(frames, 64, 48, c)
        codec.decode_resized_regions(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), rects, 64, 48, ref.ptr, ref.st.data_ptr(), flags=flags,
                                     stream=stream())
        st_r, u8 = ref.read()
        assert st_r == 0
        mean, std = torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1), torch.tensor(IMAGENET_STD).view(1, 3, 1, 1)
        chain = torch.from_numpy(u8).permute(0, 3, 1, 2).float().div(255).sub(mean).div(std).contiguous()
        for host in (False, True):
            run = run_host if host else run_dev
            st, out = run(codec, conts if host else dev, rects, 64, 48, c, "float32", "chw", flags, scale=True, mean=IMAGENET_MEAN,
                          std=IMAGENET_STD)
            assert st == 0 and torch.equal(torch.from_numpy(out), chain), host
    finally:
        codec.close()


def test_null_and_explicit_u8_hwc_are_the_u8_call(mi, orc):
    w, h, c = 300, 200, 3
    imgs, conts = make_batch(orc, 3, w, h, c, 64, 64, True)
    codec = mi.Codec(3, w, h, c, 64, 64, True, device=0)
    rects = [(0, 0, 300, 200), (10, 20, 50, 30), (299, 199, 1, 1)]
    flags = np.array([1, 0, 1], np.uint8)
    try:
        dev = packed(mi, conts)
        ref = Out(3, 80, 60, c)
        codec.decode_resized_regions(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), rects, 80, 60, ref.ptr, ref.st.data_ptr(), flags=flags,
                                     stream=stream())
        st_r, want = ref.read()
        assert st_r == 0 and np.array_equal(want, expected(mi, imgs, rects, 80, 60, flags))
        # fmt = NULL through the C entry points themselves
        import ctypes as C

        L = mi._lib.load()
        o = TOut(3, 80, 60, c, "uint8", "hwc")
        assert L.llcomp_mi_codec_decode_resized_regions_ex(codec._h, dev[0].data_ptr(), dev[1], dev[2].data_ptr(),
                                                           (C.c_uint32 * 12)(*[v for r in rects for v in r]), flags.ctypes.data, 80, 60, None,
                                                           o.ptr, o.st.data_ptr(), stream()) == mi.OK
        st, out = o.read()
        assert st == 0 and np.array_equal(out, want)
        # {U8, HWC} explicitly
        for host in (False, True):
            st, out = (run_host(codec, conts, rects, 80, 60, c, "uint8", "hwc", flags) if host
                       else run_dev(codec, dev, rects, 80, 60, c, "uint8", "hwc", flags))
            assert st == 0 and np.array_equal(out, want), host
    finally:
        codec.close()


@pytest.mark.parametrize("c", [3, 4])
def test_f16_at_a_two_byte_boundary(mi, orc, c):
    """an f16 output 2-byte aligned but not 4-byte aligned: HWC at c = 4 takes the per-element path, the bits are the same"""
    w, h = 300, 200
    imgs, conts = make_batch(orc, 3, w, h, c, 64, 64, False)
    codec = mi.Codec(3, w, h, c, 64, 64, False, device=0)
    rects = [(0, 0, 120, 90), (150, 60, 40, 33), (299, 199, 1, 1)]
    flags = np.array([1, 0, 1], np.uint8)
    kw = norm(c, "float16")
    try:
        table = mi.output_table(c, "float16", **kw)
        u8 = expected(mi, imgs, rects, 57, 43, flags)
        for layout in ("hwc", "chw"):
            st, out = run_host(codec, conts, rects, 57, 43, c, "float16", layout, flags, offset=2, **kw)
            assert st == 0 and same_bits(out, place(table, u8, layout)), layout
    finally:
        codec.close()


def test_misaligned_and_bad_formats_write_nothing(mi, orc):
    import ctypes as C

    w, h, c = 300, 200, 3
    imgs, conts = make_batch(orc, 2, w, h, c, 64, 64, True)
    codec = mi.Codec(2, w, h, c, 64, 64, True, device=0)
    dev = packed(mi, conts)
    rects = [(0, 0, 100, 100), (5, 5, 30, 20)]
    L = mi._lib.load()
    tab = (C.c_uint32 * 8)(*[v for r in rects for v in r])
    nan3 = (C.c_float * 3)(0.5, float("nan"), 0.5)
    zero3 = (C.c_float * 3)(0.5, 0.0, 0.5)
    fp = C.POINTER(C.c_float)
    size = C.sizeof(mi.OutputFormat)
    bad = [("f32_odd", mi.OutputFormat(size, mi.DTYPE_F32, mi.LAYOUT_CHW, 1, None, None), 1),
           ("f32_2", mi.OutputFormat(size, mi.DTYPE_F32, mi.LAYOUT_HWC, 1, None, None), 2),
           ("f16_odd", mi.OutputFormat(size, mi.DTYPE_F16, mi.LAYOUT_CHW, 0, None, None), 3),
           ("small_struct", mi.OutputFormat(size - 8, mi.DTYPE_F32, mi.LAYOUT_CHW, 1, None, None), 0),
           ("dtype", mi.OutputFormat(size, 7, mi.LAYOUT_CHW, 1, None, None), 0),
           ("layout", mi.OutputFormat(size, mi.DTYPE_F32, 3, 1, None, None), 0),
           ("u8_scale", mi.OutputFormat(size, mi.DTYPE_U8, mi.LAYOUT_CHW, 1, None, None), 0),
           ("u8_mean", mi.OutputFormat(size, mi.DTYPE_U8, mi.LAYOUT_HWC, 0, C.cast(zero3, fp), None), 0),
           ("mean_nan", mi.OutputFormat(size, mi.DTYPE_BF16, mi.LAYOUT_CHW, 1, C.cast(nan3, fp), None), 0),
           ("std_zero", mi.OutputFormat(size, mi.DTYPE_F16, mi.LAYOUT_HWC, 1, None, C.cast(zero3, fp)), 0)]
    try:
        for name, fmt, offset in bad:
            for host in (False, True):
                o = TOut(2, 32, 32, c, "float32", "chw", offset=offset, status=0x77)
                if host:
                    keep = [bytes(x) for x in conts]
                    ptrs = (C.c_void_p * 2)(*[C.cast(C.c_char_p(k), C.c_void_p).value for k in keep])
                    lens = (C.c_size_t * 2)(*[len(k) for k in keep])
                    rc = L.llcomp_mi_codec_decode_resized_regions_host_ex(codec._h, ptrs, lens, tab, None, 32, 32, C.byref(fmt), o.ptr,
                                                                          o.st.data_ptr(), stream())
                else:
                    rc = L.llcomp_mi_codec_decode_resized_regions_ex(codec._h, dev[0].data_ptr(), dev[1], dev[2].data_ptr(), tab, None, 32, 32,
                                                                     C.byref(fmt), o.ptr, o.st.data_ptr(), stream())
                assert rc == mi.BAD_ARGS, (name, host)
                st, out = o.read()
                assert st == 0x77 and (out.view(np.uint8) == 0x5A).all(), (name, host)
        # the same output at an aligned address: fine
        st, out = run_dev(codec, dev, rects, 32, 32, c, "float32", "chw", scale=True)
        assert st == 0 and same_bits(out, place(mi.output_table(c, "float32", scale=True), expected(mi, imgs, rects, 32, 32), "chw"))
    finally:
        codec.close()


def test_damage_gives_the_u8_verdict(mi, orc):
    w, h, c, tw, th = 512, 256, 3, 32, 32
    rects = [(100, 70, 60, 50), (300, 150, 20, 10)]
    imgs = np.stack([make_image("nat", w, h, c), make_image("mid", w, h, c)])
    n = len(orc_mod.slice_rects(w, h, c, tw, th, False))
    rng = np.random.default_rng(78)
    conts = []
    for f in range(2):
        d = orc.compress_sliced(imgs[f], tw, th, False)
        lens = np.frombuffer(d[24:24 + 4 * n], dtype="<u4").astype(np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)]) + 24 + 4 * n
        pays = [d[offs[j]:offs[j + 1]] for j in range(n)]
        if f == 1:  # tile row 6, column 11: inside frame 1's window
            res = orc_mod.adversarial_residuals(rng, th, tw, c, "small")
            pays[6 * 16 + 11] = orc.encode_residuals(res, run_at=th * tw * c // 2, run_len=33)[0]
        conts.append(orc_mod.sliced_container(w, h, c, tw, th, False, pays))
    codec = mi.Codec(2, w, h, c, tw, th, False, device=0)
    try:
        dev = packed(mi, conts)
        ref = Out(2, 40, 40, c)
        codec.decode_resized_regions(dev[0].data_ptr(), dev[1], dev[2].data_ptr(), rects, 40, 40, ref.ptr, ref.st.data_ptr(), stream=stream())
        st_u8, _ = ref.read()
        assert codec.status(st_u8) == mi.BAD_EXPONENT
        for dtype, layout in (("float32", "chw"), ("bfloat16", "hwc")):
            st, _ = run_dev(codec, dev, rects, 40, 40, c, dtype, layout, scale=True, mean=IMAGENET_MEAN, std=IMAGENET_STD)
            st_h, _ = run_host(codec, conts, rects, 40, 40, c, dtype, layout, scale=True, mean=IMAGENET_MEAN, std=IMAGENET_STD)
            assert st == st_h == st_u8, (dtype, layout)
    finally:
        codec.close()


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one", "devices00"])
def test_stream_jobs_mixed_with_u8_jobs(mi, orc, devices):
    fpj, w, h, c, tw, th = 4, 320, 48, 3, 80, 1
    n_jobs = 6
    imgs, conts = make_batch(orc, n_jobs * fpj, w, h, c, tw, th, True)
    s = mi.Stream(w, h, c, tw, th, True, depth=2, device=0, frames_per_job=fpj, devices=devices)
    rng = np.random.default_rng(23)
    ow, oh = 56, 40
    kinds = [("float32", "chw"), ("uint8", None), ("bfloat16", "hwc"), ("float16", "chw"), (None, None), ("uint8", "chw")]
    try:
        for j, (dtype, layout) in enumerate(kinds):
            part = conts[j * fpj:(j + 1) * fpj]
            rects = [random_resized_crop(rng, w, h) for _ in range(fpj)]
            flags = np.array([(j + f) % 2 for f in range(fpj)], np.uint8)
            kw = norm(c, dtype or "uint8")
            if layout:
                kw["layout"] = layout
            assert s.submit_decode_resized_regions(list(part), rects, ow, oh, flags=flags, tag=j, dtype=dtype, **kw)
            job = s.wait()
            assert (job.status, job.kind, job.tag) == (mi.OK, mi.JOB_DECODE_RESIZED_REGIONS, j)
            u8 = expected(mi, imgs[j * fpj:(j + 1) * fpj], rects, ow, oh, flags)
            table = mi.output_table(c, dtype or "uint8", **{k: v for k, v in kw.items() if k != "layout"})
            want = place(table, u8, layout or "hwc")
            assert job.data.dtype == NP[dtype or "uint8"] and job.data.shape == want.shape, (job.data.dtype, job.data.shape)
            assert same_bits(job.data, want), (dtype, layout)
            s.release(job)
        # an f32 output that a slot holds as u8 but not as f32: BAD_ARGS at submit, nothing queued
        with pytest.raises(mi.LlcompError) as e:
            s.submit_decode_resized_regions(list(conts[:fpj]), [(0, 0, 10, 10)] * fpj, w, h, dtype="float32")
        assert e.value.status == mi.BAD_ARGS
        assert s.submit_decode_resized_regions(list(conts[:fpj]), [(0, 0, 10, 10)] * fpj, w, h)  # (u8 of that size fits)
        job = s.wait()
        assert job.status == mi.OK and job.data.shape == (fpj, h, w, c)
        s.release(job)
        assert s.pending() == 0
    finally:
        s.close()


@pytest.mark.parametrize("c", [3, 5])
def test_buffers_stay_within_workspace_bytes(mi, orc, c):
    frames, w, h = 6, 600, 400
    imgs, conts = make_batch(orc, frames, w, h, c, 64, 64, True)
    codec = mi.Codec(frames, w, h, c, 64, 64, True, device=0)
    kw = norm(c, "float32")
    table = mi.output_table(c, "float32", **kw)
    try:
        dev = packed(mi, conts)
        rng = np.random.default_rng(c)
        for hmax in (90, 150, 250, 380, 400):
            rects = [(0, int(rng.integers(0, h - hmax + 1)), w, hmax)] + [random_resized_crop(rng, w, h, scale=(0.02, 0.2)) for _ in range(frames - 1)]
            rects[1:] = [(x, y, min(rw, w), min(rh, hmax)) for x, y, rw, rh in rects[1:]]
            st, out = run_dev(codec, dev, rects, w, 64, c, "float32", "chw", **kw)
            assert st == 0 and same_bits(out, place(table, expected(mi, imgs, rects, w, 64), "chw")), hmax
            assert codec.allocated_bytes() <= codec.workspace_bytes, hmax
    finally:
        codec.close()
