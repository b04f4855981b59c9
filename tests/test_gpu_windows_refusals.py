"""The pointer refusals of the eighteen windowed decodes (llcomp_mi_codec_decode_regions, _resized_regions(_ex), _padded_regions,
_views, _padded_views, _photo_views, _warped_views, _photo_warped_views and their _host forms), each through the raw C function: a
null source pointer, a status word at an address of 2 mod 4 and, where the call has one, a null d_px are LLCOMP_MI_BAD_ARGS, one
bad argument at a time with every other argument that of a call that decodes.  Every refusal is decided before anything is queued or
grown: afterwards the codec has counted no decode and holds the bytes it held after prepare().  The same arguments with nothing wrong
then decode, so each refusal was the one bad pointer's."""
import ctypes as C

import pytest
from conftest import make_image

pytestmark = pytest.mark.gpu

FRAMES, W, H, CH, TILE = 2, 32, 32, 3, 16


def test_every_windowed_decode_refuses_bad_pointers_before_it_queues_anything():
    import torch

    import llcomp_amd as mi

    assert mi.device_count() >= 1, "GPU tests need a HIP device"
    L = mi._lib.load()
    imgs = [make_image(gen, W, H, CH) for gen in ("nat", "g3")]
    conts = [mi.compress_image(im, W, H, CH, format=mi.FORMAT_SLICED, tile_w=TILE, tile_h=TILE, device=0) for im in imgs]
    pay, lens = mi.pack_batch(conts)
    d_pay, d_len = torch.from_numpy(pay).cuda(), torch.from_numpy(lens).cuda()
    d_out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")  # (room for every call's output, float32 included)
    d_status = torch.zeros(4, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ptrs, sizes, _keep = mi._containers(conts)

    xy, _ = mi._xy_table([(3, 5), (12, 9)], FRAMES)
    rects, _ = mi._rects_table([(3, 5, 20, 17), (0, 0, 32, 32)], FRAMES)
    srects, _ = mi._signed_rects_table([(-4, 5, 20, 17), (10, 20, 30, 30)], FRAMES)
    flags = mi._flags_table([1, 0], FRAMES, "bilinear")
    fmt, _, _keep_fmt = mi._output_format(CH, "float32", "chw", True, None, None)
    pad, _keep_pad = mi._pad(CH, "reflect", None)
    views = [mi.ViewGroup([(0, 2, 3, 20, 21, 0), (1, 8, 0, 24, 16, 0), (1, 0, 0, 32, 32, 1)], 8, 8, d_out.data_ptr(), photo=[("brightness", 1.2), "invert"])]
    varr, vn, _keep_v = mi._view_groups(views, CH, signed=True)
    vphoto, _keep_vp = mi._photo_groups(views, [3])
    warps = [mi.WarpGroup([(0, 1.1, 0.2, -1.0, -0.2, 0.9, 2.0), (1, 1.0, 0.0, 4.0, 0.0, 1.0, 3.0)], 8, 8, d_out.data_ptr(), filter="bilinear",
                          photo=["grayscale"])]
    warr, wn, _keep_w = mi._warp_groups(warps, CH)
    wphoto, _keep_wp = mi._photo_groups(warps, [2])

    # name -> (the arguments between the source and d_px / d_status, whether the call has a d_px)
    families = {
        "regions": ((xy, 20, 17), True),
        "resized_regions": ((rects, flags, 8, 8), True),
        "resized_regions_ex": ((rects, flags, 8, 8, C.byref(fmt)), True),
        "padded_regions": ((srects, flags, 8, 8, C.byref(pad), C.byref(fmt)), True),
        "views": ((varr, vn), False),
        "padded_views": ((varr, vn, C.byref(pad)), False),
        "photo_views": ((varr, vn, C.byref(pad), vphoto), False),
        "warped_views": ((warr, wn), False),
        "photo_warped_views": ((warr, wn, wphoto), False),
    }

    def entry(name, host):
        stem, ex = (name[:-3], "_ex") if name.endswith("_ex") else (name, "")
        return getattr(L, "llcomp_mi_codec_decode_" + stem + ("_host" if host else "") + ex)

    k = mi.Codec(FRAMES, W, H, CH, TILE, TILE, device=0)
    try:
        k.prepare(regions=True, resized=True, views=True)
        held = k.allocated_bytes()
        good_status, bad_status = d_status.data_ptr(), d_status.data_ptr() + 2
        calls = 0
        for name, (mid, has_px) in families.items():
            for host in (False, True):
                fn = entry(name, host)
                src = (ptrs, sizes) if host else (d_pay.data_ptr(), pay.size, d_len.data_ptr())
                px = (d_out.data_ptr(),) if has_px else ()
                no_payload = (None,) + src[1:]                       # a null d_payload / data
                no_table = src[:-1] + (None,)                        # a null d_slice_len / lens
                cases = [(no_payload, px, good_status), (no_table, px, good_status), (src, px, bad_status)]
                if has_px:
                    cases.append((src, (None,), good_status))
                for s, p, st in cases:
                    rc = fn(k._h, *s, *mid, *p, st, stream)
                    assert rc == mi.BAD_ARGS, f"{fn.__name__}: status {rc} for source {s} d_px {p} d_status {st:#x}"
                    calls += 1
        assert calls == 8 * 4 + 10 * 3  # (eight entries with a d_px, ten without)
        torch.cuda.synchronize()
        assert not any(k.counters().values()), k.counters()
        assert k.get_profile()[2] == 0
        assert k.allocated_bytes() == held
        # ... and with nothing wrong every one of them decodes
        for name, (mid, has_px) in families.items():
            for host in (False, True):
                src = (ptrs, sizes) if host else (d_pay.data_ptr(), pay.size, d_len.data_ptr())
                px = (d_out.data_ptr(),) if has_px else ()
                assert entry(name, host)(k._h, *src, *mid, *px, good_status, stream) == mi.OK, (name, host)
                torch.cuda.synchronize()
                assert int(d_status[0].item()) == 0, (name, host)
        assert k.get_profile()[2] == 18
    finally:
        k.close()
