#!/usr/bin/env python3
"""Child process of tests/test_gpu_alloc_failures.py: the allocation failure sweep of one group of entry points, through the guard
build libllcomp_mi_failalloc.so that LLCOMP_MI_LIB names (csrc/devmem.hip: the injector; csrc/codec.hip: llmi_test_codec_consistent).

    python tests/helpers/alloc_failure_child.py GROUP      prints one JSON line {case: {"R": requests of the call, "failed": [...]}}

Per case: a dry pass on a fresh codec counts the call's allocation requests R and keeps its outputs; then request j alone fails, for
EVERY j in 0..R-1, and then requests j.. for j = 0 and R // 2 -- each time on a fresh codec, with sentinels in the outputs and the
status word and guard bytes around them.  A failure that is not on the optional list is LLCOMP_MI_NOMEM with every output byte as it
was; the codec object's invariants hold (only then is anything called on it again), its device bytes are what it says, the same call
with the injection off gives the dry pass's bytes, and closing it leaves no block behind.  Nothing here provokes a GPU fault: the
injector fails allocations on the host, and no call is made on an object whose invariants are broken."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

GUARD = 256
FROM_HERE_ON = 1 << 62
FRAMES, W, CH = 3, 100, 3  # the two geometries of tests/test_gpu_windows_mixed.py


class Arena:
    """the buffers a call writes: guard bytes on both sides of each, sentinels (0x5A; 0x77 in a status word) or the batch an in-place
    call works on inside"""

    def __init__(self):
        self.bufs, self.words, self.before = [], [], None

    def out(self, nbytes, fill=0x5A, init=None):
        import torch

        t = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device="cuda")
        if init is not None:
            t[GUARD:GUARD + nbytes] = torch.from_numpy(np.ascontiguousarray(init).view(np.uint8).reshape(-1)).cuda()
        self.bufs.append((t, nbytes))
        return t.data_ptr() + GUARD

    def status(self):
        self.words.append(len(self.bufs))
        return self.out(4, 0x77)

    def host(self):
        import torch

        torch.cuda.synchronize()
        return [t.cpu().numpy() for t, _ in self.bufs]

    def seal(self):
        self.before = self.host()

    def untouched(self):
        return all(np.array_equal(a, b) for a, b in zip(self.host(), self.before))

    def read(self):
        """the outputs after a call that returned OK: guards intact, every status word 0"""
        res = []
        for (t, n), now, was in zip(self.bufs, self.host(), self.before):
            assert np.array_equal(now[:GUARD], was[:GUARD]) and np.array_equal(now[GUARD + n:], was[GUARD + n:]), "a byte outside an output was written"
            res.append(now[GUARD:GUARD + n].copy())
        for i in self.words:
            assert not res[i].any(), f"status word {res[i].view(np.uint32)[0]:#x}"
        return res


class Lib:
    """the guard build's test exports"""

    def __init__(self, mi):
        self.L = L = mi._lib.load()
        for name in ("llmi_test_alloc_requests", "llmi_test_live_blocks", "llmi_test_live_requested_bytes", "llmi_test_live_pinned"):
            getattr(L, name).restype = C.c_uint64
            getattr(L, name).argtypes = []
        L.llmi_test_fail_requests.restype = None
        L.llmi_test_fail_requests.argtypes = [C.c_uint64, C.c_uint64]
        L.llmi_test_fail_raw.restype = None
        L.llmi_test_fail_raw.argtypes = [C.c_uint32]
        L.llmi_test_fail_raw_left.restype = C.c_uint32
        L.llmi_test_fail_raw_left.argtypes = []
        L.llmi_test_codec_consistent.restype = C.c_int
        L.llmi_test_codec_consistent.argtypes = [C.c_void_p]
        self.requests, self.live_bytes = L.llmi_test_alloc_requests, L.llmi_test_live_requested_bytes
        self.fail, self.fail_raw, self.fail_raw_left = L.llmi_test_fail_requests, L.llmi_test_fail_raw, L.llmi_test_fail_raw_left

    def live_blocks(self):
        """device blocks handed out and not parked, and pinned buffers not freed"""
        return self.L.llmi_test_live_blocks() + self.L.llmi_test_live_pinned()

    def consistent(self, codec):
        return self.L.llmi_test_codec_consistent(codec._h)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


class Sweep:
    def __init__(self, mi, lib):
        self.mi, self.lib, self.results = mi, lib, {}

    def attempt(self, call, first, count):
        """the call with requests first .. first + count - 1 of ITS OWN failing -> its status"""
        import torch

        lib, mi = self.lib, self.mi
        lib.fail(lib.requests() + first, count)
        try:
            call()
            status = mi.OK
        except mi.LlcompError as e:
            status = int(e.status)
        finally:
            lib.fail(0, 0)
        torch.cuda.synchronize()
        return status

    def codec_case(self, name, new_codec, build, expect=None, optional=(), nomem=None):
        """new_codec() -> a fresh codec (injection off); build(codec) -> (arena, call): whatever a case calls FIRST, to leave smaller
        buffers behind, build does itself.  expect(outputs): the dry pass against its reference.  optional: ordinals whose failure the
        call swallows by design ("last": R - 1).  nomem: the status a failure gives (default NOMEM)."""
        mi, lib = self.mi, self.lib
        nomem = mi.NOMEM if nomem is None else nomem
        res = self.results[name] = {"R": 0, "failed": []}
        base = lib.live_blocks()
        codec = new_codec()
        try:
            arena, call = build(codec)
            arena.seal()
            r0 = lib.requests()
            call()
            R = res["R"] = lib.requests() - r0
            dry = arena.read()
            if expect:
                expect(dry)
            assert lib.consistent(codec) == 0, f"invariant {lib.consistent(codec)}"
        except (AssertionError, mi.LlcompError) as e:  # (the case ends here: there is nothing to compare a failure pass with)
            res["failed"].append(f"dry pass: {e!r}")
            return
        finally:
            codec.close()
        if lib.live_blocks() != base:
            res["failed"].append("dry pass: blocks left behind")
            return
        opt = {R - 1 if o == "last" else o for o in optional}
        if opt:
            res["optional"] = sorted(opt)
        for first, count in [(j, 1) for j in range(R)] + [(j, FROM_HERE_ON) for j in sorted({0, R // 2}) if R]:
            what = f"request {first}" + (" on" if count > 1 else "")
            codec = new_codec()
            try:
                live0, held0 = lib.live_bytes(), codec.allocated_bytes()
                arena, call = build(codec)
                arena.seal()
                status = self.attempt(call, first, count)
                swallowed = set(range(first, R if count > 1 else first + 1)) <= opt
                if swallowed:
                    if status != mi.OK or not same(arena.read(), dry):
                        res["failed"].append(f"{what}: optional, but status {status} or other bytes than the dry pass")
                        continue
                else:
                    if status != nomem:
                        res["failed"].append(f"{what}: status {status}, not {nomem}")
                    if not arena.untouched():
                        res["failed"].append(f"{what}: an output, status word or guard byte was written")
                broken = lib.consistent(codec)
                if broken:
                    res["failed"].append(f"{what}: invariant {broken} of the codec object broken; no further call on it")
                    continue
                if lib.live_bytes() - live0 != codec.allocated_bytes() - held0:
                    res["failed"].append(f"{what}: allocated_bytes moved by {codec.allocated_bytes() - held0}, live bytes by {lib.live_bytes() - live0}")
                if not swallowed:  # (the same call on the same buffers: they still hold what they held)
                    again = self.attempt(call, 0, 0)
                    if again != mi.OK or not same(arena.read(), dry):
                        res["failed"].append(f"{what}: the call after it gives status {again} or other bytes than the dry pass")
                    if lib.consistent(codec):
                        res["failed"].append(f"{what}: invariant {lib.consistent(codec)} broken after the call that followed")
            except AssertionError as e:
                res["failed"].append(f"{what}: {e}")
            finally:
                codec.close()
            if lib.live_blocks() != base:
                res["failed"].append(f"{what}: {lib.live_blocks() - base} blocks left behind at close")
                base = lib.live_blocks()

    def plain_case(self, name, prepare, build, expect=None, nomem=None, after=None):
        """an entry point without a codec object of the caller's (create, host API, streams): prepare() empties the library's caches,
        build() -> (arena, call, undo): undo() gives back what a successful call made; after(status): more to assert on a failure"""
        mi, lib = self.mi, self.lib
        nomem = mi.NOMEM if nomem is None else nomem
        res = self.results[name] = {"R": 0, "failed": []}
        prepare()
        base = lib.live_blocks()
        try:
            arena, call, undo = build()
            arena.seal()
            r0 = lib.requests()
            call()
            R = res["R"] = lib.requests() - r0
            dry = arena.read()
            if expect:
                expect(dry)
            undo()
            prepare()
            assert lib.live_blocks() == base, "blocks left behind"
        except (AssertionError, mi.LlcompError) as e:  # (the case ends here: there is nothing to compare a failure pass with)
            res["failed"].append(f"dry pass: {e!r}")
            return
        for first, count in [(j, 1) for j in range(R)] + [(j, FROM_HERE_ON) for j in sorted({0, R // 2}) if R]:
            what = f"request {first}" + (" on" if count > 1 else "")
            try:
                arena, call, undo = build()
                arena.seal()
                status = self.attempt(call, first, count)
                if status != nomem:
                    res["failed"].append(f"{what}: status {status}, not {nomem}")
                    if status == mi.OK:  # (the object is given back; there is nothing to call again)
                        undo()
                        prepare()
                        continue
                if status != mi.OK and not arena.untouched():
                    res["failed"].append(f"{what}: an output or guard byte was written")
                if after:
                    after(what, status, res["failed"])
                again = self.attempt(call, 0, 0)
                if again != mi.OK or not same(arena.read(), dry):
                    res["failed"].append(f"{what}: the call after it gives status {again} or other bytes than the dry pass")
                else:
                    undo()
            except AssertionError as e:
                res["failed"].append(f"{what}: {e}")
            prepare()
            if lib.live_blocks() != base:
                res["failed"].append(f"{what}: {lib.live_blocks() - base} blocks left behind")
                base = lib.live_blocks()


def device_status(mi):
    """the status of the device behind this thread's last DEVICE_FAILED"""
    e = mi.last_device_error()
    return e[2] if e else None


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def set_env(mi, **kv):
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    mi.reload_tuning()


class Batch:
    """frames of one shape: the images, the oracle's containers and the packed batch in HBM"""

    def __init__(self, mi, orc, frames, w, h, c, tw, th, planar):
        import torch
        from test_gpu_regions_host import make_batch
        from test_gpu_resized_regions import packed

        self.shape = (frames, w, h, c, tw, th, planar)
        self.imgs, self.conts = make_batch(orc, frames, w, h, c, tw, th, planar)
        self.d_pay, self.n, self.d_len = packed(mi, self.conts)
        self.pay, self.lens = mi.pack_batch(self.conts)
        self.d_px = torch.from_numpy(self.imgs).cuda()
        self.mi = mi

    def codec(self):
        return self.mi.Codec(*self.shape, device=0)

    def src(self):
        return self.d_pay.data_ptr(), self.n, self.d_len.data_ptr()


def encode_case(b):
    """encode -> the oracle's payload, table and total"""
    def build(codec):
        a = Arena()
        cap = codec.max_payload_bytes
        pay, lens, total, st = a.out(cap + 16), a.out(4 * codec.n_slices), a.out(8), a.status()
        return a, lambda: codec.encode(b.d_px.data_ptr(), pay, cap, lens, total, st, stream())

    def expect(out):
        n = int(out[2].view(np.uint64)[0])
        assert n == len(b.pay) and np.array_equal(out[0][:n], b.pay), "payload is not the oracle's"
        assert np.array_equal(out[1].view(np.uint32), b.lens.view(np.uint32).reshape(-1)), "slice table is not the oracle's"
    return build, expect


def decode_case(b):
    def build(codec):
        a = Arena()
        px, st = a.out(b.imgs.size), a.status()
        return a, lambda: codec.decode(*b.src(), px, st, stream())

    def expect(out):
        assert np.array_equal(out[0], b.imgs.reshape(-1)), "pixels are not the source's"
    return build, expect


def find_family(mi, key, tw, th, planar, more=lambda k: True):
    """the smallest of a few shapes up to 8 frames of 404 x 328 x 3 whose codec is of family `key`"""
    for frames, w, h in ((1, 128, 128), (1, 256, 192), (1, 404, 328), (2, 404, 328), (4, 404, 328), (8, 404, 328)):
        k = mi.Codec(frames, w, h, 3, tw, th, planar, device=0)
        try:
            if k.family[key] and more(k):
                return frames, w, h
        finally:
            k.close()
    raise AssertionError(f"no shape up to 8 x 404 x 328 x 3 in {tw} x {th} tiles runs the {key} family")


# ---- groups ---------------------------------------------------------------------------------------------------------------------------

def group_core(sw, mi, orc):
    lib = sw.lib
    shape = (FRAMES, W, 44, CH, 32, 16, False)

    def build():
        made = []

        def call():
            made.append(mi.Codec(*shape, device=0))
        return Arena(), call, lambda: made.pop().close()
    sw.plain_case("codec_create_ex", lambda: None, build)

    # prepare: every flag alone and all together, on a codec whose state tables live in HBM (the bank cache's family) and on one that runs
    # the chunked snapshot pass
    set_env(mi, LLCOMP_MI_LANE_SHIFT="6")
    try:
        flags = ("encode", "decode", "region", "regions", "resized", "update", "views")
        hbm = (lambda f: (f[0], f[1], f[2], 3, 32, 32, False))(find_family(mi, "bank_cache", 32, 32, False))
        for tag, shp in (("hbm_32x32i", hbm), ("chunked_128x48p", (1, 128, 96, 3, 128, 48, True))):
            for on in [(f,) for f in flags] + [flags]:
                kw = {f: f in on for f in flags}
                sw.codec_case(f"prepare({'+'.join(on) if len(on) == 1 else 'all'})@{tag}", lambda: mi.Codec(*shp, device=0),
                              lambda codec: (Arena(), lambda: codec.prepare(**kw)))
    finally:
        set_env(mi, LLCOMP_MI_LANE_SHIFT=None)


def group_families(sw, mi, orc):
    cases = [("rows_fused_100x6_50x1p", (FRAMES, 100, 6, 3, 50, 1, True), "rows"), ("rows_interleaved_100x6_32x1i", (FRAMES, 100, 6, 3, 32, 1, False), "rows"),
             ("lds_table_200x150_64x64i", (1, 200, 150, 3, 64, 64, False), "lds_table")]
    f = find_family(mi, "bank_cache", 32, 32, False)
    cases.append(("hbm_bank_cache_32x32i", (f[0], f[1], f[2], 3, 32, 32, False), "bank_cache"))
    f = find_family(mi, "snapshot", 64, 64, True)
    cases.append(("snapshot_64x64p", (f[0], f[1], f[2], 3, 64, 64, True), "snapshot"))
    for name, shp, key in cases:
        b = Batch(mi, orc, *shp)
        k = b.codec()
        try:
            assert k.family[key], (name, k.family)
            cached = k.family["bank_cache"]
        finally:
            k.close()
        sw.codec_case(f"encode@{name}", b.codec, *encode_case(b))
        # (the 2-D decoder's feedback mailbox is the last request of the first cached decode: optional by design)
        sw.codec_case(f"decode@{name}", b.codec, *decode_case(b), optional=("last",) if cached else ())


def group_chunked(sw, mi, orc):
    """slices above 4096 samples: pass and coder in chunks, under every setting of LLCOMP_MI_OVERLAP"""
    try:
        set_env(mi, LLCOMP_MI_LANE_SHIFT="6")
        shapes = [("chunked_128x48p", (1, 128, 96, 3, 128, 48, True))]
        f = find_family(mi, "snapshot", 64, 64, False)
        shapes.append(("chunked_64x64i", (f[0], f[1], f[2], 3, 64, 64, False)))
        for name, shp in shapes:
            b = Batch(mi, orc, *shp)
            for overlap in (None, "0", "1"):
                set_env(mi, LLCOMP_MI_OVERLAP=overlap)
                k = b.codec()
                try:
                    assert k.family["snapshot"], (name, k.family)
                finally:
                    k.close()
                tag = f"{name},overlap={'unset' if overlap is None else overlap}"
                sw.codec_case(f"encode@{tag}", b.codec, *encode_case(b))
                sw.codec_case(f"decode@{tag}", b.codec, *decode_case(b), optional=("last",) if k.family["bank_cache"] else ())
    finally:
        set_env(mi, LLCOMP_MI_LANE_SHIFT=None, LLCOMP_MI_OVERLAP=None)


def second(first, then):
    """`first` once with the injection off, then the case is `then` on the same codec: it finds smaller buffers to grow"""
    def build(codec):
        a, call = first(codec)
        a.seal()
        call()
        a.read()
        return then(codec)
    return build


def crop(imgs, x, y, rw, rh):
    return np.ascontiguousarray(imgs[:, y:y + rh, x:x + rw]).reshape(-1)


def region_cases(sw, mi, orc, name, b, region, update, small=None):
    x, y, rw, rh = region

    def build_region(codec):
        a = Arena()
        px, st = a.out(b.imgs.shape[0] * rw * rh * b.imgs.shape[3]), a.status()
        return a, lambda: codec.decode_region(*b.src(), x, y, rw, rh, px, st, stream())

    def expect_region(out):
        assert np.array_equal(out[0], crop(b.imgs, x, y, rw, rh)), "pixels are not the source's"
    cached = (lambda k: (k.region_family(x, y, rw, rh)["bank_cache"], k.close())[0])(b.codec())
    sw.codec_case(f"decode_region@{name}", b.codec, build_region, expect_region, optional=("last",) if cached else ())

    enc, upd, expect_update = update_builders(mi, orc, b, update)
    sw.codec_case(f"encode_region@{name}", b.codec, enc)
    sw.codec_case(f"update_region@{name}", b.codec, upd, expect_update)
    if small:  # ... and behind an update of a smaller box, which leaves a smaller box buffer to grow (ensure_grown: free, then allocate)
        enc0, upd0, _ = update_builders(mi, orc, b, small)
        sw.codec_case(f"encode_region,second@{name}", b.codec, second(enc0, enc))
        sw.codec_case(f"update_region,second@{name}", b.codec, second(upd0, upd), expect_update)
    # (an unaligned rectangle: the box is decoded first)
    ucached = (lambda k: (k.region_family(*update)["bank_cache"], k.close())[0])(b.codec())
    assert not ucached, "the optional list of this file has no mailbox for the update cases"


def update_builders(mi, orc, b, rect):
    """encode_region and update_region of `rect` with new pixels -> (build of the one, build of the other, the update against the oracle's
    containers of the modified frames)"""
    import torch

    ux, uy, uw, uh = rect
    d_rect = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (b.imgs.shape[0], uh, uw, b.imgs.shape[3]), dtype=np.uint8)).cuda()

    def build_encode_region(codec):
        a = Arena()
        cap = min(codec.max_payload_bytes, 2 * b.imgs.size + 4096)  # (twice the raw bytes: what the host calls give a first attempt)
        pay, lens, total, st = a.out(cap + 16), a.out(4 * codec.n_slices), a.out(8), a.status()
        return a, lambda: codec.encode_region(*b.src(), ux, uy, uw, uh, d_rect.data_ptr(), pay, cap, lens, total, st, stream())

    def build_update_region(codec):
        a = Arena()
        cap = min(codec.max_payload_bytes, 2 * b.imgs.size + 4096)
        pay, lens, total, st = a.out(cap + 16), a.out(4 * codec.n_slices), a.out(8), a.status()
        return a, lambda: codec.update_region(*b.src(), ux, uy, uw, uh, d_rect.data_ptr(), pay, cap, lens, total, st, stream())

    def expect_update(out):
        new = b.imgs.copy()
        new[:, uy:uy + uh, ux:ux + uw] = d_rect.cpu().numpy()
        _, w, h, c, tw, th, planar = b.shape
        pay, lens = mi.pack_batch([orc.compress_sliced(new[f], tw, th, planar) for f in range(new.shape[0])])
        n = int(out[2].view(np.uint64)[0])
        assert n == len(pay) and np.array_equal(out[0][:n], pay) and np.array_equal(out[1].view(np.uint32), lens.view(np.uint32).reshape(-1)), \
            "the updated batch is not the oracle's of the modified frames"
    return build_encode_region, build_update_region, expect_update


def windowed_cases(sw, mi, orc, name, b, geo):
    """the windowed calls with the rectangles of tests/test_gpu_windows_mixed.py: every one alone on a fresh codec, and as a second call
    behind a smaller one that leaves smaller buffers to grow"""
    from test_gpu_resized_output import norm

    frames, c, h = b.imgs.shape[0], b.imgs.shape[3], b.imgs.shape[1]
    esize = {"uint8": 1, "float16": 2, "float32": 4}

    def regions(host, key="regions"):
        def build(codec):
            xy, rw, rh = geo[key]
            a = Arena()
            px, st = a.out(frames * rw * rh * c), a.status()
            if host:
                return a, lambda: codec.decode_regions_host(b.conts, xy, rw, rh, px, st, stream())
            return a, lambda: codec.decode_regions(*b.src(), xy, rw, rh, px, st, stream())
        return build

    def expect_regions(out):
        xy, rw, rh = geo["regions"]
        assert np.array_equal(out[0], np.stack([b.imgs[f, y:y + rh, x:x + rw] for f, (x, y) in enumerate(xy)]).reshape(-1)), "pixels are not the source's"

    def resized(host, fmt, small=False, pad=False):
        def build(codec):
            rects, ow, oh = geo["resized_host" if host else "resized"]
            if small:
                rects, ow, oh = [(x, y, max(1, rw // 3), max(1, rh // 2)) for x, y, rw, rh in rects], max(1, ow // 3), max(1, oh // 2)
            kw = dict(dtype="float32", layout="chw", filter="bicubic", **norm(c, "float32")) if fmt else {}
            if pad:
                rects, kw = [(x - 3, y - 2, rw + 5, rh + 4) for x, y, rw, rh in rects], dict(kw, pad_mode="reflect")
            a = Arena()
            px, st = a.out(frames * ow * oh * c * (4 if fmt else 1)), a.status()
            if host:
                return a, lambda: codec.decode_resized_regions_host(b.conts, rects, ow, oh, px, st, flags=[0, 1, 0], stream=stream(), **kw)
            return a, lambda: codec.decode_resized_regions(*b.src(), rects, ow, oh, px, st, flags=[1, 0, 0], stream=stream(), **kw)
        return build

    def views(host, kind="views", few=False, photo=None):
        def build(codec):
            a = Arena()
            groups = []
            for gi, ((v, ow, oh), (dtype, layout)) in enumerate(zip(geo["views"], (("uint8", "hwc"), ("float16", "hwc")))):
                v = v[:1] if few else v
                if few:
                    ow, oh = max(1, ow // 2), max(1, oh // 2)
                ptr = a.out(len(v) * ow * oh * c * esize[dtype])
                fmt = {} if dtype == "uint8" else dict(dtype=dtype, layout=layout, **norm(c, dtype))
                ph = dict(photo=photo) if photo else {}
                if kind == "views":
                    groups.append(mi.ViewGroup(v, ow, oh, ptr, **fmt, **ph))
                elif kind == "warped":  # the view's rectangle, rotated by 10 degrees about its centre
                    s, co = math.sin(math.radians(10)), math.cos(math.radians(10))
                    ws = []
                    for (f, x, y, rw, rh, _fl) in v:
                        sx, sy = rw / ow, rh / oh
                        m = [sx * co, sy * s, 0.0, -sx * s, sy * co, 0.0]
                        m[2] = x + rw / 2 - (m[0] * ow / 2 + m[1] * oh / 2)
                        m[5] = y + rh / 2 - (m[3] * ow / 2 + m[4] * oh / 2)
                        ws.append((f, *m, 1 << 4))
                    groups.append(mi.WarpGroup(ws, ow, oh, ptr, fill=[1, 2, 3], **fmt, **ph))
                else:  # perspective: the rectangle under a mild keystone
                    ps = [(f, rw / ow, 0.0, float(x), 0.0, rh / oh, float(y), 0.002, 0.001, 1 << 4) for (f, x, y, rw, rh, _fl) in v]
                    groups.append(mi.PerspectiveGroup(ps, ow, oh, ptr, fill=[1, 2, 3], **fmt, **ph))
            st = a.status()
            conts = [b.conts[0], None, b.conts[2]]
            if kind == "views":
                return a, (lambda: codec.decode_views_host(conts, groups, st, stream())) if host else (lambda: codec.decode_views(*b.src(), groups, st, stream()))
            if kind == "warped":
                return a, (lambda: codec.decode_warped_views_host(conts, groups, st, stream())) if host else \
                    (lambda: codec.decode_warped_views(*b.src(), groups, st, stream()))
            return a, (lambda: codec.decode_perspective_views_host(conts, groups, st, stream())) if host else \
                (lambda: codec.decode_perspective_views(*b.src(), groups, st, stream()))
        return build

    k = b.codec()
    try:
        fams = (k.regions_family(*geo["regions"]) or []) + (k.regions_family(*geo["regions_again"]) or [])
        assert not any(f["bank_cache"] for f in fams) and not k.family["bank_cache"], "the optional list of this file has no mailbox for the windowed cases"
    finally:
        k.close()
    chain = [("brightness", 1.2), "autocontrast", ("gaussian_blur", 1.0), ("adjust_sharpness", 1.5)]  # table ops, a blur and a sharpness
    made = [("decode_regions", regions(False), expect_regions), ("decode_regions_host", regions(True), expect_regions),
            ("decode_resized_regions", resized(False, False), None), ("decode_resized_regions_ex", resized(False, True), None),
            ("decode_resized_regions_host", resized(True, True), None), ("decode_padded_regions", resized(False, True, pad=True), None),
            ("decode_views", views(False), None), ("decode_views_host", views(True), None),
            ("decode_warped_views", views(False, "warped"), None), ("decode_perspective_views", views(False, "perspective"), None),
            ("decode_photo_views", views(False, photo=chain), None),
            # ... and each kind once more as a second call behind a smaller one of its kind
            ("decode_regions_host,second", second(regions(True), regions(True, "regions_again")), None),
            ("decode_resized_regions_host,second", second(resized(True, True, small=True), resized(True, True)), None),
            ("decode_resized_regions,second", second(resized(False, False, small=True), resized(False, False)), None),
            ("decode_resized_regions_ex,second", second(resized(False, True, small=True), resized(False, True)), None),
            ("decode_padded_regions,second", second(resized(False, True, small=True, pad=True), resized(False, True, pad=True)), None),
            ("decode_views,second", second(views(False, few=True), views(False)), None),
            ("decode_views_host,second", second(views(True, few=True), views(True)), None),
            ("decode_warped_views,second", second(views(False, "warped", few=True), views(False, "warped")), None),
            ("decode_perspective_views,second", second(views(False, "perspective", few=True), views(False, "perspective")), None),
            ("decode_photo_views,second", second(views(False, few=True, photo=chain), views(False, photo=chain)), None)]
    for call_name, build, expect in made:
        sw.codec_case(f"{call_name}@{name}", b.codec, build, expect)


def group_windows(sw, mi, orc, name):
    from test_gpu_windows_mixed import GEOMETRIES

    geo = GEOMETRIES[name]
    b = Batch(mi, orc, FRAMES, W, geo["h"], CH, geo["tw"], geo["th"], geo["planar"])
    x, y, rw, rh = geo["update"]
    small = (x, y, 5, min(rh, 5) if geo["th"] > 1 else 1)  # one tile's box, where the update's own covers several
    region_cases(sw, mi, orc, name, b, geo["region"], geo["update"], small)
    windowed_cases(sw, mi, orc, name, b, geo)


def group_switch(sw, mi, orc):
    """region updates whose sub-geometry runs another family than the codec's (tests/test_gpu_update_region.py): the 1-row remainder of
    2-row tiles, which the row encoder codes, planar and interleaved"""
    for planar in (True, False):
        b = Batch(mi, orc, 1, 160, 41, 3, 40, 2, planar)
        k = b.codec()
        try:
            assert not k.family["rows"] and k.region_family(10, 40, 100, 1)["rows"]
        finally:
            k.close()
        region_cases(sw, mi, orc, f"160x41_40x2{'p' if planar else 'i'}", b, (10, 40, 100, 1), (10, 40, 100, 1))


def group_regrow(sw, mi, orc):
    """Region updates that run the snapshot pass on a codec that does not: 8 frames of 404 x 328 x 3 in 400 x 40 planar tiles are 432
    big slices, one per wavefront with the table in LDS; the last tile column alone is 4 pixels wide, 192 or 216 small slices that share
    wavefronts and take the pass.  The first such update makes snapshot arrays of the region's own size, with the coder's parking
    records (ensure_snapshot_arrays without the pass of the codec's own); a second, of one tile row more, frees and regrows them.  Both
    rectangles are whole boxes: nothing is decoded."""
    b = Batch(mi, orc, 8, 404, 328, 3, 400, 40, True)
    first, larger = (400, 0, 4, 320), (400, 0, 4, 328)
    k = b.codec()
    try:
        assert k.family["lds_table"] and not k.family["snapshot"], k.family
        assert k.region_family(*first)["snapshot"] and k.region_family(*larger)["snapshot"], (k.region_family(*first), k.region_family(*larger))
    finally:
        k.close()
    enc0, upd0, expect0 = update_builders(mi, orc, b, first)
    enc1, upd1, expect1 = update_builders(mi, orc, b, larger)
    sw.codec_case("encode_region@regrow_404x328_400x40p", b.codec, enc0)
    sw.codec_case("update_region@regrow_404x328_400x40p", b.codec, upd0, expect0)
    sw.codec_case("encode_region,second@regrow_404x328_400x40p", b.codec, second(enc0, enc1))
    sw.codec_case("update_region,second@regrow_404x328_400x40p", b.codec, second(upd0, upd1), expect1)


def group_batch(sw, mi, orc):
    """the eight batch calls on 4 samples of 33 x 9 x 3, float32 CHW, each alone and behind a call with a smaller table"""
    import torch

    n, ow, oh, c = 4, 33, 9, 3
    rng = np.random.default_rng(11)
    batch = rng.standard_normal((n, c, oh, ow)).astype(np.float32)
    src = torch.from_numpy(rng.standard_normal((n, c, oh, ow)).astype(np.float32)).cuda()
    mask8 = torch.from_numpy(rng.integers(0, 4, (n, oh, ow), dtype=np.uint8)).cuda()
    mask16 = torch.from_numpy(rng.integers(0, 600, (n, oh, ow)).astype(np.int16)).cuda()
    new_codec = lambda: mi.Codec(n, ow, oh, c, 0, 1, True, device=0)  # noqa: E731
    long_n = 2 * mi.mix_segment() + 5  # a cycle of partners longer than a segment: the second buffer, the saved heads, is asked for

    def mix(count):
        def build(codec):
            a = Arena()
            data = np.resize(batch, (count, c, oh, ow))
            ptr = a.out(data.nbytes, init=data)
            samples = mi.mix_samples(count, "roll", 0.3, None, (2, 1, 5, 4))
            return a, lambda: codec.mix_batch(ptr, count, ow, oh, samples, erase_value=[0.5, 0.25, 0.125], stream=stream())
        return build

    def orient(codes):
        def build(codec):
            a = Arena()
            ptr = a.out(batch.nbytes, init=batch)
            return a, lambda: codec.orient_batch(ptr, n, ow, oh, codes, stream=stream())
        return build

    def compose(pieces):
        def build(codec):
            a = Arena()
            dst = a.out(batch.nbytes, init=batch)
            return a, lambda: codec.compose_batch(src.data_ptr(), n, ow, oh, dst, n, ow, oh, pieces, fill=[0.5, 0.25, 0.125], stream=stream())
        return build

    def paste(pieces, wide):
        def build(codec):
            a = Arena()
            dst = a.out(batch.nbytes, init=batch)
            if wide:
                return a, lambda: codec.paste_batch16(src.data_ptr(), mask16.data_ptr(), n, ow, oh, dst, n, ow, oh, pieces, stream=stream())
            return a, lambda: codec.paste_batch(src.data_ptr(), mask8.data_ptr(), n, ow, oh, dst, n, ow, oh, pieces, stream=stream())
        return build

    def boxes(build_ids):
        def build(codec):
            a = Arena()
            if build_ids is None:
                out = a.out(n * 256 * 20)
                return a, lambda: codec.label_boxes(mask8.data_ptr(), n, ow, oh, out, stream=stream())
            out = a.out(sum(len(i) for i in build_ids) * 20)
            return a, lambda: codec.label_boxes16(mask16.data_ptr(), n, ow, oh, build_ids, out, stream=stream())
        return build

    def targets(ids, values):
        def build(codec):
            a = Arena()
            out = a.out(n * oh * ow * 8)  # (an index tensor: int64)
            return a, lambda: codec.label_targets(mask16.data_ptr(), n, ow, oh, ids, values, out, map_dtype="uint16", kind="index", dtype="int64",
                                                  default=255, stream=stream())
        return build

    some, more = [(0, 1, 2, 1, 0, 0, 9, 5), (1, 0, 0, 0, 3, 2, 12, 6)], [(i % n, (i + 1) % n, i, i % 3, i % 5, 0, 8, 4) for i in range(12)]
    p_some, p_more = [r + ([1, 2],) for r in some], [r + ([1, 3],) for r in more]
    q_some, q_more = [r + ([5, 300, 599],) for r in some], [r + (list(range(0, 600, 7)),) for r in more]
    ids_some, ids_more = [[1, 5], [2], [], [599]], [list(range(1, 600, 3))] * n
    val = lambda ids: [[(i * 7) % 250 for i in lst] for lst in ids]  # noqa: E731
    made = [("mix_batch", mix(n)), ("mix_batch,long_cycle", lambda codec: mix(long_n)(codec)), ("mix_batch,second", second(mix(n), mix(long_n))),
            ("orient_batch", orient([1, 2, 0, 4])), ("orient_batch,second", second(orient([1, 0, 0, 0]), orient([1, 2, 1, 4]))),
            ("compose_batch", compose(some)), ("compose_batch,second", second(compose(some), compose(more))),
            ("paste_batch", paste(p_some, False)), ("paste_batch,second", second(paste(p_some, False), paste(p_more, False))),
            ("paste_batch16", paste(q_some, True)), ("paste_batch16,second", second(paste(q_some, True), paste(q_more, True))),
            ("label_boxes", boxes(None)),
            ("label_boxes16", boxes(ids_some)), ("label_boxes16,second", second(boxes(ids_some), boxes(ids_more))),
            ("label_targets", targets(ids_some, val(ids_some))), ("label_targets,second", second(targets(ids_some, val(ids_some)), targets(ids_more, val(ids_more))))]
    for name, build in made:
        codec_for = (lambda: mi.Codec(long_n, ow, oh, c, 0, 1, True, device=0)) if "long" in name or name == "mix_batch,second" else new_codec
        sw.codec_case(name, codec_for, build)


def group_host(sw, mi, orc):
    """the host-buffer calls: every call starts from empty caches (llcomp_mi_trim), so the lane is made inside it"""
    from conftest import make_image

    w, h, c = 100, 44, 3
    img = make_image("nat", w, h, c)
    flat = np.ascontiguousarray(img).reshape(-1)
    sliced, legacy = orc.compress_sliced(img, 32, 16, False), orc.compress_image(img)

    def host_out(nbytes):
        return np.full(nbytes + 2 * GUARD, 0x5A, np.uint8)

    class HostArena(Arena):
        def __init__(self, nbytes):
            super().__init__()
            self.buf, self.n = host_out(nbytes), nbytes
            self.view = self.buf[GUARD:GUARD + nbytes]

        def host(self):
            return [self.buf.copy()]

        def read(self):
            assert (self.buf[:GUARD] == 0x5A).all() and (self.buf[GUARD + self.n:] == 0x5A).all(), "a byte outside the output was written"
            return [self.view.copy()]

    def encode(fmt_sliced):
        def build():
            a = HostArena(len(sliced) + 4096)
            kw = dict(format=mi.FORMAT_SLICED, tile_w=32, tile_h=16, planar=False) if fmt_sliced else dict(format=mi.FORMAT_LEGACY)
            return a, lambda: mi.compress_image_into(flat, w, h, c, a.view, device=0, **kw), lambda: None
        want = sliced if fmt_sliced else legacy

        def expect(out):
            assert bytes(out[0][:len(want)]) == bytes(want), "container is not the oracle's"
        return build, expect

    def decode(data):
        arr = np.frombuffer(bytes(data), np.uint8)

        def build():
            a = HostArena(flat.size)
            return a, lambda: mi.decompress_image_into(arr, a.view, device=0), lambda: None
        return build, lambda out: np.testing.assert_array_equal(out[0], flat)

    x, y, rw, rh = 33, 13, 50, 25
    arr = np.frombuffer(bytes(sliced), np.uint8)

    def region():
        a = HostArena(rw * rh * c)
        return a, lambda: mi.decompress_region_into(arr, a.view, x, y, rw, rh, device=0), lambda: None

    patch = np.random.default_rng(3).integers(0, 256, (12, 30, c), dtype=np.uint8)
    new = img.copy()
    new[5:17, 10:40] = patch
    want_update = orc.compress_sliced(new, 32, 16, False)

    def update():
        a = HostArena(len(want_update) + 4096)
        return a, lambda: mi.update_region_into(arr, a.view, 10, 5, patch, device=0), lambda: None

    sw.plain_case("llcomp_mi_encode,sliced", mi.trim, *encode(True))
    sw.plain_case("llcomp_mi_encode,legacy", mi.trim, *encode(False))
    sw.plain_case("llcomp_mi_decode,sliced", mi.trim, *decode(sliced))
    sw.plain_case("llcomp_mi_decode,legacy", mi.trim, *decode(legacy))
    sw.plain_case("llcomp_mi_decode_region", mi.trim, region, lambda out: np.testing.assert_array_equal(out[0], img[y:y + rh, x:x + rw].reshape(-1)))
    sw.plain_case("llcomp_mi_update_region", mi.trim, update, lambda out: np.testing.assert_array_equal(out[0][:len(want_update)], np.frombuffer(want_update, np.uint8)))

    # streams: the create calls, and one submit after a successful create
    def stream_create(devices):
        def build():
            made = []

            def call():
                made.append(mi.Stream(w, h, c, 32, 16, False, depth=2, device=0, devices=devices))
            return Arena(), call, lambda: made.pop().close()
        return build

    def device_nomem(what, status, failed):
        if status == mi.DEVICE_FAILED and device_status(mi) != mi.NOMEM:
            failed.append(f"{what}: last_device_error {mi.last_device_error()}, not NOMEM")
    def pinned():
        made = []

        def call():
            made.append(mi.PinnedBuffer(4096))
        return Arena(), call, lambda: made.pop().close()
    sw.plain_case("llcomp_mi_host_alloc", mi.trim, pinned)
    sw.plain_case("llcomp_mi_stream_create", mi.trim, stream_create(None))
    sw.plain_case("llcomp_mi_stream_create_multi", mi.trim, stream_create([0, 0]), nomem=mi.DEVICE_FAILED, after=device_nomem)

    # One submit after a successful create, on a shape whose state tables live in HBM: the slot's lane is the stream's own, and its first
    # encode allocates them.  Every stream is new, so every pass starts from the same state.
    from test_gpu_regions_host import make_batch

    frames, sw_, sh_ = find_family(mi, "bank_cache", 32, 32, False)
    imgs, conts = make_batch(orc, frames, sw_, sh_, 3, 32, 32, False)
    want = b"".join(bytes(x) for x in conts)
    px = np.ascontiguousarray(imgs).reshape(-1)

    def submit():
        st = mi.Stream(sw_, sh_, 3, 32, 32, False, depth=2, device=0, frames_per_job=frames)
        a = HostArena(len(want))

        def call():
            if not st.submit_encode(px):
                raise mi.LlcompError(mi.BUSY)
            job = st.wait()
            data = job.data if isinstance(job.data, list) else [job.data]
            got = np.concatenate([np.asarray(d) for d in data]) if job.status == mi.OK else None
            st.release(job)
            if job.status != mi.OK:
                raise mi.LlcompError(job.status)
            a.view[:] = got
        return a, call, st.close
    sw.plain_case("llcomp_mi_stream_submit_encode", mi.trim, submit, lambda out: np.testing.assert_array_equal(out[0], np.frombuffer(want, np.uint8)))


def group_devices(sw, mi, orc):
    """a device list {0, 0}: the workers' allocation order is not fixed, so requests fail from ordinal 0 and R // 2 on, and what is
    asserted is the outcome: DEVICE_FAILED with NOMEM behind it, the caller's buffer untouched, the next call good"""
    from conftest import make_image

    lib = sw.lib
    w, h, c = 100, 64, 3
    img = make_image("nat", w, h, c)
    flat = np.ascontiguousarray(img).reshape(-1)
    want = orc.compress_sliced(img, 50, 1, True)
    arr = np.frombuffer(bytes(want), np.uint8)
    for name, size, run, good in (
            ("llcomp_mi_encode,devices", len(want) + 4096,
             lambda out: mi.compress_image_into(flat, w, h, c, out, format=mi.FORMAT_SLICED, tile_w=50, tile_h=1, planar=True, devices=[0, 0]),
             lambda out: bytes(out[:len(want)]) == bytes(want)),
            ("llcomp_mi_decode,devices", flat.size, lambda out: mi.decompress_image_into(arr, out, devices=[0, 0]), lambda out: np.array_equal(out, flat))):
        res = sw.results[name] = {"R": 0, "failed": []}
        mi.trim()
        base = lib.live_blocks()
        out = np.full(size, 0x5A, np.uint8)
        r0 = lib.requests()
        run(out)
        R = res["R"] = lib.requests() - r0
        assert good(out), f"{name}: dry pass is not the oracle's"
        for first in sorted({0, R // 2}):
            mi.trim()
            out = np.full(size + 2 * GUARD, 0x5A, np.uint8)
            status = sw.attempt(lambda: run(out[GUARD:GUARD + size]), first, FROM_HERE_ON)
            if status != mi.DEVICE_FAILED or device_status(mi) != mi.NOMEM:
                res["failed"].append(f"request {first} on: status {status}, last_device_error {mi.last_device_error()}")
            if not (out == 0x5A).all():
                res["failed"].append(f"request {first} on: the caller's buffer was written")
            if sw.attempt(lambda: run(out[GUARD:GUARD + size]), 0, 0) != mi.OK or not good(out[GUARD:GUARD + size]):
                res["failed"].append(f"request {first} on: the call after it is not the oracle's")
            if not ((out[:GUARD] == 0x5A).all() and (out[GUARD + size:] == 0x5A).all()):
                res["failed"].append(f"request {first} on: a guard byte was written")
        mi.trim()
        if lib.live_blocks() != base:
            res["failed"].append(f"{lib.live_blocks() - base} blocks left behind")


def group_pool(sw, mi, orc):
    """dev_alloc's own pressure path: a raw allocation fails while blocks are parked -> every parked block of the device goes back to the
    driver and the allocation is tried once more"""
    lib = sw.lib
    res = sw.results["pool_pressure"] = {"R": 0, "failed": []}
    big = Batch(mi, orc, 1, 404, 328, 3, 64, 64, False)
    mi.trim()
    base = lib.live_blocks()
    mi.Codec(1, 200, 150, 3, 64, 64, False, device=0).close()  # parks its blocks
    parked = mi.pool_idle_bytes()
    assert parked > 0, "closing a codec parks its blocks"
    # The codec made again is a LARGER one: the same shape would take every block out of the cache and never reach the driver.  Its
    # first request, the image-order array, fits no parked block, so the raw allocation that fails is that one.
    r0 = lib.requests()
    lib.fail_raw(1)
    try:
        k = big.codec()
        left = lib.fail_raw_left()
    finally:
        lib.fail_raw(0)
    if left != 0:
        res["failed"].append("the raw allocation that was to fail never happened: the pressure path did not run")
    res["R"] = lib.requests() - r0
    try:
        if mi.pool_idle_bytes() != 0:
            res["failed"].append(f"{mi.pool_idle_bytes()} of {parked} bytes still parked behind the failed raw allocation")
        if lib.consistent(k):
            res["failed"].append(f"invariant {lib.consistent(k)}")
        for build, expect in (encode_case(big), decode_case(big)):
            a, call = build(k)
            a.seal()
            call()
            expect(a.read())
    except AssertionError as e:
        res["failed"].append(str(e))
    finally:
        k.close()
    mi.trim()
    if lib.live_blocks() != base:
        res["failed"].append(f"{lib.live_blocks() - base} blocks left behind")


GROUPS = {"core": group_core, "families": group_families, "chunked": group_chunked, "switch": group_switch, "regrow": group_regrow, "batch": group_batch, "host": group_host,
          "devices": group_devices, "pool": group_pool,
          "windows_100x44_32x16i": lambda sw, mi, orc: group_windows(sw, mi, orc, "100x44_32x16i"),
          "windows_100x6_50x1p": lambda sw, mi, orc: group_windows(sw, mi, orc, "100x6_50x1p")}


def main():
    import llcomp_amd as mi
    import orc as orc_mod

    assert mi.device_count() >= 1
    sw = Sweep(mi, Lib(mi))
    GROUPS[sys.argv[1]](sw, mi, orc_mod.Orc())
    print(json.dumps(sw.results))


if __name__ == "__main__":
    main()
