#!/usr/bin/env python3
"""Child process of tests/test_gpu_alpha_paste_alloc.py: the allocation failure sweep of the batch alpha paste
(llcomp_mi_codec_alpha_paste_batch), through the guard build libllcomp_mi_failalloc.so that LLCOMP_MI_LIB names, with the arena, the
injector's exports and the sweep of tests/helpers/alloc_failure_child.py (its contract is in its docstring).

    python tests/helpers/alpha_paste_alloc_child.py      prints one JSON line {case: {"R": requests of the call, "failed": [...]}}

Nothing here provokes a GPU fault: the injector fails allocations on the host, and no call is made on an object whose invariants are
broken."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from alloc_failure_child import Arena, Lib, Sweep, second, stream  # noqa: E402  (puts the repository, the oracle and tests/ on the path)


def main():
    import torch

    import alpha_paste_spec as spec
    import llcomp_amd as mi

    assert mi.device_count() >= 1
    sw = Sweep(mi, Lib(mi))
    rng = np.random.default_rng(77)
    n, ow, oh = 4, 33, 9
    new_codec = {c: (lambda c=c: mi.Codec(n, ow, oh, c, 0, 1, True, device=0)) for c in (3, 4)}
    matte = spec.gen_matte(rng, n, oh, ow)
    d_matte = torch.from_numpy(matte).cuda()
    f32 = rng.standard_normal((2, n, 3, oh, ow)).astype(np.float32)
    rgba = rng.integers(0, 256, (2, n, oh, ow, 4), dtype=np.uint8)
    rgba[..., 3] = spec.gen_matte(rng, 2 * n, oh, ow).reshape(2, n, oh, ow)
    d_f32, d_rgba = torch.from_numpy(f32[0]).cuda(), torch.from_numpy(rgba[0]).cuda()

    def paste(pieces, want):
        def build(codec):
            a = Arena()
            dst = a.out(f32[1].nbytes, init=f32[1])
            return a, lambda: codec.alpha_paste_batch(d_f32.data_ptr(), d_matte.data_ptr(), 1, 0, n, ow, oh, dst, n, ow, oh, pieces, stream=stream())
        return build, lambda out: same_bits(out[0], want)

    def over(pieces, want):
        def build(codec):
            a = Arena()
            dst = a.out(rgba[1].nbytes, init=rgba[1])
            return a, lambda: codec.alpha_paste_batch(d_rgba.data_ptr(), d_rgba.data_ptr(), 4, 3, n, ow, oh, dst, n, ow, oh, pieces, dtype="uint8", layout="hwc",
                                                      stream=stream())
        return build, lambda out: same_bits(out[0], want)

    def same_bits(got, want):
        assert np.array_equal(got, np.ascontiguousarray(want).reshape(-1).view(np.uint8)), "the dry pass differs from the spec"

    some = [(0, 1, 2, 1, 0, 0, 9, 5), (1, 0, 0, 0, 3, 2, 12, 6)]
    more = [(i % n, (i + 1) % n, i, i % 3, i % 5, 0, 8, 4) for i in range(12)]
    mixed = [p + ((mi.ALPHA_OVER,) if i % 2 else ()) for i, p in enumerate(more)]
    b_some, e_some = paste(some, spec.apply(f32[0], matte, f32[1], some, "float32", "chw"))
    b_more, e_more = paste(more, spec.apply(f32[0], matte, f32[1], more, "float32", "chw"))
    b_over, e_over = over(mixed, spec.apply(rgba[0], rgba[0], rgba[1], mixed, "uint8", "hwc", 3))
    sw.codec_case("alpha_paste_batch", new_codec[3], b_some, e_some)
    sw.codec_case("alpha_paste_batch,second", new_codec[3], second(b_some, b_more), e_more)
    sw.codec_case("alpha_paste_batch,over", new_codec[4], b_over, e_over)
    # no pass of the sweep, failed or not, wrote src or alpha (the arenas check the guard bytes around every dst)
    for dev, host in ((d_f32, f32[0]), (d_matte, matte), (d_rgba, rgba[0])):
        assert np.array_equal(dev.cpu().numpy().view(np.uint8).reshape(-1), np.ascontiguousarray(host).view(np.uint8).reshape(-1)), "src or alpha was written"
    print(json.dumps(sw.results))


if __name__ == "__main__":
    main()
