#!/usr/bin/env python3
"""Child process of tests/test_gpu_wide_id_maps_alloc.py: the allocation failure sweep of the calls on id maps of 3 and 4 bytes per pixel,
through the guard build libllcomp_mi_failalloc.so that LLCOMP_MI_LIB names, with the arena, the injector's exports and the sweep of
tests/helpers/alloc_failure_child.py (its contract is in its docstring).

    python tests/helpers/wide_ids_alloc_child.py      prints one JSON line {case: {"R": requests of the call, "failed": [...]}}

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

    import llcomp_amd as mi

    assert mi.device_count() >= 1
    sw = Sweep(mi, Lib(mi))
    n, ow, oh, c = 4, 33, 9, 3
    rng = np.random.default_rng(32)
    wide = lambda k: k | ((k % 200 + 1) << 16)  # noqa: E731  (ids of three bytes, above 65535)
    ids = wide(rng.integers(0, 600, (n, oh, ow)))
    maps = {3: torch.from_numpy(np.stack([(ids >> (8 * b)) & 0xFF for b in range(3)], axis=-1).astype(np.uint8)).cuda(),
            4: torch.from_numpy(ids.astype(np.int32)).cuda()}
    new_codec = lambda: mi.Codec(n, ow, oh, c, 0, 1, True, device=0)  # noqa: E731

    def boxes(mb, lists):
        def build(codec):
            a = Arena()
            out = a.out(sum(len(i) for i in lists) * 20)
            return a, lambda: codec.label_boxes32(maps[mb].data_ptr(), mb, n, ow, oh, lists, out, stream=stream())
        return build

    def targets(mb, lists, values):
        def build(codec):
            a = Arena()
            out = a.out(n * oh * ow * 8)  # (an index tensor: int64)
            return a, lambda: codec.label_targets32(maps[mb].data_ptr(), mb, n, ow, oh, lists, values, out, kind="index", dtype="int64", default=255, stream=stream())
        return build

    ids_some, ids_more = [[wide(1), wide(5)], [wide(2)], [], [wide(599)]], [sorted(wide(i) for i in range(1, 600, 3))] * n
    val = lambda lists: [[(i * 7) % 250 for i in lst] for lst in lists]  # noqa: E731
    for mb in (3, 4):
        sw.codec_case(f"label_boxes32@{mb}", new_codec, boxes(mb, ids_some))
        sw.codec_case(f"label_boxes32,second@{mb}", new_codec, second(boxes(mb, ids_some), boxes(mb, ids_more)))
        sw.codec_case(f"label_targets32@{mb}", new_codec, targets(mb, ids_some, val(ids_some)))
        sw.codec_case(f"label_targets32,second@{mb}", new_codec, second(targets(mb, ids_some, val(ids_some)), targets(mb, ids_more, val(ids_more))))
    batch = rng.standard_normal((n, c, oh, ow)).astype(np.float32)
    src = torch.from_numpy(rng.standard_normal((n, c, oh, ow)).astype(np.float32)).cuda()

    def paste(mb, pieces):
        def build(codec):
            a = Arena()
            dst = a.out(batch.nbytes, init=batch)
            return a, lambda: codec.paste_batch32(src.data_ptr(), maps[mb].data_ptr(), mb, n, ow, oh, dst, n, ow, oh, pieces, stream=stream())
        return build

    some, more = [(0, 1, 2, 1, 0, 0, 9, 5), (1, 0, 0, 0, 3, 2, 12, 6)], [(i % n, (i + 1) % n, i, i % 3, i % 5, 0, 8, 4) for i in range(12)]
    q_some, q_more = [r + ([wide(5), wide(300), wide(599)],) for r in some], [r + ([wide(i) for i in range(0, 600, 12)],) for r in more]
    for mb in (3, 4):
        sw.codec_case(f"paste_batch32@{mb}", new_codec, paste(mb, q_some))
        sw.codec_case(f"paste_batch32,second@{mb}", new_codec, second(paste(mb, q_some), paste(mb, q_more)))
    # the two widths' calls share the 16-bit calls' table buffers: a wide call behind a 16-bit one grows the same buffer
    mask16 = torch.from_numpy(rng.integers(0, 600, (n, oh, ow)).astype(np.int16)).cuda()

    def boxes16(lists):
        def build(codec):
            a = Arena()
            out = a.out(sum(len(i) for i in lists) * 20)
            return a, lambda: codec.label_boxes16(mask16.data_ptr(), n, ow, oh, lists, out, stream=stream())
        return build

    sw.codec_case("label_boxes32,behind_label_boxes16", new_codec, second(boxes16([[1, 5], [2], [], [599]]), boxes(3, ids_more)))
    print(json.dumps(sw.results))


if __name__ == "__main__":
    main()
