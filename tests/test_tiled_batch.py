"""The shortcut behind tests/test_gpu_large.py, checked on the CPU: the container tests/tiled_batch.py assembles from per-bank-entry
streams equals the oracle's container of the whole image byte for byte, and the placement keeps neighbours apart."""
import numpy as np
import pytest
import torch

from tiled_batch import TiledBatch

MIX = ("noise", "grad", "flat", "noise", "noise")

# (name, frames, w, h, c, tile_w, tile_h, planar, small model)
CASES = [
    ("rows_480x1p", 3, 1200, 5, 3, 480, 1, True, False),
    ("tiles_64x64i", 2, 200, 150, 3, 64, 64, False, False),
    ("tiles_128x128p", 2, 300, 260, 3, 128, 128, True, False),
    ("partial_32x32i_c1", 3, 100, 70, 1, 32, 32, False, False),
    ("c5_32x16i", 2, 100, 41, 5, 32, 16, False, False),
    ("small_model_40x16p", 2, 130, 50, 3, 40, 16, True, True),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_assembled_container_is_the_oracles(orc, case):
    name, frames, w, h, c, tw, th, planar, small = case
    tb = TiledBatch(orc, frames, w, h, c, tw, th, planar, MIX, small_model=small, seed=len(name))
    imgs = tb.frames_host()
    assert imgs.shape == (frames, h, w, c)
    orc.set_small_model(small)
    try:
        want = [orc.compress_sliced(imgs[f], tw, th, planar) for f in range(frames)]
    finally:
        orc.set_small_model(False)
    for f in range(frames):
        assert tb.container(f) == want[f], f"frame {f}"
    # the batch form: the tables and payloads back to back, in numpy and in torch
    lens = np.concatenate([np.frombuffer(d, "<u4", count=tb.slices_per_frame, offset=24) for d in want])
    assert np.array_equal(tb.lengths(), lens)
    pay = b"".join(d[24 + 4 * tb.slices_per_frame:] for d in want)
    sids = tb.stream_ids()
    assert tb.payload(sids).tobytes() == pay
    assert tb.payload_bytes() == len(pay)
    got = tb.payload(torch.from_numpy(sids), *tb.stream_tensors("cpu"))
    assert got.numpy().tobytes() == pay
    # the device builder's arithmetic, on the CPU
    out = torch.empty((frames, h, w, c), dtype=torch.uint8)
    tb.fill_device(out, step=2)
    assert np.array_equal(out.numpy(), imgs)
    tail = torch.empty((frames - 1, h, w, c), dtype=torch.uint8)
    tb.fill_device(tail, f0=1)
    assert np.array_equal(tail.numpy(), imgs[1:])


def test_placement_keeps_neighbours_apart(orc):
    tb = TiledBatch(orc, 200, 3840, 8, 3, 480, 1, True, ("noise",) * 11 + ("grad", "flat"))
    m = tb.tile_map()
    assert (m[:, :, 1:] != m[:, :, :-1]).all() and (m[:, 1:, :] != m[:, :-1, :]).all() and (m[1:] != m[:-1]).all()
    for f in range(1, 200):
        assert tb.frames_differ(f, f - 1)
        assert tb.frames_differ(f, 0) == (f % 13 != 0)
