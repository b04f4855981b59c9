"""The three batch calls on ONE codec and ONE stream with no synchronise between them (mix_batch, orient_batch, compose_batch, mix_batch
again): they share the driver of the table copy (codec.hip: batch_table_call) and the pinned ring, and keep a table buffer each.  The
batch and the canvases against the same chain of the three host references, bit for bit, with guard bytes around both, and the codec's
memory against the sum of what the three calls may add to it."""
import numpy as np
import pytest

from batch_support import ESIZE, bits_of, gen_batch, guards_intact, mi, put, stream  # noqa: F401

pytestmark = pytest.mark.gpu

VALUE = (3, 114, 255)  # exact in all four dtypes


@pytest.mark.parametrize("dtype,layout", [("float16", "chw"), ("uint8", "hwc")])
def test_mix_orient_compose_mix_on_one_codec_and_stream(mi, dtype, layout):
    import torch

    c, side, cw, ch = 3, 9, 20, 11
    n = 2 * mi.mix_segment() + 5
    blends = dtype != "uint8"
    batch = gen_batch(dtype, n, c, side, side, layout, seed=n)
    canvases = gen_batch(dtype, 2, c, ch, cw, layout, seed=n + 1)  # (not under KEEP: every element of them is written)
    first = mi.mix_samples(n, "roll", lam=[0.37 if blends and i % 3 == 0 else None for i in range(n)],
                           boxes=[(2, 3, 4, 5) if i % 3 == 1 else None for i in range(n)],
                           erase=[(1, 1, 3, 2) if i % 4 == 2 else None for i in range(n)])
    order, seg_first, n_saved = mi.mix_plan(first)
    assert len(seg_first) - 1 == 3 and n_saved == 3  # one cycle, cut
    codes = [i % 8 for i in range(n)]  # (a square batch: the transposing codes are legal)
    pieces = [(0, 3, 1, 1, 0, 0, 9, 9), (0, n - 1, 8, 2, 2, 1, 7, 8), (1, 0, 5, 5, 0, 0, 4, 3, mi.COMPOSE_FILL), (1, 7, 11, 0, 0, 0, 9, 9)]
    second = mi.mix_samples(n, "flip", lam=0.37 if blends else None, boxes=None if blends else (2, 3, 4, 5))

    mixed = mi.mix_reference(batch, first, layout, erase_value=VALUE, dtype=dtype)
    oriented = mi.orient_reference(mixed, codes, layout, dtype=dtype)
    want_canvases = mi.compose_reference(oriented, canvases, pieces, layout, fill=VALUE, dtype=dtype)
    want_batch = mi.mix_reference(oriented, second, layout, dtype=dtype)
    assert not np.array_equal(bits_of(want_batch), bits_of(oriented)) and not np.array_equal(bits_of(mixed), bits_of(batch))

    codec = mi.Codec(1, 32, 16, c, 32, 16, False, device=0)
    try:
        bbuf, blo = put(batch, ESIZE[dtype])  # one element past a 256-byte boundary
        cbuf, clo = put(canvases, 3 * ESIZE[dtype])
        d_batch, d_canvases, s = bbuf.data_ptr() + blo, cbuf.data_ptr() + clo, stream()
        codec.mix_batch(d_batch, n, side, side, first, dtype=dtype, layout=layout, erase_value=VALUE, stream=s)
        codec.orient_batch(d_batch, n, side, side, codes, dtype=dtype, layout=layout, stream=s)
        codec.compose_batch(d_batch, n, side, side, d_canvases, 2, cw, ch, pieces, dtype=dtype, layout=layout, fill=VALUE, stream=s)
        codec.mix_batch(d_batch, n, side, side, second, dtype=dtype, layout=layout, stream=s)
        torch.cuda.synchronize()
        for buf, lo, want, what in ((bbuf, blo, want_batch, "batch"), (cbuf, clo, want_canvases, "canvases")):
            host = buf.cpu().numpy()
            assert guards_intact(host, lo, want.nbytes), f"a byte outside the {what} was written"
            got = bits_of(host[lo:lo + want.nbytes].copy().view(want.dtype).reshape(want.shape))
            assert np.array_equal(got, bits_of(want)), (what, dtype, layout, np.argwhere(got != bits_of(want))[:4].tolist())
        W = mi._lib.load().llcomp_mi_codec_workspace_bytes(codec._h)
        assert codec.allocated_bytes() <= W + (codec.mix_workspace_bytes(n, side, side, dtype) - W) + (codec.orient_workspace_bytes(n) - W) + \
            (codec.compose_workspace_bytes(2, 4) - W)
    finally:
        codec.close()
