"""The device compilation of the batch alpha paste's rules (llcomp_amd/csrc/alpha_rule.hpp in k_alpha_paste) over whole domains: U8
PASTE on all 2^24 (m, d, s) and OVER on every (sa, da) against 256 colour pairs, against the numpy statement that
tests/test_alpha_paste_rule.py holds equal to PIL; the float PASTE on every dst bit pattern x every alpha byte x src witnesses (F16,
BF16) and on every exponent x the witnesses (F32), against torch's expression on the CPU.  One call per leg, one piece that covers the
whole batch, between 256 guard bytes, src and alpha byte-identical afterwards; the expected values are computed once per leg."""
import numpy as np
import pytest

import alpha_paste_spec as spec
import device_domains as dom
from alpha_paste_spec import ALPHA_OVER
from batch_support import guards_intact, mi, put, stream  # noqa: F401
from test_alpha_paste_rule import over_domain, torch_expression

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codecs(mi):
    made = {c: mi.Codec(1, 32, 16, c, 32, 16, False, device=0) for c in (1, 4)}
    yield made
    for k in made.values():
        k.close()


def device_result(codec, src, alpha, dst, piece, dtype, layout, n_src, iw, ih):
    import torch

    dbuf, dlo = put(dst, 0)
    sbuf, slo = put(src, 0)
    abuf, alo = put(alpha, 0) if alpha is not None else (None, 0)
    (oh, ow) = dst.shape[2:] if layout == "chw" else dst.shape[1:3]
    codec.alpha_paste_batch(sbuf.data_ptr() + slo, None if abuf is None else abuf.data_ptr() + alo, 1, 0, n_src, iw, ih, dbuf.data_ptr() + dlo, len(dst), ow, oh,
                            piece, dtype=dtype, layout=layout, stream=stream())
    torch.cuda.synchronize()
    host = dbuf.cpu().numpy()
    assert guards_intact(host, dlo, dst.nbytes), "a byte outside the dst batch was written"
    for buf, lo, arr in ((sbuf, slo, src), (abuf, alo, alpha)):
        if buf is not None:
            h = buf.cpu().numpy()
            assert guards_intact(h, lo, arr.nbytes) and np.array_equal(h[lo:lo + arr.nbytes], arr.reshape(-1).view(np.uint8)), "src or alpha was written"
    return host[dlo:dlo + dst.nbytes].copy().view(dst.dtype).reshape(dst.shape)


def test_u8_paste_on_all_triples(mi, codecs):
    m, d, s = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    m, d, s = (np.ascontiguousarray(a.reshape(1, 1, 4096, 4096)) for a in (m, d, s))
    want = spec.paste_rule(d, s, m, "uint8").astype(np.uint8)
    got = device_result(codecs[1], s, m[0], d, [(0, 0, 0, 0, 0, 0, 4096, 4096)], "uint8", "chw", 1, 4096, 4096)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} of 2^24 differ"


def test_over_on_every_alpha_pair(mi, codecs):
    src, dst = over_domain()
    want = spec.over_rule(dst, src)
    got = device_result(codecs[4], src[None], None, dst[None], [(0, 0, 0, 0, 0, 0, 65536, 256, ALPHA_OVER)], "uint8", "hwc", 1, 65536, 256)
    assert np.array_equal(got[0], want), f"{np.count_nonzero((got[0] != want).any(axis=-1))} pixels differ"


def float_leg(mi, codec, dtype, own, witnesses, alphas):
    """dst sample k: a row per alpha byte, every own pattern along it; src sample k: constant at witness k; the alpha rows constant"""
    t = spec.NP_NAME[dtype]
    bt = spec.BITS[np.dtype(t).itemsize]
    n, rows, width = len(witnesses), len(alphas), len(own)
    d = np.broadcast_to(own.astype(bt)[None, None, None, :], (n, 1, rows, width)).copy()
    s = np.broadcast_to(np.array(witnesses, bt)[:, None, None, None], (n, 1, rows, width)).copy()
    m = np.broadcast_to(np.array(alphas, np.uint8)[None, :, None], (n, rows, width)).copy()
    pieces = [(k, k, 0, 0, 0, 0, width, rows) for k in range(n)]
    got = device_result(codec, s.view(t), m, d.view(t), pieces, dtype, "chw", n, width, rows).view(bt)
    for k in range(n):  # (sample by sample: the expression's temporaries stay small)
        dk, sk, mk = d[k, 0].reshape(-1).astype(np.uint32), s[k, 0].reshape(-1).astype(np.uint32), m[k].reshape(-1).astype(np.uint32)
        want = torch_expression(dk, sk, mk, dtype)
        want = np.where(mk == 0, dk, np.where(mk == 255, sk, want))
        bad = got[k, 0].reshape(-1) != want
        i = int(np.argmax(bad))
        assert not bad.any(), f"witness {witnesses[k]:#x}: {np.count_nonzero(bad)} differ, first d {dk[i]:#x} m {mk[i]}: {got[k, 0].reshape(-1)[i]:#x}, want {want[i]:#x}"


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_16_bit_floats_on_every_dst_pattern_and_alpha_byte(mi, codecs, dtype):
    w = dom.PARTNERS[dtype]
    witnesses = [w[2], w[5], w[10], w[6]]  # 1, -max, the smallest subnormal, +inf
    float_leg(mi, codecs[1], dtype, dom.own_bits(dtype).reshape(-1), witnesses, list(range(256)))


def test_float32_on_every_exponent_against_the_witnesses(mi, codecs):
    alphas = [0, 1, 2, 3, 51, 85, 127, 128, 129, 170, 204, 252, 253, 254, 255, 64]
    float_leg(mi, codecs[1], "float32", dom.own_bits("float32").reshape(-1), dom.PARTNERS["float32"], alphas)
