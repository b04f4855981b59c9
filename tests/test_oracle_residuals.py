"""The oracle's coder of chosen residuals (orc_encode_residuals), the source of the decoder tests' adversarial streams: exponents up
to 31, int16 wrap-around of rebuilt samples and unary runs of 32 and more ones, none of which an 8-bit image produces.  Pinned to the
oracle's own encoder on real residuals, to its decoder, and (where it is built) to the real reference's decoder."""
import numpy as np
import pytest

import orc as orc_mod


def _small_model(orc, on):
    orc.set_small_model(on)


@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("c", [1, 2, 3, 4, 5])
def test_real_residuals_code_like_the_encoder(orc, c, small):
    rng = np.random.default_rng(10 * c + small)
    _small_model(orc, small)
    try:
        for gen in ("g3", "mid", "checker"):
            w, h = int(rng.integers(1, 40)), int(rng.integers(1, 30))
            s = orc.forward_rct(orc_mod.GENERATORS[gen](w, h, c))
            _, res = orc.model_samples(s)
            stream, view = orc.encode_residuals(res.astype(np.int64))
            assert stream == orc.encode_samples(s)
            assert np.array_equal(view, s)
    finally:
        _small_model(orc, False)


@pytest.mark.parametrize("small", [False, True])
@pytest.mark.parametrize("kind", ["sparse", "wrap", "ex31", "small"])
def test_decoder_rebuilds_the_decoder_view(orc, kind, small):
    rng = np.random.default_rng(["sparse", "wrap", "ex31", "small"].index(kind) * 2 + small)
    _small_model(orc, small)
    try:
        for c in (1, 3, 5):
            w, h = int(rng.integers(1, 48)), int(rng.integers(1, 24))
            res = orc_mod.adversarial_residuals(rng, h, w, c, kind)
            stream, view = orc.encode_residuals(res)
            rc, out = orc.decode_samples(stream, w, h, c)
            assert rc == orc_mod.OK and np.array_equal(out, view)
            if kind == "wrap" and h * w * c > 40:  # the content does what it says: rebuilt samples reach the ends of int16
                assert np.abs(view.astype(np.int64)).max() > 30000
    finally:
        _small_model(orc, False)


@pytest.mark.parametrize("run_len", [32, 33, 40])
def test_runs_of_32_or_more_ones_are_bad_exponents_at_their_sample(orc, run_len):
    rng = np.random.default_rng(run_len)
    for c in (1, 3, 4):
        w, h = int(rng.integers(2, 30)), int(rng.integers(1, 12))
        n = w * h * c
        res = orc_mod.adversarial_residuals(rng, h, w, c, "sparse")
        for at in (0, n // 2, n - 1):
            stream, view = orc.encode_residuals(res, run_at=at, run_len=run_len)
            rc, out = orc.decode_samples(stream, w, h, c)
            assert rc == orc_mod.BAD_EXPONENT
            flat = out.reshape(-1)
            assert np.array_equal(flat[:at], view.reshape(-1)[:at]) and not flat[at:].any()
    # a run of 31 is the largest legal exponent: it decodes
    res = np.zeros((1, 1, 1), np.int64)
    res[0, 0, 0] = -(2**32 - 1)
    stream, view = orc.encode_residuals(res)
    rc, out = orc.decode_samples(stream, 1, 1, 1)
    assert rc == orc_mod.OK and np.array_equal(out, view) and int(view[0, 0, 0]) == np.int16(128 + 1)


@pytest.mark.parametrize("seed", range(24))
def test_crafted_legacy_streams_decode_like_the_reference(orc, ref, seed):
    """Exponents up to 30 only: at 31 the reference's int32 `value += value + bit` overflows (UB), and only the oracle's
    modulo-2^32 rule defines the result -- the GPU tests hold the decoder to that rule."""
    rng = np.random.default_rng(7000 + seed)
    c = 3 + seed % 2
    w, h = int(rng.integers(1, 30)), int(rng.integers(1, 20))
    kind = ("sparse", "wrap", "ex31", "small")[seed % 4]
    res = orc_mod.adversarial_residuals(rng, h, w, c, kind, max_ex=30)
    run = {} if seed % 3 else {"run_at": int(rng.integers(0, w * h * c)), "run_len": int(rng.choice([32, 33, 40]))}
    stream, _ = orc.encode_residuals(res, **run)
    data = orc_mod.legacy_stream(w, h, c, stream)
    rc_o, px_o = orc.decompress(data)
    rc_r, px_r = ref.o1_decompress_image(data)
    assert rc_o == rc_r == (orc_mod.BAD_EXPONENT if run else orc_mod.OK)
    if rc_o == orc_mod.OK:
        assert np.array_equal(px_o, px_r)


@pytest.mark.parametrize("seed", range(16))
def test_legacy_streams_with_trailing_bytes_decode_like_the_reference(orc, ref, seed):
    """The reference reads what the samples need and ignores the rest of its input"""
    rng = np.random.default_rng(7100 + seed)
    c = 3 + seed % 2
    w, h = (1, 1) if seed < 4 else (2, 2) if seed < 8 else (int(rng.integers(1, 40)), int(rng.integers(1, 30)))
    img = rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)
    n = int(rng.integers(0, 401))
    tail = (bytes(n), bytes([0xFF]) * n, rng.integers(0, 256, size=n, dtype=np.uint8).tobytes())[seed % 3]
    data = orc.compress_image(img) + tail
    rc_o, px_o = orc.decompress(data)
    rc_r, px_r = ref.o1_decompress_image(data)
    assert rc_o == rc_r == orc_mod.OK
    assert np.array_equal(px_o, px_r)
    if not any(tail):  # zeros are what the decoder reads past the end: the stream alone
        assert np.array_equal(px_o, img)
