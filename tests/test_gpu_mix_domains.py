"""The blend of the batch mixing as the DEVICE compiler built it, on every bit pattern (mix_kernels.hip with mix_rule.hpp): F16 and BF16
on all 65536 patterns, F32 on every exponent crossed with 32 mantissas and both signs, each against 16 partners -- +-0, +-1, +-max,
+-inf, a quiet NaN and one with a payload, the smallest subnormal and normal, 1.5 x the smallest normal, eps, -2.5, 1/3 -- as own value
and as partner, under six lambdas.  For F16 the device runs the hardware conversions, not the host's integer restatement that
tests/test_mix_rule.py pins.  Expected: torch's bits of tests/mix_spec.py's expressions on the CPU, and the dtype's quiet NaN where
torch gives a NaN (include/llcomp_mi.h: "Batch mixing"); the batches and the inputs that flip under named mistakes:
tests/device_domains.py."""
import time

import numpy as np
import pytest

import device_domains as dd
import test_gpu_mix_batch as base
from batch_support import mi  # noqa: F401  (the fixture)
from mix_batches import Case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec(mi):
    made = mi.Codec(1, 32, 16, 1, 32, 16, False, device=0)
    yield made
    made.close()


@pytest.mark.parametrize("lam", dd.LAMBDAS, ids=["lam%d" % i for i in range(len(dd.LAMBDAS))])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float32"])
def test_every_pattern_as_own_and_as_partner(mi, codec, dtype, lam):
    """[2 P, 1, h, w]: sample 2 k every pattern, sample 2 k + 1 constant at partner k, the two swapped; base.run checks the guard bytes
    on both sides of the batch"""
    assert dd.LAM == base.LAM
    t0 = time.perf_counter()
    batch, want = dd.mix_expected(dtype, lam)
    print("host s %.2f" % (time.perf_counter() - t0))
    got = base.run(mi, codec, batch, Case(dd.swap_pairs(len(batch)), lam), "chw").astype(np.uint32)
    bad = np.argwhere(got != want)
    if len(bad):
        n, _, y, x = (int(t) for t in bad[0])
        bits = dd.mix_batch_bits(dtype)
        raise AssertionError("%s lam %r: %d differ; own 0x%X partner 0x%X gives 0x%X, want 0x%X" % (
            dtype, lam, len(bad), bits[n, 0, y, x], bits[n ^ 1, 0, y, x], got[n, 0, y, x], want[n, 0, y, x]))
