"""llcomp_mi_resize_weights (host only): the Q22 triangle-filter weights the resized regions decode runs on the GPU, checked against an
independent float64 restatement of the rule, and the whole rule against torch's interpolate(antialias=True)."""
import numpy as np
import pytest

import llcomp_amd as mi
from resize_spec import ref_weights, resize

GRID = [(1, 1), (1, 300), (224, 224), (17, 5), (4096, 224), (64, 1), (192, 3), (64 * 224, 224), (5, 17), (64, 2), (1000, 999),
        (999, 1000), (7, 3), (2, 5), (3840, 224), (480, 160)]


@pytest.mark.parametrize("n_in,n_out", GRID, ids=[f"{a}to{b}" for a, b in GRID])
def test_weights_against_float64_restatement(n_in, n_out):
    lo, q = mi.resize_weights(n_in, n_out)
    rlo, rw = ref_weights(n_in, n_out)
    assert lo.shape == (n_out,) and q.shape[0] == n_out
    assert np.array_equal(lo.astype(np.int64), rlo)
    assert (q >= 0).all()
    k = q.shape[1]
    assert k <= 129
    for i in range(n_out):
        want = np.floor(0.5 + rw[i] * (1 << 22)).astype(np.int64)
        m = min(k, len(want))
        assert np.abs(q[i, :m].astype(np.int64) - want[:m]).max() <= 1, i
        assert (want[m:] <= 1).all()          # taps left out are zero
        assert (q[i, len(want):] == 0).all()  # padding is zero
        assert lo[i] + len(want) <= n_in


@pytest.mark.parametrize("n", [1, 2, 17, 224, 4096])
def test_identity(n):
    lo, q = mi.resize_weights(n, n)
    assert np.array_equal(lo, np.arange(n, dtype=np.uint32))
    assert (q[:, 0] == 1 << 22).all() and (q[:, 1:] == 0).all()


def test_refused():
    L = mi._lib.load()
    assert L.llcomp_mi_resize_weights(0, 5, None, None) == 0
    assert L.llcomp_mi_resize_weights(5, 0, None, None) == 0
    assert L.llcomp_mi_resize_weights(64 * 7 + 1, 7, None, None) == 0
    assert 0 < L.llcomp_mi_resize_weights(64 * 7, 7, None, None) <= 129
    with pytest.raises(mi.LlcompError) as e:
        mi.resize_weights(65, 1)
    assert e.value.status == mi.BAD_ARGS


def test_rule_matches_torch_antialias():
    torch = pytest.importorskip("torch")
    import torch.nn.functional as F

    rng = np.random.default_rng(60)
    worst, diffs = 0, []
    for t in range(40):
        h, w = (int(v) for v in rng.integers(4, 400, size=2))
        oh, ow = (int(v) for v in rng.integers(4, 200, size=2))
        if w > 64 * ow or h > 64 * oh:
            continue
        c = int(rng.integers(1, 5))
        if t % 2:
            img = rng.integers(0, 256, size=(h, w, c), dtype=np.uint8)
        else:
            yy, xx = np.mgrid[0:h, 0:w]
            img = np.stack([((xx * (3 + k) + yy * (5 - k)) % 256) for k in range(c)], axis=-1).astype(np.uint8)
        mine = resize(mi, img, ow, oh).astype(np.int64)
        x = torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None]
        ref = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False, antialias=True)
        ref = ref[0].permute(1, 2, 0).round().clamp(0, 255).numpy().astype(np.int64)
        d = np.abs(mine - ref)
        worst = max(worst, int(d.max()))
        diffs.append(d.mean())
    assert worst <= 1, worst
    assert np.mean(diffs) < 0.25


def test_identity_and_mirror_of_the_rule():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(31, 45, 3), dtype=np.uint8)
    assert np.array_equal(resize(mi, img, 45, 31), img)
    assert np.array_equal(resize(mi, img, 45, 31, flip=True), img[:, ::-1])
