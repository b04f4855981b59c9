"""Region decode, host side: llcomp_mi_region_plan against a Python model, the sub-geometry check of geometry.hpp (compiled helper),
and no CPU path behind the region calls.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd
    from llcomp_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "llcomp_amd", "csrc")])
    return llcomp_amd


def model_plan(w, h, c, tw, th, planar, x, y, rw, rh):
    """the definition: tiles [x / tw, min(ceil((x + rw) / tw), ntx)) and the same for rows; None = BAD_ARGS"""
    if rw < 1 or rh < 1 or x + rw > w or y + rh > h:
        return None
    tw = w if tw == 0 or tw > w else tw
    th = h if th == 0 or th > h else th
    ntx, nty = -(-w // tw), -(-h // th)
    box = (x // tw, y // th, min(-(-(x + rw) // tw), ntx), min(-(-(y + rh) // th), nty))
    return box, (box[2] - box[0]) * (box[3] - box[1]) * (c if planar else 1)


def _cases():
    rng = np.random.default_rng(1015)
    out = []
    for _ in range(170):
        w, h = int(rng.integers(1, 5000)), int(rng.integers(1, 3000))
        c, planar = int(rng.integers(1, 6)), bool(rng.integers(0, 2))
        tw = 0 if rng.integers(0, 4) == 0 else int(rng.integers(1, w + 1))
        th = 0 if rng.integers(0, 4) == 0 else (int(rng.integers(1, 3)) if rng.integers(0, 3) == 0 else int(rng.integers(1, h + 1)))
        ttw, tth = (w if tw == 0 else tw), (h if th == 0 else th)
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        lx, ly = (w - 1) // ttw * ttw, (h - 1) // tth * tth
        tx, ty = x // ttw * ttw, y // tth * tth
        for r in ((x, y, int(rng.integers(1, w - x + 1)), int(rng.integers(1, h - y + 1))),  # random
                  (x, y, 1, 1),                                                             # one pixel
                  (0, 0, w, h),                                                             # whole image
                  (tx, ty, min(ttw, w - tx), min(tth, h - ty)),                             # exactly one tile
                  (x, y, w - x, h - y),                                                     # touching the right and bottom edges
                  (lx, ly, w - lx, h - ly),                                                 # the partial last tile column and row only
                  (0, ly, w, h - ly)):                                                      # the last tile row only
            out.append((w, h, c, tw, th, planar) + r)
    return out


def test_region_plan_matches_the_model(mi):
    cases = _cases()
    assert len(cases) >= 1000
    for case in cases:
        want = model_plan(*case)
        assert want is not None, case
        assert mi.region_plan(*case) == want, case


def test_region_plan_refuses_bad_rectangles(mi):
    bad = [
        (100, 50, 3, 16, 16, False, 0, 0, 0, 10),           # rw = 0
        (100, 50, 3, 16, 16, False, 0, 0, 10, 0),           # rh = 0
        (100, 50, 3, 16, 16, True, 95, 0, 6, 10),           # past the right edge
        (100, 50, 3, 16, 16, True, 0, 45, 10, 6),           # past the bottom edge
        (100, 50, 3, 16, 16, True, 100, 0, 1, 1),           # x outside the image
        (100, 50, 3, 16, 16, False, 10, 0, 2**32 - 5, 1),   # x + rw wraps 2^32: refused, not taken as 5
        (100, 50, 3, 16, 16, False, 0, 10, 1, 2**32 - 5),   # y + rh wraps
        (100, 50, 0, 16, 16, False, 0, 0, 1, 1),            # no channels
    ]
    for case in bad:
        assert model_plan(*case) is None or case[2] == 0
        with pytest.raises(mi.LlcompError) as e:
            mi.region_plan(*case)
        assert e.value.status == mi.BAD_ARGS, case


def test_sub_geometry_fits_the_codec_workspace(tmp_path):
    """geometry.hpp: sub-slice j is full slice region_full_id(j) (same rectangle, frame, plane), and the sub-geometry's arrays fit the
    full geometry's -- always with the default tuning; under forced LANE_SHIFT / LPW it fits or is refused (never written past)"""
    exe = str(tmp_path / "region_fit_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "llcomp_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "helpers", "region_fit_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, cases, fits, refused = out.stdout.split()
    assert word == "ok" and int(cases) >= 20000 and int(fits) + int(refused) == int(cases)


def test_region_calls_have_no_cpu_path(mi):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    good = bytes([0x9C, 1, 3, 1]) + b"".join(int(v).to_bytes(4, "little") for v in (8, 8, 8, 4, 6)) + (4).to_bytes(4, "little") * 6 + bytes(24)
    for data in (good, bytes([0x79, 3, 2, 0, 2, 0, 1, 2, 3, 4])):
        with pytest.raises(mi.LlcompError) as e:
            mi.decompress_region(data, 0, 0, 1, 1)
        assert e.value.status == mi.NO_DEVICE
        out = np.zeros(64, np.uint8)
        with pytest.raises(mi.LlcompError) as e:
            mi.decompress_region_into(np.frombuffer(data, np.uint8).copy(), out, 0, 0, 1, 1)
        assert e.value.status == mi.NO_DEVICE
    # the rectangle is checked first, on the host: a bad one is BAD_ARGS with or without a device
    with pytest.raises(mi.LlcompError) as e:
        mi.decompress_region(good, 0, 0, 9, 1)
    assert e.value.status == mi.BAD_ARGS
    with pytest.raises(mi.LlcompError) as e:
        mi.Codec(1, 64, 64, 3, 16, 16, True)
    assert e.value.status == mi.NO_DEVICE
