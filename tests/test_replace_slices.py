"""The host-only splice of a region update (llcomp_mi_replace_slices, no GPU): replacing the slices of the tiles a rectangle covers by
the slices of the oracle's container of the modified covered box gives, byte for byte, the oracle's container of the modified picture --
every slice is the reference stream of its own crop.  Every error is decided before anything is written.  And the fit rule of the
encoder on a sub-geometry (geometry.hpp: region_encode_fits) holds over a grid of shapes and hooks."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, make_image


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


# (name, w, h, c, tile_w, tile_h, planar, generator)
GEOMETRIES = [
    ("rows_480x1p", 1100, 24, 3, 480, 1, True, "nat"),
    ("tiles_64x64i", 200, 150, 3, 64, 64, False, "mid"),
    ("c1_40x24p", 300, 200, 1, 40, 24, True, "g3"),
    ("two_row_40x2p", 160, 41, 3, 40, 2, True, "nat"),
    ("odd_19x13p", 100, 37, 3, 19, 13, True, "checker"),
    ("c4_48x16i", 300, 200, 4, 48, 16, False, "mid"),
]


def twelve_rects(w, h, tw, th, seed):
    """ten seeded random rectangles, the partial (or last) tile alone, the first tile alone"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(10):
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        out.append((x, y, int(rng.integers(1, w - x + 1)), int(rng.integers(1, h - y + 1))))
    lx, ly = (w - 1) // tw * tw, (h - 1) // th * th
    out.append((lx, ly, w - lx, h - ly))
    out.append((0, 0, min(tw, w), min(th, h)))
    return out


def split(container):
    """(u32 lengths, payload bytes) of a SLICED container"""
    n = int.from_bytes(container[20:24], "little")
    return np.frombuffer(container[24:24 + 4 * n], dtype="<u4"), container[24 + 4 * n:]


def modified(img, x, y, rw, rh, seed):
    new = img.copy()
    rng = np.random.default_rng(seed)
    patch = rng.integers(0, 256, size=(rh, rw, img.shape[2]), dtype=np.uint8)
    patch[: rh // 2] = (img[y:y + rh // 2, x:x + rw].astype(np.int32) + 3).clip(0, 255).astype(np.uint8)  # (half noise, half a near copy)
    new[y:y + rh, x:x + rw] = patch
    return new


def covered_box_pixels(mi, img, tw, th, planar, rect):
    h, w, c = img.shape
    (tx0, ty0, tx1, ty1), n = mi.region_plan(w, h, c, tw, th, planar, *rect)
    return (tx0, ty0, tx1, ty1), n, img[ty0 * th:min(ty1 * th, h), tx0 * tw:min(tx1 * tw, w)]


@pytest.mark.parametrize("geo", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_splice_equals_full_encode(mi, orc, geo):
    name, w, h, c, tw, th, planar, gen = geo
    img = make_image(gen, w, h, c)
    old = orc.compress_sliced(img, tw, th, planar)
    for i, rect in enumerate(twelve_rects(w, h, tw, th, seed=len(name) * 131 + w)):
        new_img = modified(img, *rect, seed=i)
        box, n, sub_px = covered_box_pixels(mi, new_img, tw, th, planar, rect)
        lens, pay = split(orc.compress_sliced(sub_px, tw, th, planar))
        assert len(lens) == n
        got = mi.replace_slices(old, box, lens, pay)
        assert got == orc.compress_sliced(new_img, tw, th, planar), (name, rect)
        out = np.full(len(got) + 9, 0xA5, np.uint8)
        assert mi.replace_slices_into(np.frombuffer(old, np.uint8), box, lens, pay, out) == len(got)
        assert out[:len(got)].tobytes() == got and (out[len(got):] == 0xA5).all()


def test_whole_picture_box(mi, orc):
    """every slice replaced: the sub-container's table and payload under the old header"""
    img, other = make_image("nat", 200, 90, 3), make_image("g3", 200, 90, 3)
    old, new = orc.compress_sliced(img, 64, 32, True), orc.compress_sliced(other, 64, 32, True)
    (box, n) = mi.region_plan(200, 90, 3, 64, 32, True, 0, 0, 200, 90)
    lens, pay = split(new)
    assert n == len(lens)
    got = mi.replace_slices(old, box, lens, pay)
    assert got == old[:24] + new[24:] == new
    # the old covered slices are never read: garbage in their place, and even a payload cut away, changes nothing
    assert mi.replace_slices(old[:24 + 4 * n], box, lens, pay) == new


def test_errors_leave_the_output_untouched(mi, orc):
    img = make_image("mid", 200, 150, 3)
    old = orc.compress_sliced(img, 64, 64, False)  # 4 x 3 tiles
    lens_old, _ = split(old)
    box = (1, 1, 3, 2)
    sub = orc.compress_sliced(img[64:128, 64:192], 64, 64, False)
    lens, pay = split(sub)
    good = mi.replace_slices(old, box, lens, pay)
    assert good == old  # (the same pixels: the same slices)
    src = np.frombuffer(old, np.uint8)
    out = np.full(len(old) + 64, 0xA5, np.uint8)

    def refused(status, data=src, b=box, ln=lens, cap=None, pay=pay):
        o = out if cap is None else out[:cap]
        with pytest.raises(mi.LlcompError) as e:
            mi.replace_slices_into(data, b, ln, pay, o)
        assert e.value.status == status, (e.value.status, status)
        assert (out == 0xA5).all(), "an error wrote to the output"
        return e.value

    legacy = np.frombuffer(orc.compress_image(img), np.uint8)
    refused(mi.BAD_ARGS, data=legacy)
    for bad in ((1, 1, 5, 2), (1, 1, 3, 4), (2, 1, 2, 2), (1, 2, 3, 2), (3, 1, 1, 2), (4, 0, 5, 1)):  # outside the 4 x 3 grid, or empty
        refused(mi.BAD_ARGS, b=bad)
    refused(mi.TRUNCATED, data=src[:20])                     # header cut short, as probe
    refused(mi.TRUNCATED, data=src[:24 + 4 * len(lens_old) - 1])  # table cut short, as probe
    too_long = lens.copy()
    too_long[1] = 64 * 64 * 3 * 13 + 48 - 16 + 1               # one above the SLICED limit of this tiling
    refused(mi.TRUNCATED, ln=too_long, pay=pay + bytes(int(too_long[1])))  # (the bytes are there: the length itself is refused)
    refused(mi.TRUNCATED, data=src[:len(old) - 1])           # the last slice is uncovered and runs past the data
    e = refused(mi.OUTPUT_OVERFLOW, cap=len(old) - 1)
    assert e.needed == len(old)
    L = mi._lib.load()
    n = mi.C.c_size_t()
    b4 = (mi.C.c_uint32 * 4)(*box)
    for args in ((None, len(old), b4, lens.ctypes.data, src.ctypes.data), (src.ctypes.data, len(old), None, lens.ctypes.data, src.ctypes.data),
                 (src.ctypes.data, len(old), b4, None, src.ctypes.data), (src.ctypes.data, len(old), b4, lens.ctypes.data, None)):
        assert L.llcomp_mi_replace_slices_into(*args, out.ctypes.data, out.size, mi.C.byref(n)) == mi.BAD_ARGS
        assert (out == 0xA5).all()
    # a covered slice that runs past the data is NOT an error: it is never read (the last tile row is covered, the data ends inside it)
    cut = 24 + 4 * len(lens_old) + int(lens_old[:9].sum()) + 1
    l2, p2 = split(orc.compress_sliced(img[128:150], 64, 64, False))
    assert mi.replace_slices(old[:cut], (0, 2, 4, 3), l2, p2) == old


def test_region_encode_fit_rule(tmp_path):
    """geometry.hpp: region_sub_id inverts region_full_id, and the arrays the encoder touches for a box's sub-geometry fit what the codec
    sized for the full one -- with the default tuning always; under the forced hooks (LANE_SHIFT, LPW, NOROWS, NOSNAP, NOLDSTAB) none of
    the grid's cases is refused either, so the refusal count is asserted to be zero"""
    exe = str(tmp_path / "region_encode_fit_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "llcomp_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "helpers", "region_encode_fit_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, cases, fits, refused, refused_decode = out.stdout.split()
    assert word == "ok" and int(cases) >= 100000 and int(fits) == int(cases)
    assert int(refused) == 0 and int(refused_decode) == 0
