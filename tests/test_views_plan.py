"""llcomp_mi_views_plan (host only): what a views decode decodes -- per frame the bounding box of its views over all groups, and from the
used frames' boxes alone the windows and classes of llcomp_mi_resized_regions_plan.  Compared with a few-line restatement, and every
refusal with the outputs untouched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import llcomp_amd as mi
from resize_spec import random_resized_crop
from test_resized_regions_plan import SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restated(w, h, c, tw, th, planar, frames, groups):
    """bounding box per frame, then resized_regions_plan of the used frames"""
    uni = np.zeros((frames, 4), np.uint32)
    for f in range(frames):
        mine = [v for views, _, _ in groups for v in views if v[0] == f]
        if mine:
            x0, y0 = min(v[1] for v in mine), min(v[2] for v in mine)
            uni[f] = (x0, y0, max(v[1] + v[3] for v in mine) - x0, max(v[2] + v[4] for v in mine) - y0)
    used = [f for f in range(frames) if uni[f, 2]]
    win = np.zeros((frames, 4), np.uint32)
    win[used], ncls = mi.resized_regions_plan(w, h, c, tw, th, planar, uni[used])
    return uni, win, len(used), ncls


def random_groups(rng, w, h, frames, kind):
    """two or three groups of views as (frame, x, y, rw, rh, flags); outputs no smaller than 1/16 of the image, so no downscale limit is met"""
    outs = [(max(1, -(-w // 16)), max(1, -(-h // 16))), (w, h), (max(1, w // 3), max(1, h // 2))][:int(rng.integers(2, 4))]
    busy = [f for f in range(frames) if kind != "gaps" or f % 2 == 0] or [0]
    groups = []
    for ow, oh in outs:
        views = []
        for _ in range(int(rng.integers(1, 7))):
            f = int(busy[rng.integers(0, len(busy))])
            views.append((f,) + tuple(random_resized_crop(rng, w, h, scale=(0.02, 0.6))) + (int(rng.integers(0, 2)) | (int(rng.integers(0, 6)) << 4),))
        groups.append((views, ow, oh))
    if kind == "whole":  # two views whose union is the whole image, and nothing else of that frame matters
        groups[0][0].append((busy[0], 0, 0, w, 1, 0))
        groups[-1][0].append((busy[0], 0, 0, 1, h, 0))
    elif kind == "last_pixel":
        groups[0][0].append((busy[-1], w - 1, h - 1, 1, 1, 1))
    return groups


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}_{s[3]}x{s[4]}" for s in SHAPES])
def test_plan_equals_bounding_boxes_then_resized_regions_plan(shape):
    w, h, c, tw, th, planar = shape
    rng = np.random.default_rng(w * 11 + h)
    for i in range(48):
        frames = int(rng.integers(1, 7))
        kind = ("random", "gaps", "whole", "last_pixel")[i % 4]
        groups = random_groups(rng, w, h, frames, kind)
        uni, win, n_used, ncls = mi.views_plan(w, h, c, tw, th, planar, frames, groups)
        want = restated(w, h, c, tw, th, planar, frames, groups)
        assert np.array_equal(uni, want[0]) and np.array_equal(win, want[1]) and (n_used, ncls) == want[2:], (kind, groups)
        if kind == "whole":
            assert (0, 0, w, h) in [tuple(r) for r in uni.tolist()]
        if kind == "gaps" and frames > 1:
            assert n_used < frames and not uni[1].any() and not win[1].any()


def test_one_last_pixel_view_alone():
    w, h = 100, 70
    uni, win, n_used, ncls = mi.views_plan(w, h, 3, 32, 32, True, 3, [([(2, w - 1, h - 1, 1, 1)], 8, 8)])
    assert uni.tolist() == [[0] * 4, [0] * 4, [w - 1, h - 1, 1, 1]] and win.tolist() == [[0] * 4, [0] * 4, [3, 2, 4, 3]] and (n_used, ncls) == (1, 1)


def raw_plan(L, w, h, frames, arr, n):
    """the C call itself with sentinel-filled outputs -> (status, outputs untouched?)"""
    uni, win = np.full(4 * frames, 0xA5A5A5A5, np.uint32), np.full(4 * frames, 0xA5A5A5A5, np.uint32)
    used, k = C.c_uint32(0xA5A5A5A5), C.c_uint32(0xA5A5A5A5)
    u32p = C.POINTER(C.c_uint32)
    rc = L.llcomp_mi_views_plan(w, h, 3, 32, 16, 1, frames, arr, n, uni.ctypes.data_as(u32p), win.ctypes.data_as(u32p), C.byref(used), C.byref(k))
    return rc, bool((uni == 0xA5A5A5A5).all() and (win == 0xA5A5A5A5).all() and used.value == k.value == 0xA5A5A5A5)


def test_refusals_leave_the_outputs_untouched():
    L = mi._lib.load()
    w, h, frames = 200, 100, 3
    good = [(0, 0, 0, 50, 50, 0), (2, 10, 10, 20, 20, 1)]
    arr, n, keep = mi._view_groups([(good, 32, 32)], 3)
    assert raw_plan(L, w, h, frames, arr, n) == (mi.OK, False)
    bicubic, lanczos = mi.FILTER_BICUBIC << 4, mi.FILTER_LANCZOS << 4
    cases = {
        "no groups": [],
        "a group with no views": [(good, 32, 32), ([], 32, 32)],
        "65536 views": [([(0, 0, 0, 8, 8, 0)] * 65536, 8, 8)],
        "frame >= frames": [(good + [(3, 0, 0, 5, 5, 0)], 32, 32)],
        "empty width": [(good + [(1, 0, 0, 0, 5, 0)], 32, 32)],
        "empty height": [(good, 32, 32), ([(1, 0, 0, 5, 0, 0)], 8, 8)],
        "past the right edge": [(good + [(1, 151, 0, 50, 50, 0)], 32, 32)],
        "past the bottom edge": [(good + [(1, 0, 51, 50, 50, 0)], 32, 32)],
        "x + rw wraps": [(good + [(1, 0xFFFFFFFF, 0, 2, 1, 0)], 32, 32)],
        "filter code 6": [(good + [(1, 0, 0, 5, 5, 6 << 4)], 32, 32)],
        "filter code 7": [(good + [(1, 0, 0, 5, 5, 7 << 4 | 1)], 32, 32)],
        "downscale above 64x (width)": [(good, 32, 32), ([(1, 0, 0, 193, 10, 0)], 3, 3)],
        "downscale above 64x (height)": [(good, 32, 32), ([(1, 0, 0, 10, 65, 0)], 3, 1)],
        "bicubic above 32x": [([(1, 0, 0, 97, 10, bicubic)], 3, 3)],
        "lanczos above 64/3": [([(1, 0, 0, 10, 65, lanczos)], 3, 3)],
        "ow 0": [(good, 0, 32)],
        "oh 0": [(good, 32, 0)],
    }
    for name, groups in cases.items():
        arr, n, keep = mi._view_groups(groups, 3)
        assert raw_plan(L, w, h, frames, arr, n) == (mi.BAD_ARGS, True), name
        with pytest.raises(mi.LlcompError) as e:
            mi.views_plan(w, h, 3, 32, 16, True, frames, groups)
        assert e.value.status == mi.BAD_ARGS, name
    # the limits themselves pass: 65535 views, exactly 64x, 32x for bicubic, 63 -> 3 for Lanczos, and the same rectangle for another group's output
    for groups in ([([(0, 0, 0, 8, 8, 0)] * 65535, 8, 8)], [([(1, 0, 0, 192, 64, 0)], 3, 1)], [([(1, 0, 0, 96, 10, bicubic)], 3, 3)],
                   [([(1, 0, 0, 10, 63, lanczos)], 3, 3)], [([(1, 0, 0, 193, 10, 0)], 4, 3)]):
        mi.views_plan(w, h, 3, 32, 16, True, frames, groups)
    # NULL pointers and a struct_size that is not the struct's
    arr, n, keep = mi._view_groups([(good, 32, 32)], 3)
    used, k = C.c_uint32(), C.c_uint32()
    assert L.llcomp_mi_views_plan(w, h, 3, 32, 16, 1, frames, None, 1, None, None, C.byref(used), C.byref(k)) == mi.BAD_ARGS
    assert L.llcomp_mi_views_plan(w, h, 3, 32, 16, 1, frames, arr, n, None, None, None, C.byref(k)) == mi.BAD_ARGS
    assert L.llcomp_mi_views_plan(w, h, 3, 32, 16, 1, frames, arr, n, None, None, C.byref(used), None) == mi.BAD_ARGS
    assert L.llcomp_mi_views_plan(w, h, 3, 32, 16, 1, frames, arr, n, None, None, C.byref(used), C.byref(k)) == mi.OK and used.value == 2
    arr[0].struct_size -= 8
    assert raw_plan(L, w, h, frames, arr, n) == (mi.BAD_ARGS, True)


def test_plan_and_frame_list_gather_under_sanitizers(tmp_path):
    """the host side of a views decode as a stand-alone program under AddressSanitizer and UBSan (tests/helpers/views_plan_check.cpp):
    the plan against a brute-force bounding box with outputs of exactly 4 * frames values, and the gather over the frame list with
    every unused frame's container NULL"""
    exe = str(tmp_path / "views_plan_check")
    csrc = os.path.join(ROOT, "llcomp_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "helpers", "views_plan_check.cpp"), os.path.join(csrc, "container.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, plans, gathers = out.stdout.split()
    assert word == "ok" and int(plans) == int(gathers) == 1000
