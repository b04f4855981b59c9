"""The seeded map families of tests/test_warp_rule.py and tests/test_perspective_rule.py through the device gathers (warp_kernels.hip
with warp_rule.hpp): 300 affine maps and 300 keystones on the 48 x 40 frames of test_gpu_warped_views.py, with 1, 3 and 4 channels,
binned into eight output shapes from 1 x 1 to 39 x 39 -- dozens of views a group -- and the committed contraction-sensitive vector
of each rule, under NEAREST, BILINEAR and BICUBIC, one call per filter and channel count; every tenth group is float16 CHW.  Expected: llcomp_mi_warp_reference / llcomp_mi_perspective_reference
through llcomp_mi_output_table, bit for bit, and Image.transform itself for one filter where PIL is installed.  The families and what
they have to be like: tests/warp_families.py, tests/test_device_domains.py."""
import time

import numpy as np
import pytest

import test_gpu_perspective_views as persp
import test_gpu_warped_views as warped
import warp_families as wf
from test_gpu_resized_output import same_bits
from test_gpu_resized_regions import packed
from test_gpu_warped_views import BICUBIC, BILINEAR, NEAREST, flag, mi  # noqa: F401  (mi: the fixture)

pytestmark = pytest.mark.gpu

CHANNELS = (1, 3, 4)
FILTERS = {"nearest": NEAREST, "bilinear": BILINEAR, "bicubic": BICUBIC}
CALLS = [(c, name) for c in CHANNELS for name in FILTERS]


def family_groups(mod, members, name, call):
    """the family as groups of one call, a group per output shape: u8 HWC, and float16 CHW for every tenth group of all the calls"""
    groups = []
    for gi, (si, ms) in enumerate(wf.groups(members)):
        views = [(frame, *m, flag(FILTERS[name], mirrored)) for _, frame, m, mirrored in ms]
        half = (call * len(wf.SHAPES) + gi) % 10 == 9
        cls = mod.PG if mod is persp else mod.WG
        groups.append(cls(views, *wf.SHAPES[si], *(("float16", "chw") if half else ()), fill=wf.FILL))
    return groups


def run_family(mi, orc, mod, members, c, name, one=None):
    imgs, conts = mod.batch(orc, c, 16, 16, False)
    groups = family_groups(mod, members, name, CALLS.index((c, name)))
    assert len(groups) <= 8 and sum(len(g.views) for g in groups) == wf.N + 1 and min(len(g.views) for g in groups) >= 24
    t0 = time.perf_counter()
    want = [g.expected(mi, imgs, one) for g in groups]
    print("host s %.2f" % (time.perf_counter() - t0))
    codec = mi.Codec(wf.FRAMES, wf.W, wf.H, c, 16, 16, False, device=0)
    try:
        st, outs = (persp.run_persp if mod is persp else warped.run_warp)(mi, codec, groups, c, dev=packed(mi, conts))
        assert st == 0
        for g, out, exp in zip(groups, outs, want):
            if not same_bits(out, exp):
                at = np.argwhere(out.view(np.uint8).reshape(len(g.views), -1) != exp.view(np.uint8).reshape(len(g.views), -1))[0]
                raise AssertionError((name, c, g.ow, g.oh, g.dtype, g.views[int(at[0])], int(at[1])))
    finally:
        codec.close()


@pytest.mark.parametrize("c,name", CALLS, ids=["c%d_%s" % k for k in CALLS])
def test_affine_family(mi, orc, c, name):
    run_family(mi, orc, warped, wf.affine() + [wf.witness(False)[0]], c, name)


@pytest.mark.parametrize("c,name", CALLS, ids=["c%d_%s" % k for k in CALLS])
def test_keystone_family(mi, orc, c, name):
    run_family(mi, orc, persp, wf.keystones(mi)[0] + [wf.witness(True)[0]], c, name)


@pytest.mark.parametrize("c", CHANNELS)
def test_families_are_pil_under_bilinear(mi, orc, c):
    Image = pytest.importorskip("PIL.Image")
    run_family(mi, orc, warped, wf.affine() + [wf.witness(False)[0]], c, "bilinear", warped.pil_one(Image))
    run_family(mi, orc, persp, wf.keystones(mi)[0] + [wf.witness(True)[0]], c, "bilinear", persp.pil_one(Image))
