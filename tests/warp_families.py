"""The seeded map families of the CPU rule tests, restated for one fixed batch -- the 4 frames of 48 x 40 of test_gpu_warped_views.py --
so that the device gathers run them (test_gpu_warp_families.py; their own checks, without a GPU: test_device_domains.py): 300 affine
maps with the distribution of test_warp_rule.family and 300 keystones of perspective_cases.keystone, binned into eight output shapes.
A view is (frame, the map's numbers, mirrored); the filter is the call's."""
import functools
import math

import numpy as np

from perspective_cases import keystone

W, H, FRAMES = 48, 40, 4
N = 300
SHAPES = ((1, 1), (2, 3), (5, 4), (9, 13), (16, 16), (24, 17), (33, 39), (39, 39))  # (ow, oh)
FILTERS = ("nearest", "bilinear", "bicubic")
AFFINE_SEED, KEYSTONE_SEED = 4242, 1207  # test_warp_rule.family's and test_perspective_rule.family's
FILL = 200


def fill_of(c):
    return [(FILL + 31 * ch) % 256 for ch in range(c)]


@functools.lru_cache(None)
def affine(seed=AFFINE_SEED):
    """[(shape index, frame, m, mirrored)]: rotations, shears and scales of 0.5 .. 2, the translations from the frame's size; every fifth
    a pure scale, mirrored in x for an even index; every seventh an integer translate; every fourth view's mirror bit set"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(N):
        si = int(rng.integers(0, len(SHAPES)))
        ow, oh = SHAPES[si]
        ang, sx, sy, sh = rng.uniform(0, 2 * math.pi), rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0), rng.uniform(-0.7, 0.7)
        m = [sx * math.cos(ang), sx * (math.sin(ang) + sh), 0.0, -sy * math.sin(ang), sy * math.cos(ang), 0.0]
        if i % 5 == 0:
            m[0], m[1], m[3], m[4] = sx * (1 if i % 2 else -1), 0.0, 0.0, sy
        if i % 7 == 0:
            m[0], m[1], m[3], m[4] = 1.0, 0.0, 0.0, 1.0
        # the translation: the output's centre reads a point of the frame widened by an eighth of its size on every side
        px, py = rng.uniform(-W / 8, 9 * W / 8), rng.uniform(-H / 8, 9 * H / 8)
        m[2], m[5] = px - (m[0] * ow + m[1] * oh) / 2, py - (m[3] * ow + m[4] * oh) / 2
        if i % 7 == 0:
            m[2], m[5] = float(round(m[2])), float(round(m[5]))
        out.append((si, int(rng.integers(0, FRAMES)), tuple(float(t) for t in m), i % 4 == 3))
    return out


@functools.lru_cache(None)
def keystones(mi, seed=KEYSTONE_SEED):
    """([(shape index, frame, a, mirrored)], refused): the frame's corners moved by up to a quarter of a side, every fourth family member
    shifted by up to half a side as well.  A map outside the rule's limits under any filter is counted in `refused` and the next draw
    takes its place, so the family always has N members"""
    rng = np.random.default_rng(seed)
    out, refused = [], 0
    probe = np.zeros((H, W, 1), np.uint8)
    while len(out) < N:
        i = len(out)
        si, frame = int(rng.integers(0, len(SHAPES))), int(rng.integers(0, FRAMES))
        ow, oh = SHAPES[si]
        a = keystone(mi, rng, W, H, ow, oh, shift=rng.uniform(-0.5, 0.5, 2) if i % 4 == 1 else 0.0)
        try:
            for name in FILTERS:
                mi.perspective_reference(probe, a, name, ow, oh)
        except mi.LlcompError:
            refused += 1
            continue
        out.append((si, frame, tuple(float(t) for t in a), i % 4 == 3))
    return out, refused


def witness(persp):
    """the committed vector that a fused multiply-add changes (tests/golden/warp_rule.json, perspective_rule.json), as one more member:
    a 16 x 16 view of frame 0, whose top left corner holds the vector's image in both batches -> (member, filter name, (x, y) of the
    output pixel, its byte, its byte under a fused multiply-add).  A seeded family cannot be relied on to hold such a pixel: in binary64
    a contraction moves a byte once in some 10^13 pixels"""
    from conftest import load_golden

    v = [v for v in load_golden("perspective_rule.json" if persp else "warp_rule.json")["vectors"] if v.get("contraction_sensitive")][0]
    name = "nearest" if persp else "bilinear"
    x, y = v["pixel"] if persp else (0, 0)
    at = y * v["ow"] + x
    return (4, 0, tuple(float.fromhex(t) for t in v["a" if persp else "m"]), False), name, (x, y), v[name][at], v[name + "_fused"][at]


def groups(members):
    """the family by output shape: [(shape index, [member, ...])], empty shapes left out"""
    return [(si, [m for m in members if m[0] == si]) for si in range(len(SHAPES)) if any(m[0] == si for m in members)]


def reference(mi, imgs, members, name, persp):
    """the rule's u8 HWC output of every member of one shape: [n, oh, ow, c], mirrored where the member says so"""
    c = imgs.shape[-1]
    ref = mi.perspective_reference if persp else mi.warp_reference
    outs = []
    for si, frame, m, mirrored in members:
        o = ref(imgs[frame], list(m), name, SHAPES[si][0], SHAPES[si][1], fill_of(c))
        outs.append(o[:, ::-1] if mirrored else o)
    return np.stack(outs)


def fill_share(mi, imgs, members, name, persp):
    """the share of the family's views that are constant fill under the filter"""
    c = imgs.shape[-1]
    fill = np.array(fill_of(c), np.uint8)
    n = 0
    for si, ms in groups(members):
        n += int((reference(mi, imgs, ms, name, persp) == fill).all(axis=(1, 2, 3)).sum())
    return n / len(members)
