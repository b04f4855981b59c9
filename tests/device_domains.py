"""What the whole-domain GPU tests of the device arithmetic share (test_gpu_photo_domains.py, test_gpu_mix_domains.py; their own
checks, without a GPU: test_device_domains.py): the frames, the factor set F with its contraction witnesses, the hue factor of every
shift byte, the blur's threshold radii, and the bit patterns, partners and lambdas of the blend.  Nothing here calls the library: the
expected values are tests/photo_spec.py's and tests/mix_spec.py's, and a witness is an input on which a NAMED mistake of the device
compilation -- a product and a sum contracted into a fused multiply-add, a subnormal flushed to zero, a tie rounded the other way --
gives other bits than the rule, so that the sweeps cannot stay green under it."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import photo_spec

F32 = np.float32
WORKERS = 8  # threads of the expected values: numpy releases the lock inside its loops


def pmap(fn, items):
    """fn over items on WORKERS threads, in order"""
    items = list(items)
    with ThreadPoolExecutor(WORKERS) as pool:
        return list(pool.map(fn, items))


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
SIDE = 4096


@functools.lru_cache(None)
def all_colours():
    """4096 x 4096 RGB, every colour once: pixel i = y * 4096 + x is (i >> 16, (i >> 8) & 255, i & 255) -- test_photo_area_rule.py's"""
    a = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([a >> 16, (a >> 8) & 255, a & 255], axis=-1).astype(np.uint8).reshape(SIDE, SIDE, 3)


@functools.lru_cache(None)
def all_levels():
    """the one-channel frame of the c = 1 legs: 4096 x 4096, every value in every 16 x 16 square"""
    y, x = np.mgrid[0:SIDE, 0:SIDE]
    return (((y & 15) << 4) | (x & 15)).astype(np.uint8)[..., None]


def tiles(side=SIDE, step=1024):
    """the own-size rectangles (x, y, w, h) that cover a square frame"""
    return [(x, y, step, step) for y in range(0, side, step) for x in range(0, side, step)]


PAIRS_SIDE = 512


@functools.lru_cache(None)
def pairs_frame():
    """512 x 512 RGB with every (max - min, max) pair of a pixel -- the pair that S and V are computed from -- in every order of the
    three channels, the middle channel seeded: 32896 pairs x 6 orders, and seeded colours behind them.  (No 512 x 512 rectangle of
    all_colours() can hold every pair: its red spans 32 values, a pixel's max is at least its red and its min at most.)"""
    rng = np.random.default_rng(512)
    mx, d = np.array([(m, m - n) for m in range(256) for n in range(m + 1)]).T
    mn = mx - d
    px = []
    for order in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        mid = mn + (rng.random(len(mx)) * (d + 1)).astype(np.int64)
        p = np.empty((len(mx), 3), np.int64)
        p[:, order[0]], p[:, order[1]], p[:, order[2]] = mx, mid, mn
        px.append(p)
    px = np.concatenate(px)
    rest = rng.integers(0, 256, (PAIRS_SIDE * PAIRS_SIDE - len(px), 3))
    return np.concatenate([px, rest]).astype(np.uint8).reshape(PAIRS_SIDE, PAIRS_SIDE, 3)


def pair_classes(img):
    """the set of (max - min, max) of an RGB image's pixels, as a [256, 256] mask"""
    v = img.reshape(-1, 3).astype(np.int64)
    seen = np.zeros((256, 256), bool)
    seen[v.max(1) - v.min(1), v.max(1)] = True
    return seen


@functools.lru_cache(None)
def white_heavy(c):
    """4352 x 4096: white but for one pixel in 64, which takes seeded values from 40 to 239, the low ones more often, and for one pixel
    of 16 -- the sum of L passes 2^32 (4096 x 4096 pixels cannot: 2^24 * 255 < 2^32), autocontrast stretches from a value that a
    single lost count would move, and equalize's table is far from the identity"""
    rng = np.random.default_rng(4352 + c)
    img = np.full((SIDE, 4352, c), 255, np.uint8)
    flat = img.reshape(-1, c)
    flat[::64] = (40 + 200 * rng.random((len(flat[::64]), c)) ** 2).astype(np.uint8)
    flat[64 * 7777] = 16
    return img


# ---- blend: the contraction witnesses and the factor set F -----------------------------------------------------------------------------
def blend_fused(d, v, a):
    """photo_spec.blend with t = d + a * (v - d) rounded ONCE: computed in binary64, then rounded to binary32 -- what a fused
    multiply-add gives"""
    a = F32(a)
    d = np.asarray(d, np.int64)
    t = (d.astype(np.float64) + np.float64(a) * (np.asarray(v, np.int64) - d).astype(np.float64)).astype(F32)
    if 0 <= a <= 1:
        return np.trunc(t).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def colour_of(d, v):
    """an RGB pixel with L == d and a channel == v, or None: COLOR blends such a pixel's channel from d"""
    g, b = np.mgrid[0:256, 0:256]
    for ch in range(3):
        p = [g, b]
        p.insert(ch, np.full_like(g, v))
        hit = np.argwhere(photo_spec.luma(np.stack(p, axis=-1).astype(np.uint8)) == d)
        if len(hit):
            q = [int(hit[0][0]), int(hit[0][1])]
            q.insert(ch, int(v))
            return tuple(q)
    return None


def blend_witnesses(ds, n_factors=256, seed=2024, top=2.0):
    """(a, d, v, byte, fused byte) with d in ds, a of n_factors seeded binary32 factors in [0, top): triples on which the fused
    evaluation of photo_blend gives another byte than the separate one"""
    rng = np.random.default_rng(seed)
    ds = np.asarray(list(ds), np.int64)
    d, v = np.meshgrid(ds, np.arange(256), indexing="ij")
    out = []
    for a in rng.uniform(0.0, top, n_factors).astype(F32):
        sep, fus = photo_spec.blend(d, v, a), blend_fused(d, v, a)
        out += [(float(a), int(d[i, j]), int(v[i, j]), int(sep[i, j]), int(fus[i, j])) for i, j in np.argwhere(sep != fus)]
    return out


CONTRAST_MEANS = range(64, 192)  # what a widened view of ramp_frame() can have as its mean


@functools.lru_cache(None)
def witnesses():
    """the first three witnesses of general d whose d a contrast view can have as its mean and whose (d, v) some colour has as (L, a
    channel).  d = 0 has none: 0 + a * v rounds once either way, so BRIGHTNESS cannot tell a fused multiply-add (brightness_has_none)"""
    found = []
    for w in blend_witnesses(CONTRAST_MEANS):
        if colour_of(w[1], w[2]) is not None and w[0] not in [f[0] for f in found]:
            found.append(w)
            if len(found) == 3:
                break
    return found


def brightness_has_none(n_factors=256):
    return not blend_witnesses([0], n_factors) and not blend_witnesses([0], n_factors, seed=7, top=256.0)


@functools.lru_cache(None)
def factors():
    """F: the witnesses' factors first; 0, 1, the two binary32 neighbours of 1, 0.5, 0.25, 1.5, 2, 255/256, 1e-8, the binary32 subnormal
    1e-40, 100.3, 256; then 40 seeded ones, half uniform in [0, 2], half log-uniform in [2^-30, 256] -- all rounded to binary32"""
    rng = np.random.default_rng(77)
    fixed = [0.0, 1.0, np.nextafter(F32(1), F32(0)), np.nextafter(F32(1), F32(2)), 0.5, 0.25, 1.5, 2.0, 255 / 256, 1e-8, 1e-40, 100.3, 256.0]
    seeded = list(rng.uniform(0.0, 2.0, 20)) + list(2.0 ** rng.uniform(-30.0, 8.0, 20))
    return [w[0] for w in witnesses()] + [float(F32(f)) for f in fixed + seeded]


def more_factors(n=512, seed=78):
    rng = np.random.default_rng(seed)
    return [float(F32(f)) for f in list(rng.uniform(0.0, 2.0, n // 2)) + list(2.0 ** rng.uniform(-30.0, 8.0, n - n // 2))]


# ---- hue: a factor for every shift byte -------------------------------------------------------------------------------------------------
def hue_factor(shift):
    """a binary32 factor within -0.5 .. 0.5 whose photo_spec.hue_shift is the byte `shift`: 0 .. 127 from above, 129 .. 255 from below;
    128 is no factor's byte (-0.5 gives -127.5, truncated to -127 = 129)"""
    s = shift if shift < 128 else shift - 256
    f = F32((s + (0.5 if s >= 0 else -0.5)) / 255.0)
    return float(f)


SHIFTS = [s for s in range(256) if s != 128]


# ---- the small frames of the parameter sweeps ---------------------------------------------------------------------------------------
BANDS = 256


@functools.lru_cache(None)
def ramp_frame(c):
    """32 x 4096: band k, the 16 rows from 16 k, holds all 256 values in every channel of its left 16 columns (a different order in
    each channel) and the gray k in its right 16.  (0, 16 k, 16, 16) is a view of all 256 values, (0, 16 k, 32, 16) the same widened
    by a constant half: its mean L runs from 64 to 191 with k"""
    y, x = np.mgrid[0:16, 0:16]
    ramp = (y * 16 + x).astype(np.uint8)
    left = np.stack([ramp, 255 - ramp, (ramp.astype(np.int64) * 7 + 3).astype(np.uint8)][:c], axis=-1)
    img = np.empty((16 * BANDS, 32, c), np.uint8)
    for k in range(BANDS):
        img[16 * k:16 * k + 16, :16] = left
        img[16 * k:16 * k + 16, 16:] = k
    return img


def mean_l(img):
    """CONTRAST's degenerate value of a view (include/llcomp_mi.h): (int)((double)sum of L / (double)n + 0.5)"""
    lum = photo_spec.luma(img)
    return int(float(int(lum.sum())) / float(lum.size) + 0.5)


@functools.lru_cache(None)
def band_means(c):
    f = ramp_frame(c)
    return [mean_l(f[16 * k:16 * k + 16]) for k in range(BANDS)]


def contrast_views(c):
    """(band, factor) of every contrast view: each factor of F on four bands 64 apart, and each witness's factor on a band whose mean
    is the witness's d"""
    means = band_means(c)
    out = [(means.index(w[1]), w[0]) for w in witnesses()]
    for j, a in enumerate(factors()):
        out += [((37 * j + 64 * i) % BANDS, a) for i in range(4)]
    return out


NOISE_W, NOISE_H = 96, 48


@functools.lru_cache(None)
def noise_frames(c):
    """two frames of 96 x 48 noise: the sharpness's 70 x 33 views"""
    return np.random.default_rng(7033 + c).integers(0, 256, (2, NOISE_H, NOISE_W, c), dtype=np.uint8)


@functools.lru_cache(None)
def block_frames(c):
    """two frames of 96 x 48 of seeded 0 / 255 blocks, 4 x 4 in frame 0 and 3 x 5 in frame 1: the blur's 24 x 24 views"""
    rng = np.random.default_rng(2424 + c)
    out = np.empty((2, NOISE_H, NOISE_W, c), np.uint8)
    for f, (bw, bh) in enumerate(((4, 4), (3, 5))):
        cells = rng.integers(0, 2, (-(-NOISE_H // bh), -(-NOISE_W // bw), c), dtype=np.uint8) * 255
        out[f] = np.repeat(np.repeat(cells, bh, axis=0), bw, axis=1)[:NOISE_H, :NOISE_W]
    return out


def spots(n, vw, vh, seed):
    """n seeded (frame, x, y) of vw x vh views inside the 96 x 48 frames"""
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(0, 2)), int(rng.integers(0, NOISE_W - vw + 1)), int(rng.integers(0, NOISE_H - vh + 1))) for _ in range(n)]


# ---- blur: the radii at which the box radius steps ---------------------------------------------------------------------------------------
def _f32_of(bits):
    return np.array([bits], np.uint32).view(F32)[0]


def _bits_of(f):
    return int(np.array([f], F32).view(np.uint32)[0])


TOP_R = photo_spec.blur_weights(32.0)[1]  # 31: the largest whole box radius the limit of 32 lets through, so no radius steps to 32


@functools.lru_cache(None)
def blur_thresholds():
    """for every whole box radius r in 1 .. TOP_R the smallest binary32 radius whose photo_spec.blur_weights gives r (by bisection
    over the bit patterns: r - 1 just below it)"""
    out = []
    for r in range(1, TOP_R + 1):
        lo, hi = _bits_of(F32(0.0)), _bits_of(F32(32.0))  # r(lo) < r <= r(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if photo_spec.blur_weights(_f32_of(mid))[1] >= r:
                hi = mid
            else:
                lo = mid
        out.append(float(_f32_of(hi)))
    return out


def blur_radii():
    """every threshold with its two binary32 neighbours on each side, and 64 seeded radii in [0, 32]"""
    out = []
    for t in blur_thresholds():
        b = _bits_of(F32(t))
        out += [float(_f32_of(b + k)) for k in (-2, -1, 0, 1, 2)]
    return out + [float(F32(v)) for v in np.random.default_rng(3232).uniform(0.0, 32.0, 64)]


# ---- the blend's bit patterns ------------------------------------------------------------------------------------------------------------
# per dtype: +-0, +-1, +-max, +-inf, a quiet NaN, a NaN with a payload, the smallest subnormal, the smallest normal, 1.5 x the smallest
# normal, eps, -2.5, 1/3
PARTNERS = {
    "float16": [0x0000, 0x8000, 0x3C00, 0xBC00, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0x7D55, 0x0001, 0x0400, 0x0600, 0x1400, 0xC100, 0x3555],
    "bfloat16": [0x0000, 0x8000, 0x3F80, 0xBF80, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0, 0x7FA5, 0x0001, 0x0080, 0x00C0, 0x3C00, 0xC020, 0x3EAB],
    "float32": [0x00000000, 0x80000000, 0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FA55555, 0x00000001,
                0x00800000, 0x00C00000, 0x34000000, 0xC0200000, 0x3EAAAAAB],
}
QUIET_NAN = {"float16": 0x7E00, "bfloat16": 0x7FC0, "float32": 0x7FC00000}
LAM = 0.3712345678901234  # test_gpu_mix_batch.LAM (that module needs a GPU to import; test_device_domains.py holds the two equal)
LAMBDAS = [LAM, 0.5, 0.0, 1.0, 2.0 ** -20, float(np.random.default_rng(616).random())]


def own_bits(dtype):
    """[h, w] of the own values: all 65536 patterns of a 16-bit dtype as 256 x 256; float32: every exponent 0 .. 255 x 32 mantissas (0,
    1, all ones, 0x400000 and 28 seeded) x both signs as 128 x 128"""
    if dtype != "float32":
        return np.arange(65536, dtype=np.uint32).reshape(256, 256)
    man = np.concatenate([[0, 1, 0x7FFFFF, 0x400000], np.random.default_rng(23).integers(0, 1 << 23, 28)]).astype(np.uint32)
    e, s, m = np.meshgrid(np.arange(256, dtype=np.uint32), np.arange(2, dtype=np.uint32), man, indexing="ij")
    return ((s << 31) | (e << 23) | m).reshape(128, 128)


def mix_batch_bits(dtype):
    """[2 P, 1, h, w]: sample 2 k holds own_bits, sample 2 k + 1 is constant at partner pattern k"""
    own = own_bits(dtype)
    out = np.empty((2 * len(PARTNERS[dtype]), 1) + own.shape, np.uint32)
    out[0::2, 0] = own
    out[1::2, 0] = np.array(PARTNERS[dtype], np.uint32)[:, None, None]
    return out


def swap_pairs(n):
    return [i ^ 1 for i in range(n)]


def is_nan_bits(b, dtype):
    exp, man = {"float16": (0x7C00, 0x03FF), "bfloat16": (0x7F80, 0x007F), "float32": (0x7F800000, 0x007FFFFF)}[dtype]
    return ((b & exp) == exp) & ((b & man) != 0)


def mix_expected(dtype, lam):
    """the batch after the swap-pairs blend: torch's bits of mix_spec's two expressions (one lam for the batch: torchvision's line; one
    per sample: timm's), which agree wherever the result is no NaN; where it is one, the dtype's quiet NaN (include/llcomp_mi.h)"""
    import mix_spec

    bits = mix_batch_bits(dtype)
    batch = mix_spec.from_bits(bits, dtype)
    perm = swap_pairs(len(bits))
    one = mix_spec.bits(mix_spec.apply(batch, perm, float(lam))).astype(np.uint32)
    each = mix_spec.bits(mix_spec.apply(batch, perm, [float(lam)] * len(bits))).astype(np.uint32)
    nan = is_nan_bits(one, dtype)
    assert np.array_equal(nan, is_nan_bits(each, dtype)) and np.array_equal(one[~nan], each[~nan])
    return batch, np.where(nan, np.uint32(QUIET_NAN[dtype]), one)


def widen(bits, dtype):
    """bit patterns -> their values in binary64 (exact)"""
    import mix_spec

    return mix_spec.from_bits(bits, dtype).double().numpy()


def narrow(v, dtype):
    """rd of the rule on exact binary64 values: rounded to binary32, then to the dtype (ties to even), as binary64 again"""
    import mix_spec
    import torch

    return torch.from_numpy(np.ascontiguousarray(v).astype(F32)).to(mix_spec.DTYPES[dtype]).double().numpy()


def blend_parts(dtype, lam, k):
    """own values of sample 2 k against partner k, in binary64: (own, w_own, rd(own * w_own), rd(partner * w_partner)); a product of
    two binary32 values is exact in binary64"""
    w_own, w_par = float(F32(lam)), float(F32(1.0 - lam))
    own = widen(own_bits(dtype), dtype)
    par = widen(np.array([PARTNERS[dtype][k]], np.uint32), dtype)[0]
    with np.errstate(all="ignore"):
        return own, w_own, narrow(own * w_own, dtype), narrow(np.array([par * w_par]), dtype)[0]


