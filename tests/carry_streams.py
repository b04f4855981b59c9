"""Tiles that make the range encoder hold back a LONG run of undecided 0xFF bytes, built with the oracle alone (for
test_carry_streams.py, test_gpu_carry_runs.py and helpers/guard_child.py).

The reference resolves a carry lazily (llcomp.hpp:40-57: one byte held back, a count of the 0xFF bytes behind it); the HIP encoders
write every byte at once and walk back through what they wrote when the carry arrives, so the length and the position of such a run
are a dimension of their correctness.  Noise never produces more than 3-5 such bytes (256^-n).  A stream `prefix, K, 00 x n, suffix`
has a value just above K.000...: an encoder that reproduces it approaches that value from below, emits K-1, FF, FF, ... as undecided
bytes and carries once its interval has narrowed enough; `prefix, K, FF x n, suffix` gives the run that stays FF.  Decoding such a
stream with the oracle gives samples; where those are legal pixel values the tile that holds them re-encodes through the run.

A tile is QUALIFIED by the oracle's event log (orc.carry_log: which run, how long, how it went out, between which samples), never by
its bytes.  CASES is the table of crafted tiles the GPU tests use; test_carry_streams.py checks every row of it on the CPU.
"""
import collections
import functools

import numpy as np

BUDGET = 64  # seeds tried per case, from 0: the first that qualifies is the case's seed


@functools.lru_cache(maxsize=None)
def _nat_rgb():
    from llcomp_amd.synth import gen_nat

    return gen_nat(1024, 256, 3)


def natural(orc, w, h, nch=1):
    """int16 (h, w, nch) SAMPLES of a photo-like crop: the green plane (nch = 1), or the colour-transformed crop (nch >= 3)"""
    if nch == 1:
        return _nat_rgb()[100:100 + h, 200:200 + w, 1:2].astype(np.int16)
    from llcomp_amd.synth import gen_nat

    return orc.forward_rct(np.ascontiguousarray(gen_nat(1024, 256, nch)[100:100 + h, 200:200 + w]))


def legal(orc, s):
    """can these samples be the samples of 8-bit pixels?  One plane: 0..255.  Interleaved colour: the transform must give them back."""
    if s.shape[2] < 3:
        return bool(s.min() >= 0 and s.max() <= 255)
    return bool(np.array_equal(orc.forward_rct(orc.inverse_rct(s)), s))


def encode_logged(orc, tile):
    """(stream, every run of the oracle's encoder on this tile)"""
    orc.carry_stats(reset=True)
    stream = orc.encode_samples(tile)
    return stream, orc.carry_log()


def craft_tile(orc, base, rows_before, n, carry, seed, first=None):
    """`base`: int16 (h, w, nch) natural samples.  The stream of its first `rows_before` rows (none: 8..72 random bytes, or exactly
    `first` of them), less 3..18 bytes at its end -- which also shifts the run against the encoders' 16-byte units --, then K, n bytes
    00 (`carry`) or FF, and 48 random bytes, is decoded; the tile is what the decoder saw down to the last row the run can reach
    (n * 4 // w + 2 rows behind the head: no sample here takes less than a quarter byte), natural rows below.  What follows a resolved
    run cannot change it.  -> (tile, log of its encoding), or None where the decoded rows are no pixels."""
    h, w, nch = base.shape
    rng = np.random.default_rng([seed, n, int(carry), w, h])
    if rows_before:
        head = orc.encode_samples(base[:rows_before])
        head = head[:max(len(head) - int(rng.integers(3, 19)), 0)]
    else:
        head = rng.integers(0, 256, size=int(rng.integers(8, 73)) if first is None else first, dtype=np.uint8).tobytes()
    k = int(rng.integers(1, 255))
    stream = head + bytes([k]) + (b"\x00" if carry else b"\xff") * n + rng.integers(0, 256, size=48, dtype=np.uint8).tobytes()
    rows = min(h, rows_before + (n * 4) // (w * nch) + 2)
    rc, got = orc.decode_samples(stream, w, rows, nch)
    if rc != 0 or not legal(orc, got):
        return None
    tile = base.copy()
    tile[:rows] = got
    return (tile,) + encode_logged(orc, tile)[1:]


def craft_open_end(orc, w, n, carry, seed):
    """A one-row tile of w samples whose stream is cut inside the run: random bytes that cost about what w samples take, with K and
    00 / FF from n + 2..12 bytes before the end on, so that the samples run out while the run is open and finish() has to resolve it.
    -> (tile, log) or None."""
    rng = np.random.default_rng([seed, n, int(carry), w])
    noise = rng.integers(0, 256, size=4 * w + 64, dtype=np.uint8).tobytes()
    rc, got = orc.decode_samples(noise, w, 1, 1)
    if rc != 0:
        return None
    used = len(orc.encode_samples(got))  # what w samples took of it, give or take a byte
    at = used - n - int(rng.integers(2, 13))
    if at < 2:
        return None
    stream = noise[:at] + bytes([int(rng.integers(1, 255))]) + (b"\x00" if carry else b"\xff") * (2 * n + 64)
    rc, got = orc.decode_samples(stream, w, 1, 1)
    if rc != 0 or not legal(orc, got):
        return None
    return got, encode_logged(orc, got)[1]


Crafted = collections.namedtuple("Crafted", "seed tile event log")  # `event`: the run that qualified the tile

# ---- the conditions (on the event log) ------------------------------------------------------------------------------------------
SEG = 4096  # samples per launch of the segmented coder (csrc/geometry.hpp: kSnapMaxSamples)


def _pick(log, ok):
    got = [e for e in log if ok(e)]
    return max(got, key=lambda e: e.run) if got else None


def run_of(n, carry, *, in_finish=False, first=None, crosses=None, ends=None):
    """condition: a run of at least n bytes that carried (or stayed FF), resolved before finish() (or in it); `first`: its held byte is
    at an offset <= first; `crosses`: opened before sample `crosses` and resolved at or behind it; `ends`: the last byte of the run is at
    an offset congruent to `ends` modulo 16"""
    def ok(e):
        return (e.run >= n and e.carried == carry and e.in_finish == in_finish and (first is None or e.offset <= first)
                and (crosses is None or e.opened < crosses <= e.resolved) and (ends is None or (e.offset + e.run) % 16 == ends))
    return lambda log: _pick(log, ok)


def search(make, want, budget=BUDGET):
    """the first seed of the budget whose tile is legal and whose log meets `want` -> Crafted, or None"""
    for seed in range(budget):
        got = make(seed)
        if got is None:
            continue
        ev = want(got[1])
        if ev is not None:
            return Crafted(seed, got[0], ev, got[1])
    return None


# ---- the case table ---------------------------------------------------------------------------------------------------------------
# w, h, nch of the tile; rows of natural content in front of the run; bytes of 00 / FF put into the stream; carry?; the condition: a run of
# at least min_run bytes that went out that way, plus `cond` (run_of's keywords; open_end: craft_open_end and "resolved in finish()";
# prefix: exactly that many random bytes in front of K).  seed, run, how: what the search finds -- the first qualifying seed of the budget,
# the measured length of the qualifying run and how it went out; test_carry_streams.py CHECKS all three against a fresh search and prints them.
# Conditions, by the letters of test_carry_streams.py's docstring:
#   (a) carry through >= 17 bytes: a whole 16-byte unit            (b) carry through >= 33: two unit boundaries, more than the 28 staged bytes
#   (c) >= 33 bytes that stay FF   (d) >= 17 bytes still open at finish(), carried / FF   (e) the held byte among the first two of the stream
#   (f) tiles above 4096 samples: opened before sample 4096, resolved at or behind it     (g) the run ends at an offset = 15, 0, 1 mod 16
# Runs >= 64 on 2-D tiles: found for 64x64 (both ways) and for 64x16 staying FF; NOT found in the budget for a 64x16 carry (no row for it).
Case = collections.namedtuple("Case", "w h nch rows_before n carry min_run cond seed run how")
_T, _F = True, False
CASES = {
    # one-row tiles, 600 and 300 wide
    "row600-carry17":  Case(600, 1, 1, 0, 17, _T, 17, (), 6, 17, "carry"),                      # (a)
    "row600-carry33":  Case(600, 1, 1, 0, 33, _T, 33, (), 3, 33, "carry"),                      # (b)
    "row600-ff33":     Case(600, 1, 1, 0, 33, _F, 33, (), 1, 33, "FF"),                         # (c)
    "row600-carry64":  Case(600, 1, 1, 0, 64, _T, 60, (), 8, 64, "carry"),
    "row600-ff64":     Case(600, 1, 1, 0, 64, _F, 60, (), 6, 64, "FF"),
    "row300-carry17":  Case(300, 1, 1, 0, 17, _T, 17, (), 3, 17, "carry"),                      # (a)
    "row300-carry33":  Case(300, 1, 1, 0, 33, _T, 33, (), 27, 33, "carry"),                     # (b)
    "row300-ff33":     Case(300, 1, 1, 0, 33, _F, 33, (), 33, 33, "FF"),                        # (c)
    "row600-open-carry": Case(600, 1, 1, 0, 33, _T, 33, (("open_end", True),), 14, 47, "carry in finish()"),  # (d)
    "row600-open-ff":  Case(600, 1, 1, 0, 33, _F, 33, (("open_end", True),), 44, 33, "FF in finish()"),      # (d)
    "row300-open-carry": Case(300, 1, 1, 0, 20, _T, 17, (("open_end", True),), 1, 24, "carry in finish()"),   # (d)
    "row300-open-ff":  Case(300, 1, 1, 0, 17, _F, 17, (("open_end", True),), 3, 34, "FF in finish()"),       # (d)
    "row600-first0":   Case(600, 1, 1, 0, 24, _T, 2, (("prefix", 0), ("first", 1)), 2, 24, "carry"),   # (e) held byte = byte 0
    "row600-first1":   Case(600, 1, 1, 0, 24, _T, 2, (("prefix", 1), ("first", 1)), 0, 24, "carry"),   # (e) held byte = byte 1
    "row600-ends15":   Case(600, 1, 1, 0, 20, _T, 17, (("ends", 15),), 44, 20, "carry"),        # (g)
    "row600-ends0":    Case(600, 1, 1, 0, 20, _T, 17, (("ends", 0),), 13, 19, "carry"),         # (g)
    "row600-ends1":    Case(600, 1, 1, 0, 20, _T, 17, (("ends", 1),), 7, 19, "carry"),          # (g)
    # 64x16 tiles, the run behind row 6
    "64x16-carry17":   Case(64, 16, 1, 6, 17, _T, 17, (), 23, 17, "carry"),                     # (a)
    "64x16-carry33":   Case(64, 16, 1, 6, 33, _T, 33, (), 27, 33, "carry"),                     # (b)
    "64x16-ff33":      Case(64, 16, 1, 6, 33, _F, 33, (), 1, 33, "FF"),                         # (c)
    "64x16-ff64":      Case(64, 16, 1, 6, 64, _F, 64, (), 15, 64, "FF"),
    "64x16-first0":    Case(64, 16, 1, 0, 24, _T, 2, (("prefix", 0), ("first", 1)), 4, 23, "carry"),   # (e)
    "64x16-first1":    Case(64, 16, 1, 0, 24, _T, 2, (("prefix", 1), ("first", 1)), 0, 24, "carry"),   # (e)
    "64x16-ends15":    Case(64, 16, 1, 6, 20, _T, 17, (("ends", 15),), 62, 20, "carry"),        # (g)
    "64x16-ends0":     Case(64, 16, 1, 6, 20, _T, 17, (("ends", 0),), 53, 20, "carry"),         # (g)
    "64x16-ends1":     Case(64, 16, 1, 6, 18, _T, 17, (("ends", 1),), 17, 18, "carry"),         # (g)
    # 64x64 tiles (4096 samples: the largest that one launch codes), the run behind row 30
    "64x64-carry17":   Case(64, 64, 1, 30, 17, _T, 17, (), 0, 17, "carry"),                     # (a)
    "64x64-carry33":   Case(64, 64, 1, 30, 33, _T, 33, (), 2, 33, "carry"),                     # (b)
    "64x64-ff33":      Case(64, 64, 1, 30, 33, _F, 33, (), 19, 33, "FF"),                       # (c)
    "64x64-carry64":   Case(64, 64, 1, 30, 64, _T, 64, (), 7, 64, "carry"),
    "64x64-ff64":      Case(64, 64, 1, 30, 64, _F, 64, (), 7, 64, "FF"),
    # 6144 samples, two launches of the segmented coder: the run opens in the first and goes out in the second       (f)
    "128x48-seg-carry": Case(128, 48, 1, 32, 40, _T, 17, (("crosses", SEG),), 25, 39, "carry"),
    "128x48-seg-ff":   Case(128, 48, 1, 32, 40, _F, 17, (("crosses", SEG),), 3, 39, "FF"),
    "128x48-seg-carry33": Case(128, 48, 1, 32, 64, _T, 33, (("crosses", SEG),), 6, 54, "carry"),
    "96x64-seg-carry": Case(96, 64, 1, 42, 40, _T, 17, (("crosses", SEG),), 0, 40, "carry"),
    "96x64-seg-ff":    Case(96, 64, 1, 42, 40, _F, 17, (("crosses", SEG),), 3, 40, "FF"),
    "96x64-seg-carry33": Case(96, 64, 1, 42, 64, _T, 33, (("crosses", SEG),), 5, 49, "carry"),
    # interleaved colour: all channels in one stream, legal where the colour transform gives the decoded samples back
    "il3-64x16-carry": Case(64, 16, 3, 6, 17, _T, 17, (), 19, 38, "carry"),
    "il3-64x16-ff":    Case(64, 16, 3, 6, 17, _F, 17, (), 4, 17, "FF"),
    "il3-200x1-carry": Case(200, 1, 3, 0, 17, _T, 17, (), 12, 17, "carry"),
    "il5-40x16-carry": Case(40, 16, 5, 6, 17, _T, 17, (), 20, 27, "carry"),
    "il5-120x1-carry": Case(120, 1, 5, 0, 17, _T, 17, (), 27, 17, "carry"),
    "il5-120x1-ff":    Case(120, 1, 5, 0, 17, _F, 17, (), 39, 17, "FF"),
}


def build(orc, name):
    """the crafted tile of a row of CASES (searched afresh from the budget; cached per process) -> Crafted, or None when no seed of the
    budget qualifies"""
    if name not in _built:
        c = CASES[name]
        base = natural(orc, c.w, c.h, c.nch)
        cond = dict(c.cond)
        open_end = cond.pop("open_end", False)
        first_bytes = cond.pop("prefix", None)
        if open_end:
            make = lambda seed: craft_open_end(orc, c.w, c.n, c.carry, seed)  # noqa: E731
        else:
            make = lambda seed: craft_tile(orc, base, c.rows_before, c.n, c.carry, seed, first=first_bytes)  # noqa: E731
        _built[name] = search(make, run_of(c.min_run, c.carry, in_finish=open_end, **cond))
    return _built[name]


_built = {}


def how_of(e):
    return ("carry" if e.carried else "FF") + (" in finish()" if e.in_finish else "")


# ---- mosaics: slices are independent, so an image is a grid of tiles ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nat(c):
    from llcomp_amd.synth import gen_nat

    return gen_nat(1024, 256, c)


def pixels(orc, tile, c):
    """a tile of samples as (h, w, c) pixels: one plane -> grey (r = g = b = v, alpha = v: the Y plane and the alpha plane are v, both
    chroma planes zero, so a planar container codes the tile's stream in them); interleaved colour samples -> the inverse transform"""
    if tile.shape[2] == 1:
        return np.repeat(tile.astype(np.uint8), c, axis=2)
    assert tile.shape[2] == c
    return orc.inverse_rct(tile)


def filler(w, h, c, i):
    """pixels of an ordinary tile, another one for every i: a photo-like crop, every fourth one noise (neighbours that renormalise at
    other samples than the crafted lanes)"""
    if i % 4 == 3:
        return np.random.default_rng(1000 + i).integers(0, 256, size=(h, w, c), dtype=np.uint8)
    x0, y0 = (37 * i) % (1024 - w), (11 * i) % (256 - h)
    return _nat(3)[y0:y0 + h, x0:x0 + w, 1:2] if c == 1 else _nat(c)[y0:y0 + h, x0:x0 + w]


def grid_image(orc, cols, rows, tw, th, crafted, c=1, edge_w=0, edge_h=0):
    """(H, W, c) image of cols x rows tiles of tw x th, plus a last column edge_w wide and a last row edge_h high where those are set;
    `crafted`: {tile index (row-major over the whole grid): case name}, the case's tile must have its slot's size; ordinary tiles elsewhere.
    One-plane cases give grey pixels of c channels, interleaved ones need c == their channel count."""
    ncols, nrows = cols + (edge_w > 0), rows + (edge_h > 0)
    lines = []
    for r in range(nrows):
        line = []
        for q in range(ncols):
            w, h, i = tw if q < cols else edge_w, th if r < rows else edge_h, r * ncols + q
            if i in crafted:
                t = build(orc, crafted[i]).tile
                assert t.shape[:2] == (h, w), (crafted[i], i, w, h)
                line.append(pixels(orc, t, c))
            else:
                f = filler(w, h, 1 if CASES[next(iter(crafted.values()))].nch == 1 else c, i)
                line.append(np.repeat(f, c, axis=2) if f.shape[2] == 1 and c > 1 else f)
        lines.append(np.concatenate(line, axis=1))
    return np.ascontiguousarray(np.concatenate(lines, axis=0))


def names(prefix):
    return sorted(n for n in CASES if n.startswith(prefix))


# The mosaics of the GPU tests, by placement: 1 = crafted tiles at chosen slices among ordinary ones (with 64 slices per wavefront: lane 0,
# a middle lane, lane 63, and the last, partial lane group); 2 = every tile the same crafted tile (all lanes of a wavefront carry at the
# same sample); 3 = the family's cases in turn (lanes carry at different samples while their neighbours renormalise).
# -> (image, tile_w, tile_h, {slice of a one-plane container: case})
def rows_mosaic(orc, placement, c=1):
    """one-row tiles: two columns 600 wide and a ragged one of 300; 70 rows (210 tiles) for placements 1 and 3, 100 rows of 2 for 2"""
    w6, w3 = names("row600-"), names("row300-")
    if placement == 2:
        at = {i: "row600-carry33" for i in range(200)}
        return grid_image(orc, 2, 100, 600, 1, at, c), 600, 1, at
    if placement == 1:
        slots6 = [0, 63, 31, 193] + [3 * r + (r & 1) for r in range(2, 60, 5)]
        slots3 = [3 * r + 2 for r in (1, 11, 21, 40, 69, 50, 33)]
    else:
        slots6 = [i for i in range(210) if i % 3 != 2]
        slots3 = [i for i in range(210) if i % 3 == 2]
    at = {s: w6[j % len(w6)] for j, s in enumerate(slots6)}
    at.update({s: w3[j % len(w3)] for j, s in enumerate(slots3)})
    return grid_image(orc, 2, 70, 600, 1, at, c, edge_w=300), 600, 1, at


def tiles_mosaic(orc, tw, th, placement, c=1, prefix=None):
    """8 columns of 2-D tiles, 26 rows of them (208 tiles; 25 rows = 200 tiles for 64 rows high ones)"""
    pool = names(prefix or "%dx%d-" % (tw, th))
    n = 8 * (25 if th >= 64 else 26)
    if placement == 2:
        at = {i: pool[1] for i in range(n)}
    elif placement == 1:
        slots = [0, 63, 31, n - 3] + list(range(70, n - 8, 13))
        at = {s: pool[j % len(pool)] for j, s in enumerate(slots)}
    else:
        at = {i: pool[i % len(pool)] for i in range(n)}
    return grid_image(orc, 8, n // 8, tw, th, at, c), tw, th, at


def segmented_mosaic(orc, tw, th, placement):
    """tiles of 6144 samples (two launches of the segmented coder), 4 columns and 8 rows of them, with a ragged column 40 wide and a ragged
    row 20 high: those tiles end in the first launch while their neighbours go on"""
    pool = names("%dx%d-seg-" % (tw, th))
    full = [r * 5 + q for r in range(8) for q in range(4)]
    at = {s: pool[(0 if placement == 2 else j // 3 if placement == 1 else j) % len(pool)] for j, s in enumerate(full) if placement != 1 or j % 3 == 0}
    return grid_image(orc, 4, 8, tw, th, at, 1, edge_w=40, edge_h=20), tw, th, at
