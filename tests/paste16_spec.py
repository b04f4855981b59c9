"""The spec of the batch copy-paste by 16-bit ids (include/llcomp_mi.h: "Batch copy-paste by 16-bit ids") in numpy alone, as
paste_spec.py: for every piece in list order, which is painter's order, out = np.where(sel, piece, out) with, on the uint16 mask m,
sel = ((m - base) & 0xFFFFFFFF < 256) & lut[(m - base) & 255] for a window of 256 id bits from base on.  It calls nothing of the
library.  A piece is a tuple (dst, src, dx, dy, sx, sy, w, h, ids[, value_bits]); ids: ints 0..65535 (the WHOLE set, however wide: the
union of its windows), "nonzero", or Window(base, lut) for one window as the C struct has it.  value_bits are the element's bits."""
from collections import namedtuple

import numpy as np

from batch_support import BITS, bits_of, gen_batch  # noqa: F401  (the tests take them from here)

Window = namedtuple("Window", "base lut")  # lut: 256 bools, bit j for id base + j


def select(m, ids):
    """the pixels of the uint16 array m that the ids select"""
    if isinstance(ids, Window):
        d = (m.astype(np.int64) - int(ids.base)) & 0xFFFFFFFF
        return (d < 256) & np.asarray(ids.lut, bool)[d & 255]
    if isinstance(ids, str):
        assert ids == "nonzero"
        return m != 0
    sel = np.zeros(m.shape, bool)
    for base in range(0, 65536, 256):  # the union of the set's windows
        lut = np.zeros(256, bool)
        inside = [int(v) - base for v in ids if base <= int(v) < base + 256]
        if inside:
            lut[inside] = True
            sel |= select(m, Window(base, lut))
    return sel


def apply(src, mask, dst, pieces, layout):
    """src [n_src, c, ih, iw] / [n_src, ih, iw, c], mask [n_src, ih, iw] uint16, dst as src -> the pasted dst, a new array"""
    assert mask.dtype == np.uint16
    out = np.ascontiguousarray(dst).copy()
    ob, sb = out.view(BITS[out.itemsize]), np.ascontiguousarray(src).view(BITS[out.itemsize])
    for p in pieces:
        d, s, dx, dy, sx, sy, w, h = (int(v) for v in p[:8])
        sel = select(mask[s, sy:sy + h, sx:sx + w], p[8])
        value = None
        if len(p) > 9 and p[9] is not None:
            value = BITS[out.itemsize](int(p[9]))
        if layout == "chw":
            piece = value if value is not None else sb[s, :, sy:sy + h, sx:sx + w]
            ob[d][:, dy:dy + h, dx:dx + w] = np.where(sel, piece, ob[d][:, dy:dy + h, dx:dx + w])
        else:
            piece = value if value is not None else sb[s, sy:sy + h, sx:sx + w, :]
            ob[d][dy:dy + h, dx:dx + w, :] = np.where(sel[..., None], piece, ob[d][dy:dy + h, dx:dx + w, :])
    return out


HIGH_BYTE = (0x0001, 0x0101, 0x0201, 0xFF01, 0x0002, 0x0102, 0x0000, 0xFF00)  # ids that share low bytes and differ in the high byte


def gen_mask(rng, n, ih, iw, pool=HIGH_BYTE):
    """id maps with ids uniform in the pool"""
    return np.asarray(pool, np.uint16)[rng.integers(0, len(pool), size=(n, ih, iw))]


def random_pieces(rng, n_src, iw, ih, n_dst, ow, oh, n, esize, pool=HIGH_BYTE):
    """n drawn pieces: they overlap and hide each other, some are empty, some VALUE; each selects a drawn half of the pool"""
    out = []
    for _ in range(n):
        mw, mh = min(iw, ow), min(ih, oh)
        w = 0 if rng.integers(8) == 0 else int(rng.integers(1, mw + 1))
        h = 0 if rng.integers(8) == 0 else int(rng.integers(1, mh + 1))
        dx, dy = int(rng.integers(0, ow - w + 1)), int(rng.integers(0, oh - h + 1))
        chosen = sorted(int(m) for m in rng.choice(pool, len(pool) // 2, replace=False))
        p = (int(rng.integers(n_dst)), int(rng.integers(n_src)), dx, dy, int(rng.integers(0, iw - w + 1)), int(rng.integers(0, ih - h + 1)), w, h, chosen)
        if rng.integers(4) == 0:
            p += (int(rng.integers(0, 1 << (8 * esize), dtype=np.uint64)),)
        out.append(p)
    return out

