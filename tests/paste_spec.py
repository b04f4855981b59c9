"""The spec of the batch copy-paste (include/llcomp_mi.h: "Batch copy-paste") in numpy alone: for every piece in list order, which is
painter's order, sel = lut[mask[s, sy:sy+h, sx:sx+w]] and out[d][..., ys, xs] = np.where(sel, piece, out[d][..., ys, xs]).  It calls
nothing of the library.  A VALUE piece's value is torch.tensor(value).to(dtype) on the CPU; batches are drawn from random BITS, so NaNs
with payloads, infinities, negative zeros and subnormals occur, and the spec moves bit patterns.  A piece is a tuple
(dst, src, dx, dy, sx, sy, w, h, ids[, value]); ids: ints 0..255 or "nonzero"."""
import numpy as np

from batch_support import BITS, bits_of, gen_batch  # noqa: F401  (the tests take them from here)
from compose_spec import fill_bits


def lut_of(ids):
    lut = np.zeros(256, bool)
    if isinstance(ids, str):
        assert ids == "nonzero"
        lut[1:] = True
    else:
        lut[[int(m) for m in ids]] = True
    return lut


def apply(src, mask, dst, pieces, layout, dtype, stats=None):
    """src [n_src, c, ih, iw] / [n_src, ih, iw, c], mask [n_src, ih, iw] uint8, dst as src -> the pasted dst, a new array.  stats: a
    list that gets (covered pixels, selected pixels) summed over the pieces"""
    out = np.ascontiguousarray(dst).copy()
    ob, sb = out.view(BITS[out.itemsize]), np.ascontiguousarray(src).view(BITS[out.itemsize])
    covered = selected = 0
    for p in pieces:
        d, s, dx, dy, sx, sy, w, h = (int(v) for v in p[:8])
        sel = lut_of(p[8])[mask[s, sy:sy + h, sx:sx + w]]
        covered, selected = covered + sel.size, selected + int(sel.sum())
        value = None
        if len(p) > 9 and p[9] is not None:
            value = fill_bits(p[9], 1, dtype).view(BITS[out.itemsize])[0]
        if layout == "chw":
            piece = value if value is not None else sb[s, :, sy:sy + h, sx:sx + w]
            ob[d][:, dy:dy + h, dx:dx + w] = np.where(sel, piece, ob[d][:, dy:dy + h, dx:dx + w])
        else:
            piece = value if value is not None else sb[s, sy:sy + h, sx:sx + w, :]
            ob[d][dy:dy + h, dx:dx + w, :] = np.where(sel[..., None], piece, ob[d][dy:dy + h, dx:dx + w, :])
    if stats is not None:
        stats.append((covered, selected))
    return out


def gen_mask(rng, n, ih, iw, ids=8):
    """id maps with bytes uniform in 0..ids-1"""
    return rng.integers(0, ids, size=(n, ih, iw), dtype=np.uint8)


def random_pieces(rng, n_src, iw, ih, n_dst, ow, oh, n, dtype, ids=8):
    """n drawn pieces: they overlap and hide each other, some are empty, some VALUE; each selects a drawn half of the ids"""
    out = []
    for _ in range(n):
        mw, mh = min(iw, ow), min(ih, oh)
        w = 0 if rng.integers(8) == 0 else int(rng.integers(1, mw + 1))
        h = 0 if rng.integers(8) == 0 else int(rng.integers(1, mh + 1))
        dx, dy = int(rng.integers(0, ow - w + 1)), int(rng.integers(0, oh - h + 1))
        chosen = sorted(int(m) for m in rng.choice(ids, ids // 2, replace=False))
        p = (int(rng.integers(n_dst)), int(rng.integers(n_src)), dx, dy, int(rng.integers(0, iw - w + 1)), int(rng.integers(0, ih - h + 1)), w, h, chosen)
        if rng.integers(4) == 0:
            p += (float(rng.integers(0, 256)) if dtype == "uint8" else float(rng.integers(-4000, 4000)) / 7.0,)
        out.append(p)
    return out
