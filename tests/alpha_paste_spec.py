"""The batch alpha paste (include/llcomp_mi.h "Batch alpha paste") stated in numpy: both rules on arrays of bit patterns, generators of
batches, mattes and pieces, and apply(), which runs a call's pieces in order.  It calls nothing of the library.

Batches are the numpy arrays the library takes: uint8, float16, float32, and uint16 holding bfloat16 bits for "bfloat16"."""
import numpy as np

ALPHA_VALUE, ALPHA_VALUE_PIXEL, ALPHA_OVER = 1, 2, 4
NP_NAME = {"uint8": np.uint8, "float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}
BITS = {1: np.uint8, 2: np.uint16, 4: np.uint32}
QNAN = {"float32": 0x7FC00000, "float16": 0x7E00, "bfloat16": 0x7FC0}
WEIGHTS = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)


def widen(bits, dtype):
    """bit patterns of the dtype -> float32 values (exact)"""
    bits = np.asarray(bits)
    if dtype == "float32":
        return bits.astype(np.uint32).view(np.float32)
    if dtype == "float16":
        return bits.astype(np.uint16).view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def narrow(f, dtype):
    """float32 values -> bit patterns of the dtype as uint32: round to nearest even, a NaN the dtype's one quiet NaN"""
    f = np.asarray(f, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        if dtype == "float32":
            out = f.view(np.uint32).copy()
        elif dtype == "float16":
            out = f.astype(np.float16).view(np.uint16).astype(np.uint32)
        else:
            x = f.view(np.uint32).astype(np.uint64)
            out = ((x + 0x7FFF + ((x >> 16) & 1)) >> 16).astype(np.uint32) & 0xFFFF
    return np.where(np.isnan(f), np.uint32(QNAN[dtype]), out)


def paste_rule(d, s, m, dtype):
    """THE PASTE rule on arrays of bit patterns d and s (any unsigned type) and alpha bytes m, broadcast -> bit patterns as uint32"""
    d, s, m = np.broadcast_arrays(np.asarray(d).astype(np.uint32), np.asarray(s).astype(np.uint32), np.asarray(m).astype(np.uint32))
    if dtype == "uint8":
        t = d * (255 - m) + s * m + 128
        mid = ((t >> 8) + t) >> 8
    else:
        a = WEIGHTS[m]
        with np.errstate(all="ignore"):
            pd = (widen(d, dtype) * (np.float32(1.0) - a)).astype(np.float32)
            ps = (widen(s, dtype) * a).astype(np.float32)
            mid = narrow((pd + ps).astype(np.float32), dtype)
    return np.where(m == 0, d, np.where(m == 255, s, mid)).astype(np.uint32)


def over_rule(d, s):
    """THE OVER rule on uint8 arrays [..., 4] (R, G, B, A) -> uint8 [..., 4]"""
    d, s = np.broadcast_arrays(np.asarray(d, np.uint8), np.asarray(s, np.uint8))
    d32, s32 = d.astype(np.uint32), s.astype(np.uint32)
    sa, da = s32[..., 3], d32[..., 3]
    outa255 = sa * 255 + da * (255 - sa)
    coef1 = sa * 255 * 255 * 128 // np.maximum(outa255, 1)
    coef2 = 255 * 128 - coef1
    out = np.empty(d.shape, np.uint32)
    for ch in range(3):
        t = s32[..., ch] * coef1 + d32[..., ch] * coef2 + (0x80 << 7)
        out[..., ch] = (((t >> 8) + t) >> 8) >> 7
    t = outa255 + 0x80
    out[..., 3] = ((t >> 8) + t) >> 8
    return np.where((sa == 0)[..., None], d32, out).astype(np.uint8)


def _pixels(batch, layout):
    """a view [n, h, w, c] of the batch's bit patterns"""
    b = batch.view(BITS[batch.itemsize])
    return b if layout == "hwc" else np.moveaxis(b, 1, 3)


def alpha_plane(alpha, alpha_byte=0):
    """alpha [n, h, w] or [n, h, w, px_bytes] uint8 -> the pixels' alpha bytes [n, h, w]"""
    return alpha if alpha.ndim == 3 else alpha[..., alpha_byte]


def apply(src, alpha, dst, pieces, dtype, layout, alpha_byte=0):
    """dst with the pieces (dst, src, dx, dy, sx, sy, w, h[, flags[, value_bits]]) applied in order, a new array"""
    out = np.ascontiguousarray(dst).copy()
    o = _pixels(out, layout)
    s = None if src is None else _pixels(np.ascontiguousarray(src), layout)
    c = o.shape[3]
    for p in pieces:
        p = tuple(p) + (0,) * (10 - len(p))
        di, si, dx, dy, sx, sy, w, h, flags, value = (int(v) for v in p)
        if not w or not h:
            continue
        box = o[di, dy:dy + h, dx:dx + w, :]
        if flags & ALPHA_OVER:
            box[...] = over_rule(box, s[si, sy:sy + h, sx:sx + w, :])
            continue
        if flags & ALPHA_VALUE_PIXEL:
            sv = np.array([(value >> (8 * ch)) & 0xFF for ch in range(c)], np.uint32)[None, None, :]
        elif flags & ALPHA_VALUE:
            sv = np.uint32(value)
        else:
            sv = s[si, sy:sy + h, sx:sx + w, :]
        m = alpha_plane(alpha, alpha_byte)[si, sy:sy + h, sx:sx + w, None]
        box[...] = paste_rule(box, sv, m, dtype).astype(box.dtype)
    return out


def gen_matte(rng, n, h, w, px_bytes=1, alpha_byte=0):
    """a soft matte: runs of 0 and of 255 with ramps and noise between them, every byte value somewhere in a large one; the other bytes
    of a pixel are noise"""
    a = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    kind = rng.integers(0, 4, (n, h, w))
    a[kind == 0] = 0
    a[kind == 1] = 255
    if px_bytes == 1:
        return a
    full = rng.integers(0, 256, (n, h, w, px_bytes), dtype=np.uint8)
    full[..., alpha_byte] = a
    return full


def gen_pieces(rng, n_pieces, n_src, iw, ih, n_dst, ow, oh, dtype, layout, c, over=False):
    """drawn pieces that overlap: soft ones from src, VALUE ones, VALUE_PIXEL ones where the shape takes them, OVER ones where asked"""
    es = np.dtype(NP_NAME[dtype]).itemsize
    out = []
    for _ in range(n_pieces):
        w, h = int(rng.integers(1, min(iw, ow) + 1)), int(rng.integers(1, min(ih, oh) + 1))
        rec = [int(rng.integers(0, n_dst)), int(rng.integers(0, n_src)), int(rng.integers(0, ow - w + 1)), int(rng.integers(0, oh - h + 1)),
               int(rng.integers(0, iw - w + 1)), int(rng.integers(0, ih - h + 1)), w, h]
        kind = int(rng.integers(0, 6))
        if over and kind < 3:
            rec += [ALPHA_OVER, 0]
        elif kind == 4:
            rec += [ALPHA_VALUE, int(rng.integers(0, 1 << (8 * es)))]
        elif kind == 5 and dtype == "uint8" and layout == "hwc" and c <= 4:
            rec += [ALPHA_VALUE | ALPHA_VALUE_PIXEL, int(rng.integers(0, 1 << (8 * c)))]
        else:
            rec += [0, 0]
        out.append(tuple(rec))
    return out
