"""The spec of the batch composition (include/llcomp_mi.h: "Batch composition") in numpy alone: slice assignments in list order, which
is painter's order.  It calls nothing of the library.  The fill value is torch.tensor(value).to(dtype) on the CPU; batches are drawn
from random BITS, so NaNs with payloads, infinities, negative zeros and subnormals occur.  The same file writes out the expressions of
torchvision.utils.make_grid and of the mosaic placement of Ultralytics' load_mosaic, for the two helpers.  A piece is a tuple
(dst, src, dx, dy, sx, sy, w, h[, flags]); flags 1: a FILL piece."""
import math

import numpy as np

from batch_support import bits_of, gen_batch  # noqa: F401  (the tests take them from here)

FILL = 1


def fill_bits(value, c, dtype):
    """c fill values (one value: for every channel; None: zeros) as the dtype's elements, converted as torch converts them on the CPU"""
    import torch

    t = {"uint8": torch.uint8, "float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}[dtype]
    v = [0.0] * c if value is None else [float(x) for x in np.broadcast_to(np.asarray(value, np.float64).reshape(-1), (c,))]
    out = torch.tensor(v, dtype=torch.float32).to(t)
    if dtype == "bfloat16":
        return out.view(torch.int16).numpy().view(np.uint16)
    return out.numpy()


def apply(src, dst, pieces, layout, dtype, fill=None, keep=False):
    """src [n_src, c, ih, iw] / [n_src, ih, iw, c] or None, dst the same way -> the composed dst, a new array"""
    c = dst.shape[1] if layout == "chw" else dst.shape[3]
    fv = fill_bits(fill, c, dtype).astype(dst.dtype) if dtype != "bfloat16" else fill_bits(fill, c, dtype)
    fv_b = fv.reshape(c, 1, 1) if layout == "chw" else fv.reshape(1, 1, c)
    if keep:
        out = dst.copy()
    else:
        out = np.empty_like(dst)
        for d in range(len(out)):
            out[d] = np.broadcast_to(fv_b, out[d].shape)
    for p in pieces:
        d, s, dx, dy, sx, sy, w, h = (int(v) for v in p[:8])
        flags = int(p[8]) if len(p) > 8 else 0
        if layout == "chw":
            out[d, :, dy:dy + h, dx:dx + w] = fv_b if flags & FILL else src[s, :, sy:sy + h, sx:sx + w]
        else:
            out[d, dy:dy + h, dx:dx + w, :] = fv_b if flags & FILL else src[s, sy:sy + h, sx:sx + w, :]
    return out


def random_pieces(rng, n_src, iw, ih, n_dst, ow, oh, n):
    """n drawn pieces: they overlap and hide each other, some are empty, some FILL (all of them without a src)"""
    out = []
    for _ in range(n):
        fill = n_src == 0 or rng.integers(4) == 0
        mw, mh = (ow, oh) if fill else (min(iw, ow), min(ih, oh))
        w = 0 if rng.integers(8) == 0 else int(rng.integers(1, mw + 1))
        h = 0 if rng.integers(8) == 0 else int(rng.integers(1, mh + 1))
        dx, dy = int(rng.integers(0, ow - w + 1)), int(rng.integers(0, oh - h + 1))
        if fill:
            out.append((int(rng.integers(n_dst)), 0, dx, dy, 0, 0, w, h, FILL))
        else:
            out.append((int(rng.integers(n_dst)), int(rng.integers(n_src)), dx, dy, int(rng.integers(0, iw - w + 1)), int(rng.integers(0, ih - h + 1)), w, h, 0))
    return out


def make_grid(batch, nrow=8, padding=2, pad_value=0.0):
    """torchvision.utils.make_grid's expressions on a [n, c, h, w] array -> [c, H, W]"""
    nmaps = batch.shape[0]
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    height, width = int(batch.shape[2] + padding), int(batch.shape[3] + padding)
    grid = np.full((batch.shape[1], height * ymaps + padding, width * xmaps + padding), pad_value, batch.dtype)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid[:, y * height + padding:y * height + height, x * width + padding:x * width + width] = batch[k]
            k += 1
    return grid


def mosaic(imgs, xc, yc, s, fill=114):
    """load_mosaic's placement of four [h, w, c] pictures on a canvas of 2s x 2s around (xc, yc) -> [2s, 2s, c]"""
    img4 = np.full((s * 2, s * 2, imgs[0].shape[2]), fill, dtype=imgs[0].dtype)
    for i, img in enumerate(imgs):
        h, w = img.shape[:2]
        if i == 0:  # top left
            x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
            x1b, y1b, x2b, y2b = w - (x2a - x1a), h - (y2a - y1a), w, h
        elif i == 1:  # top right
            x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, s * 2), yc
            x1b, y1b, x2b, y2b = 0, h - (y2a - y1a), min(w, x2a - x1a), h
        elif i == 2:  # bottom left
            x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(s * 2, yc + h)
            x1b, y1b, x2b, y2b = w - (x2a - x1a), 0, w, min(y2a - y1a, h)
        else:  # bottom right
            x1a, y1a, x2a, y2a = xc, yc, min(xc + w, s * 2), min(s * 2, yc + h)
            x1b, y1b, x2b, y2b = 0, 0, min(w, x2a - x1a), min(y2a - y1a, h)
        img4[y1a:y2a, x1a:x2a] = img[y1b:y2b, x1b:x2b]
    return img4
