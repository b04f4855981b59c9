"""The spec of the batch orientation (include/llcomp_mi.h: "Batch orientation") in numpy alone: np.flip, np.rot90 and a transposition of
the sample seen as [c, h, w] or [h, w, c].  It calls nothing of the library.  A code is 0 for none, otherwise PIL's Image.Transpose value
plus 1; np.rot90 turns counter-clockwise, as PIL's ROTATE_90 does."""
import numpy as np

from batch_support import bits_of, gen_batch  # noqa: F401  (the tests take them from here)

NAMES = ("none", "flip_left_right", "flip_top_bottom", "rotate_90", "rotate_180", "rotate_270", "transpose", "transverse")
TRANSPOSING = (3, 5, 6, 7)


def orient_sample(a, code, layout):
    """one sample [c, h, w] ("chw") or [h, w, c] ("hwc") under the code -> a new array"""
    ay, ax = (1, 2) if layout == "chw" else (0, 1)
    if code == 0:
        out = a
    elif code == 1:
        out = np.flip(a, ax)
    elif code == 2:
        out = np.flip(a, ay)
    elif code == 3:
        out = np.rot90(a, 1, (ay, ax))
    elif code == 4:
        out = np.rot90(a, 2, (ay, ax))
    elif code == 5:
        out = np.rot90(a, 3, (ay, ax))
    elif code == 6:
        out = np.swapaxes(a, ay, ax)
    elif code == 7:
        out = np.flip(np.flip(np.swapaxes(a, ay, ax), ay), ax)  # (the transposition about the other diagonal)
    else:
        raise ValueError(code)
    return np.ascontiguousarray(out)


def apply(batch, codes, layout):
    """the batch [n, c, h, w] or [n, h, w, c] with sample i under codes[i] -> a new batch of the same shape (the transposing codes
    take square samples)"""
    out = np.empty_like(batch)
    for i, code in enumerate(codes):
        out[i] = orient_sample(batch[i], int(code), layout)
    return out
