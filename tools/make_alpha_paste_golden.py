#!/usr/bin/env python3
"""Writes tests/golden/alpha_paste_pil.json from PIL: a few hundred recorded results of Image.paste with an L mask and of
Image.alpha_composite, for the machines where tests/test_alpha_paste_rule.py cannot import PIL.

    python tools/make_alpha_paste_golden.py

"paste": rows of [m, d, s, out]; "over": rows of [src R, G, B, A, dst R, G, B, A, out R, G, B, A]."""
import json
import os

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    rng = np.random.default_rng(1234)
    ends = np.array([0, 1, 127, 128, 254, 255], np.uint8)
    m, d, s = (a.reshape(-1) for a in np.meshgrid(ends, ends, ends, indexing="ij"))
    more = rng.integers(0, 256, (3, 184), dtype=np.uint8)
    m, d, s = np.concatenate([m, more[0]]), np.concatenate([d, more[1]]), np.concatenate([s, more[2]])
    bg = Image.fromarray(d[None, :], "L")
    bg.paste(Image.fromarray(s[None, :], "L"), (0, 0), Image.fromarray(m[None, :], "L"))
    paste = np.stack([m, d, s, np.asarray(bg)[0]], axis=1)
    alphas = np.array([0, 1, 128, 254, 255], np.uint8)
    sa, da = (a.reshape(-1) for a in np.meshgrid(alphas, alphas, indexing="ij"))
    n = 300
    src, dst = rng.integers(0, 256, (n, 4), dtype=np.uint8), rng.integers(0, 256, (n, 4), dtype=np.uint8)
    src[:25, 3], dst[:25, 3] = sa, da
    src[25:50, :3], dst[25:50, :3] = rng.choice(np.array([0, 255], np.uint8), (25, 3)), rng.choice(np.array([0, 255], np.uint8), (25, 3))
    out = np.asarray(Image.alpha_composite(Image.fromarray(dst[None], "RGBA"), Image.fromarray(src[None], "RGBA")))[0]
    over = np.concatenate([src, dst, out], axis=1)
    path = os.path.join(ROOT, "tests", "golden", "alpha_paste_pil.json")
    with open(path, "w") as f:
        json.dump({"pil": Image.__version__, "paste": paste.tolist(), "over": over.tolist()}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{path}: {len(paste)} paste rows, {len(over)} over rows")


if __name__ == "__main__":
    main()
