"""What the batch mixing has to give, bit for bit (include/llcomp_mi.h: "Batch mixing"): torchvision's and timm's own torch expressions for
RandomErasing, MixUp and CutMix, run by torch on the CPU.  torchvision and timm are not needed: the expressions are written out here,
each under the line of the library it comes from.  Nothing of llcomp_mi_mix_reference or of the kernels is in this file.

A batch is a CPU tensor [n, c, h, w] of uint8, float32, float16 or bfloat16 (a [n, h, w, c] batch is this one permuted: every
expression is per element).  The one thing here that is no library's line: a sample that is its own partner (the middle sample of a
flip of odd n, every sample without a partner) is not mixed at all, where timm would blend it with itself."""
import numpy as np
import torch

DTYPES = {"uint8": torch.uint8, "float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
_INT_VIEW = {torch.uint8: torch.uint8, torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
_NP_BITS = {torch.uint8: np.uint8, torch.float32: np.uint32, torch.float16: np.uint16, torch.bfloat16: np.uint16}


def bits(t):
    """the elements' bit patterns as an unsigned numpy array of the tensor's shape"""
    t = t.contiguous()
    return t.view(_INT_VIEW[t.dtype]).numpy().view(_NP_BITS[t.dtype]).copy()


def from_bits(a, dtype):
    """a tensor of `dtype` (a name or a torch dtype) with these bit patterns"""
    dtype = DTYPES.get(dtype, dtype)
    a = np.ascontiguousarray(a, dtype=_NP_BITS[dtype])
    return torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32}[a.itemsize]).copy()).view(dtype)


def partners(n, partner):
    """None / "roll" / "flip" / indices -> the partner of every sample"""
    if partner is None:
        return list(range(n))
    if isinstance(partner, str):
        return {"roll": [(i - 1) % n for i in range(n)], "flip": [n - 1 - i for i in range(n)]}[partner]
    return [int(p) for p in partner]


def _per_sample(v, n):
    if v is None:
        return [None] * n
    if isinstance(v, (int, float)) or (len(v) == 4 and all(isinstance(q, int) for q in v)):
        return [v] * n
    assert len(v) == n
    return list(v)


def random_erasing(x, rects, value):
    """torchvision.transforms.v2.functional.erase, per sample ahead of the collate:
        img[..., i : i + h, j : j + w] = v        with v = torch.tensor(value)[:, None, None]"""
    c = x.shape[1]
    value = [0.0] * c if value is None else ([float(value)] * c if isinstance(value, (int, float)) else [float(q) for q in value])
    v = torch.tensor(value)[:, None, None]
    for img, r in zip(x, rects):
        if r is None or not r[2] or not r[3]:
            continue
        j, i, w, h = r
        img[..., i:i + h, j:j + w] = v
    return x


def mixed(x, partner):
    """the batch every sample's partner comes from: torchvision's inpt.roll(1, 0), timm's x.flip(0), or x[perm]"""
    if partner == "roll":
        return x.roll(1, 0)
    if partner == "flip":
        return x.flip(0)
    return x[torch.tensor(partners(len(x), partner), dtype=torch.long)]


def apply(batch, partner=None, lam=None, boxes=None, erase=None, erase_value=None):
    """batch -> the batch after RandomErasing (erase: one rectangle (x, y, w, h), one per sample or None), then per sample CutMix inside
    its box (boxes, the same way) and MixUp outside it (lam: one double or one per sample, None = no blend)"""
    n = len(batch)
    part = partners(n, partner)
    lams, bxs = _per_sample(lam, n), _per_sample(boxes, n)
    x = random_erasing(batch.clone(), _per_sample(erase, n), erase_value)
    rolled = mixed(x, partner)
    if isinstance(lam, float):
        # torchvision MixUp._mixup:       output = inpt.roll(1, 0).mul(1.0 - lam).add_(inpt.mul(lam))
        # timm Mixup._mix_batch:          x_flipped = x.flip(0).mul_(1. - lam); x.mul_(lam).add_(x_flipped)
        out = rolled.mul(1.0 - lam).add_(x.mul(lam)) if partner != "flip" else x.clone().mul_(lam).add_(x.flip(0).mul_(1. - lam))
    else:
        out = x.clone()
        for i in range(n):  # timm Mixup._mix_elem:  x[i] = x[i] * lam + x_orig[j] * (1 - lam)
            if lams[i] is not None:
                out[i] = x[i] * float(lams[i]) + rolled[i] * (1 - float(lams[i]))
    for i in range(n):
        if part[i] == i:
            out[i] = x[i]
            continue
        r = bxs[i]
        if r is None or not r[2] or not r[3]:
            continue
        # torchvision CutMix._mixup:      output[..., y1:y2, x1:x2] = rolled[..., y1:y2, x1:x2]
        # timm Mixup._mix_batch:          x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
        x1, y1, w, h = r
        out[i][..., y1:y1 + h, x1:x1 + w] = rolled[i][..., y1:y1 + h, x1:x1 + w]
    return out


def gen_batch(dtype, n, c, h, w, seed, special=True):
    """A seeded batch [n, c, h, w]: noise as a normalised batch has it, and -- special -- +-0, the largest finite value, subnormals and
    tiny and huge magnitudes sprinkled in (uint8: noise, 0 and 255)"""
    dtype = DTYPES.get(dtype, dtype)
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 256, (n, c, h, w), generator=g, dtype=torch.uint8)
    x = (torch.randn((n, c, h, w), generator=g) * 1.5).to(dtype)
    if special:
        fi = torch.finfo(dtype)
        vals = torch.tensor([0.0, -0.0, fi.max, -fi.max, fi.tiny, -fi.tiny, fi.tiny / 4, -fi.tiny / 8, fi.smallest_normal * 1.5, 1.0, -1.0, fi.max / 2,
                             fi.eps, 3e-5, 6.1e-5, 65504.0], dtype=torch.float64).to(dtype)
        flat = x.view(-1)
        where = torch.randperm(flat.numel(), generator=g)[:max(1, flat.numel() // 3)]
        flat[where] = vals[torch.randint(0, len(vals), (len(where),), generator=g)]
    return x
