"""The torch formulations that the large legs of the calls on id maps of 3 and 4 bytes per pixel compare against
(tests/test_gpu_large_wide_id_maps.py), where a numpy spec on the host would take minutes: ids rebuilt from the bytes of 3-byte
pixels, the INDEX and PLANES targets of a row band (the default, then out[m == id] = value per listed id: there are 2^32 ids, so no
table), one windowed paste piece, and a VALUE_PIXEL piece's bytes.  Each works on the device of the tensors it is given;
tests/test_large_wide_formulations.py checks each against the numpy specs of the small tests on the CPU.  Nothing here touches the
library."""


def ids_of_bytes(b):
    """uint8 [..., 3], a 3-byte pixel's bytes in memory order (little-endian) -> its id, int64 [...]"""
    return b[..., 0].long() | (b[..., 1].long() << 8) | (b[..., 2].long() << 16)


def ids_of_words(w):
    """int32 [...], the 4-byte pixels as torch holds them (signed) -> their ids 0 .. 2^32 - 1, int64 [...]"""
    return w.long() & 0xFFFFFFFF


def ids_of_maps(m, mb):
    """the pixels of a map of mb bytes -- uint8 [..., 3] or int32 [...] -> int64 ids"""
    return ids_of_bytes(m) if mb == 3 else ids_of_words(m)


def value_of(m, listed, values, default):
    """int64 ids m -> the int64 value of every pixel: that of its id in `listed`, or the default"""
    import torch

    v = torch.full(m.shape, int(default), dtype=torch.int64, device=m.device)
    for i, val in zip(listed, values):
        v = torch.where(m == int(i), int(val), v)  # (v[m == i] = val, without the host waiting for the count of the pixels)
    return v


def index_of(m, listed, values, default, tdtype):
    """the INDEX target of the ids m as elements of the torch integer type (the low bits of the value, as a cast keeps them)"""
    return value_of(m, listed, values, default).to(tdtype)


def planes_of(m, listed, values, default, planes, on_bits, off_bits, tdtype):
    """the PLANES target [planes, ...] of the ids m: on_bits where the pixel's value is the plane, off_bits elsewhere, as elements
    of the torch integer type that holds the element's bits"""
    import torch

    v = value_of(m, listed, values, default)
    k = torch.arange(planes, device=m.device).view((planes,) + (1,) * m.dim())
    on, off = torch.tensor(on_bits, dtype=tdtype, device=m.device), torch.tensor(off_bits, dtype=tdtype, device=m.device)
    return torch.where(v[None] == k, on, off)


def window_selects(m, base, lut):
    """int64 ids m against the window of 256 ids from `base` on, lut 256 bools: no id below the base and none at base + 256 or above
    is selected, whatever 32-bit arithmetic would wrap there"""
    import torch

    d = m - int(base)
    bits = torch.as_tensor([bool(x) for x in lut], dtype=torch.bool, device=m.device)
    return (d >= 0) & (d < 256) & bits[d.clamp(0, 255)]


def value_pixel_bytes(value_bits, c):
    """the c bytes a VALUE_PIXEL piece writes into a selected pixel: channel ch takes byte ch of value_bits"""
    return [(int(value_bits) >> (8 * ch)) & 0xFF for ch in range(c)]


def paste_piece32(dv, sv, m, p, window, value=None, pixel=False):
    """a paste piece (dx, dy, sx, sy, w, h) between two HWC samples dv [oh, ow, c] and sv [ih, iw, c] of an integer type, in place on
    dv; m: the int64 ids [ih, iw] of the src sample's map, or of the rows the piece reads when given as (ids, first_row).  The
    selected pixels take the src pixel, the value in every channel (value) or a byte per channel (value and pixel).  -> the number of
    pixels the piece selected"""
    import torch

    dx, dy, sx, sy, w, h = p
    ids, r0 = m if isinstance(m, tuple) else (m, 0)
    sel = window_selects(ids[sy - r0:sy - r0 + h, sx:sx + w], window[0], window[1])
    if value is None:
        piece = sv[sy:sy + h, sx:sx + w]
    elif pixel:
        piece = torch.as_tensor(value_pixel_bytes(value, dv.shape[2]), dtype=dv.dtype, device=dv.device).view(1, 1, -1)
    else:
        piece = torch.as_tensor(int(value), dtype=torch.int64, device=dv.device).to(dv.dtype)
    dv[dy:dy + h, dx:dx + w] = torch.where(sel[..., None], piece, dv[dy:dy + h, dx:dx + w])
    return int(sel.sum())  # the pixels it selected
