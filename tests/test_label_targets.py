"""The rule of the label targets on the host (llcomp_mi_label_targets_reference; include/llcomp_mi.h: "Label targets") against a numpy
spec written here -- np.searchsorted per sample for the value of a pixel, a comparison with np.arange(K) for the planes -- and against
torch on the CPU: lut[map.long()], (t[:, None] == torch.arange(K).view(1, K, 1, 1)).to(dtype), map[None] == ids[:, None, None]; the
refusals.  value_spec, index_spec and planes_spec are what the GPU tests compare with too."""
import ctypes as C

import numpy as np
import pytest

from test_label_boxes16 import HIGH_BYTE, blobs16


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


INDEX_DTYPES = ("uint8", "int32", "int64")
PLANE_DTYPES = ("uint8", "float32", "float16", "bfloat16")


def value_spec(maps, ids, values, default):
    """maps [n, oh, ow], ids and values: n sequences -> v [n, oh, ow] int64: the value of the pixel's id, or default"""
    v = np.full(maps.shape, default, np.int64)
    for i in range(len(maps)):
        l, val = np.asarray(list(ids[i]), np.int64), np.asarray(list(values[i]), np.int64)
        if not l.size:
            continue
        j = np.minimum(np.searchsorted(l, maps[i]), l.size - 1)
        v[i] = np.where(l[j] == maps[i], val[j], default)
    return v


def index_spec(maps, ids, values, default, dtype):
    return value_spec(maps, ids, values, default).astype(dtype)


def element_bits(value, dtype):
    """the element of `dtype` that holds value, as the numpy type the library takes for it (bfloat16: its bits, converted by torch)"""
    if dtype == "bfloat16":
        import torch

        return np.uint16(torch.tensor(float(value), dtype=torch.bfloat16).view(torch.int16).item() & 0xFFFF)
    return np.dtype(dtype).type(value)


def planes_spec(maps, ids, values, default, counts, on, off, dtype):
    """-> [sum(counts), oh, ow]: plane k of sample i holds on where v(i, p) == k, else off"""
    v = value_spec(maps, ids, values, default)
    out = [np.where(v[i][None] == np.arange(k)[:, None, None], element_bits(on, dtype), element_bits(off, dtype)) for i, k in enumerate(counts)]
    return np.concatenate(out).astype(element_bits(0, dtype).dtype)


def shapes(S):
    """(oh, ow) of S - 1, S, S + 1 and 2 * S + 3 pixels, and of one"""
    assert S == 4096
    return ((1, 1), (7, 585), (64, 64), (17, 241), (5, 1639))


def at_offset(maps, off):
    """a copy of the maps `off` bytes past a 16-byte boundary"""
    raw = np.zeros(maps.nbytes + 48, np.uint8)
    base = (-raw.ctypes.data) % 16 + off
    raw[base:base + maps.nbytes] = maps.reshape(-1).view(np.uint8)
    return raw[base:base + maps.nbytes].view(maps.dtype).reshape(maps.shape)


def draw(rng, map_dtype, n, oh, ow):
    """maps of blobs, and per sample a list of some ids the map has and some it has not, with values that several ids share; the
    sample in the middle lists nothing"""
    pool = HIGH_BYTE if map_dtype == np.uint16 else (0, 1, 2, 3, 200, 255)
    maps = blobs16(rng, n, oh, ow, pool).astype(map_dtype)
    ids = [sorted({int(m) for m in pool if rng.integers(0, 3)} | {int(x) for x in rng.integers(0, 256 if map_dtype == np.uint8 else 65536, size=2)}) for _ in range(n)]
    ids[n // 2] = []
    return maps, ids


def test_index_is_numpy_and_torch(mi):
    import torch

    rng = np.random.default_rng(41)
    for map_dtype in (np.uint8, np.uint16):
        for k, (oh, ow) in enumerate(shapes(mi.label_targets_segment())):
            maps, ids = draw(rng, map_dtype, 3, oh, ow)
            off = (2 * k + 1) % 16 if map_dtype == np.uint8 else (2 * k + 2) % 16
            for dtype in INDEX_DTYPES:
                lo, hi = (0, 256) if dtype == "uint8" else (-100, 20)
                values = [rng.integers(lo, hi, size=len(l)).tolist() for l in ids]
                default = 255 if dtype == "uint8" else -100
                got = mi.label_targets_reference(at_offset(maps, off), ids, values, dtype=dtype, default=default)
                assert got.dtype == np.dtype(dtype) and got.shape == maps.shape
                assert np.array_equal(got, index_spec(maps, ids, values, default, dtype)), (map_dtype, oh, ow, dtype)
                for i in range(3):  # torch: a lut of every id, gathered by the int64 copy of the map
                    lut = torch.full((65536,), default, dtype=torch.int64)
                    lut[torch.tensor(ids[i], dtype=torch.int64)] = torch.tensor(values[i], dtype=torch.int64)
                    assert torch.equal(torch.from_numpy(got[i].astype(np.int64)), lut[torch.from_numpy(maps[i].astype(np.int64))])


@pytest.mark.parametrize("dtype", PLANE_DTYPES)
def test_planes_are_numpy_and_torch(mi, dtype):
    import torch

    K, eps = 5, 0.1
    rng = np.random.default_rng(43)
    tdt = {"uint8": torch.uint8, "float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}[dtype]
    for map_dtype in (np.uint8, np.uint16):
        for k, (oh, ow) in enumerate(shapes(mi.label_targets_segment())):
            maps, ids = draw(rng, map_dtype, 3, oh, ow)
            values = [rng.integers(-1, K + 2, size=len(l)).tolist() for l in ids]  # (shared values; -1, K and K + 1 select no plane)
            for default, on, off in ((0, 1, 0), (-1, 1, 0), (K, 1, 0)) + (() if dtype == "uint8" else ((2, 1 - eps + eps / K, eps / K),)):
                got = mi.label_targets_reference(at_offset(maps, 2 * k), ids, values, kind="planes", dtype=dtype, default=default, planes=K, on=on, off=off)
                assert got.shape == (3, K, oh, ow)
                assert np.array_equal(got.reshape(3 * K, oh, ow), planes_spec(maps, ids, values, default, [K] * 3, on, off, dtype)), (map_dtype, oh, ow, default)
                t = torch.from_numpy(value_spec(maps, ids, values, default))
                hot = t[:, None] == torch.arange(K).view(1, K, 1, 1)
                want = hot.to(tdt) if (on, off) == (1, 0) else torch.where(hot, torch.tensor(on, dtype=tdt), torch.tensor(off, dtype=tdt))
                bits = want.view(torch.int16).numpy().view(np.uint16) if dtype == "bfloat16" else want.numpy()
                assert np.array_equal(got, bits)
            # a count per sample: the sample in the middle owns no plane
            got = mi.label_targets_reference(maps, ids, values, kind="planes", dtype=dtype, default=1, planes=[2, 0, 7])
            assert got.shape == (9, oh, ow) and np.array_equal(got, planes_spec(maps, ids, values, 1, [2, 0, 7], 1, 0, dtype))


def test_instance_masks_high_bytes_negative_values_and_empty_lists(mi):
    import torch

    S = mi.label_targets_segment()
    rng = np.random.default_rng(47)
    high = blobs16(rng, 3, 67, S // 64 + 3, HIGH_BYTE)  # ids that differ only in the high byte: a test of the low byte alone fails
    high[:, 0, :6] = HIGH_BYTE
    ids = [[0x0001, 0x0101, 0xFF01], [], [0x0101, 0x0201]]
    masks = mi.label_targets_reference(high, ids, [range(len(l)) for l in ids], kind="planes", default=-1, planes=[len(l) for l in ids])
    want = torch.cat([torch.from_numpy(high[i].astype(np.int64))[None] == torch.tensor(ids[i], dtype=torch.int64)[:, None, None] for i in range(3)]).numpy()
    assert masks.dtype == np.uint8 and np.array_equal(masks, want.astype(np.uint8)) and masks.shape[0] == 5
    assert masks[0].sum() < ((high[0] & 0xFF) == 1).sum()  # (what a test of the low byte alone would select)
    # instance -> class with an "ignore" of -100, into int64: the sign is extended; the sample with an empty list is all default
    got = mi.label_targets_reference(high, ids, [[7, -1, -2 ** 31], [], [2 ** 31 - 1, 7]], default=-100)
    assert got.dtype == np.int64 and (got[1] == -100).all() and got.min() == -2 ** 31 and got.max() == 2 ** 31 - 1
    assert np.array_equal(got, value_spec(high, ids, [[7, -1, -2 ** 31], [], [2 ** 31 - 1, 7]], -100))
    assert (mi.label_targets_reference(high, [[], [], []], [[], [], []], dtype="uint8", default=9) == 9).all()
    # every byte id listed for a 1-byte map is a plain lut
    narrow = rng.integers(0, 256, size=(2, 37, 29), dtype=np.uint8)
    lut = rng.integers(-5, 19, size=256)
    assert np.array_equal(mi.label_targets_reference(narrow, [range(256)] * 2, [lut] * 2, dtype="int32"), lut[narrow])
    assert np.array_equal(mi.label_targets_reference(narrow.astype(np.uint16), [range(256)] * 2, [lut] * 2, dtype="int32"), lut[narrow])


@pytest.mark.parametrize("count", [1, 256, 257, 1024, 1025, 4096])
def test_list_lengths_around_the_capacities(mi, count):
    rng = np.random.default_rng(count)
    listed = np.sort(rng.choice(65536, size=count, replace=False))
    others = np.setdiff1d(np.arange(65536), listed)[:50]
    pool = np.concatenate([listed[:: max(2, count // 300)], others])
    maps = pool[rng.integers(0, len(pool), size=(2, 45, 93))].astype(np.uint16)
    ids = [listed.tolist(), listed[: count // 2 + 1].tolist()]
    values = [(np.arange(len(l)) % 11 - 1).tolist() for l in ids]
    assert np.array_equal(mi.label_targets_reference(maps, ids, values, default=-100), value_spec(maps, ids, values, -100))
    got = mi.label_targets_reference(maps, ids, values, kind="planes", dtype="float16", default=-1, planes=[10, 3])
    assert np.array_equal(got, planes_spec(maps, ids, values, -1, [10, 3], 1, 0, "float16"))


def test_refusals(mi):
    L = mi._lib.load()
    T = mi._lib.LabelTargets
    maps = np.zeros((2, 4, 5), np.uint16)
    ids, values, first = np.array([0, 3, 9, 1, 2], np.uint16), np.array([0, 1, 2, 3, 4], np.int32), np.array([0, 3, 5], np.uint32)
    planes = np.array([0, 2, 6], np.uint32)
    out = np.full(6 * 20 + 2, 0x5A5A, np.uint16)
    m, o = maps.ctypes.data, out.ctypes.data

    def call(mp=m, n=2, ow=5, oh=4, op=o, **kw):
        f = dict(struct_size=C.sizeof(T), map_bytes=2, kind=mi.TARGET_PLANES, dtype=mi.DTYPE_F16, default_value=-1, on_bits=0x3C00, off_bits=0,
                 ids=ids.ctypes.data, values=values.ctypes.data, first=first.ctypes.data, plane_first=planes.ctypes.data)
        f.update(kw)
        t = T(**f)
        rc = L.llcomp_mi_label_targets_reference(mp, n, ow, oh, C.byref(t), op)
        assert (L.llcomp_mi_label_targets_out_bytes(n, ow, oh, C.byref(t)) == 0) == (rc != mi.OK) or mp != m or op != o
        return rc

    def u32(*v):
        return np.array(v, np.uint32)

    keep = [u32(1, 3, 5), u32(0, 4, 3), np.array([0, 3, 3, 1, 2], np.uint16), np.array([0, 3, 9, 2, 1], np.uint16), u32(1, 2, 6), u32(0, 4, 3), u32(0, 4097, 4097),
            np.array([0, 3, 300, 1, 2], np.uint16), np.array([0, 1, 2, 256, 4], np.int32), np.array([0, -1, 2, 3, 4], np.int32)]
    for kw in (dict(mp=None), dict(op=None), dict(mp=m + 1), dict(op=o + 1), dict(n=0), dict(n=65536), dict(ow=0), dict(oh=0), dict(n=1, ow=65536, oh=65536),
               dict(struct_size=C.sizeof(T) - 1), dict(map_bytes=0), dict(map_bytes=4), dict(kind=2), dict(dtype=4), dict(ids=None), dict(values=None), dict(first=None),
               dict(plane_first=None), dict(first=keep[0].ctypes.data), dict(first=keep[1].ctypes.data), dict(ids=keep[2].ctypes.data), dict(ids=keep[3].ctypes.data),
               dict(plane_first=keep[4].ctypes.data), dict(plane_first=keep[5].ctypes.data), dict(plane_first=keep[6].ctypes.data),
               dict(on_bits=0x10000), dict(off_bits=0x10000), dict(dtype=mi.DTYPE_U8, on_bits=256),
               dict(map_bytes=1, ids=keep[7].ctypes.data),                                   # an id above 255 in a 1-byte map
               dict(kind=mi.TARGET_INDEX, dtype=mi.TARGET_U8, default_value=0, values=keep[8].ctypes.data),   # a value above 255 into uint8
               dict(kind=mi.TARGET_INDEX, dtype=mi.TARGET_U8, default_value=0, values=keep[9].ctypes.data),   # a negative one
               dict(kind=mi.TARGET_INDEX, dtype=mi.TARGET_U8, default_value=-1),             # a default outside uint8
               dict(kind=mi.TARGET_INDEX, dtype=3)):
        assert call(**kw) == mi.BAD_ARGS, kw
    assert (out == 0x5A5A).all()
    assert call(op=o + 2) == mi.OK  # aligned to the element and to nothing more
    assert out[0] == 0x5A5A and out[-1] == 0x5A5A and out[1] == 0x3C00 and set(out[1:-1].tolist()) == {0, 0x3C00}
    assert call(kind=mi.TARGET_INDEX, dtype=mi.TARGET_U8, default_value=255, op=o + 1) == mi.OK
    for bad, lists, vals, kw in ((np.zeros((2, 4), np.uint16), [[1], [1]], [[1], [1]], {}), (np.zeros((2, 4, 5), np.int32), [[1], [1]], [[1], [1]], {}),
                                 (maps, [[1]], [[1]], {}), (maps, [[1], [2]], [[1], []], {}), (maps, [[1], [70000]], [[1], [1]], {}), (maps, [[2, 1], []], [[0, 0], []], {}),
                                 (maps, [[1], [2]], [[1], [2 ** 31]], {}), (maps, [[1], [2]], [[1], [2]], dict(kind="mask")), (maps, [[1], [2]], [[1], [2]], dict(dtype="float32")),
                                 (maps, [[1], [2]], [[1], [2]], dict(kind="planes")), (maps, [[1], [2]], [[1], [2]], dict(kind="planes", planes=[1])),
                                 (maps, [[1], [2]], [[1], [2]], dict(kind="planes", planes=4097)), (maps, [[1], [2]], [[1], [2]], dict(kind="planes", planes=2, dtype="int64")),
                                 (maps, [[1], [2]], [[1], [2]], dict(kind="planes", planes=2, on=256)), (maps.astype(np.uint8), [[1], [256]], [[1], [2]], {})):
        with pytest.raises(mi.LlcompError):
            mi.label_targets_reference(bad, lists, vals, **kw)
    assert C.sizeof(T) == 64 and T.ids.offset == 32 and mi.label_targets_max_planes() == 4096
