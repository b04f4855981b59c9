"""llcomp_mi_output_table (host only): the output rule of the resized calls' _ex forms -- the u8 value, divided by 255, minus mean, over
std, cast -- as a [c, 256] table, checked bit for bit against torch's CPU ops in the same order (ToTensor() + Normalize() + a cast);
every BAD_ARGS case of llcomp_mi_output_format; the struct's layout as C sees it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import llcomp_amd as mi
from conftest import ROOT

IMAGENET_MEAN = [0.485, 0.456, 0.406]
IMAGENET_STD = [0.229, 0.224, 0.225]
TORCH = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
BITS = {"float32": torch.int32, "float16": torch.int16, "bfloat16": torch.int16}


def channel_values(c, base):
    """c values: ImageNet's for the first three channels, then more of the same kind"""
    return [base[i] if i < 3 else base[i % 3] + 0.01 * i for i in range(c)]


def torch_table(c, dtype, scale, mean, std):
    """the rule with torch's CPU ops, channel by channel: [c, 256] of the dtype's bit patterns (uint8 for uint8)"""
    v = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    if dtype == "uint8":
        return np.tile(v.numpy(), (c, 1))
    rows = []
    for ch in range(c):
        t = v.float()
        if scale:
            t = t.div(255)
        if mean is not None:
            t = t.sub(torch.tensor(mean, dtype=torch.float32)[ch])
        if std is not None:
            t = t.div(torch.tensor(std, dtype=torch.float32)[ch])
        rows.append(t.to(TORCH[dtype]).view(BITS[dtype]).numpy())
    return np.stack(rows)


def bits(table):
    return table.view({4: np.int32, 2: np.int16, 1: np.uint8}[table.dtype.itemsize])


CASES = [(c, dtype, scale, norm) for c in (1, 3, 4, 5) for dtype in ("float32", "float16", "bfloat16") for scale in (False, True)
         for norm in ("none", "mean", "std", "both")] + [(c, "uint8", False, "none") for c in (1, 3, 4, 5)]


@pytest.mark.parametrize("c,dtype,scale,norm", CASES, ids=[f"c{c}_{d}_{'s' if s else 'ns'}_{n}" for c, d, s, n in CASES])
def test_table_is_the_torch_chain_bit_for_bit(c, dtype, scale, norm):
    mean = channel_values(c, IMAGENET_MEAN) if norm in ("mean", "both") else None
    std = channel_values(c, IMAGENET_STD) if norm in ("std", "both") else None
    t = mi.output_table(c, dtype, scale=scale, mean=mean, std=std)
    assert t.shape == (c, 256)
    assert t.dtype == {"float32": np.float32, "float16": np.float16, "bfloat16": np.uint16, "uint8": np.uint8}[dtype]
    assert np.array_equal(bits(t), torch_table(c, dtype, scale, mean, std))


def test_bfloat16_is_the_integer_rounding_of_the_float32_table():
    f32 = mi.output_table(3, "float32", scale=True, mean=IMAGENET_MEAN, std=IMAGENET_STD).view(np.uint32).astype(np.uint64)
    want = ((f32 + 0x7FFF + ((f32 >> 16) & 1)) >> 16).astype(np.uint16)
    assert np.array_equal(mi.output_table(3, "bfloat16", scale=True, mean=IMAGENET_MEAN, std=IMAGENET_STD), want)


def test_scale_is_a_division():
    """a multiply by 1/255 differs from the division on many values: the table divides"""
    t = mi.output_table(1, "float32", scale=True)[0]
    v = np.arange(256, dtype=np.float32)
    assert np.array_equal(t, v / np.float32(255))
    assert (t != v * (np.float32(1) / np.float32(255))).sum() > 0


def test_tiny_std_overflows_float16_to_inf():
    std = [1e-6, 1e-3, 1e-30]
    for dtype in ("float16", "bfloat16", "float32"):
        t = mi.output_table(3, dtype, mean=[0.5, -0.5, 0.0], std=std)
        assert np.array_equal(bits(t), torch_table(3, dtype, False, [0.5, -0.5, 0.0], std))
    f16 = mi.output_table(3, "float16", mean=[0.5, -0.5, 0.0], std=std)
    assert np.isposinf(f16[0, 1:]).all() and f16[0, 0] == -np.inf  # (0 - 0.5) / 1e-6
    assert np.isinf(f16[1]).sum() > 0 and np.isfinite(f16[1]).sum() > 0


def _fmt(**kw):
    f = mi.OutputFormat(C.sizeof(mi.OutputFormat), mi.DTYPE_F32, mi.LAYOUT_CHW, 1, None, None)
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def _floats(vals):
    return C.cast((C.c_float * len(vals))(*vals), C.POINTER(C.c_float))


BAD = [
    ("struct_size_small", dict(struct_size=C.sizeof(mi.OutputFormat) - 1)),
    ("struct_size_zero", dict(struct_size=0)),
    ("dtype_4", dict(dtype=4)),
    ("layout_2", dict(layout=2)),
    ("scale_2", dict(scale=2)),
    ("u8_scale", dict(dtype=mi.DTYPE_U8, scale=1)),
    ("u8_mean", dict(dtype=mi.DTYPE_U8, scale=0, mean=[0.5, 0.5, 0.5])),
    ("u8_std", dict(dtype=mi.DTYPE_U8, scale=0, std=[0.5, 0.5, 0.5])),
    ("mean_nan", dict(mean=[0.5, float("nan"), 0.5])),
    ("mean_inf", dict(mean=[0.5, 0.5, float("inf")])),
    ("std_zero", dict(std=[0.5, 0.0, 0.5])),
    ("std_negative_zero", dict(std=[-0.0, 0.5, 0.5])),
    ("std_nan", dict(std=[0.5, 0.5, float("nan")])),
    ("std_inf", dict(std=[float("-inf"), 0.5, 0.5])),
]


@pytest.mark.parametrize("name,kw", BAD, ids=[b[0] for b in BAD])
def test_bad_formats(name, kw):
    L = mi._lib.load()
    kw = {k: (_floats(v) if k in ("mean", "std") else v) for k, v in kw.items()}
    table = np.full((3, 256), 0x5A5A5A5A, np.uint32)
    assert L.llcomp_mi_output_table(C.byref(_fmt(**kw)), 3, table.ctypes.data) == mi.BAD_ARGS
    assert (table == 0x5A5A5A5A).all()


@pytest.mark.parametrize("dtype,kw", [("uint8", dict(scale=True)), ("uint8", dict(mean=IMAGENET_MEAN)), ("uint8", dict(std=IMAGENET_STD)),
                                      ("float32", dict(mean=[0.5, float("nan"), 0.5])), ("bfloat16", dict(std=[0.5, 0.0, 0.5])),
                                      ("float16", dict(std=[0.5, 0.5, float("inf")]))])
def test_bad_formats_through_the_binding(dtype, kw):
    with pytest.raises(mi.LlcompError) as e:
        mi.output_table(3, dtype, **kw)
    assert e.value.status == mi.BAD_ARGS


def test_bad_calls():
    L = mi._lib.load()
    table = np.zeros((256, 256), np.uint32)
    good = _fmt()
    assert L.llcomp_mi_output_table(None, 3, table.ctypes.data) == mi.BAD_ARGS
    assert L.llcomp_mi_output_table(C.byref(good), 3, None) == mi.BAD_ARGS
    assert L.llcomp_mi_output_table(C.byref(good), 0, table.ctypes.data) == mi.BAD_ARGS
    assert L.llcomp_mi_output_table(C.byref(good), 256, table.ctypes.data) == mi.BAD_ARGS
    assert L.llcomp_mi_output_table(C.byref(good), 255, table.ctypes.data) == mi.OK
    big = _fmt(struct_size=C.sizeof(mi.OutputFormat) + 8)  # (a larger struct from a later header is accepted)
    assert L.llcomp_mi_output_table(C.byref(big), 3, table.ctypes.data) == mi.OK
    for bad in ("int8", "float64", "chw"):
        with pytest.raises(mi.LlcompError):
            mi.output_table(3, bad)


def test_struct_layout_in_c(tmp_path):
    """the header compiles as C99 -pedantic with llcomp_mi_output_format at 32 bytes and the offsets of the ctypes mirror"""
    F = mi.OutputFormat
    assert C.sizeof(F) == 32
    assert [F.struct_size.offset, F.dtype.offset, F.layout.offset, F.scale.offset, F.mean.offset, F.std.offset] == [0, 4, 8, 12, 16, 24]
    src = tmp_path / "fmt.c"
    src.write_text(
        '#include <stddef.h>\n#include "llcomp_mi.h"\n'
        "typedef char size_ok[sizeof(llcomp_mi_output_format) == 32 ? 1 : -1];\n"
        "typedef char off_ok[offsetof(llcomp_mi_output_format, dtype) == 4 && offsetof(llcomp_mi_output_format, layout) == 8 &&\n"
        "                    offsetof(llcomp_mi_output_format, scale) == 12 && offsetof(llcomp_mi_output_format, mean) == 16 &&\n"
        "                    offsetof(llcomp_mi_output_format, std) == 24 ? 1 : -1];\n"
        "int main(void) { llcomp_mi_output_format f = {0}; size_ok a; off_ok b; f.struct_size = sizeof f; f.dtype = LLCOMP_MI_DTYPE_BF16;\n"
        "  f.layout = LLCOMP_MI_LAYOUT_CHW; (void)a; (void)b;\n"
        "  return sizeof(llcomp_mi_output_format) == 32 && LLCOMP_MI_DTYPE_U8 == 0 && LLCOMP_MI_DTYPE_F32 == 1 && LLCOMP_MI_DTYPE_F16 == 2 &&\n"
        "         f.dtype == 3 && LLCOMP_MI_LAYOUT_HWC == 0 && f.layout == 1 ? 0 : 1; }\n")
    exe = tmp_path / "fmt"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0
