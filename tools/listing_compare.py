#!/usr/bin/env python3
"""Compares two `hipcc -S --cuda-device-only` listings kernel by kernel: every kernel of OLD must be in NEW with the same instructions
and the same kernel descriptor.  The order of the functions in a listing, the number a function's local labels carry (.LBB<n>_) and the
compile unit's hash in internal names do not count.  Kernels that only NEW has are listed with their registers, LDS and scratch.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -S --cuda-device-only -o old.s <parent>/resize_kernels.hip
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -S --cuda-device-only -o new.s llcomp_amd/csrc/resize_kernels.hip
    python tools/listing_compare.py old.s new.s

Exit status 1 if a kernel of OLD is missing from NEW or differs."""
import re
import sys


def normal(line):
    line = re.sub(r"\s*;.*$", "", line)  # (comments: the listing pads them to a column that moves with a label's width)
    line = re.sub(r"\.LBB\d+_", ".LBB_", line)
    line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
    return re.sub(r"[0-9a-f]{16,}", "HASH", line)


def kernels(path):
    """{symbol: (code lines, descriptor lines)}"""
    text = open(path).read().splitlines()
    out, name, code = {}, None, []
    for ln in text:
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name, code = m.group(1), []
            continue
        if name is None:
            continue
        if ln.strip().startswith(".amdhsa_kernel"):
            desc = []
            out[name] = (code, desc)
            code = desc  # (the descriptor's lines follow, up to .end_amdhsa_kernel)
            continue
        if ln.strip().startswith(".end_amdhsa_kernel"):
            name = None
            continue
        if ln.strip().startswith(";"):
            continue
        code.append(normal(ln))
    return out


def field(desc, key):
    for ln in desc:
        if key in ln:
            return ln.split()[-1]
    return "?"


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(old):
        if name not in new:
            print(f"MISSING    {name}")
            bad += 1
        elif old[name] != new[name]:
            print(f"DIFFERS    {name}")
            bad += 1
        else:
            print(f"identical  {name}  ({len(old[name][0])} lines)")
    for name in sorted(set(new) - set(old)):
        d = new[name][1]
        print(f"new        {name}  vgpr {field(d, 'next_free_vgpr')} sgpr {field(d, 'next_free_sgpr')} "
              f"lds {field(d, 'group_segment_fixed_size')} scratch {field(d, 'private_segment_fixed_size')}")
    print(f"{len(old)} kernels of the old listing, {bad} missing or different; {len(set(new) - set(old))} new")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
