"""The host planner of the batch mixing (llcomp_mi_mix_plan; llcomp_amd/csrc/mix_plan.cpp): the partner permutation cycle by cycle, the
cycles longer than llcomp_mi_mix_segment() cut into segments, the heads that are saved first -- and its refusals."""
import ctypes as C
import random

import numpy as np
import pytest


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    return llcomp_amd


def cycles_of(partner):
    seen, out = set(), []
    for i0 in range(len(partner)):
        if i0 in seen:
            continue
        cyc, i = [], i0
        while i not in seen:
            seen.add(i)
            cyc.append(i)
            i = partner[i]
        out.append(cyc)
    return out


def check_plan(mi, partner):
    S = mi.mix_segment()
    n = len(partner)
    order, seg_first, n_saved = mi.mix_plan(mi.mix_samples(n, partner))
    order, seg_first = order.tolist(), seg_first.tolist()
    assert sorted(order) == list(range(n))
    assert seg_first[0] == 0 and seg_first[-1] == n and all(0 < b - a <= S for a, b in zip(seg_first, seg_first[1:]))
    at, want_saved = 0, 0
    for cyc in cycles_of(partner):  # cycle by cycle, each along its partners from its smallest sample
        got = order[at:at + len(cyc)]
        assert got == cyc
        inside = [s for s in seg_first if at < s < at + len(cyc)]
        assert at in seg_first and len(inside) + 1 == -(-len(cyc) // S)  # as few segments as the length allows
        if len(cyc) > S:
            want_saved += len(inside) + 1
        at += len(cyc)
    assert n_saved == want_saved
    return n_saved


def test_cycles_around_the_segment_length(mi):
    S = mi.mix_segment()
    assert S >= 2
    for length, saved in ((1, 0), (2, 0), (S - 1, 0), (S, 0), (S + 1, 2), (2 * S + 1, 3)):
        roll = [(i - 1) % length for i in range(length)]
        assert check_plan(mi, roll) == saved, length
    # all six lengths in one permutation, their samples interleaved
    rng = random.Random(5)
    lengths = [1, 2, S - 1, S, S + 1, 2 * S + 1, 1, 3 * S]
    ids = list(range(sum(lengths)))
    rng.shuffle(ids)
    partner, at = [0] * len(ids), 0
    for length in lengths:
        cyc = ids[at:at + length]
        for a, b in zip(cyc, cyc[1:] + cyc[:1]):
            partner[a] = b
        at += length
    assert check_plan(mi, partner) == 2 + 3 + 3
    for n in (1, 2, 5, 64, 257):
        assert check_plan(mi, [n - 1 - i for i in range(n)]) == 0  # flip: cycles of two and a fixed point
        perm = list(range(n))
        rng.shuffle(perm)
        check_plan(mi, perm)


def test_refusals_leave_the_outputs_untouched(mi):
    L = mi._lib.load()
    n = 4

    def call(samples, n_=n, with_counts=(True, True)):
        order, seg = np.full(n + 8, 77, np.uint32), np.full(n + 9, 77, np.uint32)
        ns, nv = C.c_uint32(77), C.c_uint32(77)
        u32p = C.POINTER(C.c_uint32)
        rc = L.llcomp_mi_mix_plan(n_, samples, order.ctypes.data_as(u32p), seg.ctypes.data_as(u32p), C.byref(ns) if with_counts[0] else None,
                                  C.byref(nv) if with_counts[1] else None)
        if rc:
            assert (order == 77).all() and (seg == 77).all() and ns.value == 77 and nv.value == 77
        return rc

    assert call(mi.mix_samples(n, "roll", 0.5)) == 0
    assert call(None) == mi.BAD_ARGS and call(mi.mix_samples(n, "roll"), n_=0) == mi.BAD_ARGS
    assert call(mi.mix_samples(n, "roll"), with_counts=(False, True)) == mi.BAD_ARGS
    assert call(mi.mix_samples(n, "roll"), with_counts=(True, False)) == mi.BAD_ARGS
    big = (mi._lib.MixSample * 65536)()
    for i in range(65536):
        big[i].partner = i
    assert L.llcomp_mi_mix_plan(65536, big, None, None, C.byref(C.c_uint32()), C.byref(C.c_uint32())) == mi.BAD_ARGS
    assert L.llcomp_mi_mix_plan(65535, big, None, None, C.byref(C.c_uint32()), C.byref(C.c_uint32())) == 0
    for field, i, value in (("partner", 0, n), ("partner", 0, 0xFFFFFFFF), ("partner", 1, 1), ("flags", 2, 2), ("flags", 2, 3),
                            ("w_own", 3, float("nan")), ("w_partner", 0, float("-inf"))):
        s = mi.mix_samples(n, "roll", 0.5)
        setattr(s[i], field, value)
        assert call(s) == mi.BAD_ARGS, (field, value)
