"""tests/arena.py on the CPU: the helper reports a stray byte in front of a buffer, behind it and inside an input at the right offset
-- the GPU tests that use it (test_gpu_caller_buffers.py) are only as good as this."""
import numpy as np
import pytest
from arena import ZONE, Arena, pattern


def make():
    a = Arena(Arena.room(100, 333, 8, 0), device="cpu")
    a.carve("in", 100, skew=1)
    a.carve("out", 333, skew=7)
    a.carve("total", 8)
    a.carve("empty", 0, skew=3)
    a.load("in", np.arange(100, dtype=np.uint8))
    return a


def flip(a, address):
    """a byte that differs from whatever lies there"""
    a.buf[address - a.base] ^= 0xFF


def test_addresses_skews_and_zones():
    a = make()
    assert a.ptr("in") % ZONE == 1 and a.ptr("out") % ZONE == 7 and a.ptr("total") % ZONE == 0 and a.ptr("empty") % ZONE == 3
    assert a.ptr("in") - a.base >= ZONE
    assert a.ptr("out") - (a.ptr("in") + 100) >= ZONE and a.ptr("total") - (a.ptr("out") + 333) >= ZONE
    assert a.base + a.capacity - (a.ptr("empty") + 0) >= ZONE
    assert a.view("out").data_ptr() == a.ptr("out") and a.view("out").numel() == 333
    # position-dependent: not a constant, and the carved bytes hold it too
    first = a.ptr("out") - a.base
    assert np.array_equal(a.read("out"), pattern(first, 333)) and len(set(pattern(0, 256).tolist())) == 256
    a.check()
    a.unchanged("in")
    a.untouched("out")
    a.all_untouched()
    with pytest.raises(AssertionError, match="no room"):
        a.carve("more", 10 * ZONE)


@pytest.mark.parametrize("rel", [-1, -4, -ZONE])
def test_stray_byte_in_front_of_a_buffer(rel):
    a = make()
    flip(a, a.ptr("out") + rel)
    with pytest.raises(AssertionError, match=rf"offset \{rel:+d} from the start of buffer 'out'"):
        a.check()


@pytest.mark.parametrize("rel", [0, 3, 15, ZONE - 1])
def test_stray_byte_behind_a_buffer(rel):
    a = make()
    flip(a, a.ptr("out") + 333 + rel)
    with pytest.raises(AssertionError, match=rf"offset \{rel:+d} from the end of buffer 'out'"):
        a.check()
    b = make()  # ... and behind the last one, which is empty: its end is its start
    flip(b, b.ptr("empty") + rel)
    with pytest.raises(AssertionError, match=rf"offset \{rel:+d} from the end of buffer 'empty'"):
        b.check()


def test_the_first_damaged_byte_is_named():
    a = make()
    for rel in (9, 2, 5):
        flip(a, a.ptr("in") + 100 + rel)
    with pytest.raises(AssertionError, match=r"offset \+2 from the end of buffer 'in'.*3 byte"):
        a.check()


def test_stray_byte_in_an_input():
    a = make()
    flip(a, a.ptr("in") + 42)
    a.check()  # (not a red zone)
    with pytest.raises(AssertionError, match=r"input buffer 'in' was written: offset 42 "):
        a.unchanged("in")
    with pytest.raises(AssertionError, match=r"offset 42 "):
        a.all_untouched()


def test_a_constant_fill_would_hide_what_the_pattern_shows():
    """a copy of a buffer's own bytes one byte further on -- the stray store of a kernel that is off by one -- changes the zone"""
    a = make()
    end = a.ptr("out") + 333 - a.base
    a.buf[end] = a.buf[end - 1]
    with pytest.raises(AssertionError, match=r"offset \+0 from the end of buffer 'out'"):
        a.check()


def test_untouched_and_reset():
    a = make()
    a.view("out")[10] = 0
    a.view("out")[200] ^= 0xFF
    with pytest.raises(AssertionError, match=r"buffer 'out' was written at offset 200 "):
        a.untouched("out", first=11)
    a.reset("out")
    a.untouched("out")
    a.check()
