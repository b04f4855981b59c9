"""One allocation per test, out of which every buffer of a call is carved at a chosen byte address, with red zones around it.

The allocator hands out 256-byte aligned blocks with slack behind them, so a test that passes its tensors straight to the codec can
see neither a kernel that is wrong at an odd base address nor one that stores a few bytes outside what the call may write.  An Arena
is ONE uint8 tensor (device "cuda", or "cpu" for the helper's own test), filled with a position-dependent pattern -- a constant would
hide a stray copy of the same value.  carve() hands out `nbytes` at an address that is `skew` modulo 256, with at least 256 bytes of
pattern on both sides; an output buffer is carved at exactly the size the call may write, so the byte behind it is a red-zone byte.

    a = Arena(Arena.room(n_px, n_pay), device="cuda")
    px = a.carve("px", n_px, skew=1); a.load("px", pixels)        # an input: unchanged("px") afterwards
    pay = a.carve("payload", n_pay, skew=7)                        # an output: read("payload") afterwards
    ... the call, torch.cuda.synchronize() ...
    a.check(); a.unchanged("px")
"""
import numpy as np

ZONE = 256  # bytes of red zone on both sides of every buffer, at least; also the modulus of a skew


def pattern(first, n):
    """the fill of arena bytes [first, first + n): (37 * i + 11) & 0xFF"""
    return ((np.arange(first, first + n, dtype=np.int64) * 37 + 11) & 0xFF).astype(np.uint8)


class Arena:
    def __init__(self, capacity, device="cpu"):
        import torch

        self.torch = torch
        self.capacity = int(capacity)
        self.buf = torch.from_numpy(pattern(0, self.capacity)).to(device)
        self.base = self.buf.data_ptr()
        self._bufs = {}   # name -> (first byte, nbytes), in address order
        self._loaded = {}  # name -> what load() put there
        self._end = 0     # one past the last carved byte

    @staticmethod
    def room(*sizes):
        """a capacity that holds buffers of these sizes at any skews"""
        return sum(int(n) + 3 * ZONE for n in sizes) + 2 * ZONE

    def carve(self, name, nbytes, skew=0):
        """`nbytes` at an address with address % 256 == skew, a red zone of at least 256 bytes on both sides -> the address"""
        assert name not in self._bufs and 0 <= skew < ZONE and nbytes >= 0
        first = self._end + (2 * ZONE if self._bufs else ZONE)  # (a zone of its own for either neighbour: damage is blamed on the nearer)
        first += (skew - (self.base + first)) % ZONE
        assert first + nbytes + ZONE <= self.capacity, f"arena of {self.capacity} bytes has no room for {name} ({nbytes} bytes)"
        self._bufs[name] = (first, int(nbytes))
        self._end = first + int(nbytes)
        assert (self.base + first) % ZONE == skew
        return self.base + first

    def __contains__(self, name):
        return name in self._bufs

    def ptr(self, name):
        return self.base + self._bufs[name][0]

    def size(self, name):
        return self._bufs[name][1]

    def view(self, name):
        """the buffer as a uint8 tensor that shares the arena's memory"""
        first, n = self._bufs[name]
        return self.buf[first:first + n]

    def load(self, name, data):
        """fill the buffer (all of it) with `data` (anything numpy turns into bytes); unchanged(name) compares with it later"""
        a = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        first, n = self._bufs[name]
        assert a.size == n, f"{name} holds {n} bytes, got {a.size}"
        if n:
            self.buf[first:first + n] = self.torch.from_numpy(a.copy()).to(self.buf.device)
        self._loaded[name] = a.copy()
        return self.base + first

    def read(self, name, dtype=np.uint8):
        first, n = self._bufs[name]
        return self.buf[first:first + n].cpu().numpy().copy().view(dtype)

    def reset(self, name):
        """the pattern again (an output buffer before the next call)"""
        first, n = self._bufs[name]
        if n:
            self.buf[first:first + n] = self.torch.from_numpy(pattern(first, n)).to(self.buf.device)
        self._loaded.pop(name, None)

    def _zones(self):
        """(first, end, name, side) of every red zone: the gap between two buffers belongs half to each"""
        items = sorted(self._bufs.items(), key=lambda kv: kv[1][0])
        out, at = [], 0
        for i, (name, (first, n)) in enumerate(items):
            if i == 0:
                out.append((at, first, name, "start"))
            else:
                pname, (pfirst, pn) = items[i - 1]
                mid = at + (first - at) // 2
                out.append((at, mid, pname, "end"))
                out.append((mid, first, name, "start"))
            at = first + n
        if items:
            out.append((at, self.capacity, items[-1][0], "end"))
        return out

    def check(self):
        """every red zone still holds the pattern; else the buffer it belongs to and the first damaged offset relative to the buffer's
        start (negative: bytes in front of it) or to its end (0 = the byte right behind the buffer)"""
        host = self.buf.cpu().numpy()
        if not self._bufs:
            assert np.array_equal(host, pattern(0, self.capacity)), "an arena without buffers was written"
            return
        for z0, z1, name, side in self._zones():
            bad = np.nonzero(host[z0:z1] != pattern(z0, z1 - z0))[0]
            if bad.size:
                at = z0 + int(bad[0])
                first, n = self._bufs[name]
                rel = at - first if side == "start" else at - (first + n)
                raise AssertionError(f"red zone damaged: offset {rel:+d} from the {side} of buffer '{name}' ({n} bytes, skew "
                                     f"{(self.base + first) % ZONE}): {int(bad.size)} byte(s) in this zone, first holds "
                                     f"0x{int(host[at]):02x}, the pattern is 0x{int(pattern(at, 1)[0]):02x}")

    def unchanged(self, name):
        """an input buffer still holds what load() put there"""
        got, want = self.read(name), self._loaded[name]
        bad = np.nonzero(got != want)[0]
        if bad.size:
            raise AssertionError(f"input buffer '{name}' was written: offset {int(bad[0])} holds 0x{int(got[bad[0]]):02x}, "
                                 f"was 0x{int(want[bad[0]]):02x} ({int(bad.size)} byte(s) differ)")

    def untouched(self, name, first=0):
        """bytes [first, size) of a buffer that was never loaded still hold the pattern (an output a refused call must not write)"""
        start, n = self._bufs[name]
        got = self.read(name)[first:]
        bad = np.nonzero(got != pattern(start + first, n - first))[0]
        if bad.size:
            raise AssertionError(f"buffer '{name}' was written at offset {first + int(bad[0])} (0x{int(got[bad[0]]):02x}); "
                                 f"{int(bad.size)} byte(s) from offset {first} on differ from the pattern")

    def all_untouched(self):
        """no byte of the arena changed since the buffers were carved and loaded: red zones, inputs, and outputs still the pattern"""
        self.check()
        for name in self._bufs:
            if name in self._loaded:
                self.unchanged(name)
            else:
                self.untouched(name)
