"""Tile-periodic batches whose SLICED containers are known without coding them (test helper, not a conftest).

Every slice of a SLICED container is an independent stream with fresh state and slice-local borders.  So a batch
whose tiles are all crops of a few bank tiles has a known container: the oracle's bare stream of each bank tile (or of its right-edge,
bottom-edge or corner crop, and of each plane when planar), placed in slice order.  That gives the expected payload of batches far too
large for the single-thread oracle to code: tests/test_tiled_batch.py proves the shortcut against orc.compress_sliced of whole images,
tests/test_gpu_large.py uses it past 2^31 and 2^32 samples.

Placement: tile (tx, ty) of frame f is bank entry (A·f + B·ty + tx) mod K, K prime.  Horizontal and vertical neighbours and
neighbouring frames never share an entry, and frame f repeats frame 0's tiles only when K divides f (TiledBatch.frames_differ).
"""
import struct

import numpy as np

HEADER = 24  # magic, version, channels, flags, then w, h, tile_w, tile_h, n_slices as u32 (oracle/orc.py: sliced_container)
K_PRIMES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31)
A, B = 5, 3  # frame and tile-row steps of the placement (neither is a multiple of any K past 5; K = 2, 3, 5 use A = B = 1)


def bank_tile(kind, rng, th, tw, c):
    """one bank tile [th, tw, c] u8: "noise" (payload volume), "grad" (smooth, small residuals), "flat" (one value with a few spikes:
    long zero runs broken by large residuals)"""
    if kind == "noise":
        return rng.integers(0, 256, size=(th, tw, c), dtype=np.uint8)
    if kind == "grad":
        y, x = np.mgrid[0:th, 0:tw]
        ax, ay = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        base = (x[:, :, None] * ax + y[:, :, None] * ay + np.arange(c)[None, None, :] * 37 + int(rng.integers(0, 256)))
        return (base % 256).astype(np.uint8)
    if kind == "flat":
        t = np.full((th, tw, c), int(rng.integers(0, 256)), np.uint8)
        n = max(1, t.size // 97)
        idx = rng.integers(0, t.size, size=n)
        t.reshape(-1)[idx] = rng.integers(0, 256, size=n, dtype=np.uint8)
        return t
    raise ValueError(kind)


def split_container(data):
    """(header fields dict, per-slice payloads as a list of bytes) of a SLICED container"""
    assert data[0] == 0x9C and data[1] == 1, "not a SLICED container"
    w, h, tw, th, n = struct.unpack_from("<5I", data, 4)
    lens = np.frombuffer(data, dtype="<u4", count=n, offset=HEADER).astype(np.int64)
    pos = HEADER + 4 * n
    out = []
    for ln in lens:
        out.append(bytes(data[pos:pos + ln]))
        pos += int(ln)
    assert pos == len(data)
    return dict(c=data[2], flags=data[3], w=w, h=h, tile_w=tw, tile_h=th, n=n), out


class TiledBatch:
    """`frames` frames of w x h x c, sliced into tile_w x tile_h tiles (planar or interleaved), every tile a crop of one of
    len(kinds) bank tiles.  len(kinds) must be prime."""

    def __init__(self, orc, frames, w, h, c, tile_w, tile_h, planar, kinds, small_model=False, seed=0):
        K = len(kinds)
        if K not in K_PRIMES:
            raise ValueError("the bank size must be a small prime")
        self.frames, self.w, self.h, self.c, self.planar, self.small_model = frames, w, h, c, bool(planar), bool(small_model)
        self.tile_w = w if tile_w <= 0 or tile_w > w else tile_w
        self.tile_h = h if tile_h <= 0 or tile_h > h else tile_h
        self.ntx, self.nty = -(-w // self.tile_w), -(-h // self.tile_h)
        self.np_ = c if planar else 1  # slices per tile
        self.K = K
        self.a, self.b = (A, B) if K > 5 else (1, 1)
        rng = np.random.default_rng(seed)
        self.bank = np.stack([bank_tile(k, rng, self.tile_h, self.tile_w, c) for k in kinds])  # [K, th, tw, c]
        # streams of every (entry, edge class, plane): class bit 0 = the partial last tile column, bit 1 = the partial last tile row
        rw, rh = w - (self.ntx - 1) * self.tile_w, h - (self.nty - 1) * self.tile_h
        pieces = []
        orc.set_small_model(self.small_model)
        try:
            for e in range(K):
                for cls in range(4):
                    sw, sh = (rw if cls & 1 else self.tile_w), (rh if cls & 2 else self.tile_h)
                    crop = np.ascontiguousarray(self.bank[e, :sh, :sw])
                    _, pays = split_container(orc.compress_sliced(crop, sw, sh, self.planar))
                    assert len(pays) == self.np_
                    pieces += pays
        finally:
            orc.set_small_model(False)
        self.stream_len = np.array([len(p) for p in pieces], np.int64)
        self.stream_off = np.concatenate([[0], np.cumsum(self.stream_len)[:-1]]).astype(np.int64)
        self.stream_bytes = np.frombuffer(b"".join(pieces), np.uint8)

    # ---- placement ------------------------------------------------------------------------------------------------------------
    @property
    def samples_per_frame(self):
        return self.w * self.h * self.c

    @property
    def slices_per_frame(self):
        return self.ntx * self.nty * self.np_

    def tile_map(self, f0=0, f1=None):
        """bank entry of every tile of frames [f0, f1): int64 [f1 - f0, nty, ntx]"""
        f1 = self.frames if f1 is None else f1
        f = np.arange(f0, f1, dtype=np.int64)[:, None, None]
        ty = np.arange(self.nty, dtype=np.int64)[None, :, None]
        tx = np.arange(self.ntx, dtype=np.int64)[None, None, :]
        return (self.a * f + self.b * ty + tx) % self.K

    def frames_differ(self, f, g):
        """True when frames f and g share no tile at the same place"""
        return bool((self.tile_map(f, f + 1) != self.tile_map(g, g + 1)).all())

    def stream_ids(self, f0=0, f1=None):
        """stream of every slice of frames [f0, f1) in container order (frame, tile row, tile column, plane): int64"""
        m = self.tile_map(f0, f1)
        cls = np.zeros((self.nty, self.ntx), np.int64)
        if self.w % self.tile_w:
            cls[:, -1] |= 1
        if self.h % self.tile_h:
            cls[-1, :] |= 2
        sid = ((m * 4 + cls[None]) * self.np_)[..., None] + np.arange(self.np_, dtype=np.int64)
        return sid.reshape(-1)

    def lengths(self, f0=0, f1=None):
        """the expected slice-length table of frames [f0, f1): uint32"""
        return self.stream_len[self.stream_ids(f0, f1)].astype(np.uint32)

    # ---- pixels ---------------------------------------------------------------------------------------------------------------
    def frames_host(self, f0=0, f1=None):
        """frames [f0, f1) as a host array u8 [n, h, w, c]"""
        m = self.tile_map(f0, f1)
        n = m.shape[0]
        t = self.bank[m]  # [n, nty, ntx, th, tw, c]
        full = t.transpose(0, 1, 3, 2, 4, 5).reshape(n, self.nty * self.tile_h, self.ntx * self.tile_w, self.c)
        return np.ascontiguousarray(full[:, :self.h, :self.w])

    def fill_device(self, out, f0=0, step=None):
        """write frames [f0, f0 + len(out)) into the device tensor `out` (u8 [n, h, w, c]), `step` frames (default: about 256 MB) at a time:
        only the bank crosses PCIe"""
        import torch

        step = step or max(1, (1 << 28) // self.samples_per_frame)
        bank = torch.from_numpy(self.bank).to(out.device)
        for i in range(0, out.shape[0], step):
            j = min(out.shape[0], i + step)
            m = torch.from_numpy(self.tile_map(f0 + i, f0 + j)).to(out.device)
            t = bank[m]
            full = t.permute(0, 1, 3, 2, 4, 5).reshape(j - i, self.nty * self.tile_h, self.ntx * self.tile_w, self.c)
            out[i:j].copy_(full[:, :self.h, :self.w])

    # ---- containers -----------------------------------------------------------------------------------------------------------
    def header(self):
        """the 24 header bytes of a single-frame container"""
        return bytes([0x9C, 1, self.c, (1 if self.planar else 0) | (2 if self.small_model else 0)]) + struct.pack(
            "<5I", self.w, self.h, self.tile_w, self.tile_h, self.slices_per_frame)

    def payload(self, sids, bank_bytes=None, off=None, ln=None):
        """the payload bytes of the slices `sids` back to back, by index arithmetic: numpy for numpy `sids`; for torch `sids` the stream
        bank arrays must be passed as torch tensors on the same device (stream_tensors)"""
        if isinstance(sids, np.ndarray):
            bank_bytes, off, ln = self.stream_bytes, self.stream_off, self.stream_len
            L, O = ln[sids], off[sids]
            n = int(L.sum())
            src = np.repeat(O - (np.cumsum(L) - L), L) + np.arange(n, dtype=np.int64)
            return bank_bytes[src]
        import torch

        L, O = ln[sids], off[sids]
        n = int(L.sum())
        src = torch.repeat_interleave(O - (torch.cumsum(L, 0) - L), L, output_size=n) + torch.arange(n, dtype=torch.int64, device=L.device)
        return bank_bytes[src]

    def stream_tensors(self, device):
        import torch

        return (torch.from_numpy(self.stream_bytes.copy()).to(device), torch.from_numpy(self.stream_off).to(device),
                torch.from_numpy(self.stream_len).to(device))

    def container(self, f):
        """the single-frame SLICED container of frame f (bytes)"""
        sids = self.stream_ids(f, f + 1)
        return self.header() + self.stream_len[sids].astype("<u4").tobytes() + self.payload(sids).tobytes()

    def payload_bytes(self, f0=0, f1=None):
        return int(self.stream_len[self.stream_ids(f0, f1)].sum())
