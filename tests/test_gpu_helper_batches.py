"""k_pack_payload, k_stage_streams and k_model_rows_inv move their data in load batches (model_kernels.hip: BATCH chunks of
128 bytes of every stream of a lane group per memory round trip, the first batch of the pack kernel requested before the lengths
are known; the extra lanes of the row inverse in the batch of its rows).  What such a batch can get wrong is a stream length at or
next to a chunk or batch boundary, very unequal lengths inside one lane group, streams of many batches, narrow and partly live
groups, and the verdicts.  Encode checks go through Codec.encode and compare the slice table and the payload with the oracle's
sliced containers; decode checks go through Codec.decode of the ORACLE's table and payload and compare the pixels: the pack path
and the stage path are each checked against the reference, not against each other.  The assertions on the oracle's slice table
(test_cases_cover_the_boundaries) keep the coverage from silently going away when a generator changes."""
import numpy as np
import pytest
from conftest import make_image

pytestmark = pytest.mark.gpu

CHUNK = 128  # bytes of every stream per LDS tile (kChunkDwords * 4)
BATCH = 4    # chunks per load batch as shipped (LLMI_PACK_BATCH == LLMI_STAGE_BATCH)


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


def noise(seed, frames, w, h, c):
    return np.random.default_rng(seed).integers(0, 256, size=(frames, h, w, c), dtype=np.uint8)


def flat(frames, w, h, c, value=90):
    return np.full((frames, h, w, c), value, np.uint8)


def alternating(seed, frames, w, h, c):
    """noise and flat frames in turn: one lane group holds streams of a few bytes next to streams of several hundred"""
    imgs = noise(seed, frames, w, h, c)
    imgs[1::2] = 90
    return imgs


def generated(gen, frames, w, h, c):
    imgs = np.stack([make_image(gen, w, h, c) for _ in range(frames)])
    for i in range(frames):
        imgs[i] = np.roll(imgs[i], 11 * i, axis=1)
    return imgs


# name -> (images [frames][h][w][c], tile_w).  Noise codes to about 1.29 bytes per sample: tile widths near 100, 200, 400 and
# 800 put the stream lengths around 128, 256, 512 (the first batch boundary) and 1024 bytes (the second).
CASES = {
    # lengths at and around chunk and batch boundaries (seeds and widths chosen on the CPU, see test_cases_cover_the_boundaries)
    "chunk_128": lambda: (noise(1, 3, 297, 6, 3), 99),
    "chunk_256": lambda: (noise(2, 3, 597, 5, 3), 199),
    "batch_512": lambda: (noise(3, 4, 1191, 4, 3), 397),
    "batch_512_b": lambda: (noise(4, 3, 800, 8, 3), 398),
    "batch_1024": lambda: (noise(5, 3, 1590, 4, 3), 795),
    # ... and the longest stream of a group ending at, just before and just behind a chunk (256) and a batch boundary (512)
    "edge_256": lambda: (noise(1, 3, 544, 6, 3), 182),
    "edge_512": lambda: (noise(1, 3, 1114, 6, 3), 372),
    # very unequal lengths inside one lane group; all flat: max_len is tiny, most of the speculative first batch is dropped
    "unequal_400": lambda: (alternating(6, 12, 400, 4, 3), 400),
    "unequal_797": lambda: (alternating(7, 14, 797, 4, 3), 797),
    "all_flat": lambda: (flat(12, 400, 4, 3), 400),
    # many batches: streams of about 5 KB
    "many_batches": lambda: (noise(8, 2, 4000, 2, 1), 4000),
    # fewer than 64 slices in total (lane_shift < 6); 65 and 130 slices: the last group is partly live
    "narrow_30": lambda: (noise(9, 1, 250, 5, 3), 125),
    "narrow_3": lambda: (noise(10, 1, 401, 1, 3), 401),
    "ragged_65": lambda: (noise(11, 1, 1001, 13, 1), 201),
    "ragged_130": lambda: (noise(12, 1, 1983, 13, 2), 397),
    # row inverse: 1 to 4 channels, tile widths that are no multiple of 64 (the last 64-sample chunk partly filled), tiles whose
    # planes straddle two lane groups, and the last group of the batch, behind which no extra lanes exist
    "inv_c1": lambda: (generated("g3", 3, 700, 8, 1), 96),
    "inv_c2": lambda: (generated("mid", 2, 333, 7, 2), 65),
    "inv_c3": lambda: (generated("nat", 2, 1100, 6, 3), 480),
    "inv_c4": lambda: (generated("nat", 3, 250, 9, 4), 50),
    "straddle_c3_many_groups": lambda: (generated("mid", 3, 640, 40, 3), 32),
    "c4_straddle": lambda: (generated("g3", 2, 300, 30, 4), 20),
    "straddle_c3_noise": lambda: (noise(13, 2, 330, 43, 3), 110),
}
BOUNDARY_CASES = ["chunk_128", "chunk_256", "batch_512", "batch_512_b", "batch_1024", "edge_256", "edge_512"]
_ORACLE = {}


def oracle_case(orc, name):
    """(images, tile_w, the oracle's slice lengths, the oracle's payload) of a case: computed once, shared, left unchanged"""
    if name not in _ORACLE:
        imgs, tw = CASES[name]()
        lens, pays = [], []
        for img in imgs:
            d = orc.compress_sliced(np.ascontiguousarray(img), tw, 1, True)
            n = int.from_bytes(d[20:24], "little")
            lens.append(np.frombuffer(d[24:24 + 4 * n], dtype="<u4"))
            pays.append(d[24 + 4 * n:])
        lens = np.concatenate(lens)
        lens.setflags(write=False)
        imgs.setflags(write=False)
        _ORACLE[name] = (imgs, tw, lens, b"".join(pays))
    return _ORACLE[name]


def lane_groups(lens):
    """the slice lengths of every lane group: 64 consecutive slice ids (one narrower group when there are fewer in all)"""
    return [lens[i:i + 64] for i in range(0, len(lens), 64)]


def encode(mi, imgs, tw, cap=None, sentinel=None):
    """one Codec.encode of the batch -> (status, slice lengths, total, the whole payload buffer incl. what lies behind `cap`)"""
    import torch

    frames, h, w, c = imgs.shape
    k = mi.Codec(frames, w, h, c, tw, 1, True, device=0)
    try:
        assert k.family["rows"]
        cap = k.max_payload_bytes if cap is None else cap
        d_px = torch.from_numpy(np.array(imgs).reshape(-1)).cuda()  # (a copy: the shared case is read-only)
        d_pay = torch.full((cap + 4096,), 0 if sentinel is None else sentinel, dtype=torch.uint8, device="cuda")
        d_len = torch.zeros(k.n_slices, dtype=torch.int32, device="cuda")
        d_tot = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
        k.encode(d_px.data_ptr(), d_pay.data_ptr(), cap, d_len.data_ptr(), d_tot.data_ptr(), d_st.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return k.status(int(d_st.item()) & 0xFFFFFFFF), d_len.cpu().numpy().view(np.uint32), int(d_tot.item()), d_pay.cpu().numpy()
    finally:
        k.close()


class Decoder:
    """a Codec and the oracle's table and payload of one case in HBM; decode(payload_bytes) -> (status, pixels)"""

    def __init__(self, mi, imgs, tw, lens, pay):
        import torch

        self.shape = imgs.shape
        frames, h, w, c = imgs.shape
        self.k = mi.Codec(frames, w, h, c, tw, 1, True, device=0)
        assert self.k.family["rows"] and self.k.n_slices == len(lens)
        self.d_pay = torch.from_numpy(np.frombuffer(pay + bytes(16), dtype=np.uint8).copy()).cuda()
        self.d_len = torch.from_numpy(lens.view(np.int32).copy()).cuda()

    def decode(self, payload_bytes):
        import torch

        d_px = torch.full(self.shape, 0x5A, dtype=torch.uint8, device="cuda")
        d_st = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.k.decode(self.d_pay.data_ptr(), payload_bytes, self.d_len.data_ptr(), d_px.data_ptr(), d_st.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return self.k.status(int(d_st.item()) & 0xFFFFFFFF), d_px.cpu().numpy()

    def close(self):
        self.k.close()


@pytest.mark.parametrize("name", list(CASES))
def test_pack_equals_oracle(mi, orc, name):
    imgs, tw, want_lens, want_pay = oracle_case(orc, name)
    status, lens, total, buf = encode(mi, imgs, tw)
    assert status == mi.OK
    assert np.array_equal(lens, want_lens)
    assert total == len(want_pay)
    assert buf[:total].tobytes() == want_pay
    assert not buf[total:].any(), "nothing may be written behind the payload"


@pytest.mark.parametrize("name", list(CASES))
def test_stage_and_inverse_decode_the_oracles_container(mi, orc, name):
    imgs, tw, lens, pay = oracle_case(orc, name)
    d = Decoder(mi, imgs, tw, lens, pay)
    try:
        status, px = d.decode(len(pay))
        assert status == mi.OK
        assert np.array_equal(px, imgs)
    finally:
        d.close()


def test_cases_cover_the_boundaries(orc):
    """the oracle's slice tables of the boundary cases really hold what the batches can get wrong (checked on the CPU):
    in one lane group lengths on both sides of a chunk boundary and of a batch boundary; a group whose longest stream ends one to
    four bytes behind a chunk boundary (the last chunk holds one dword of it); and one whose longest stream ends at a chunk
    boundary or up to four bytes before it (there the zero dword that k_stage_streams stages behind every stream, its "+ 4",
    lies in a chunk, or a batch, that no stream reaches)"""
    both_sides_chunk = both_sides_batch = just_behind_a_chunk = ends_at_a_chunk = ends_at_a_batch = False
    for name in BOUNDARY_CASES:
        for grp in lane_groups(oracle_case(orc, name)[2]):
            lo, hi = int(grp.min()), int(grp.max())
            # a boundary b with lengths <= b and lengths > b in the same group
            both_sides_chunk |= any(lo <= b < hi for b in range(CHUNK, hi + 1, CHUNK) if b % (CHUNK * BATCH))
            both_sides_batch |= any(lo <= b < hi for b in range(CHUNK * BATCH, hi + 1, CHUNK * BATCH))
            just_behind_a_chunk |= 1 <= hi % CHUNK <= 4
            ends_at_a_chunk |= hi % CHUNK == 0 or hi % CHUNK >= CHUNK - 4
            ends_at_a_batch |= hi % (CHUNK * BATCH) == 0 or hi % (CHUNK * BATCH) >= CHUNK * BATCH - 4
    assert both_sides_chunk, "no group with lengths on both sides of a chunk boundary"
    assert both_sides_batch, "no group with lengths on both sides of a batch boundary"
    assert just_behind_a_chunk, "no group whose max_len mod 128 is in 1..4"
    assert ends_at_a_chunk, "no group whose max_len mod 128 is 0 or in 124..127"
    assert ends_at_a_batch, "no group whose max_len ends a batch"


def test_unequal_cases_are_unequal(orc):
    for name in ("unequal_400", "unequal_797"):
        groups = lane_groups(oracle_case(orc, name)[2])
        assert any(g.min() <= 16 and g.max() > 3 * CHUNK for g in groups), name  # (a flat stream: 7 to 9 bytes)
    assert oracle_case(orc, "all_flat")[2].max() <= 16
    assert oracle_case(orc, "many_batches")[2].min() > 8 * CHUNK * BATCH
    assert len(oracle_case(orc, "narrow_30")[2]) == 30 and len(oracle_case(orc, "narrow_3")[2]) == 3
    assert len(oracle_case(orc, "ragged_65")[2]) == 65 and len(oracle_case(orc, "ragged_130")[2]) == 130


def second_batch_cap(lens):
    """a payload capacity that ends inside the second load batch of a stream: (cap, the slice it cuts)"""
    offs = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
    for i, n in enumerate(lens):
        if n > CHUNK * BATCH + 100 and i >= 70:  # (not in the first group: the groups before it are written whole)
            return int(offs[i]) + CHUNK * BATCH + 77, i
    raise AssertionError("no stream reaches into its second batch")


@pytest.mark.parametrize("which", ["total_minus_1", "inside_second_batch"])
def test_overflow_verdict_and_nothing_behind_the_cap(mi, orc, which):
    imgs, tw, want_lens, want_pay = oracle_case(orc, "batch_1024")
    if which == "total_minus_1":
        cap, cut = len(want_pay) - 1, len(want_lens) - 1
    else:
        cap, cut = second_batch_cap(want_lens)
    status, lens, total, buf = encode(mi, imgs, tw, cap=cap, sentinel=0xAB)
    assert status == mi.OUTPUT_OVERFLOW
    assert np.array_equal(lens, want_lens) and total == len(want_pay)
    assert (buf[cap:] == 0xAB).all(), "nothing may be written past the caller's capacity"
    # a slice that would pass the capacity is not written; the slices in front of it are
    start = int(want_lens[:cut].astype(np.int64).sum())
    assert buf[:start].tobytes() == want_pay[:start]
    assert (buf[start:cap] == 0xAB).all()


def test_truncated_verdict_then_intact_decode(mi, orc):
    imgs, tw, lens, pay = oracle_case(orc, "batch_1024")
    inside = second_batch_cap(lens)[0]
    d = Decoder(mi, imgs, tw, lens, pay)
    try:
        for cut in (len(pay) - 1, inside):
            status, _ = d.decode(cut)
            assert status == mi.TRUNCATED, cut
        status, px = d.decode(len(pay))  # the same codec object, the intact container
        assert status == mi.OK
        assert np.array_equal(px, imgs)
    finally:
        d.close()
