"""What the tests of the three batch calls share (mix_batch, orient_batch, compose_batch; test_gpu_batch_chain.py runs them together): the
element types, batches of arbitrary bit patterns, and a batch in device memory between guard bytes.  It calls nothing of the library
but device_count() in the fixture."""
import numpy as np
import pytest

DTYPES = ("uint8", "float32", "float16", "bfloat16")
ESIZE = {"uint8": 1, "float32": 4, "float16": 2, "bfloat16": 2}
NP_NAME = {"uint8": np.uint8, "float32": np.float32, "float16": np.float16, "bfloat16": np.uint16}
BITS = {1: np.uint8, 2: np.uint16, 4: np.uint32}
GUARD = 256


def gen_batch(dtype, n, c, h, w, layout, seed):
    """arbitrary bit patterns -- NaNs with payloads, infinities, negative zeros and subnormals among them -- as the numpy type the
    library takes for the dtype (bfloat16: uint16)"""
    t = np.dtype(NP_NAME[dtype])
    shape = (n, c, h, w) if layout == "chw" else (n, h, w, c)
    raw = np.random.default_rng(seed).integers(0, 256, size=int(np.prod(shape)) * t.itemsize, dtype=np.uint8)
    return raw.view(t).reshape(shape)


def bits_of(a):
    """an array of any of the four element types -> its bit patterns (a NaN compares equal to itself there)"""
    a = np.ascontiguousarray(a)
    return a.view(BITS[a.itemsize])


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def put(batch, offset_bytes):
    """the numpy batch in a device buffer, offset_bytes past a 256-byte boundary behind GUARD bytes of 0x5A, GUARD more behind it
    -> (the buffer, the batch's offset in it)"""
    import torch

    lo = GUARD + offset_bytes
    buf = torch.full((lo + batch.nbytes + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    if batch.nbytes:
        buf[lo:lo + batch.nbytes] = torch.from_numpy(np.ascontiguousarray(batch).reshape(-1).view(np.uint8).copy()).cuda()
    return buf, lo


def guards_intact(buf, lo, nbytes):
    """every byte of put()'s buffer -- or of its copy on the host -- outside the batch's nbytes at lo is still 0x5A"""
    host = buf.cpu().numpy() if hasattr(buf, "cpu") else buf
    return bool((host[:lo] == 0x5A).all() and (host[lo + nbytes:] == 0x5A).all())
