"""Every entry point under a failed allocation (include/llcomp_mi.h, LLCOMP_MI_NOMEM: returned before anything is queued or written, the
object stays usable, allocated_bytes stays true, nothing leaks).  The guard build libllcomp_mi_failalloc.so (`make -C llcomp_amd/csrc
guards`, built by __graft_entry__.build()) numbers every device and pinned allocation request of the library and fails the ones it is
told to, on the host, without touching the driver; tests/helpers/alloc_failure_child.py sweeps one group of entry points per child
process: per case a dry pass counts the call's requests R, then EVERY request 0..R-1 fails alone, then requests 0.. and R // 2.. fail.

After every failure: the status is NOMEM (DEVICE_FAILED with NOMEM behind it over a device list), every output byte, status word and
guard byte is as it was, llmi_test_codec_consistent finds the codec object's invariants whole -- only then is the object called again --
the live device bytes moved as allocated_bytes did, the same call with the injection off gives the dry pass's bytes (the oracle's
container for encodes, the source pixels for decodes and regions), and closing the codec leaves no block live.

Measured on an MI355X (pytest --durations): a test function, which is one child, takes 4.5 to 5.7 s of wall time, the interpreter's
start and the oracle's containers included (the two windows groups 5.7 and 5.0 s, regrow 5.2 s); whichever child runs first in a
session also pays the cold start of the GPU runtime, 12.5 to 14 s measured.  The time limit of a child is 120 s.

Nothing here shows a fault on the GPU: the injector fails allocations on the host, and a broken invariant is a failed assertion, never a
kernel launched on a null pointer."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CHILD = os.path.join(ROOT, "tests", "helpers", "alloc_failure_child.py")
LIB = os.path.join(ROOT, "llcomp_amd", "libllcomp_mi_failalloc.so")

# Requests whose failure a call swallows by design: the call returns OK with exactly the dry pass's bytes.  The child reports the ordinals
# it treated as optional per case, and they have to be exactly these; a request that is not listed and gets swallowed fails its case.
#   - the 2-D decoder's 16-byte feedback mailbox (codec.hip: queue_feedback), the LAST request of the first decode that runs with the bank
#     cache: without it the cache stays on in every launch.  Cases: decode@hbm_bank_cache_32x32i, and any decode / decode_region case
#     whose (sub-)geometry reports bank_cache.
#   - the events of the chunked encoder's second stream (codec.hip: ensure_snapshot_arrays; their failure sets overlap = false) are no
#     allocation requests: event creation is not injected, so no ordinal stands for them.
MAILBOX = [1]  # (behind the state tables, request 0)
OPTIONAL = {"decode@hbm_bank_cache_32x32i": MAILBOX, "decode@snapshot_64x64p": MAILBOX,
            **{f"decode@{f},overlap={o}": MAILBOX for f in ("chunked_128x48p", "chunked_64x64i") for o in ("unset", "0", "1")}}

# Cases whose call makes no allocation request at all, by name, with the reason; any other case with R = 0 is vacuous and fails.
ON_CHIP = "the family keeps its state tables on chip and runs no snapshot pass: the codec is complete when it is created"
NO_REQUEST = {
    "label_boxes": "keeps no table of its own: the codec only names the device",
    "encode@rows_fused_100x6_50x1p": ON_CHIP, "decode@rows_fused_100x6_50x1p": ON_CHIP,
    "encode@rows_interleaved_100x6_32x1i": ON_CHIP, "decode@rows_interleaved_100x6_32x1i": ON_CHIP,
    "encode@lds_table_200x150_64x64i": ON_CHIP, "decode@lds_table_200x150_64x64i": ON_CHIP,
}

# Calls of the windows groups that have no second-call case, by name, with the reason: nothing of theirs grows with the call's size.
# Every other call of WINDOWED has to come back from the child with a ",second" case too (checked below).
NO_SECOND = {
    "decode_region": "its two arrays are sized by the codec's slices when the first call makes them",
    "decode_regions": "from device memory only the per-frame table crosses, sized by the codec's frames",
}

# group (one child process each) -> the calls it has to have swept, so that a case cannot drop out of the child unnoticed
WINDOWED = ["decode_region", "encode_region", "update_region", "decode_regions", "decode_regions_host", "decode_resized_regions", "decode_resized_regions_ex", "decode_resized_regions_host", "decode_padded_regions", "decode_views", "decode_views_host", "decode_warped_views", "decode_perspective_views", "decode_photo_views", "encode_region,second", "update_region,second", "decode_regions_host,second", "decode_resized_regions,second", "decode_resized_regions_ex,second", "decode_resized_regions_host,second", "decode_padded_regions,second", "decode_views,second", "decode_views_host,second", "decode_warped_views,second", "decode_perspective_views,second", "decode_photo_views,second"]
GROUPS = {
    "core": ["codec_create_ex"] + [f"prepare({f})" for f in ("encode", "decode", "region", "regions", "resized", "update", "views", "all")],
    "families": [f"{d}@{f}" for f in ("rows_fused_100x6_50x1p", "rows_interleaved_100x6_32x1i", "lds_table_200x150_64x64i", "hbm_bank_cache_32x32i",
                                      "snapshot_64x64p") for d in ("encode", "decode")],
    "chunked": [f"{d}@{f},overlap={o}" for f in ("chunked_128x48p", "chunked_64x64i") for o in ("unset", "0", "1") for d in ("encode", "decode")],
    "windows_100x44_32x16i": WINDOWED,
    "windows_100x6_50x1p": WINDOWED,
    "regrow": [f"{d}{s}@regrow_404x328_400x40p" for d in ("encode_region", "update_region") for s in ("", ",second")],
    "switch": [f"{d}@160x41_40x2{p}" for p in "pi" for d in ("decode_region", "encode_region", "update_region")],
    "batch": [f"{b}{s}" for b in ("mix_batch", "orient_batch", "compose_batch", "paste_batch", "paste_batch16", "label_boxes16", "label_targets")
              for s in ("", ",second")] + ["mix_batch,long_cycle", "label_boxes"],
    "host": ["llcomp_mi_encode,sliced", "llcomp_mi_encode,legacy", "llcomp_mi_decode,sliced", "llcomp_mi_decode,legacy", "llcomp_mi_decode_region",
             "llcomp_mi_update_region", "llcomp_mi_host_alloc", "llcomp_mi_stream_create", "llcomp_mi_stream_create_multi", "llcomp_mi_stream_submit_encode"],
    "devices": ["llcomp_mi_encode,devices", "llcomp_mi_decode,devices"],
    "pool": ["pool_pressure"],
}


@pytest.fixture(scope="module")
def mi():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    return llcomp_amd


def run_child(group):
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} missing: run `make -C llcomp_amd/csrc guards` (or __graft_entry__.build())")
    env = dict(os.environ, LLCOMP_MI_LIB=LIB)
    for hook in ("LLCOMP_MI_LANE_SHIFT", "LLCOMP_MI_OVERLAP"):  # (the child sets the hooks its cases name)
        env.pop(hook, None)
    r = subprocess.run([sys.executable, CHILD, group], capture_output=True, text=True, env=env, timeout=120)
    # (a child that ends abnormally ends its test here: nothing further is started on the GPU)
    assert r.returncode == 0, f"{group}: rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("group", list(GROUPS))
def test_every_request_of_every_call_fails_cleanly(mi, group):
    got = run_child(group)
    missing = [c for c in GROUPS[group] if not any(name == c or name.startswith(c + "@") for name in got)]
    assert not missing, f"{group}: not swept: {missing}"
    if GROUPS[group] is WINDOWED:
        calls = {name.split("@")[0] for name in got}
        alone = [c for c in calls if "," not in c and c + ",second" not in calls and c not in NO_SECOND]
        assert not alone, f"{group}: no second call that grows a buffer, and no reason listed, for {alone}"
    print("\n" + "\n".join(f"ALLOC {group} {name}: R={v['R']}" for name, v in got.items()))
    optional = {name: v["optional"] for name, v in got.items() if v.get("optional")}
    assert optional == {name: o for name, o in OPTIONAL.items() if name in got}, f"{group}: requests treated as optional: {optional}"
    vacuous = [name for name, v in got.items() if v["R"] == 0 and name not in NO_REQUEST]
    assert not vacuous, f"no allocation request in the dry pass of {vacuous}"
    failed = {name: v["failed"] for name, v in got.items() if v["failed"]}
    assert not failed, json.dumps(failed, indent=1)
