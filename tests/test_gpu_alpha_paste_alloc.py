"""The batch alpha paste under a failed allocation (llcomp_mi_codec_alpha_paste_batch), with the contract and the guard build of
tests/test_gpu_alloc_failures.py: every allocation request of a call fails in turn; the status is NOMEM before anything is queued or
written, the codec object's invariants hold and it stays usable, allocated_bytes stays true, the same call with the injection off gives
the dry pass's bytes -- which are the spec's -- and closing leaves no block live.  One child process
(tests/helpers/alpha_paste_alloc_child.py) sweeps every case: the call alone, behind a call with a smaller table, and with OVER pieces
on an RGBA batch that is its own alpha.

Nothing here shows a fault on the GPU: the injector fails allocations on the host, and a broken invariant is a failed assertion."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CHILD = os.path.join(ROOT, "tests", "helpers", "alpha_paste_alloc_child.py")
LIB = os.path.join(ROOT, "llcomp_amd", "libllcomp_mi_failalloc.so")
CASES = ["alpha_paste_batch", "alpha_paste_batch,second", "alpha_paste_batch,over"]


def test_every_request_of_the_alpha_paste_fails_cleanly():
    import llcomp_amd

    assert llcomp_amd.device_count() >= 1, "GPU tests need a HIP device"
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} missing: run `make -C llcomp_amd/csrc guards` (or __graft_entry__.build())")
    env = dict(os.environ, LLCOMP_MI_LIB=LIB)
    for hook in ("LLCOMP_MI_LANE_SHIFT", "LLCOMP_MI_OVERLAP"):
        env.pop(hook, None)
    r = subprocess.run([sys.executable, CHILD], capture_output=True, text=True, env=env, timeout=120)
    # (a child that ends abnormally ends the test here: nothing further is started on the GPU)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert sorted(got) == sorted(CASES), f"not swept: {sorted(set(CASES) - set(got))}"
    print("\n" + "\n".join(f"ALLOC {name}: R={v['R']}" for name, v in got.items()))
    assert not any(v.get("optional") for v in got.values()), "no request of this call is optional"
    failed = {name: v["failed"] for name, v in got.items() if v["failed"]}
    assert not failed, json.dumps(failed, indent=1)
    vacuous = [name for name, v in got.items() if v["R"] == 0]
    assert not vacuous, f"no allocation request in the dry pass of {vacuous}"
