"""The relay's peer transport on the GPU: the C ABI's exported pool, its mapping in a second process and the SDMA copy
(`sdy_relay_pool_create`, `sdy_ipc_open`, `sdy_copy_nocu`), then `tools/c4_rollout.py --transport peer` against the default
transport on ranks that share one device.  Every process here is a fresh child under a time limit; the test itself touches no
HIP."""
import hashlib
import json
import math
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FLOATS = 3 << 20          # a pool of three 4 MiB slots

_OWNER = r"""
import ctypes as C, os, sys, time
sys.path.insert(0, sys.argv[1])
import torch
import sdy_amd
from sdy_amd._lib import check, lib
d, n = sys.argv[2], int(sys.argv[3])
torch.cuda.set_device(0)
base, handle = C.c_void_p(), (C.c_ubyte * 64)()
check(lib.sdy_relay_pool_create(n // 3 * 4, 3, C.byref(base), handle), "sdy_relay_pool_create")
pattern = torch.arange(n, dtype=torch.float32, device="cuda") * 0.5 - 7.0
check(lib.sdy_copy_nocu(base.value, pattern.data_ptr(), n * 4, torch.cuda.current_stream().cuda_stream), "sdy_copy_nocu")
torch.cuda.synchronize()
with open(os.path.join(d, "handle.tmp"), "wb") as f:
    f.write(bytes(handle))
os.replace(os.path.join(d, "handle.tmp"), os.path.join(d, "handle"))
deadline = time.monotonic() + 120
while not os.path.exists(os.path.join(d, "closed")):
    if time.monotonic() > deadline:
        print("the opener never reported its mapping closed", flush=True)
        sys.exit(3)
    time.sleep(0.01)
check(lib.sdy_relay_pool_destroy(base.value), "sdy_relay_pool_destroy")
print("freed", flush=True)
"""

_OPENER = r"""
import ctypes as C, hashlib, os, sys, time
sys.path.insert(0, sys.argv[1])
import torch
import sdy_amd
from sdy_amd._lib import check, lib
d, n = sys.argv[2], int(sys.argv[3])
deadline = time.monotonic() + 120
while not os.path.exists(os.path.join(d, "handle")):
    if time.monotonic() > deadline:
        sys.exit(3)
    time.sleep(0.01)
handle = (C.c_ubyte * 64).from_buffer_copy(open(os.path.join(d, "handle"), "rb").read())
torch.cuda.set_device(0)
ptr = C.c_void_p()
rc = lib.sdy_ipc_open(handle, C.byref(ptr))
if rc != 0:
    open(os.path.join(d, "closed"), "w").close()          # nothing mapped: the owner may free
    print("OPEN_FAILED", rc, lib.sdy_error_string(rc).decode(), flush=True)
    sys.exit(2)
out = torch.empty(n, dtype=torch.float32, device="cuda")
side = torch.cuda.Stream()
check(lib.sdy_copy_nocu(out.data_ptr(), ptr.value, n * 4, side.cuda_stream), "sdy_copy_nocu")
side.synchronize()
check(lib.sdy_ipc_close(ptr.value), "sdy_ipc_close")
open(os.path.join(d, "closed"), "w").close()
print("sha256", hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest(), flush=True)
"""


def test_pool_exported_mapped_and_pulled_by_another_process(tmp_path):
    """One process creates a pool and fills it; a second one maps it, pulls it with sdy_copy_nocu, unmaps it and reports a
    checksum; the owner frees the pool only after that report."""
    results = {}

    def run(name, code):
        results[name] = subprocess.run([sys.executable, "-c", code, ROOT, str(tmp_path), str(N_FLOATS)], cwd=ROOT,
                                       capture_output=True, text=True, timeout=300)

    threads = [threading.Thread(target=run, args=("owner", _OWNER)), threading.Thread(target=run, args=("opener", _OPENER))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    owner, opener = results["owner"], results["opener"]
    assert opener.returncode == 0, f"opener rc {opener.returncode}: {opener.stdout[-2000:]} {opener.stderr[-2000:]}"
    assert owner.returncode == 0 and "freed" in owner.stdout, f"owner rc {owner.returncode}: {owner.stderr[-2000:]}"
    want = hashlib.sha256((np.arange(N_FLOATS, dtype=np.float32) * np.float32(0.5) - np.float32(7.0)).tobytes()).hexdigest()
    got = [ln.split()[1] for ln in opener.stdout.splitlines() if ln.startswith("sha256")]
    assert got == [want]


def _c4(steps, members, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "c4_rollout.py"), "--steps", str(steps), "--members", str(members),
           "--layers", "2", "--embed", "16", "--grid", "32", "64", *extra]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.parametrize("gpus,steps,members", [(2, 12, 5), (3, 18, 7)])
def test_c4_rollout_peer_transport_equals_the_default_one(gpus, steps, members):
    """`c4_rollout.py --gpus N --share-gpu --transport peer`: the relay trajectory's final carried state is the default
    transport's bit for bit, the time-mean statistics are the one-process run's, and the hand-over times are reported."""
    one = _c4(steps, members)
    default = _c4(steps, members, "--gpus", str(gpus), "--share-gpu", "--transport", "default")
    peer = _c4(steps, members, "--gpus", str(gpus), "--share-gpu", "--transport", "peer")
    assert default["relay"]["transport"] == "default" and peer["relay"]["transport"] == "peer"
    relayed = {str(u) for u in range(gpus * (members // gpus), members)}
    assert set(peer["relay"]["final_sha256"]) == relayed
    assert peer["relay"]["final_sha256"] == default["relay"]["final_sha256"]
    ref = one["time_mean_rmse_channel_mean"]
    for r in (default, peer):
        assert r["finite"] and r["n_gpus"] == gpus
        assert abs(ref - r["time_mean_rmse_channel_mean"]) < 2e-4 * ref
    ho = peer["relay"]["handover_ms"]
    assert ho["n"] == gpus - 1                        # one relayed trajectory, one hand-over per slice boundary
    assert math.isfinite(ho["median"]) and math.isfinite(ho["max"]) and 0.0 < ho["median"] <= ho["max"]
