"""The ranged filter beyond 2^31 records: n = 2^31 + 2^26 records (S-pan shape, 9,900 genome pairs) generated on the device,
pair-major and shuffled, the sweep flags and the CLI defaults.  swg_filter_device and swg_filter are two independent ranged
implementations (device plan, slices or gathered ranges, renumbering on the device / host genome-pair plan, pinned-ring
gather, renumbering on host threads) and must agree record for record; the kept chains of every pair are contiguous, run from 1
with no gaps and follow the pairs' first retained records; 8 sampled genome pairs match the oracle run on each pair alone
(status exact, chain numbers up to one shift per pair).  Runs in a fresh process (tests/ranged_big_check.py); about 3.5 minutes
on one MI355X (211 s measured, the four cases together).

Memory need, derived from the layouts (not measured): device 2.2e9 records x 33 bytes of columns = 73 GB, plus a shuffled copy
being built (another 73 GB at the peak of the permutation), the status / chain outputs (11 GB) and the ranges' scratch, which
the ranged path sizes to what is free; host 73 GB for the host copy of the columns plus two sets of outputs (2 x 11 GB) and the
host path's pair ids (9 GB): about 105 GB -- skipped only below that much MemAvailable."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_NEED = 105 << 30


def _mem_available():
    with open("/proc/meminfo") as f:
        for line in f:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    return 0


def test_more_than_2_31_records():
    avail = _mem_available()
    if avail < HOST_NEED:
        pytest.skip(f"needs about {HOST_NEED >> 30} GB of host memory, {avail >> 30} GB available")
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ranged_big_check.py")], cwd=ROOT, capture_output=True,
                       text=True, timeout=3600, env={**os.environ, "PYTHONPATH": ROOT})
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-4000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"2^31 + 2^26 records: wall {wall:.0f} s", json.dumps(d))
    assert d["n"] == 2**31 + 2**26
    assert set(d["cases"]) == {f"{o}/{p}" for o in ("pair_major", "shuffled") for p in ("sweep", "default")}
    for name, c in d["cases"].items():
        assert c["device_equals_host"], name
        assert c["numbering_ok"], name
        assert c["sampled_bad"] == [] and len(c["sampled_pairs"]) == 8, (name, c["sampled_bad"])
        assert c["n_out"] > 0, name
