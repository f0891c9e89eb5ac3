"""The ranged filter's host planning (sweepga_amd/csrc/host/range_plan.h) without a GPU: tests/native/range_plan_check.cpp packs
genome pairs into ranges (first-record order, pairs larger than the range size alone, 2^31-record pairs refused), computes the
chain-number shifts (kept chains numbered pair by pair in order of first retained record, numbers of 2^32 refused) and the
largest range a byte budget holds."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_range_plan_rules(tmp_path):
    exe = str(tmp_path / "range_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "range_plan_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"ok": True, "failures": 0}
