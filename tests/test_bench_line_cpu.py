"""bench.py's stdout line stays under 4 KB (the driver keeps an 8 KB tail; round 2's 20 KB line was cut and unparsable).
CPU checks: summary_line() over a committed full report of a 10^8-mapping run, and the files of --dump-outputs."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_summary_line_of_a_full_report_is_small():
    b = _bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r02_v3_bench_100m.json")))
    assert len(json.dumps(full)) > 8192   # the report that broke the driver's parse
    full["ms_per_step_unprofiled"] = full["ms_per_step"]
    line = b.summary_line(full, os.path.join(ROOT, "gpurun_out", "bench_detail.json"))
    text = json.dumps(line)
    assert len(text) < b.MAX_LINE_BYTES == 4096
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "cpu_baseline_all_cores", "parity_ok"):
        assert k in line, k
    assert line["value"] == round(full["value"], 4) and line["roofline"]["kernel"] == full["roofline"]["kernel"]
    assert line["roofline"]["frac"] == round(full["roofline"]["frac"], 5)
    assert set(line["config"]) <= {"workload", "flags", "mappings_per_gpu", "groups_per_gpu"} and "model" not in line["config"]
    assert line["sbig1_default_ms"] == round(full["sbig1"]["pipelines"]["default"]["ms_per_step"], 4)
    assert line["parity_ok"] is True and line["detail"] == "gpurun_out/bench_detail.json"


def test_summary_line_of_a_plain_report():
    """A run without --full reports the headline alone (the other legs are null in its report): the line keeps the contract keys
    and the headline's roofline, and has no key of a leg that did not run."""
    b = _bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r02_v3_bench_100m.json")))
    head = full["config"].get("pipeline") or "default"
    plain = dict(full, pipelines={head: dict(full["pipelines"][head], cpu_baseline=None, cpu_baseline_all_cores=None,
                                                    parity_vs_oracle_on_sample=None, parity_all_threads=None)},
                 ms_per_step_unprofiled=None, counts=None)
    for k in ("cpu_baseline", "cpu_baseline_all_cores", "parity_vs_oracle_on_sample", "parity_all_threads", "pcie_inclusive", "shapes",
              "sbig1", "end_to_end"):
        plain[k] = None
    line = json.loads(b.fit_line(b.summary_line(plain, None)))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline"):
        assert k in line, k
    assert line["value"] == round(full["value"], 4) and line["ms_per_step"] == round(full["ms_per_step"], 4)
    assert line["roofline"]["kernel"] == full["roofline"]["kernel"] and line["ms_per_step_unprofiled"] is None
    assert not [k for k in line if k.startswith(("sbig1_", "pcie_", "e2e_", "parity", "cpu_baseline")) or k.endswith("_pipeline_frac")]
    assert "truncated" not in line


def test_full_is_an_option_and_off_by_default():
    """`--full` exists (the help is printed without touching a GPU) and is a switch: a plain command line does not set it."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout
    assert "[--full]" in " ".join(r.stdout.split())   # takes no value


def test_line_degrades_instead_of_failing():
    """A report that outgrows the limit still yields ONE parsable line under it (optional keys go first, `truncated` says
    which) -- never an exception after a multi-minute run."""
    b = _bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r02_v3_bench_100m.json")))
    full["ms_per_step_unprofiled"] = full["ms_per_step"]
    line = b.summary_line(full, None)
    line["cpu_baseline"]["sample"] = "x" * 3000
    line["cpu_baseline_all_cores"]["sample"] = "y" * 3000
    line["config"]["workload"] = "w" * 3000
    text = b.fit_line(line)
    out = json.loads(text)
    assert len(text) < b.MAX_LINE_BYTES and out["truncated"]
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in out, k
    small = b.summary_line(full, None)
    assert "truncated" not in json.loads(b.fit_line(small))


def test_dump_outputs_is_float_bounded_and_the_same_sample_every_run(tmp_path):
    """--dump-outputs: every record of a small record set; a fixed sample (the same indices on every call) of a large one, under
    64 MB in all; float32 / float64 files holding the exact status and chain values (chain numbers are u32 in the ABI)."""
    import numpy as np
    import torch
    b = _bench()
    n = 1000
    status = torch.arange(n, dtype=torch.int32).remainder(7).to(torch.uint8)
    chain = torch.arange(n, dtype=torch.int32) * 3
    chain[5] = -1   # 2^32 - 1 as the library's u32
    d = b.dump_outputs(str(tmp_path / "small"), status, chain, n)
    assert d["dumped"] == n and d["sampled"] is False
    got = {k: np.load(tmp_path / "small" / f"{k}.npy") for k in ("index", "status", "chain")}
    assert got["index"].dtype == np.float64 and got["status"].dtype == np.float32 and got["chain"].dtype == np.float64
    assert np.array_equal(got["index"], np.arange(n)) and np.array_equal(got["status"], np.arange(n) % 7)
    assert got["chain"][5] == 2**32 - 1 and np.array_equal(np.delete(got["chain"], 5), np.delete(np.arange(n) * 3, 5))

    n = b.DUMP_RECORDS_MAX + 12_345
    status = torch.arange(n, dtype=torch.int64).remainder(5).to(torch.uint8)
    chain = torch.arange(n, dtype=torch.int32)
    runs = []
    for k in range(2):
        d = b.dump_outputs(str(tmp_path / f"big{k}"), status, chain, n)
        assert d["dumped"] == b.DUMP_RECORDS_MAX and d["sampled"] is True
        files = [tmp_path / f"big{k}" / f"{x}.npy" for x in ("index", "status", "chain")]
        assert sum(os.path.getsize(f) for f in files) < 64 << 20
        runs.append([np.load(f) for f in files])
    idx, st, ch = runs[0]
    assert np.array_equal(idx, runs[1][0]) and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(st, idx % 5) and np.array_equal(ch, idx)
