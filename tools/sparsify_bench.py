#!/usr/bin/env python3
"""The sparsified run at size: a synthetic PAF from the benchmark's generator (default 10^7 lines, 40 genomes),
`--sparsify tree:5:2:0.05`, default filter flags.  Two figures, the median of --runs runs each:

  stage   between "input parsed" and "filter starts", plus the filter call, through the library (ctypes):
            a build with swg_paf_tree_select:   swg_paf_tree_select, then swg_filter_subset (compaction inside)
            a build without (the parent commit): swg_paf_tree_filter + swg_paf_open_buffer, then swg_filter
          reported as select_ms (the stage proper) and select_plus_filter_ms (so that the compaction, which lives inside
          swg_filter_subset, is on the books of the new route)
  whole   the command line, file to file (wall time of the process)

Every step is a child process under its own time limit.  --lib / --cli point at another build of the library and the command
line (the parent commit's, built elsewhere); the default is this tree's.  One JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stage_child(lib_path, paf_path, kn, kf, rf):
    """One measurement inside a fresh process: prints a JSON object."""
    lib = C.CDLL(lib_path)
    sys.path.insert(0, ROOT)
    from sweepga_amd._lib import SwgConfig, SwgRecords, SwgStats
    ctx, paf = C.c_void_p(), C.c_void_p()
    lib.swg_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    assert lib.swg_create(0, C.byref(ctx)) == 0
    lib.swg_paf_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
    assert lib.swg_paf_open(paf_path.encode(), 16, C.byref(paf)) == 0
    lib.swg_paf_records.restype = C.POINTER(SwgRecords)
    lib.swg_paf_records.argtypes = [C.c_void_p]
    lib.swg_warmup.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int]
    n = int(lib.swg_paf_records(paf).contents.n)
    lib.swg_warmup(ctx, n, 4096, 1)
    cfg = SwgConfig(mapping_filter_mode=2, scaffold_filter_mode=2, overlap_threshold=0.95, scaffold_gap=50_000, min_scaffold_length=10_000,
                    scaffold_overlap_threshold=0.5, scaffold_max_deviation=0, scoring_function=3)   # the command line's defaults
    st = SwgStats()
    new = hasattr(lib, "swg_paf_tree_select")
    t0 = time.perf_counter()
    if new:
        keep = (C.c_uint8 * max(n, 1))()
        n_kept, route = C.c_uint64(), C.c_int()
        lib.swg_paf_tree_select.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_double, C.c_int, C.c_void_p,
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        assert lib.swg_paf_tree_select(ctx, paf, kn, kf, rf, 16, keep, C.byref(n_kept), C.byref(route)) == 0
        t1 = time.perf_counter()
        status, chain = (C.c_uint8 * max(n, 1))(), (C.c_uint32 * max(n, 1))()
        lib.swg_filter_subset.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.c_void_p, C.POINTER(SwgConfig), C.c_void_p, C.c_void_p, C.POINTER(SwgStats)]
        assert lib.swg_filter_subset(ctx, lib.swg_paf_records(paf), keep, C.byref(cfg), status, chain, C.byref(st)) == 0
        t2 = time.perf_counter()
        kept, how = n_kept.value, ("device mask" if route.value == 0 else "text fall-back")
    else:
        text, length, out, out_len = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        lib.swg_paf_text.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        lib.swg_paf_text(paf, C.byref(text), C.byref(length))
        lib.swg_paf_tree_filter.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        assert lib.swg_paf_tree_filter(text, length, kn, kf, rf, C.byref(out), C.byref(out_len)) == 0
        paf2 = C.c_void_p()
        lib.swg_paf_open_buffer.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]
        assert lib.swg_paf_open_buffer(out, out_len, 16, C.byref(paf2)) == 0
        t1 = time.perf_counter()
        r2 = lib.swg_paf_records(paf2)
        kept = int(r2.contents.n)
        status, chain = (C.c_uint8 * max(kept, 1))(), (C.c_uint32 * max(kept, 1))()
        lib.swg_filter.argtypes = [C.c_void_p, C.POINTER(SwgRecords), C.POINTER(SwgConfig), C.c_void_p, C.c_void_p, C.POINTER(SwgStats)]
        assert lib.swg_filter(ctx, r2, C.byref(cfg), status, chain, C.byref(st)) == 0
        t2 = time.perf_counter()
        how = "text, parsed again"
    print(json.dumps({"records": n, "kept_by_sparsification": kept, "n_out": int(st.n_out), "route": how,
                      "select_ms": (t1 - t0) * 1e3, "select_plus_filter_ms": (t2 - t0) * 1e3}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--genomes", type=int, default=40)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sparsify", default="tree:5:2:0.05")
    ap.add_argument("--lib", default=os.path.join(ROOT, "sweepga_amd", "libsweepga_gpu.so"))
    ap.add_argument("--cli", default=os.path.join(ROOT, "sweepga_amd", "bin", "sweepga-gpu"))
    ap.add_argument("--synth", default=os.path.join(ROOT, "sweepga_amd", "bin", "paf-synth"))
    ap.add_argument("--workdir", default="/tmp")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--stage-child", nargs=5, metavar=("LIB", "PAF", "NEAR", "FAR", "RANDOM"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.stage_child:
        lib, paf, kn, kf, rf = a.stage_child
        return stage_child(lib, paf, int(kn), int(kf), float(rf))
    paf = os.path.join(a.workdir, f"sparsify_bench_{a.lines}_{a.genomes}.paf")
    if not os.path.exists(paf):
        with open(paf + ".tmp", "wb") as f:
            subprocess.run([a.synth, str(a.lines), str(a.genomes), "2025", "150000000", "query"], stdout=f, check=True, timeout=a.step_timeout)
        os.replace(paf + ".tmp", paf)
    parts = a.sparsify.split(":")[1:]
    kn, kf, rf = parts[0], (parts[1] if len(parts) > 1 else "0"), (parts[2] if len(parts) > 2 else "0")
    out = paf + ".out"
    stage, whole = [], []
    for _ in range(a.runs):   # a failing or over-long step ends the script (check=True, timeout): nothing is started after it
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--stage-child", a.lib, paf, kn, kf, rf], capture_output=True,
                           text=True, check=True, timeout=a.step_timeout)
        stage.append(json.loads(r.stdout.strip().splitlines()[-1]))
        t0 = time.perf_counter()
        subprocess.run([a.cli, paf, "--sparsify", a.sparsify, "--output-file", out, "--quiet"], check=True, timeout=a.step_timeout)
        whole.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median
    print(json.dumps({"lines": a.lines, "genomes": a.genomes, "sparsify": a.sparsify, "runs": a.runs, "lib": a.lib,
                      "route": stage[0]["route"], "records": stage[0]["records"], "kept_by_sparsification": stage[0]["kept_by_sparsification"],
                      "n_out": stage[0]["n_out"], "output_bytes": os.path.getsize(out),
                      "select_ms_median": med(s["select_ms"] for s in stage), "select_ms": [round(s["select_ms"], 1) for s in stage],
                      "select_plus_filter_ms_median": med(s["select_plus_filter_ms"] for s in stage),
                      "whole_run_ms_median": med(whole), "whole_run_ms": [round(w, 1) for w in whole]}))


if __name__ == "__main__":
    main()
