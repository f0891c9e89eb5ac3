"""On-device alnstats (swg_alnstats_records_device) timed over resident columns of the benchmark's shape -- bench.gen_shard:
G single-chromosome genomes, every ordered pair, pair-major -- and over the same records shuffled, against
  (a) the host path, swg_alnstats_open_buffer with 16 threads, over the first N_HOST of those records as PAF text
      (reported per record: the text of 10^8 records does not fit a tool run), and
  (b) one `prepare` pass of the filter over the same columns in the same run (the streaming pass the `sweep` pipeline,
      --num-mappings 1:1 --scaffold-jump 0, starts with; the default pipeline's pair-resident path has no such pass).
Times: a host clock around calls that end in a device synchronise, warmed up, median of REPS; the per-kernel split comes from
the library's HIP-event profile in a run of its own after the timed ones.

    python tools/alnstats_bench.py [n_records] [n_genomes] [n_host_records]      -> one JSON line on standard output
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import sweepga_amd as sw  # noqa: E402
from sweepga_amd import _lib  # noqa: E402
from sweepga_amd.alnstats import AlnStats, alnstats_counts  # noqa: E402

REPS = 7


def timed(fn, sync):
    sync()   # the library works on its own stream: torch's writes to the columns must be complete before it reads them
    fn()
    fn()   # warm: code objects, the arena at its final size
    ts = []
    for _ in range(REPS):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    n_host = int(sys.argv[3]) if len(sys.argv) > 3 else 2_000_000
    if not torch.cuda.is_available():
        raise SystemExit("alnstats_bench: no GPU (there is no CPU path to time)")
    device = torch.device("cuda:0")
    ctx = sw.Context(0)
    cols, _ = bench.gen_shard(torch, n, G, 2025, device)
    status = (torch.rand(n, device=device) < 0.3).to(torch.uint8)
    out = {"n": n, "n_genomes": G, "reps": REPS}

    def device_stats(c, st):
        rec = bench.make_records(_lib, c, n, G)
        return lambda: alnstats_counts(ctx, rec, c["seq_genome_last"].data_ptr(), G, st.data_ptr(), device=True)

    def kernel_split(fn):
        ctx.profile_reset()
        ctx.profile(True)
        fn()
        ctx.profile(False)
        return {k: round(v[1], 3) for k, v in ctx.profile_table().items()}

    sync = lambda: (torch.cuda.synchronize(), ctx.synchronize())   # noqa: E731
    f = device_stats(cols, status)
    out["pair_major_ms"] = [round(x, 3) for x in timed(f, sync)]
    out["pair_major_kernels_ms"] = kernel_split(f)

    # (b) the filter's first streaming pass over the same columns
    rec = bench.make_records(_lib, cols, n, G)
    ccfg = bench.make_config(sw, "sweep").to_c()
    st_out = torch.zeros(n, dtype=torch.uint8, device=device)
    ch_out = torch.zeros(n, dtype=torch.int32, device=device)
    run_filter = lambda: ctx.check(ctx.lib.swg_filter_device(ctx.handle, C.byref(rec), C.byref(ccfg), st_out.data_ptr(), ch_out.data_ptr(), None))   # noqa: E731
    run_filter()
    ctx.profile_select("prepare")
    ctx.profile_reset()
    ctx.profile(True)
    for _ in range(3):
        run_filter()
    ctx.profile(False)
    launches, ms = ctx.profile_table()["prepare"]
    ctx.profile_select(None)
    out["prepare_pass_ms"] = round(ms / launches, 3)
    # the statistics on the status the filter left (what --stats computes)
    f2 = device_stats(cols, st_out)
    out["pair_major_filter_status_ms"] = [round(x, 3) for x in timed(f2, sync)]
    del st_out, ch_out

    perm = torch.randperm(n, device=device)
    shuf = {k: (cols[k][perm].contiguous() if k in bench.REC_COLS else cols[k]) for k in cols}
    st_sh = status[perm].contiguous()
    del perm
    f3 = device_stats(shuf, st_sh)
    out["shuffled_ms"] = [round(x, 3) for x in timed(f3, sync)]
    out["shuffled_kernels_ms"] = kernel_split(f3)

    # (a) the host path over the first n_host records as text, 16 threads
    m = min(n, n_host)
    h = {k: cols[k][:m].cpu().numpy() for k in ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end", "matches", "block_len")}
    names = bench.span_names(G)
    lines = ["%s\t150000000\t%d\t%d\t+\t%s\t150000000\t%d\t%d\t%d\t%d\t60" % (names[q], a, b, names[t], c, d, mm, bl)
             for q, t, a, b, c, d, mm, bl in zip(*(h[k].tolist() for k in h))]
    text = ("\n".join(lines) + "\n").encode()
    del lines
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        s = AlnStats(text=text, threads=16)
        ts.append((time.perf_counter() - t0) * 1e3)
        s.close()
    out["host_16_threads"] = {"records": m, "text_bytes": len(text), "ms": round(min(ts), 3), "ns_per_record": round(min(ts) * 1e6 / m, 2)}
    out["device_ns_per_record"] = {"pair_major": round(out["pair_major_ms"][0] * 1e6 / n, 3), "shuffled": round(out["shuffled_ms"][0] * 1e6 / n, 3)}
    out["pair_major_over_prepare"] = round(out["pair_major_ms"][0] / out["prepare_pass_ms"], 2)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    np.seterr(all="raise")
    main()
