"""On-device windows (swg_windows_records_device) timed over resident columns of the benchmark's shape -- bench.gen_shard: G
single-chromosome genomes, every ordered pair, pair-major -- under the status of ONE default-flags swg_filter_device call, and
over the same records and status under a random permutation.  From one run:
  (a) the whole call with both want bits (query axis, W = 10 k, any other genome) into arrays of the exact capacity, a host clock
      around calls that end in a device synchronise, warmed up, median of REPS;
  (b) the HIP-event split per kernel of one more call (the library's per-launch profile; memsets and read-backs between the
      launches carry no events, so the split sums to less than (a)), and the ratio of (a) to that sum;
  (c) as the yardstick, one swg_breadth_records_device call over the same columns -- the nearest existing report: one sort and one
      union walk per axis, both axes -- timed as (a), and the ratio of (a) to it;
  (d) the call on 4,096 records that all lie inside ONE window of one sequence (every update of the call meets on one address of
      each table), timed as (a).
Every sequence gets one length: the generator's chromosome length, or the largest end if the generator's rounding put one beyond it.
NOT measured: other window sizes, the target axis, a named other genome, the host seam.

    python tools/windows_bench.py [n_records] [n_genomes] [out.json] [commit]      -> one JSON line on standard output (and in out.json)
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
from sweepga_amd.breadth import _call as breadth_call  # noqa: E402
from sweepga_amd.windows import ANY, ROW_DTYPE, SEQ_DTYPE  # noqa: E402
from sweepga_amd.windows import _call as windows_call  # noqa: E402

REPS = 7
WINDOW = 10_000
OWN = ("windows_keys", "windows_counts", "windows_gather", "windows_walk", "windows_rows", "windows_seqs")
SCOPES = ("windows_sort",)   # brackets the whole sort: it overlaps the sort's own kernels


def timed(fn, sync, reps=REPS):
    sync()   # the library works on its own stream: torch's writes to the columns must be complete before it reads them
    fn()
    fn()   # warm: code objects, the arena at its final size
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return [round(x, 3) for x in (statistics.median(ts), min(ts), max(ts))]


def one_window(ctx, sync, device):
    """4,096 records of sequence 0 inside its window [10,000, 20,000), half of them kept; -> median, min, max in ms."""
    n = 4_096
    g = torch.Generator(device=device)
    g.manual_seed(5)
    a = 10_000 + torch.randint(0, 50, (n,), generator=g, device=device, dtype=torch.int32)
    cols = {"q_id": torch.zeros(n, dtype=torch.int32, device=device), "t_id": torch.ones(n, dtype=torch.int32, device=device), "q_start": a,
            "q_end": a + torch.randint(1, 50, (n,), generator=g, device=device, dtype=torch.int32),
            "matches": torch.randint(0, 1_000, (n,), generator=g, device=device, dtype=torch.int32)}
    status = (torch.arange(n, device=device) % 2).to(torch.uint8)
    seq_len = torch.tensor([40_000, 9], dtype=torch.int32, device=device)
    genome = torch.tensor([0, 1], dtype=torch.int32, device=device)
    rec = _lib.SwgRecords()
    rec.n, rec.n_seq = n, 2
    for k, t in cols.items():
        setattr(rec, k, t.data_ptr())
    req = _lib.SwgWindowsRequest()
    rows, seqs = np.zeros(4, dtype=ROW_DTYPE), np.zeros(1, dtype=SEQ_DTYPE)
    req.want, req.axis, req.window, req.other_genome = 3, 0, WINDOW, ANY
    req.capacity, req.rows = len(rows), C.cast(rows.ctypes.data, C.POINTER(_lib.SwgWindowRow))
    req.seq_capacity, req.seqs = len(seqs), C.cast(seqs.ctypes.data, C.POINTER(_lib.SwgWindowSeq))
    f = lambda: ctx.check(ctx.lib.swg_windows_records_device(ctx.handle, C.byref(rec), seq_len.data_ptr(), genome.data_ptr(), 2, status.data_ptr(), C.byref(req)))   # noqa: E731
    ms = timed(f, sync)
    assert rows["n"][:, 0].tolist() == [0, n, 0, 0] and rows["n"][:, 1].tolist() == [0, n // 2, 0, 0] and int(seqs["records"][0, 0]) == n
    return ms


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    if not torch.cuda.is_available():
        raise SystemExit("windows_bench: no GPU (there is no CPU path to time)")
    device = torch.device("cuda:0")
    ctx = sw.Context(0)
    cols, _ = bench.gen_shard(torch, n, G, 2025, device)
    sync = lambda: (torch.cuda.synchronize(), ctx.synchronize())   # noqa: E731
    out = {"n": n, "n_genomes": G, "reps": REPS, "axis": "query", "window": WINDOW, "other_genome": "any", "box": torch.cuda.get_device_name(0),
           "commit": sys.argv[4] if len(sys.argv) > 4 else None}
    out["one_window_4096_ms"] = one_window(ctx, sync, device)
    status = torch.zeros(n, dtype=torch.uint8, device=device)
    chain = torch.zeros(n, dtype=torch.int32, device=device)
    rec = bench.make_records(_lib, cols, n, G)
    n_seq = int(rec.n_seq)
    ccfg = sw.FilterConfig().to_c()
    filt = lambda: ctx.check(ctx.lib.swg_filter_device(ctx.handle, C.byref(rec), C.byref(ccfg), status.data_ptr(), chain.data_ptr(), None))   # noqa: E731
    out["filter_default_ms"] = timed(filt, sync)
    out["kept_records"] = int((status != 0).sum())
    del chain
    genome = cols["seq_genome_last"]
    length = max(150_000_000, int(cols["q_end"].max()), int(cols["t_end"].max()))
    out["seq_len"] = length
    seq_len = torch.full((n_seq,), length, dtype=torch.int32, device=device)

    def measure(c, st, tag):
        sync()   # the first call below comes before timed(): torch's writes to these columns (the shuffle) must be complete
        r = bench.make_records(_lib, c, n, G)
        first = windows_call(ctx, ctx.lib.swg_windows_records_device, r, seq_len.data_ptr(), genome.data_ptr(), G, st.data_ptr(), 0, WINDOW, None, None, 3)
        # what is timed is ONE library call into arrays of the exact capacity
        req = _lib.SwgWindowsRequest()
        rows, seqs = np.zeros(max(len(first.rows), 1), dtype=ROW_DTYPE), np.zeros(max(len(first.seqs), 1), dtype=SEQ_DTYPE)
        req.want, req.axis, req.window, req.other_genome = 3, 0, WINDOW, ANY
        req.capacity, req.rows = len(rows), C.cast(rows.ctypes.data, C.POINTER(_lib.SwgWindowRow))
        req.seq_capacity, req.seqs = len(seqs), C.cast(seqs.ctypes.data, C.POINTER(_lib.SwgWindowSeq))
        f = lambda: ctx.check(ctx.lib.swg_windows_records_device(ctx.handle, C.byref(r), seq_len.data_ptr(), genome.data_ptr(), G, st.data_ptr(), C.byref(req)))   # noqa: E731
        out[tag + "_windows"] = len(first.rows)
        out[tag + "_listed"] = len(first.seqs)
        out[tag + "_depth"] = [int(x) for x in first.seqs["depth"].sum(axis=0)]
        out[tag + "_covered"] = [int(x) for x in first.seqs["covered"].sum(axis=0)]
        out[tag + "_deepest_window"] = [int(x) for x in first.rows["n"].max(axis=0)]
        out[tag + "_ms"] = timed(f, sync)
        ctx.profile_reset()
        ctx.profile(True)
        f()
        ctx.profile(False)
        table = {name: round(v[1], 3) for name, v in ctx.profile_table().items()}
        out[tag + "_kernels_ms"] = table
        own = sum(v for name, v in table.items() if name in OWN)
        every = sum(v for name, v in table.items() if name not in SCOPES)
        out[tag + "_split_ms"] = {"windows_kernels": round(own, 3), "all_kernels": round(every, 3),
                                  "sorts_with_events_inside": round(sum(table.get(s, 0.0) for s in SCOPES), 3)}
        out[tag + "_call_over_kernels"] = round(out[tag + "_ms"][0] / every, 3) if every else None
        # (c): the breadth call over the same columns
        breadth = lambda: breadth_call(ctx, ctx.lib.swg_breadth_records_device, r, genome.data_ptr(), G, st.data_ptr())   # noqa: E731
        out[tag + "_breadth_call_ms"] = timed(breadth, sync)
        out[tag + "_call_over_breadth_call"] = round(out[tag + "_ms"][0] / out[tag + "_breadth_call_ms"][0], 3)
        return first

    a = measure(cols, status, "pair_major")
    perm = torch.randperm(n, device=device)
    shuf = {k: (cols[k][perm].contiguous() if k in bench.REC_COLS else cols[k]) for k in cols}
    st_sh = status[perm].contiguous()
    del perm, cols
    b = measure(shuf, st_sh, "shuffled")
    out["same_rows_both_orders"] = a.rows.tobytes() == b.rows.tobytes() and a.seqs.tobytes() == b.seqs.tobytes()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
