"""On-device intervals (swg_intervals_records_device) timed over resident columns of the benchmark's shape -- bench.gen_shard: G
single-chromosome genomes, every ordered pair, pair-major -- and over the same records shuffled.  Four numbers from one run:
  (a) the whole call wanting all six lists, rows fetched into arrays of the exact capacity (sized by one call before the
      clock starts), a host clock around calls that end in a device synchronise, warmed up, median of REPS;
  (b) the same call wanting LOST on the query axis only;
  (c) the HIP-event split per kernel of one more call of (a) (the library's per-launch profile; memsets, read-backs and row
      copies between the launches carry no events, so the split sums to less than (a));
  (d) one swg_breadth_records_device call over the same columns and status, timed as (a): the yardstick -- the same two sorts
      and one pass less per axis, and it exists on the commit before this feature.

    python tools/intervals_bench.py [n_records] [n_genomes]      -> one JSON line on standard output
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
from sweepga_amd.intervals import INTERVAL_DTYPE  # noqa: E402

REPS = 7
OWN = ("intervals_keys", "intervals_gather", "intervals_count", "intervals_write", "intervals_lost_flags", "intervals_lost_write",
       "intervals_bases")
SORT_SCOPES = ("intervals_sort_q", "intervals_sort_t")   # each brackets its axis' whole sort: they overlap the sort's own kernels


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
    return [round(x, 3) for x in (statistics.median(ts), min(ts), max(ts))]


def sized_request(ctx, rec, genome, G, status_addr, want):
    """A request whose row arrays have exactly the capacity the input needs (one call with capacity 0 says how much)."""
    req = _lib.SwgIntervalRequest()
    req.want = want
    ctx.check(ctx.lib.swg_intervals_records_device(ctx.handle, C.byref(rec), genome, C.c_uint32(G), status_addr, C.byref(req)))
    keep = []
    for s in range(3):
        for a in range(2):
            if want >> (2 * s + a) & 1:
                rows = np.zeros(max(int(req.list[s][a].n), 1), dtype=INTERVAL_DTYPE)
                keep.append(rows)
                req.list[s][a].capacity = int(req.list[s][a].n)
                req.list[s][a].rows = C.cast(rows.ctypes.data, C.POINTER(_lib.SwgInterval))
    return req, keep


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    if not torch.cuda.is_available():
        raise SystemExit("intervals_bench: no GPU (there is no CPU path to time)")
    device = torch.device("cuda:0")
    ctx = sw.Context(0)
    cols, _ = bench.gen_shard(torch, n, G, 2025, device)
    status = (torch.rand(n, device=device) < 0.3).to(torch.uint8)
    sync = lambda: (torch.cuda.synchronize(), ctx.synchronize())   # noqa: E731
    out = {"n": n, "n_genomes": G, "reps": REPS}

    def measure(c, st, tag):
        sync()   # the first call below comes before timed(): torch's writes to these columns (the shuffle) must be complete
        rec = bench.make_records(_lib, c, n, G)
        genome = c["seq_genome_last"].data_ptr()
        for name, want in (("all_six", 0x3f), ("lost_q", 1 << 4)):
            req, keep = sized_request(ctx, rec, genome, G, st.data_ptr(), want)
            f = lambda: ctx.check(ctx.lib.swg_intervals_records_device(ctx.handle, C.byref(rec), genome, C.c_uint32(G), st.data_ptr(),   # noqa: E731
                                                                      C.byref(req)))
            out[f"{tag}_{name}_ms"] = timed(f, sync)
            if want == 0x3f:
                out[tag + "_intervals"] = {"%s_%s" % (sw.intervals.SETS[s], sw.intervals.AXES[a]): int(req.list[s][a].n) for s in range(3) for a in range(2)}
                out[tag + "_bases"] = {"%s_%s" % (sw.intervals.SETS[s], sw.intervals.AXES[a]): int(req.list[s][a].bases) for s in range(3) for a in range(2)}
                ctx.profile_reset()
                ctx.profile(True)
                f()
                ctx.profile(False)
                table = {k: round(v[1], 3) for k, v in ctx.profile_table().items()}
                out[tag + "_kernels_ms"] = table
                out[tag + "_split_ms"] = {"intervals_kernels": round(sum(v for k, v in table.items() if k in OWN), 3),
                                          "scans": round(sum(v for k, v in table.items() if k.startswith("scan_")), 3),
                                          "sorts_with_events_inside": round(sum(table.get(s, 0.0) for s in SORT_SCOPES), 3)}
            del keep
        g = lambda: breadth_call(ctx, ctx.lib.swg_breadth_records_device, rec, genome, G, st.data_ptr())   # noqa: E731
        out[tag + "_breadth_ms"] = timed(g, sync)
        out[tag + "_all_six_over_breadth"] = round(out[tag + "_all_six_ms"][0] / out[tag + "_breadth_ms"][0], 3)
        out[tag + "_lost_q_over_breadth"] = round(out[tag + "_lost_q_ms"][0] / out[tag + "_breadth_ms"][0], 3)

    measure(cols, status, "pair_major")
    perm = torch.randperm(n, device=device)
    shuf = {k: (cols[k][perm].contiguous() if k in bench.REC_COLS else cols[k]) for k in cols}
    st_sh = status[perm].contiguous()
    del perm, cols
    measure(shuf, st_sh, "shuffled")
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
