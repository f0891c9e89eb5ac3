"""On-device breadth (swg_breadth_records_device) timed over resident columns of the benchmark's shape -- bench.gen_shard: G
single-chromosome genomes, every ordered pair, pair-major -- and over the same records shuffled.  Four numbers from one run:
  (a) the whole call (ALL + KEPT), a host clock around calls that end in a device synchronise, warmed up, median of REPS;
  (b) the HIP-event split per kernel of one more call (the library's per-launch profile; memsets and read-backs between the
      launches carry no events, so the split sums to less than (a));
  (c) the library's radix sort of the call's own (key, index) pairs alone, per axis: HIP events around the one
      swg_radix_sort_pairs call of the axis and around nothing else (profile entries `breadth_sort_q`, `breadth_sort_t`,
      selected one at a time so that no other event is recorded in the call), median of REPS calls -- existing code, the floor;
  (d) one swg_alnstats_records_device call over the same columns and status, timed as (a).

    python tools/breadth_bench.py [n_records] [n_genomes]      -> one JSON line on standard output
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
import sweepga_amd as sw  # noqa: E402
from sweepga_amd import _lib  # noqa: E402
from sweepga_amd.alnstats import alnstats_counts  # noqa: E402
from sweepga_amd.breadth import _call  # noqa: E402

REPS = 7
OWN = ("breadth_keys", "breadth_gather", "breadth_union", "breadth_collect")
SORT_SCOPES = ("breadth_sort_q", "breadth_sort_t")   # each brackets its axis' whole sort: they overlap the sort's own kernels


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


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    if not torch.cuda.is_available():
        raise SystemExit("breadth_bench: no GPU (there is no CPU path to time)")
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
        f = lambda: _call(ctx, ctx.lib.swg_breadth_records_device, rec, genome, G, st.data_ptr())   # noqa: E731
        a, k = f()
        out[tag + "_pairs"] = [len(a), len(k)]
        out[tag + "_mean_depth_all_kept"] = [round(float(x["q_bases"].sum()) / max(float(x["q_union"].sum()), 1.0), 3) for x in (a, k)]
        out[tag + "_ms"] = timed(f, sync)
        ctx.profile_reset()
        ctx.profile(True)
        f()
        ctx.profile(False)
        table = {name: round(v[1], 3) for name, v in ctx.profile_table().items()}
        out[tag + "_kernels_ms"] = table
        own = sum(v for name, v in table.items() if name in OWN)
        scans = sum(v for name, v in table.items() if name.startswith("scan_"))
        out[tag + "_split_ms"] = {"breadth_kernels": round(own, 3), "scans": round(scans, 3),
                                  "sorts_with_events_inside": round(sum(table.get(s, 0.0) for s in SORT_SCOPES), 3)}
        # (c): the sort alone, per axis -- only the selected scope records events
        for scope in SORT_SCOPES:
            ctx.profile_select(scope)
            ts = []
            for _ in range(REPS):
                ctx.profile_reset()
                ctx.profile(True)
                f()
                ctx.profile(False)
                launches, ms = ctx.profile_table()[scope][:2]
                assert launches == 1
                ts.append(ms)
            ctx.profile_select(None)
            out[tag + "_" + scope[len("breadth_"):] + "_ms"] = [round(x, 3) for x in (statistics.median(ts), min(ts), max(ts))]
        sorts = out[tag + "_sort_q_ms"][0] + out[tag + "_sort_t_ms"][0]
        out[tag + "_beyond_the_sorts_ms"] = round(out[tag + "_ms"][0] - sorts, 3)
        g = lambda: alnstats_counts(ctx, rec, genome, G, st.data_ptr(), device=True)   # noqa: E731
        out[tag + "_alnstats_ms"] = timed(g, sync)

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
