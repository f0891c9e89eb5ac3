"""The on-device lift (swg_lift_records_device) timed over resident columns of the benchmark's shape -- bench.gen_shard: G
single-chromosome genomes, every ordered pair, pair-major.  Per number of regions (10^4 and 10^6 unless one is given), random regions
of 1 - 100 kb on random sequences, resident too:
  (a) the whole call, both axes, the rows of the kept set under the two-call capacity protocol's second call (rows and summary come
      back to the host): a host clock around calls that end in a device synchronise, warmed up, median of REPS;
  (b) the HIP-event split per kernel of one more such call (the library's per-launch profile; memsets, read-backs and copies carry
      no events, so the split sums to less than (a));
and once, as the yardstick, (c) one swg_breadth_records_device call over the same columns and status, timed as (a).

    python tools/lift_bench.py [n_records] [n_genomes] [n_regions] [out.json]     -> one JSON line on standard output (and into out.json)

With `--hops H` (anywhere among the arguments) it times the transitive lift instead (swg_lift_closure_records_device, DESIGN.md section
24) over the same resident records and 10^4 regions (or the count given): the whole call with max_hops = H as (a); one profiled call
per max_hops = 1 .. H, whose differences are the HIP-event split and the projections per hop (raising max_hops leaves the earlier
hops as they are; the last sort and the summaries are in every call); and as the yardstick the one-hop swg_lift_records_device call
on the same input, timed as (a).  The result is kept as profiles/lift_closure_bench_100m.json.
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
from sweepga_amd.breadth import _call as breadth_call  # noqa: E402
from sweepga_amd.lift import lift_closure_records_device, lift_records_device  # noqa: E402

REPS = 7
CLOSURE_OWN = ("lift_limits", "lift_keys", "lift_sort", "lift_gather", "closure_seed", "closure_seed_pieces", "closure_ranges", "closure_count",
               "closure_totals", "closure_project", "closure_events", "closure_iota", "closure_sort", "closure_gather", "closure_deltas",
               "closure_edges", "closure_pieces", "closure_rows", "closure_finish")
OWN = ("lift_limits", "lift_keys", "lift_sort", "lift_gather", "lift_ranges", "lift_count", "lift_region_rows", "lift_rows", "lift_totals")


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


def closure_leg(ctx, cols, status, n_seq, regs, m, hops, sync, out):
    call = lambda h, cap: lift_closure_records_device(ctx, cols, cols["strand"], n_seq, regs, m, h, 100, status=status, set="kept", axes="both",   # noqa: E731
                                                      capacity=cap)
    first = call(hops, 0)
    f = lambda: call(hops, first.n)   # noqa: E731
    got = f()
    leg = {"hops": hops, "min_len": 100, "rows": got.n, "hops_run": got.hops_run, "projections": got.projections, "candidates": list(got.candidates),
           "bases": int(got.summary["bases"].sum()), "cut": int((got.summary["flags"] & 1).sum())}
    leg["call_ms"] = timed(f, sync)
    per_hop, before_ms, before_proj = [], 0.0, 0
    for h in range(1, hops + 1):
        ctx.profile_reset()
        ctx.profile(True)
        r = call(h, first.n)
        ctx.profile(False)
        table = {name: round(v[1], 3) for name, v in ctx.profile_table().items()}
        own = sum(v for name, v in table.items() if name in CLOSURE_OWN)
        per_hop.append({"max_hops": h, "own_kernels_ms": round(own, 3), "hop_ms": round(own - before_ms, 3), "projections": r.projections - before_proj,
                        "rows": r.n})
        before_ms, before_proj = own, r.projections
        if h == hops:
            leg["kernels_ms"] = table
    leg["per_hop"] = per_hop
    one = lift_records_device(ctx, cols, cols["strand"], n_seq, regs, m, status=status, set="kept", axes="both", capacity=0)
    g = lambda: lift_records_device(ctx, cols, cols["strand"], n_seq, regs, m, status=status, set="kept", axes="both", capacity=one.n)   # noqa: E731
    leg["one_hop_lift_ms"] = timed(g, sync)
    leg["call_over_one_hop_lift"] = round(leg["call_ms"][0] / leg["one_hop_lift_ms"][0], 3)
    out["closure_regions_%d" % m] = leg


def main():
    hops = 0
    if "--hops" in sys.argv:
        at = sys.argv.index("--hops")
        hops = int(sys.argv[at + 1])
        del sys.argv[at:at + 2]
        if not 1 <= hops <= 65535:
            raise SystemExit("lift_bench: --hops takes 1 .. 65535")
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    counts = [int(sys.argv[3])] if len(sys.argv) > 3 and int(sys.argv[3]) else [10_000] if hops else [10_000, 1_000_000]
    if not torch.cuda.is_available():
        raise SystemExit("lift_bench: no GPU (there is no CPU path to time)")
    device = torch.device("cuda:0")
    ctx = sw.Context(0)
    cols, _ = bench.gen_shard(torch, n, G, 2025, device)
    status = (torch.rand(n, device=device) < 0.3).to(torch.uint8)
    n_seq = int(cols["seq_genome_last"].numel())
    top = int((cols["q_end"].long() & 0xffffffff).max().item())
    sync = lambda: (torch.cuda.synchronize(), ctx.synchronize())   # noqa: E731
    out = {"n": n, "n_genomes": G, "n_seq": n_seq, "reps": REPS}
    gen = torch.Generator(device=device)
    gen.manual_seed(7)
    for m in counts:
        start = torch.randint(0, max(top, 1), (m,), device=device, generator=gen)
        width = torch.randint(1_000, 100_001, (m,), device=device, generator=gen)
        regs = torch.stack([torch.randint(0, n_seq, (m,), device=device, generator=gen), start, start + width, torch.zeros_like(start)], 1)
        regs = regs.to(torch.int32).contiguous()   # (values below 2^31: the bits are those of the uint32 the library reads)
        if hops:
            closure_leg(ctx, cols, status, n_seq, regs, m, hops, sync, out)
            continue
        first = lift_records_device(ctx, cols, cols["strand"], n_seq, regs, m, status=status, set="kept", axes="both", capacity=0)
        f = lambda: lift_records_device(ctx, cols, cols["strand"], n_seq, regs, m, status=status, set="kept", axes="both", capacity=first.n)   # noqa: E731
        got = f()
        tag = "regions_%d" % m
        hits_all = int(got.summary[:, 0].sum())
        out[tag] = {"rows": got.n, "hits_all": hits_all, "hits_kept": int(got.summary[:, 1].sum()), "candidates": list(got.candidates),
                    "candidates_per_hit": round(sum(got.candidates) / max(hits_all, 1), 3)}
        out[tag]["call_ms"] = timed(f, sync)
        ctx.profile_reset()
        ctx.profile(True)
        f()
        ctx.profile(False)
        table = {name: round(v[1], 3) for name, v in ctx.profile_table().items()}
        out[tag]["kernels_ms"] = table
        out[tag]["own_kernels_ms"] = round(sum(v for name, v in table.items() if name in OWN), 3)
    if not hops:
        rec = bench.make_records(_lib, cols, n, G)
        genome = cols["seq_genome_last"].data_ptr()
        out["breadth_ms"] = timed(lambda: breadth_call(ctx, ctx.lib.swg_breadth_records_device, rec, genome, G, status.data_ptr()), sync)
        for m in counts:
            out["regions_%d" % m]["call_over_breadth"] = round(out["regions_%d" % m]["call_ms"][0] / out["breadth_ms"][0], 3)
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
