"""The on-device dot plot (swg_dotplot_records_device) timed over resident columns of the benchmark's shape -- bench.gen_shard: G
single-chromosome genomes, every ordered pair, pair-major -- with every sequence on both axes in id order.  Per image size (2048^2
and 8192^2 unless one size is given):
  (a) the whole call with all four planes, which come back to the host: a host clock around calls that end in a device synchronise,
      warmed up, median of REPS;
  (b) the HIP-event split per kernel of one more such call (the library's per-launch profile; the memsets of the planes, the
      read-back and the copies of the planes carry no events, so the split sums to less than (a));
and once, as the yardstick, (c) one swg_breadth_records_device call over the same columns and status, timed as (a): the cheapest
report of the commit before this feature that reads the same 25 bytes per record.

    python tools/dotplot_bench.py [n_records] [n_genomes] [size] [out.json]     -> one JSON line on standard output (and into out.json)
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
from sweepga_amd.dotplot import dotplot_records_device  # noqa: E402

REPS = 7
OWN = ("dot_classify", "dot_lines", "dot_sums")


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
    sizes = [int(sys.argv[3])] if len(sys.argv) > 3 and int(sys.argv[3]) else [2048, 8192]
    if not torch.cuda.is_available():
        raise SystemExit("dotplot_bench: no GPU (there is no CPU path to time)")
    device = torch.device("cuda:0")
    ctx = sw.Context(0)
    cols, _ = bench.gen_shard(torch, n, G, 2025, device)
    status = (torch.rand(n, device=device) < 0.3).to(torch.uint8)
    n_seq = int(cols["seq_genome_last"].numel())
    seq_len = torch.zeros(n_seq, dtype=torch.int64, device=device)   # a length that holds every record of the sequence
    seq_len.scatter_reduce_(0, cols["q_id"].long(), cols["q_end"].long() & 0xffffffff, "amax")
    seq_len.scatter_reduce_(0, cols["t_id"].long(), cols["t_end"].long() & 0xffffffff, "amax")
    off = (torch.cumsum(seq_len, 0) - seq_len).contiguous()   # (int64 holds the bits of the uint64 the library reads: totals < 2^48)
    total = int(seq_len.sum().item())
    sync = lambda: (torch.cuda.synchronize(), ctx.synchronize())   # noqa: E731
    out = {"n": n, "n_genomes": G, "n_seq": n_seq, "axis_total": total, "reps": REPS}
    for size in sizes:
        f = lambda: dotplot_records_device(ctx, cols, cols["strand"], off, off, total, total, size, size, status=status, want=0xf)   # noqa: E731
        got = f()
        tag = "size_%d" % size
        out[tag] = {"drawn": list(got.drawn), "hits": got.hits, "pixels_touched": [int((p != 0).sum()) for p in got.planes]}
        out[tag]["call_ms"] = timed(f, sync)
        ctx.profile_reset()
        ctx.profile(True)
        f()
        ctx.profile(False)
        table = {name: round(v[1], 3) for name, v in ctx.profile_table().items()}
        out[tag]["kernels_ms"] = table
        out[tag]["own_kernels_ms"] = round(sum(v for name, v in table.items() if name in OWN), 3)
    rec = bench.make_records(_lib, cols, n, G)
    genome = cols["seq_genome_last"].data_ptr()
    out["breadth_ms"] = timed(lambda: breadth_call(ctx, ctx.lib.swg_breadth_records_device, rec, genome, G, status.data_ptr()), sync)
    for size in sizes:
        out["size_%d" % size]["call_over_breadth"] = round(out["size_%d" % size]["call_ms"][0] / out["breadth_ms"][0], 3)
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
