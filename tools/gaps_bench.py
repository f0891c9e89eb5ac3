"""On-device gaps (swg_gaps_records_device) timed over resident columns of the benchmark's shape -- bench.gen_shard: G
single-chromosome genomes, every ordered pair, pair-major -- under the status and chain of ONE default-flags swg_filter_device
call, and over the same records, status and chain under a random permutation (chains interleaved record by record).  From one run:
  (a) the whole call with both want bits into arrays of the exact capacity, a host clock around calls that end in a device
      synchronise, warmed up, median of REPS;
  (b) the HIP-event split per kernel of one more call (the library's per-launch profile; memsets and read-backs between the
      launches carry no events, so the split sums to less than (a)), and the ratio of (a) to that sum;
  (c) the library's radix sort of the call's own (key, index) pairs alone: HIP events around the one swg_radix_sort_pairs call
      and around nothing else (profile entry `gaps_sort`, selected so that no other event is recorded), median of REPS calls;
  (d) as the yardstick, one swg_blocks_records_device call over the same columns, timed as (a), and the ratio of (a) to it.

    python tools/gaps_bench.py [n_records] [n_genomes] [out.json]      -> one JSON line on standard output (and in out.json)
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
from sweepga_amd.blocks import BLOCK_DTYPE  # noqa: E402
from sweepga_amd.blocks import _call as blocks_call  # noqa: E402
from sweepga_amd.gaps import BINS, PAIR_DTYPE, ROW_DTYPE  # noqa: E402
from sweepga_amd.gaps import _call as gaps_call  # noqa: E402

REPS = 7
MIN_SIZE = 50
OWN = ("gaps_max", "gaps_strand", "gaps_keys", "gaps_core", "gaps_links", "gaps_rows", "gaps_collect")
SORT_SCOPE = "gaps_sort"   # brackets the whole sort: it overlaps the sort's own kernels


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


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    if not torch.cuda.is_available():
        raise SystemExit("gaps_bench: no GPU (there is no CPU path to time)")
    device = torch.device("cuda:0")
    ctx = sw.Context(0)
    cols, _ = bench.gen_shard(torch, n, G, 2025, device)
    sync = lambda: (torch.cuda.synchronize(), ctx.synchronize())   # noqa: E731
    out = {"n": n, "n_genomes": G, "reps": REPS, "min_size": MIN_SIZE}
    status = torch.zeros(n, dtype=torch.uint8, device=device)
    chain = torch.zeros(n, dtype=torch.int32, device=device)
    rec = bench.make_records(_lib, cols, n, G)
    ccfg = sw.FilterConfig().to_c()
    filt = lambda: ctx.check(ctx.lib.swg_filter_device(ctx.handle, C.byref(rec), C.byref(ccfg), status.data_ptr(), chain.data_ptr(), None))   # noqa: E731
    out["filter_default_ms"] = timed(filt, sync)
    out["records_taking_part"] = int(((status == 1) & (chain != 0)).sum())
    genome = cols["seq_genome_last"]

    def measure(c, st, ch, tag):
        sync()   # the first call below comes before timed(): torch's writes to these columns (the shuffle) must be complete
        r = bench.make_records(_lib, c, n, G)
        first = gaps_call(ctx, ctx.lib.swg_gaps_records_device, r, st.data_ptr(), ch.data_ptr(), genome.data_ptr(), G, MIN_SIZE, 3)
        # what is timed is ONE library call into arrays of the exact capacity
        req = _lib.SwgGapsRequest()
        rows, pairs = np.zeros(max(len(first.rows), 1), dtype=ROW_DTYPE), np.zeros(max(len(first.pairs), 1), dtype=PAIR_DTYPE)
        spectrum = np.zeros(2 * BINS, dtype=np.uint64)
        req.want, req.min_size = 3, MIN_SIZE
        req.capacity, req.rows = len(rows), C.cast(rows.ctypes.data, C.POINTER(_lib.SwgGapRow))
        req.pair_capacity, req.pairs = len(pairs), C.cast(pairs.ctypes.data, C.POINTER(_lib.SwgGapPair))
        req.spectrum = C.cast(spectrum.ctypes.data, C.POINTER(C.c_uint64))
        f = lambda: ctx.check(ctx.lib.swg_gaps_records_device(ctx.handle, C.byref(r), st.data_ptr(), ch.data_ptr(), genome.data_ptr(), G, C.byref(req)))   # noqa: E731
        out[tag + "_rows"] = len(first.rows)
        out[tag + "_links"] = int(first.pairs["links"].sum())
        out[tag + "_genome_pairs"] = len(first.pairs)
        out[tag + "_ms"] = timed(f, sync)
        ctx.profile_reset()
        ctx.profile(True)
        f()
        ctx.profile(False)
        table = {name: round(v[1], 3) for name, v in ctx.profile_table().items()}
        out[tag + "_kernels_ms"] = table
        own = sum(v for name, v in table.items() if name in OWN)
        every = sum(v for name, v in table.items() if name != SORT_SCOPE)
        out[tag + "_split_ms"] = {"gaps_kernels": round(own, 3), "all_kernels": round(every, 3),
                                  "sort_with_events_inside": round(table.get(SORT_SCOPE, 0.0), 3)}
        out[tag + "_call_over_kernels"] = round(out[tag + "_ms"][0] / every, 3) if every else None
        ctx.profile_select(SORT_SCOPE)   # (c): the sort alone -- only the selected scope records events
        ts = []
        for _ in range(REPS):
            ctx.profile_reset()
            ctx.profile(True)
            f()
            ctx.profile(False)
            launches, ms = ctx.profile_table()[SORT_SCOPE][:2]
            assert launches == 1
            ts.append(ms)
        ctx.profile_select(None)
        out[tag + "_sort_ms"] = [round(x, 3) for x in (statistics.median(ts), min(ts), max(ts))]
        # (d): the blocks call over the same columns
        t = blocks_call(ctx, ctx.lib.swg_blocks_records_device, r, st.data_ptr(), ch.data_ptr())
        dst, blocks = _lib.SwgBlockTable(), np.zeros(max(len(t), 1), dtype=BLOCK_DTYPE)
        dst.block_capacity, dst.blocks = len(t), C.cast(blocks.ctypes.data, C.POINTER(_lib.SwgBlock))
        b = lambda: ctx.check(ctx.lib.swg_blocks_records_device(ctx.handle, C.byref(r), st.data_ptr(), ch.data_ptr(), C.byref(dst)))   # noqa: E731
        out[tag + "_blocks_call_ms"] = timed(b, sync)
        out[tag + "_call_over_blocks_call"] = round(out[tag + "_ms"][0] / out[tag + "_blocks_call_ms"][0], 3)
        out[tag + "_links_equal_blocks_core_minus_one"] = int(first.pairs["links"].sum()) == int((t["n_core"] - 1).sum())
        return first

    a = measure(cols, status, chain, "pair_major")
    perm = torch.randperm(n, device=device)
    shuf = {k: (cols[k][perm].contiguous() if k in bench.REC_COLS else cols[k]) for k in cols}
    st_sh, ch_sh = status[perm].contiguous(), chain[perm].contiguous()
    del perm, cols
    b = measure(shuf, st_sh, ch_sh, "shuffled")
    # (the benchmark's q_start values tie inside a chain only by chance; where they do, the index tie-break may order them anew)
    out["same_links_per_pair_both_orders"] = a.pairs[["q_genome", "t_genome", "links"]].tolist() == b.pairs[["q_genome", "t_genome", "links"]].tolist()
    out["same_summary_both_orders"] = a.pairs.tobytes() == b.pairs.tobytes() and a.spectrum.tobytes() == b.spectrum.tobytes()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
