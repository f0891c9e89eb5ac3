"""On-device placement (swg_place_records_device) timed over resident columns of the benchmark's shape -- bench.gen_shard: G
single-chromosome genomes, every ordered pair, pair-major -- under the status of ONE default-flags swg_filter_device call, and
over the same records and status under a random permutation (candidates interleaved record by record).  From one run:
  (a) the whole call with both want bits (query axis, kept set, min_bases 0) into arrays of the exact capacity, a host clock
      around calls that end in a device synchronise, warmed up, median of REPS;
  (b) the HIP-event split per kernel of one more call (the library's per-launch profile; memsets and read-backs between the
      launches carry no events, so the split sums to less than (a)), and the ratio of (a) to that sum;
  (c) as the yardstick, one swg_components_records_device call over the same columns -- the nearest existing report, the
      per-sequence-pair sums -- timed as (a), and the ratio of (a) to it.
NOT measured: a fragmented shape (10^5 or more placed sequences), the target axis, the host seam.

    python tools/place_bench.py [n_records] [n_genomes] [out.json] [commit]      -> one JSON line on standard output (and in out.json)
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
from sweepga_amd.components import _call as components_call  # noqa: E402
from sweepga_amd.place import PAIR_DTYPE, ROW_DTYPE  # noqa: E402
from sweepga_amd.place import _call as place_call  # noqa: E402

REPS = 7
OWN = ("place_keys", "place_heads", "place_runs", "place_cands", "place_group_keys", "place_groups", "place_winners", "place_decide",
       "place_expand", "place_weights", "place_median", "place_rekey", "place_marks", "place_rows", "place_pairs")
SCOPES = ("place_sort", "place_cand_sort", "place_median_sort", "place_layout_sort")   # bracket whole sorts: they overlap the sorts' own kernels


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
        raise SystemExit("place_bench: no GPU (there is no CPU path to time)")
    device = torch.device("cuda:0")
    ctx = sw.Context(0)
    cols, _ = bench.gen_shard(torch, n, G, 2025, device)
    sync = lambda: (torch.cuda.synchronize(), ctx.synchronize())   # noqa: E731
    out = {"n": n, "n_genomes": G, "reps": REPS, "axis": "query", "set": "kept", "min_bases": 0, "box": torch.cuda.get_device_name(0),
           "commit": sys.argv[4] if len(sys.argv) > 4 else None}
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
    seq_len = torch.full((n_seq,), 150_000_000, dtype=torch.int32, device=device)   # the generator's chromosome length
    par = _lib.SwgComponentParams(0, 0, 0)

    def measure(c, st, tag):
        sync()   # the first call below comes before timed(): torch's writes to these columns (the shuffle) must be complete
        r = bench.make_records(_lib, c, n, G)
        first = place_call(ctx, ctx.lib.swg_place_records_device, r, seq_len.data_ptr(), genome.data_ptr(), G, st.data_ptr(), 0, 1, 0, 3)
        # what is timed is ONE library call into arrays of the exact capacity
        req = _lib.SwgPlaceRequest()
        rows, pairs = np.zeros(max(len(first.rows), 1), dtype=ROW_DTYPE), np.zeros(max(len(first.pairs), 1), dtype=PAIR_DTYPE)
        req.want, req.axis, req.set, req.min_bases = 3, 0, 1, 0
        req.capacity, req.rows = len(rows), C.cast(rows.ctypes.data, C.POINTER(_lib.SwgPlacement))
        req.pair_capacity, req.pairs = len(pairs), C.cast(pairs.ctypes.data, C.POINTER(_lib.SwgPlacePair))
        f = lambda: ctx.check(ctx.lib.swg_place_records_device(ctx.handle, C.byref(r), seq_len.data_ptr(), genome.data_ptr(), G, st.data_ptr(), C.byref(req)))   # noqa: E731
        out[tag + "_rows"] = len(first.rows)
        out[tag + "_reversed"] = int(first.pairs["reversed"].sum())
        out[tag + "_genome_pairs"] = len(first.pairs)
        out[tag + "_placed_bases"] = int(first.pairs["bases"].sum())
        out[tag + "_ms"] = timed(f, sync)
        ctx.profile_reset()
        ctx.profile(True)
        f()
        ctx.profile(False)
        table = {name: round(v[1], 3) for name, v in ctx.profile_table().items()}
        out[tag + "_kernels_ms"] = table
        own = sum(v for name, v in table.items() if name in OWN)
        every = sum(v for name, v in table.items() if name not in SCOPES)
        out[tag + "_split_ms"] = {"place_kernels": round(own, 3), "all_kernels": round(every, 3),
                                  "sorts_with_events_inside": round(sum(table.get(s, 0.0) for s in SCOPES), 3)}
        out[tag + "_call_over_kernels"] = round(out[tag + "_ms"][0] / every, 3) if every else None
        # (c): the components call over the same columns
        comp = lambda: components_call(ctx, ctx.lib.swg_components_records_device, r, seq_len.data_ptr(), st.data_ptr(), par)   # noqa: E731
        out[tag + "_components_call_ms"] = timed(comp, sync)
        out[tag + "_call_over_components_call"] = round(out[tag + "_ms"][0] / out[tag + "_components_call_ms"][0], 3)
        return first

    a = measure(cols, status, "pair_major")
    perm = torch.randperm(n, device=device)
    shuf = {k: (cols[k][perm].contiguous() if k in bench.REC_COLS else cols[k]) for k in cols}
    st_sh = status[perm].contiguous()
    del perm, cols
    b = measure(shuf, st_sh, "shuffled")
    out["same_rows_both_orders"] = a.rows.tobytes() == b.rows.tobytes() and a.pairs.tobytes() == b.pairs.tobytes()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
