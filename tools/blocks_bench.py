"""On-device blocks (swg_blocks_records_device) timed over resident columns of the benchmark's shape -- bench.gen_shard: G
single-chromosome genomes, every ordered pair, pair-major -- under the status and chain of ONE default-flags swg_filter_device
call, and over the same records, status and chain shuffled (chains interleaved record by record).  From one run:
  (a) the whole call, a host clock around calls that end in a device synchronise, warmed up, median of REPS;
  (b) the HIP-event split per kernel of one more call (the library's per-launch profile; memsets and read-backs between the
      launches carry no events, so the split sums to less than (a));
  (c) the library's radix sort of the call's own (key, index) pairs alone, per axis: HIP events around the one
      swg_radix_sort_pairs call of the axis and around nothing else (profile entries `blocks_sort_q`, `blocks_sort_t`, selected
      one at a time so that no other event is recorded in the call), median of REPS calls -- existing code, the floor;
  (d) for scale, the swg_filter_device call that made the status and chain (pair-major input), timed as (a).

    python tools/blocks_bench.py [n_records] [n_genomes]      -> one JSON line on standard output
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
from sweepga_amd.blocks import BLOCK_DTYPE, _call  # noqa: E402

REPS = 7
OWN = ("blocks_max", "blocks_reduce", "blocks_keys", "blocks_gather", "blocks_union", "blocks_collect")
SORT_SCOPES = ("blocks_sort_q", "blocks_sort_t")   # each brackets its axis' whole sort: they overlap the sort's own kernels


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
        raise SystemExit("blocks_bench: no GPU (there is no CPU path to time)")
    device = torch.device("cuda:0")
    ctx = sw.Context(0)
    cols, _ = bench.gen_shard(torch, n, G, 2025, device)
    sync = lambda: (torch.cuda.synchronize(), ctx.synchronize())   # noqa: E731
    out = {"n": n, "n_genomes": G, "reps": REPS}
    status = torch.zeros(n, dtype=torch.uint8, device=device)
    chain = torch.zeros(n, dtype=torch.int32, device=device)
    rec = bench.make_records(_lib, cols, n, G)
    ccfg = sw.FilterConfig().to_c()
    filt = lambda: ctx.check(ctx.lib.swg_filter_device(ctx.handle, C.byref(rec), C.byref(ccfg), status.data_ptr(), chain.data_ptr(), None))   # noqa: E731
    out["filter_default_ms"] = timed(filt, sync)
    out["kept_records"] = int((status != 0).sum())
    out["records_in_chains"] = int(((status != 0) & (chain != 0)).sum())

    def measure(c, st, ch, tag):
        sync()   # the first call below comes before timed(): torch's writes to these columns (the shuffle) must be complete
        r = bench.make_records(_lib, c, n, G)
        t = _call(ctx, ctx.lib.swg_blocks_records_device, r, st.data_ptr(), ch.data_ptr())
        # what is timed is ONE library call into an array of the exact capacity (the wrapper above calls twice when the blocks
        # outnumber its first guess)
        dst, rows = _lib.SwgBlockTable(), np.zeros(max(len(t), 1), dtype=BLOCK_DTYPE)
        dst.block_capacity, dst.blocks = len(t), C.cast(rows.ctypes.data, C.POINTER(_lib.SwgBlock))
        f = lambda: ctx.check(ctx.lib.swg_blocks_records_device(ctx.handle, C.byref(r), st.data_ptr(), ch.data_ptr(), C.byref(dst)))   # noqa: E731
        out[tag + "_blocks"] = len(t)
        out[tag + "_largest_chain_records"] = int((t["n_core"] + t["n_inverted"] + t["n_rescued"]).max()) if len(t) else 0
        out[tag + "_ms"] = timed(f, sync)
        ctx.profile_reset()
        ctx.profile(True)
        f()
        ctx.profile(False)
        table = {name: round(v[1], 3) for name, v in ctx.profile_table().items()}
        out[tag + "_kernels_ms"] = table
        own = sum(v for name, v in table.items() if name in OWN)
        scans = sum(v for name, v in table.items() if name.startswith("scan_"))
        out[tag + "_split_ms"] = {"blocks_kernels": round(own, 3), "scans": round(scans, 3),
                                  "sorts_with_events_inside": round(sum(table.get(s, 0.0) for s in SORT_SCOPES), 3)}
        for scope in SORT_SCOPES:   # (c): the sort alone, per axis -- only the selected scope records events
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
            out[tag + "_" + scope[len("blocks_"):] + "_ms"] = [round(x, 3) for x in (statistics.median(ts), min(ts), max(ts))]
        sorts = out[tag + "_sort_q_ms"][0] + out[tag + "_sort_t_ms"][0]
        out[tag + "_beyond_the_sorts_ms"] = round(out[tag + "_ms"][0] - sorts, 3)
        return t

    a = measure(cols, status, chain, "pair_major")
    perm = torch.randperm(n, device=device)
    shuf = {k: (cols[k][perm].contiguous() if k in bench.REC_COLS else cols[k]) for k in cols}
    st_sh, ch_sh = status[perm].contiguous(), chain[perm].contiguous()
    del perm, cols
    b = measure(shuf, st_sh, ch_sh, "shuffled")
    out["same_table_both_orders"] = len(a) == len(b) and all((a[f] == b[f]).all() for f in a.dtype.names if f != "first_record")
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
