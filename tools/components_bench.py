"""On-device components (swg_components_records_device) timed over resident columns of the benchmark's shape -- bench.gen_shard: G
single-chromosome genomes, every ordered pair, pair-major -- under the status of ONE default-flags swg_filter_device call, and
over the same records and status shuffled (every record its own run in the link pass).  From one run:
  (a) the whole call, a host clock around calls that end in a device synchronise, warmed up, median of REPS;
  (b) the HIP-event split per kernel of one more call (the library's per-launch profile; memsets and read-backs between the
      launches carry no events, so the split sums to less than (a)) and the number of hook / compress rounds of that call;
  (c) for scale, the swg_filter_device call that made the status (pair-major input), timed as (a).

    python tools/components_bench.py [n_records] [n_genomes]      -> one JSON line on standard output
"""
import ctypes as C
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
from sweepga_amd.components import _call  # noqa: E402

REPS = 7
OWN = ("components_count", "components_links", "components_list", "components_iota", "components_hook", "components_compress",
       "components_roots", "components_number", "components_sums")


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
        raise SystemExit("components_bench: no GPU (there is no CPU path to time)")
    device = torch.device("cuda:0")
    ctx = sw.Context(0)
    cols, _ = bench.gen_shard(torch, n, G, 2025, device)
    sync = lambda: (torch.cuda.synchronize(), ctx.synchronize())   # noqa: E731
    out = {"n": n, "n_genomes": G, "reps": REPS}
    status = torch.zeros(n, dtype=torch.uint8, device=device)
    chain = torch.zeros(n, dtype=torch.int32, device=device)
    rec = bench.make_records(_lib, cols, n, G)
    n_seq = int(rec.n_seq)
    ccfg = sw.FilterConfig().to_c()
    filt = lambda: ctx.check(ctx.lib.swg_filter_device(ctx.handle, C.byref(rec), C.byref(ccfg), status.data_ptr(), chain.data_ptr(), None))   # noqa: E731
    out["filter_default_ms"] = timed(filt, sync)
    out["kept_records"] = int((status != 0).sum())
    del chain
    # sequence lengths: the generator's chromosome length (under the default thresholds 0, 0 they only feed the component lengths)
    seq_len = torch.full((n_seq,), 150_000_000, dtype=torch.int32, device=device)
    par = _lib.SwgComponentParams(0, 0, 0)

    def measure(c, st, tag):
        r = bench.make_records(_lib, c, n, G)
        sync()   # (torch has just written these columns on its own stream)
        f = lambda: _call(ctx, ctx.lib.swg_components_records_device, r, seq_len.data_ptr(), st.data_ptr(), par)   # noqa: E731
        t = f()
        out[tag + "_links"], out[tag + "_components"] = len(t.links), len(t.components)
        out[tag + "_ms"] = timed(f, sync)
        ctx.profile_reset()
        ctx.profile(True)
        f()
        ctx.profile(False)
        prof = ctx.profile_table()
        table = {name: round(v[1], 3) for name, v in prof.items()}
        out[tag + "_kernels_ms"] = table
        out[tag + "_rounds"] = int(prof["components_hook"][0]) if "components_hook" in prof else 0
        out[tag + "_own_kernels_ms"] = round(sum(v for name, v in table.items() if name in OWN), 3)
        return t

    a = measure(cols, status, "pair_major")
    perm = torch.randperm(n, device=device)
    shuf = {k: (cols[k][perm].contiguous() if k in bench.REC_COLS else cols[k]) for k in cols}
    st_sh = status[perm].contiguous()
    del perm, cols
    b = measure(shuf, st_sh, "shuffled")
    out["same_table_both_orders"] = (a.components.tobytes() == b.components.tobytes() and a.seq_component.tobytes() == b.seq_component.tobytes() and
                                     a.cross == b.cross and all((a.links[f] == b.links[f]).all() for f in a.links.dtype.names if f != "first_record"))
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
