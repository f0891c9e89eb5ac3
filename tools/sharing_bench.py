"""On-device sharing (swg_sharing_records_device) timed over resident columns of the benchmark's shape -- bench.gen_shard: G
single-chromosome genomes, every ordered pair, pair-major.  Four numbers from one run:
  (a) the whole call with all four want bits: runs of both sets fetched into arrays of the exact capacity (sized by one call
      before the clock starts) and both spectra, a host clock around calls that end in a device synchronise, warmed up, median
      of REPS;
  (b) the same call wanting the two spectra only (no row comes back);
  (c) the HIP-event split per kernel of one more call of (a) (the library's per-launch profile; memsets, read-backs and copies
      between the launches carry no events, so the split sums to less than (a));
  (d) one swg_intervals_records_device call wanting all six lists over the same columns and status, timed as (a): the yardstick --
      two sorts of n entries where sharing has one of 2 n, and it exists on the commit before this feature.

    python tools/sharing_bench.py [n_records] [n_genomes] [out.json]      -> one JSON line on standard output (and into out.json)
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
from sweepga_amd.intervals import INTERVAL_DTYPE  # noqa: E402
from sweepga_amd.sharing import RUN_DTYPE  # noqa: E402

REPS = 7
OWN = ("sharing_keys", "sharing_gather", "sharing_count", "sharing_events", "sharing_group_first", "sharing_break_flags", "sharing_open_flags",
       "sharing_runs", "sharing_bases", "sharing_spectrum", "sharing_lengths", "sharing_private")
SORT_SCOPES = ("sharing_sort", "sharing_sort_events")   # each brackets a whole sort: they overlap the sort's own kernels


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
        raise SystemExit("sharing_bench: no GPU (there is no CPU path to time)")
    device = torch.device("cuda:0")
    ctx = sw.Context(0)
    cols, _ = bench.gen_shard(torch, n, G, 2025, device)
    status = (torch.rand(n, device=device) < 0.3).to(torch.uint8)
    rec = bench.make_records(_lib, cols, n, G)
    genome = cols["seq_genome_last"].data_ptr()
    n_seq = int(cols["seq_genome_last"].numel())
    seq_len = torch.zeros(n_seq, dtype=torch.int64, device=device)   # a length that holds every record of the sequence
    seq_len.scatter_reduce_(0, cols["q_id"].long(), cols["q_end"].long() & 0xffffffff, "amax")
    seq_len.scatter_reduce_(0, cols["t_id"].long(), cols["t_end"].long() & 0xffffffff, "amax")
    seq_len = seq_len.to(torch.int32)   # (the bits of the uint32 the library reads)
    sync = lambda: (torch.cuda.synchronize(), ctx.synchronize())   # noqa: E731
    out = {"n": n, "n_genomes": G, "reps": REPS}
    spectra = [np.zeros((G, G), dtype=np.uint64), np.zeros((G, G), dtype=np.uint64)]

    def request(want):
        req = _lib.SwgSharingRequest()
        req.want = want
        for s in range(2):
            req.set[s].spectrum = C.cast(spectra[s].ctypes.data, C.POINTER(C.c_uint64))
        return req

    call = lambda req: ctx.check(ctx.lib.swg_sharing_records_device(ctx.handle, C.byref(rec), genome, C.c_uint32(G), seq_len.data_ptr(),   # noqa: E731
                                                                    status.data_ptr(), C.byref(req)))
    req = request(0xf)
    sync()
    call(req)   # capacity 0: how many runs
    rows = [np.zeros(max(int(req.set[s].n), 1), dtype=RUN_DTYPE) for s in range(2)]
    for s in range(2):
        req.set[s].capacity = int(req.set[s].n)
        req.set[s].rows = C.cast(rows[s].ctypes.data, C.POINTER(_lib.SwgDepthRun))
    out["all_four_ms"] = timed(lambda: call(req), sync)
    out["runs"] = {"all": int(req.set[0].n), "kept": int(req.set[1].n)}
    out["bases"] = {"all": int(req.set[0].bases), "kept": int(req.set[1].bases)}
    out["max_depth"] = {"all": int(rows[0]["depth"].max()) if len(rows[0]) else 0, "kept": int(rows[1]["depth"].max()) if len(rows[1]) else 0}
    ctx.profile_reset()
    ctx.profile(True)
    call(req)
    ctx.profile(False)
    table = {k: round(v[1], 3) for k, v in ctx.profile_table().items()}
    out["kernels_ms"] = table
    out["split_ms"] = {"sharing_kernels": round(sum(v for k, v in table.items() if k in OWN), 3),
                       "scans_and_compactions": round(sum(v for k, v in table.items() if k.startswith(("scan_", "flag_"))), 3),
                       "sorts_with_events_inside": round(sum(table.get(s, 0.0) for s in SORT_SCOPES), 3)}
    spec = request(0xc)
    out["spectrum_only_ms"] = timed(lambda: call(spec), sync)
    # the yardstick: intervals, all six lists, rows fetched
    iv = _lib.SwgIntervalRequest()
    iv.want = 0x3f
    iv_call = lambda: ctx.check(ctx.lib.swg_intervals_records_device(ctx.handle, C.byref(rec), genome, C.c_uint32(G), status.data_ptr(), C.byref(iv)))   # noqa: E731
    sync()
    iv_call()
    keep = []
    for s in range(3):
        for a in range(2):
            r = np.zeros(max(int(iv.list[s][a].n), 1), dtype=INTERVAL_DTYPE)
            keep.append(r)
            iv.list[s][a].capacity = int(iv.list[s][a].n)
            iv.list[s][a].rows = C.cast(r.ctypes.data, C.POINTER(_lib.SwgInterval))
    out["intervals_all_six_ms"] = timed(iv_call, sync)
    out["all_four_over_intervals"] = round(out["all_four_ms"][0] / out["intervals_all_six_ms"][0], 3)
    out["spectrum_only_over_intervals"] = round(out["spectrum_only_ms"][0] / out["intervals_all_six_ms"][0], 3)
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
