"""On-device mosaic (swg_mosaic_records_device) timed over resident columns of the benchmark's shape -- bench.gen_shard: G
single-chromosome genomes, every ordered pair, pair-major.  Four numbers from one run:
  (a) the whole call with both want bits, set KEPT, query axis, weight = the matches column: the rows fetched into an array of
      the exact capacity (sized by one call before the clock starts) and the share, a host clock around calls that end in a device
      synchronise, warmed up, median of REPS;
  (b) the same call wanting the share only (no row comes back);
  (c) the HIP-event split per kernel of one more call of (a) (the library's per-launch profile; memsets, read-backs and copies
      between the launches carry no events, so the split sums to less than (a));
  (d) one swg_sharing_records_device call with both runs bits over the same columns and status, timed as (a): the yardstick -- its
      first half is one sort of 2 n pairs, as the mosaic's.

    python tools/mosaic_bench.py [n_records] [n_genomes] [out.json] [tile_build]      -> one JSON line on standard output (and into out.json)

The library does not report its tile, so "tile" in the result is worked out as the library does: tile_build -- the fourth argument,
the T the library was compiled with (512 unless built with -DSWG_MOSAIC_TILE_LOG=8 or 10) -- unless SWG_MOSAIC_TILE names a smaller
power of two.
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
from sweepga_amd.mosaic import ROW_DTYPE  # noqa: E402
from sweepga_amd.sharing import RUN_DTYPE  # noqa: E402

REPS = 7
OWN = ("mosaic_keys", "mosaic_flags", "mosaic_slots", "mosaic_coarse", "mosaic_push", "mosaic_tile", "mosaic_breaks", "mosaic_open", "mosaic_rows",
       "mosaic_bases", "mosaic_share")
SORT_SCOPES = ("mosaic_sort",)   # brackets the whole sort: it overlaps the sort's own kernels


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
        raise SystemExit("mosaic_bench: no GPU (there is no CPU path to time)")
    device = torch.device("cuda:0")
    ctx = sw.Context(0)
    cols, _ = bench.gen_shard(torch, n, G, 2025, device)
    status = (torch.rand(n, device=device) < 0.3).to(torch.uint8)
    rec = bench.make_records(_lib, cols, n, G)
    genome = cols["seq_genome_last"].data_ptr()
    sync = lambda: (torch.cuda.synchronize(), ctx.synchronize())   # noqa: E731
    tile_build = int(sys.argv[4]) if len(sys.argv) > 4 else 512
    asked = os.environ.get("SWG_MOSAIC_TILE", "")
    asked = int(asked) if asked.isdigit() else 0
    tile = asked if 2 <= asked <= tile_build and asked & (asked - 1) == 0 else tile_build   # (the library's own rule)
    out = {"n": n, "n_genomes": G, "reps": REPS, "tile": tile, "tile_build": tile_build}
    share = np.zeros((G, G), dtype=np.uint64)

    def request(want):
        req = _lib.SwgMosaicRequest()
        req.want, req.axis, req.set = want, 0, 1
        req.share = C.cast(share.ctypes.data, C.POINTER(C.c_uint64))
        return req

    call = lambda req: ctx.check(ctx.lib.swg_mosaic_records_device(ctx.handle, C.byref(rec), genome, C.c_uint32(G), status.data_ptr(), C.byref(req)))   # noqa: E731
    req = request(3)
    sync()
    call(req)   # capacity 0: how many rows
    rows = np.zeros(max(int(req.n), 1), dtype=ROW_DTYPE)
    req.capacity = int(req.n)
    req.rows = C.cast(rows.ctypes.data, C.POINTER(_lib.SwgMosaicRow))
    out["rows_and_share_ms"] = timed(lambda: call(req), sync)
    out["rows"], out["bases"], out["share_sum"] = int(req.n), int(req.bases), int(share.sum())
    ctx.profile_reset()
    ctx.profile(True)
    call(req)
    ctx.profile(False)
    prof = ctx.profile_table()
    table = {k: round(v[1], 3) for k, v in prof.items()}
    out["kernels_ms"] = table
    out["launches"] = {k: int(v[0]) for k, v in prof.items() if k in OWN}
    out["split_ms"] = {"mosaic_kernels": round(sum(v for k, v in table.items() if k in OWN), 3),
                       "scans_and_compactions": round(sum(v for k, v in table.items() if k.startswith(("scan_", "flag_"))), 3),
                       "sort": round(sum(table.get(s, 0.0) for s in SORT_SCOPES), 3)}
    only = request(2)
    out["share_only_ms"] = timed(lambda: call(only), sync)
    # the yardstick: sharing, the runs of both sets, rows fetched
    sh = _lib.SwgSharingRequest()
    sh.want = 0x3
    sh_call = lambda: ctx.check(ctx.lib.swg_sharing_records_device(ctx.handle, C.byref(rec), genome, C.c_uint32(G), None, status.data_ptr(), C.byref(sh)))   # noqa: E731
    sync()
    sh_call()
    keep = []
    for s in range(2):
        r = np.zeros(max(int(sh.set[s].n), 1), dtype=RUN_DTYPE)
        keep.append(r)
        sh.set[s].capacity = int(sh.set[s].n)
        sh.set[s].rows = C.cast(r.ctypes.data, C.POINTER(_lib.SwgDepthRun))
    out["sharing_both_runs_ms"] = timed(sh_call, sync)
    out["rows_and_share_over_sharing"] = round(out["rows_and_share_ms"][0] / out["sharing_both_runs_ms"][0], 3)
    out["share_only_over_sharing"] = round(out["share_only_ms"][0] / out["sharing_both_runs_ms"][0], 3)
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
