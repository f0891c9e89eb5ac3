"""The difference list (swg_diff_records_device) timed over resident columns of the benchmark's shape --
bench.gen_shard: G single-chromosome genomes, every ordered pair, pair-major -- with the input, the batch and the method of
tools/ucsc_chain_bench.py.  The set is the first kept records (a random 30 % status) whose CIGAR text fits a default batch: 1/64 of
the free device memory, at most 1 GiB.  Each gets the synthetic CIGAR of tools/lift_exact_bench.py with diff_every = DIFF_EVERY:
`198=2X` per 200 bases, every DIFF_EVERY-th unit `99=1X48=2I50=2D` instead, so that the run has insertions and deletions to list:
  (a) the whole call with all four kinds, min_indel 1, under the two-call capacity protocol's second call (rows, pairs, spectrum
      and states come back to the host): a host clock around calls that end in a device synchronise, warmed up, median of REPS; and
      the same with the counts, pairs and spectrum only (no row is built);
  (b) the HIP-event split per kernel of one more call with rows (the library's per-launch profile; memsets, read-backs and copies
      carry no events, so the split sums to less than (a));
and once, as the yardstick, (c) cigar_build alone on the same set -- parse, scans, entries: swg_lift_exact_records_device without
regions -- timed as (a).

    python tools/diffs_bench.py [n_records] [n_genomes] [out.json] [diff_every]     -> one JSON line on standard output (and into out.json)

The result is kept as profiles/diffs_bench_100m.json.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
import sweepga_amd as sw  # noqa: E402
from sweepga_amd.diffs import diff_records_device  # noqa: E402
from sweepga_amd.lift import lift_exact_records_device  # noqa: E402
from tools.lift_bench import REPS, timed  # noqa: E402
from tools.lift_exact_bench import CIGAR_OWN, DIFF_UNIT, synthetic_cigar  # noqa: E402

DIFFS_OWN = ("diffs_letters", "diffs_entries", "diffs_ops", "diffs_rows", "diffs_collect")
DIFF_EVERY = 4


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    every = int(sys.argv[4]) if len(sys.argv) > 4 else DIFF_EVERY
    if not torch.cuda.is_available():
        raise SystemExit("diffs_bench: no GPU (there is no CPU path to time)")
    device = torch.device("cuda:0")
    ctx = sw.Context(0)
    cols, _ = bench.gen_shard(torch, n, G, 2025, device)
    status = (torch.rand(n, device=device) < 0.3).to(torch.uint8)
    n_seq = int(cols["seq_genome_last"].numel())
    sync = lambda: (torch.cuda.synchronize(), ctx.synchronize())   # noqa: E731
    sync()
    batch = min(torch.cuda.mem_get_info()[0] // 64, 1 << 30)
    side = lambda a, b: (cols[b].long() & 0xffffffff) - (cols[a].long() & 0xffffffff)   # noqa: E731
    lq, lt = side("q_start", "q_end"), side("t_start", "t_end")
    kept = torch.nonzero(status).flatten()
    unit = len(DIFF_UNIT) if every > 0 else 6
    bound = unit * (torch.minimum(lq, lt)[kept] // 200) + 16      # at least a record's text
    k = int(torch.searchsorted(torch.cumsum(bound, 0), batch).item())
    assert k > 0
    at = kept[:k]
    texts = [synthetic_cigar(int(a), int(b), every).encode() for a, b in zip(lq[at].cpu().numpy(), lt[at].cpu().numpy())]
    offset = np.zeros(k + 1, dtype=np.int64)
    np.cumsum([len(t) for t in texts], out=offset[1:])
    assert offset[-1] <= batch
    genome = cols["seq_genome_last"]
    n_genome = int(genome.max().item()) + 1
    d_record = at.to(torch.int32).contiguous()
    d_offset = torch.from_numpy(offset).to(device)
    d_text = torch.from_numpy(np.frombuffer(b"".join(texts) or b"\0", dtype=np.uint8).copy()).to(device)
    del texts
    call = lambda cap: diff_records_device(ctx, cols, cols["strand"], n_seq, genome, n_genome, d_record, d_offset, d_text, k, status=status, set="kept",   # noqa: E731
                                           kinds=15, min_indel=1, capacity=cap)
    first = call((None, None))
    f = lambda: call((first.n_rows, first.n_pairs))   # noqa: E731
    got = f()
    assert got.rows is not None and len(got.rows) == first.n_rows
    sums = {name: int(got.pairs[name].sum()) for name in ("entries", "aligned", "eq", "snp_runs", "snp_bases", "n_ins", "ins_bases", "n_del", "del_bases")}
    out = {"n": n, "n_genomes": G, "n_seq": n_seq, "reps": REPS, "batch_bytes": int(batch), "diff_every": every, "entries": k, "cigar_bytes": int(offset[-1]),
           "ops": got.ops, "rows": got.n_rows, "pairs": got.n_pairs, "usable": got.usable, "cigar_bad": got.cigar_bad, "sums": sums}
    out["call_ms"] = timed(f, sync)
    out["counts_only_ms"] = timed(lambda: call((None, first.n_pairs)), sync)
    ctx.profile_reset()
    ctx.profile(True)
    f()
    ctx.profile(False)
    table = {name: round(v[1], 3) for name, v in ctx.profile_table().items()}
    out["kernels_ms"] = table
    out["cigar_kernels_ms"] = round(sum(v for name, v in table.items() if name in CIGAR_OWN), 3)
    out["diffs_kernels_ms"] = round(sum(v for name, v in table.items() if name in DIFFS_OWN), 3)
    regs = torch.zeros((1, 4), dtype=torch.int32, device=device)
    g = lambda: lift_exact_records_device(ctx, cols, cols["strand"], n_seq, regs, 0, d_record, d_offset, d_text, k, status=status, set="kept",   # noqa: E731
                                          capacity=0)
    assert g().ops == got.ops
    out["cigar_build_ms"] = timed(g, sync)
    out["call_over_cigar_build"] = round(out["call_ms"][0] / out["cigar_build_ms"][0], 3)
    out["counts_only_over_cigar_build"] = round(out["counts_only_ms"][0] / out["cigar_build_ms"][0], 3)
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 3 and sys.argv[3]:
        with open(sys.argv[3], "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
