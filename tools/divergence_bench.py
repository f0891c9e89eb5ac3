"""The divergence track (swg_divergence_records_device) timed over resident columns of the benchmark's shape --
bench.gen_shard: G single-chromosome genomes, every ordered pair, pair-major -- with the input, the batch and the method of
tools/diffs_bench.py.  The set is the first kept records (a random 30 % status) whose CIGAR text fits a default batch: 1/64 of the
free device memory, at most 1 GiB.  Each gets the synthetic CIGAR of tools/lift_exact_bench.py with diff_every = DIFF_EVERY.  Query
axis, W = 10,000, any other genome:
  (a) the whole call with rows and summary into arrays of the exact capacity (they come back to the host): a host clock around calls
      that end in a device synchronise, warmed up, median of REPS; and the same with the summary only;
  (b) the HIP-event split per kernel of one more call with both (the library's per-launch profile; memsets, read-backs and copies
      carry no events, so the split sums to less than (a));
and in the same run on the same set, as the two yardsticks,
  (c) cigar_build alone -- parse, scans, entries: swg_lift_exact_records_device without regions -- timed as (a);
  (d) swg_diff_records_device without rows (counts, pairs and spectrum), timed as (a).

    python tools/divergence_bench.py [n_records] [n_genomes] [out.json] [diff_every]   -> one JSON line on standard output (and into out.json)

The result is kept as profiles/divergence_bench_100m.json.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
import sweepga_amd as sw  # noqa: E402
from sweepga_amd import _lib  # noqa: E402
from sweepga_amd._marshal import records_from_tensors  # noqa: E402
from sweepga_amd.diffs import diff_records_device  # noqa: E402
from sweepga_amd.divergence import ROW_DTYPE, SEQ_DTYPE, divergence_records_device  # noqa: E402
from sweepga_amd.lift import COLUMNS, lift_exact_records_device  # noqa: E402
from tools.lift_bench import REPS, timed  # noqa: E402
from tools.lift_exact_bench import CIGAR_OWN, DIFF_UNIT, synthetic_cigar  # noqa: E402

DIVERGENCE_OWN = ("divergence_listing", "divergence_counts", "divergence_letters", "divergence_entries", "divergence_ops", "divergence_rows",
                  "divergence_seqs")
DIFF_EVERY = 4
WINDOW = 10_000


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    every = int(sys.argv[4]) if len(sys.argv) > 4 else DIFF_EVERY
    if not torch.cuda.is_available():
        raise SystemExit("divergence_bench: no GPU (there is no CPU path to time)")
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
    length = max(150_000_000, int((cols["q_end"].long() & 0xffffffff).max()), int((cols["t_end"].long() & 0xffffffff).max()))
    seq_len = torch.full((n_seq,), length, dtype=torch.int32, device=device)
    d_record = at.to(torch.int32).contiguous()
    d_offset = torch.from_numpy(offset).to(device)
    d_text = torch.from_numpy(np.frombuffer(b"".join(texts) or b"\0", dtype=np.uint8).copy()).to(device)
    del texts
    call = lambda want: divergence_records_device(ctx, cols, cols["strand"], seq_len, genome, n_genome, d_record, d_offset, d_text, k, status=status,   # noqa: E731
                                                  set="kept", axis="query", window=WINDOW, want=want)
    got = call(3)
    sums = {name: int(got.seqs[name].sum()) for name in got.seqs.dtype.names[2:]}
    out = {"n": n, "n_genomes": G, "n_seq": n_seq, "reps": REPS, "batch_bytes": int(batch), "diff_every": every, "entries": k, "cigar_bytes": int(offset[-1]),
           "axis": "query", "window": WINDOW, "seq_len": length, "ops": got.ops, "windows": got.n_rows, "listed": got.n_seqs, "usable": got.usable,
           "cigar_bad": got.cigar_bad, "sums": sums, "box": torch.cuda.get_device_name(0)}
    # what is timed is the protocol's LAST call: arrays of the exact capacity, written once
    rec = records_from_tensors(cols, {c: 4 for c in COLUMNS}, n_seq)
    rec.strand = int(cols["strand"].data_ptr())
    cs = _lib.SwgCigarSet()
    cs.record, cs.offset, cs.text, cs.k = int(d_record.data_ptr()), int(d_offset.data_ptr()), int(d_text.data_ptr()), k
    rows, seqs = np.zeros(max(got.n_rows, 1), dtype=ROW_DTYPE), np.zeros(max(got.n_seqs, 1), dtype=SEQ_DTYPE)

    def one(want):
        req = _lib.SwgDivergenceRequest()
        req.set, req.axis, req.window, req.other_genome, req.want = 1, 0, WINDOW, 0xffffffff, want
        req.capacity, req.rows, req.seq_capacity, req.seqs = len(rows), rows.ctypes.data, len(seqs), seqs.ctypes.data
        ctx.check(ctx.lib.swg_divergence_records_device(ctx.handle, C.byref(rec), int(seq_len.data_ptr()), int(genome.data_ptr()), n_genome,
                                                        int(status.data_ptr()), C.byref(cs), C.byref(req)))
        return req

    assert one(3).usable == got.usable and rows[:got.n_rows].tobytes() == got.rows.tobytes()
    out["call_ms"] = timed(lambda: one(3), sync)
    out["summary_only_ms"] = timed(lambda: one(2), sync)
    ctx.profile_reset()
    ctx.profile(True)
    one(3)
    ctx.profile(False)
    table = {name: round(v[1], 3) for name, v in ctx.profile_table().items()}
    out["kernels_ms"] = table
    out["cigar_kernels_ms"] = round(sum(v for name, v in table.items() if name in CIGAR_OWN), 3)
    out["divergence_kernels_ms"] = round(sum(v for name, v in table.items() if name in DIVERGENCE_OWN), 3)
    regs = torch.zeros((1, 4), dtype=torch.int32, device=device)
    g = lambda: lift_exact_records_device(ctx, cols, cols["strand"], n_seq, regs, 0, d_record, d_offset, d_text, k, status=status, set="kept",   # noqa: E731
                                          capacity=0)
    assert g().ops == got.ops
    out["cigar_build_ms"] = timed(g, sync)
    first = diff_records_device(ctx, cols, cols["strand"], n_seq, genome, n_genome, d_record, d_offset, d_text, k, status=status, set="kept", kinds=15,
                                capacity=(None, None))
    d = lambda: diff_records_device(ctx, cols, cols["strand"], n_seq, genome, n_genome, d_record, d_offset, d_text, k, status=status, set="kept",   # noqa: E731
                                    kinds=15, capacity=(None, first.n_pairs))
    assert d().ops == got.ops
    out["diffs_counts_only_ms"] = timed(d, sync)
    ctx.profile_reset()
    ctx.profile(True)
    d()
    ctx.profile(False)
    out["diffs_kernels_ms"] = {name: round(v[1], 3) for name, v in ctx.profile_table().items() if name.startswith("diffs_")}
    out["call_over_cigar_build"] = round(out["call_ms"][0] / out["cigar_build_ms"][0], 3)
    out["call_over_diffs_counts_only"] = round(out["call_ms"][0] / out["diffs_counts_only_ms"][0], 3)
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 3 and sys.argv[3]:
        with open(sys.argv[3], "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
