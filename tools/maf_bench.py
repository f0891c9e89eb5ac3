"""The alignment blocks (swg_maf_records_device) timed over resident columns of the benchmark's shape with the
input and the method of tools/eqx_bench.py: the first kept records (a random 30 % status) whose aligned columns stay below
2.4 * 10^9, each with the synthetic CIGAR of tools/lift_exact_bench.py at diff_every = DIFF_EVERY, over random bases generated on
the device.  On that set:
  (a) one call with counts only (no text is built) and one with blocks and text fetched to the host: a host clock around calls that
      end in a device synchronise, warmed up, median, min and max of REPS;
  (b) the HIP-event split per kernel of one more call with text (memsets, read-backs and copies carry no events); maf_text's output
      bytes per second in the dword-per-lane and in the byte-per-lane form (SWG_MAF_TEXT_FORM=1), median of 5 splits each, beside a
      device-to-device copy of as many bytes;
  (c) in the same run on the same set: cigar_build alone (swg_lift_exact_records_device without regions), and eqx_text's output
      bytes per second from one swg_eqx_records_device call with text; slice_text's from tools/lift_paf_bench.py's unbalanced leg;
  (d) the same set with split_gap = 1: every gap a breaker, the most blocks the set can give;
  (e) an unbalanced leg on the host seam: one block of 5 * 10^6 columns (10 MB of text) beside 4,000 blocks of one column, and a
      balanced one of as many blocks and nearly as many bytes (4,001 blocks of 1,250 columns): maf_text alone from the kernel split,
      both forms, and the ratio of the two rates.

    python tools/maf_bench.py [n_records] [n_genomes] [out.json] [diff_every]     -> one JSON line on standard output (and into out.json)

The result is kept as profiles/maf_bench_100m.json.  Not measured here: real sequences, and the PAF seam's host formatting.
"""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
import sweepga_amd as sw  # noqa: E402
from sweepga_amd.eqx import eqx_records_device  # noqa: E402
from sweepga_amd.lift import lift_exact_records_device  # noqa: E402
from sweepga_amd.maf import maf_records, maf_records_device  # noqa: E402
from tools.diffs_bench import DIFF_EVERY  # noqa: E402
from tools.eqx_bench import COLUMN_LIMIT, copy_ms  # noqa: E402
from tools.lift_bench import REPS, timed  # noqa: E402
from tools.lift_exact_bench import CIGAR_OWN, synthetic_cigar  # noqa: E402
from tools.lift_paf_bench import unbalanced_leg as slice_unbalanced_leg  # noqa: E402
from tools.variants_bench import device_set, split  # noqa: E402

MAF_OWN = ("maf_offsets", "maf_entries", "maf_ops", "maf_runs", "maf_gather", "maf_first", "maf_text")
FORMS = (("4", "dword"), ("1", "byte"))


def note(what):
    print("maf_bench: " + what, file=sys.stderr, flush=True)


def gbps(n_bytes, ms):
    return round(n_bytes / (ms * 1e-3) / 1e9, 1) if ms else None


def both_forms(ctx, f, text_bytes, out):
    """maf_text alone from the kernel split, in both store forms: [median, min, max] of 5 and the output bytes per second"""
    for form, key in FORMS:
        os.environ["SWG_MAF_TEXT_FORM"] = form
        f()
        ms = [split(ctx, f)["maf_text"] for _ in range(5)]
        out["maf_text_%s_ms" % key] = [round(statistics.median(ms), 3), min(ms), max(ms)]
        out["maf_text_%s_GBps_written" % key] = gbps(text_bytes, statistics.median(ms))
    del os.environ["SWG_MAF_TEXT_FORM"]


def host_leg(ctx, lengths, out, sync, device):
    """One record of `<l>M` per length over one sequence of random bases, the strands in turn, on the host seam"""
    rng = np.random.default_rng(5)
    n = len(lengths)
    starts = np.concatenate([[0], np.cumsum(np.asarray(lengths) + 3)[:-1]]).astype(np.uint32)
    lens = np.asarray(lengths, dtype=np.uint32)
    total = int(starts[-1] + lens[-1]) + 8
    seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=total).tobytes()
    texts = ["%dM" % l for l in lengths]
    cols = {"q_id": np.zeros(n, dtype=np.uint32), "t_id": np.ones(n, dtype=np.uint32), "q_start": starts, "q_end": starts + lens, "t_start": starts,
            "t_end": starts + lens}
    strand = (np.arange(n) % 2).astype(np.uint8)
    first = maf_records(ctx, cols, strand, 2, list(range(n)), texts, [seq, seq], capacity=(None, None))
    f = lambda: maf_records(ctx, cols, strand, 2, list(range(n)), texts, [seq, seq], capacity=(first.n_blocks, first.text_bytes))   # noqa: E731
    got = f()
    assert got.n_blocks == n and got.text_bytes == 2 * int(lens.sum()) and got.rows(0)[0] == seq[:lengths[0]]
    out.update(blocks=got.n_blocks, text_bytes=got.text_bytes, longest=2 * int(max(lengths)))
    both_forms(ctx, f, got.text_bytes, out)
    out["device_copy_ms"] = copy_ms(got.text_bytes, device)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    every = int(sys.argv[4]) if len(sys.argv) > 4 else DIFF_EVERY
    if not torch.cuda.is_available():
        raise SystemExit("maf_bench: no GPU (there is no CPU path to time)")
    device = torch.device("cuda:0")
    ctx = sw.Context(0)
    cols, _ = bench.gen_shard(torch, n, G, 2025, device)
    status = (torch.rand(n, device=device) < 0.3).to(torch.uint8)
    n_seq = int(cols["seq_genome_last"].numel())
    sync = lambda: (torch.cuda.synchronize(), ctx.synchronize())   # noqa: E731
    sync()
    wide = lambda name: cols[name].long() & 0xffffffff   # noqa: E731
    lq, lt = wide("q_end") - wide("q_start"), wide("t_end") - wide("t_start")
    kept = torch.nonzero(status).flatten()
    aligned = torch.minimum(lq, lt)[kept]
    k = int(torch.searchsorted(torch.cumsum(aligned, 0), min(COLUMN_LIMIT, int(aligned.sum().item()))).item())
    k = max(k, 1)
    at = kept[:k]
    lq_h, lt_h = lq[at].cpu().numpy(), lt[at].cpu().numpy()
    note("%d entries: writing their CIGARs" % k)
    texts = [synthetic_cigar(int(a), int(b), every).encode() for a, b in zip(lq_h, lt_h)]
    seq_len = torch.zeros(n_seq, dtype=torch.int64, device=device)
    seq_len.scatter_reduce_(0, cols["q_id"].long(), wide("q_end"), "amax")
    seq_len.scatter_reduce_(0, cols["t_id"].long(), wide("t_end"), "amax")
    seq_offset = torch.zeros(n_seq + 1, dtype=torch.int64, device=device)
    seq_offset[1:] = torch.cumsum(seq_len, 0)
    total_bases = int(seq_offset[-1].item())
    letters = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=device)
    bases = torch.empty(max(total_bases, 1), dtype=torch.uint8, device=device)
    for s0, s1 in zip(seq_offset[:-1].tolist(), seq_offset[1:].tolist()):
        if s1 > s0:
            bases[s0:s1] = letters[torch.randint(0, 4, (s1 - s0,), device=device)]
    d_record = at.to(torch.int32).contiguous()
    out = {"n": n, "n_genomes": G, "n_seq": n_seq, "reps": REPS, "diff_every": every, "entries": k, "bases": total_bases}
    regs = torch.zeros((1, 4), dtype=torch.int32, device=device)
    d_offset, d_text, cigar_bytes = device_set(texts, device)
    del texts
    call = lambda cap, g=0: maf_records_device(ctx, cols, cols["strand"], n_seq, d_record, d_offset, d_text, k, seq_offset, bases, status=status, set="kept",   # noqa: E731
                                               split_gap=g, capacity=cap)
    note("%d bytes of CIGAR text, the first call" % cigar_bytes)
    first = call((None, None))
    f = lambda: call((first.n_blocks, first.text_bytes))   # noqa: E731
    got = f()
    assert got.text is not None and len(got.text) == first.text_bytes == 2 * got.columns and got.usable == k == got.n_blocks
    o = {"cigar_bytes": cigar_bytes, "ops": got.ops, "usable": got.usable, "blocks": got.n_blocks, "columns": got.columns, "aligned": got.aligned,
         "text_bytes": got.text_bytes}
    note("%d columns, %d bytes: timing" % (got.columns, got.text_bytes))
    o["counts_only_ms"] = timed(lambda: call((None, None)), sync)
    o["call_ms"] = timed(f, sync)
    table = split(ctx, f)
    o["kernels_ms"] = table
    o["cigar_kernels_ms"] = round(sum(v for name, v in table.items() if name in CIGAR_OWN), 3)
    o["maf_kernels_ms"] = round(sum(v for name, v in table.items() if name in MAF_OWN), 3)
    both_forms(ctx, f, got.text_bytes, o)
    o["device_copy_ms"] = copy_ms(got.text_bytes, device)
    o["device_copy_GBps_written"] = gbps(got.text_bytes, o["device_copy_ms"])
    g = lambda: lift_exact_records_device(ctx, cols, cols["strand"], n_seq, regs, 0, d_record, d_offset, d_text, k, status=status, set="kept", capacity=0)   # noqa: E731
    assert g().ops == got.ops
    o["cigar_build_ms"] = timed(g, sync)
    o["counts_only_over_cigar_build"] = round(o["counts_only_ms"][0] / o["cigar_build_ms"][0], 3)
    del got
    note("eqx_text on the same set")
    e0 = eqx_records_device(ctx, cols, cols["strand"], n_seq, d_record, d_offset, d_text, k, seq_offset, bases, status=status, set="kept", capacity=(None, None))
    ef = lambda: eqx_records_device(ctx, cols, cols["strand"], n_seq, d_record, d_offset, d_text, k, seq_offset, bases, status=status, set="kept",   # noqa: E731
                                    capacity=(k, e0.text_bytes))
    ef()
    et = split(ctx, ef)
    o["eqx_text"] = {"text_bytes": e0.text_bytes, "eqx_text_ms": et.get("eqx_text"), "GBps_written": gbps(e0.text_bytes, et.get("eqx_text"))}
    note("split_gap = 1")
    s0 = call((None, None), 1)
    sf = lambda: call((s0.n_blocks, s0.text_bytes), 1)   # noqa: E731
    sf()
    o["split_gap_1"] = {"blocks": s0.n_blocks, "breakers": s0.breakers, "gap_only": s0.gap_only, "text_bytes": s0.text_bytes, "kernels_ms": split(ctx, sf),
                        "counts_only_ms": timed(lambda: call((None, None), 1), sync)}
    out["maf_100m"] = o
    del d_offset, d_text, bases, cols
    torch.cuda.empty_cache()
    note("the unbalanced and the balanced leg")
    out["unbalanced"], out["balanced"] = {}, {}
    host_leg(ctx, [5_000_000] + [1] * 4_000, out["unbalanced"], sync, device)
    host_leg(ctx, [1_250] * 4_001, out["balanced"], sync, device)
    out["unbalanced_over_balanced_rate_dword"] = round(out["unbalanced"]["maf_text_dword_GBps_written"] / out["balanced"]["maf_text_dword_GBps_written"], 3)
    tmp = {}
    slice_unbalanced_leg(ctx, tmp, sync)
    u = tmp["unbalanced"]
    out["slice_text_unbalanced"] = {"text_bytes": u["text_bytes"], "slice_text_dword_ms": u["slice_text_dword_ms"],
                                    "GBps_written": gbps(u["text_bytes"], u["slice_text_dword_ms"][0])}
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 3 and sys.argv[3]:
        with open(sys.argv[3], "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
