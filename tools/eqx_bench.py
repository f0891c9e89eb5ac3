"""The resolved CIGARs (swg_eqx_records_device) timed over resident columns of the benchmark's shape with the
input and the method of tools/variants_bench.py: the first kept records (a random 30 % status) whose aligned columns stay below
2.4 * 10^9 (one call takes fewer than 2^32 columns; the same cut as the variant calls' M-only leg, so that both see one set), each
with the synthetic CIGAR of tools/lift_exact_bench.py at diff_every = DIFF_EVERY, and the same CIGARs with every run of = and X
written as one M.  The sequences are random bases generated on the device, every sequence as long as its longest record needs: three
quarters of all columns then differ, so the = ops are mostly wrong and the output is close to its densest.  On both texts:
  (a) one call with counts only (no text is built) and one with entries and text fetched to the host: a host clock around calls that
      end in a device synchronise, warmed up, median, min and max of REPS;
  (b) the HIP-event split per kernel of one more call with text (memsets, read-backs and copies carry no events), the column pass's
      rate in columns per second, and the text kernel's output bytes per second beside a device-to-device copy of as many bytes;
  (c) two yardsticks in the same run on the same set: cigar_build alone (swg_lift_exact_records_device without regions) and
      swg_variant_records_device with counts only, whose variants_columns reads the same two bytes per column (on the =/X text its
      candidates are the X columns only; on the M-only text they are all columns).

    python tools/eqx_bench.py [n_records] [n_genomes] [out.json] [diff_every]     -> one JSON line on standard output (and into out.json)

The result is kept as profiles/eqx_bench_100m.json.  Not measured here: real sequences, and the PAF seam's host formatting.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
import sweepga_amd as sw  # noqa: E402
from sweepga_amd.eqx import eqx_records_device  # noqa: E402
from sweepga_amd.lift import lift_exact_records_device  # noqa: E402
from sweepga_amd.variants import variant_records_device  # noqa: E402
from tools.diffs_bench import DIFF_EVERY  # noqa: E402
from tools.lift_bench import REPS, timed  # noqa: E402
from tools.lift_exact_bench import CIGAR_OWN, synthetic_cigar  # noqa: E402
from tools.variants_bench import device_set, m_only, split  # noqa: E402

EQX_OWN = ("eqx_offsets", "eqx_letters", "eqx_entries", "eqx_ops", "eqx_columns", "eqx_generated", "eqx_verbatim", "eqx_finish", "eqx_text")
COLUMN_LIMIT = (1 << 31) + (1 << 28)


def note(what):
    print("eqx_bench: " + what, file=sys.stderr, flush=True)


def copy_ms(n_bytes, device):
    """a device-to-device copy of n_bytes: median of REPS by HIP events"""
    src = torch.empty(max(n_bytes, 1), dtype=torch.uint8, device=device)
    dst = torch.empty_like(src)
    dst.copy_(src)
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return round(float(np.median(ts)), 4)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    every = int(sys.argv[4]) if len(sys.argv) > 4 else DIFF_EVERY
    if not torch.cuda.is_available():
        raise SystemExit("eqx_bench: no GPU (there is no CPU path to time)")
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
    k = int(torch.searchsorted(torch.cumsum(aligned, 0), COLUMN_LIMIT).item())
    assert k > 0
    at = kept[:k]
    lq_h, lt_h = lq[at].cpu().numpy(), lt[at].cpu().numpy()
    note("%d entries: writing their CIGARs" % k)
    texts = [synthetic_cigar(int(a), int(b), every) for a, b in zip(lq_h, lt_h)]
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
    genome = cols["seq_genome_last"]
    n_genome = int(genome.max().item()) + 1
    d_record = at.to(torch.int32).contiguous()
    out = {"n": n, "n_genomes": G, "n_seq": n_seq, "reps": REPS, "diff_every": every, "entries": k, "bases": total_bases}
    regs = torch.zeros((1, 4), dtype=torch.int32, device=device)
    for leg, leg_texts in (("eqx_text", [t.encode() for t in texts]), ("m_only", [m_only(t).encode() for t in texts])):
        d_offset, d_text, cigar_bytes = device_set(leg_texts, device)
        del leg_texts
        call = lambda cap: eqx_records_device(ctx, cols, cols["strand"], n_seq, d_record, d_offset, d_text, k, seq_offset, bases, status=status, set="kept",   # noqa: E731,B023
                                              capacity=cap)
        note("%s: %d bytes of CIGAR text, the first call" % (leg, cigar_bytes))
        first = call((None, None))
        f = lambda: call((k, first.text_bytes))   # noqa: E731,B023
        got = f()
        assert got.text is not None and len(got.text) == first.text_bytes and got.usable == k
        o = {"cigar_bytes": cigar_bytes, "ops": got.ops, "usable": got.usable, "columns": got.columns, "out_ops": got.out_ops, "text_bytes": got.text_bytes,
             "changed": got.changed, "sums": {name: getattr(got, name) for name in ("matches", "mismatches", "n_columns", "eq_wrong", "x_wrong", "m_columns")}}
        note("%s: %d columns, %d output ops, %d bytes: timing" % (leg, got.columns, got.out_ops, got.text_bytes))
        o["counts_only_ms"] = timed(lambda: call((None, None)), sync)
        o["call_ms"] = timed(f, sync)
        table = split(ctx, f)
        o["kernels_ms"] = table
        o["cigar_kernels_ms"] = round(sum(v for name, v in table.items() if name in CIGAR_OWN), 3)
        o["eqx_kernels_ms"] = round(sum(v for name, v in table.items() if name in EQX_OWN), 3)
        col_ms, text_ms = table.get("eqx_columns", 0.0), table.get("eqx_text", 0.0)
        o["columns_per_s_kernel"] = round(got.columns / (col_ms * 1e-3)) if col_ms else None
        o["columns_kernel_read_GBps_at_2_bytes_per_column"] = round(2 * got.columns / (col_ms * 1e-3) / 1e9, 1) if col_ms else None
        o["text_kernel_GBps_written"] = round(got.text_bytes / (text_ms * 1e-3) / 1e9, 1) if text_ms else None
        o["device_copy_ms"] = copy_ms(got.text_bytes, device)
        o["device_copy_GBps_written"] = round(got.text_bytes / (o["device_copy_ms"] * 1e-3) / 1e9, 1) if o["device_copy_ms"] else None
        g = lambda: lift_exact_records_device(ctx, cols, cols["strand"], n_seq, regs, 0, d_record, d_offset, d_text, k, status=status, set="kept", capacity=0)   # noqa: E731,B023
        assert g().ops == got.ops
        o["cigar_build_ms"] = timed(g, sync)
        v = lambda: variant_records_device(ctx, cols, cols["strand"], n_seq, genome, n_genome, d_record, d_offset, d_text, k, seq_offset, bases, status=status,   # noqa: E731,B023
                                           set="kept", max_indel=10_000, capacity=(None, None, n_genome * n_genome))
        gv = v()
        assert gv.ops == got.ops and gv.usable == k
        o["variants_counts_only_ms"] = timed(v, sync)
        vt = split(ctx, v)
        vcol_ms = vt.get("variants_columns", 0.0)
        o["variants"] = {"candidates_compared": gv.columns, "variants": gv.n_variants, "variants_columns_ms": vcol_ms,
                         "columns_per_s_kernel": round(gv.columns / (vcol_ms * 1e-3)) if vcol_ms else None}
        o["counts_only_over_cigar_build"] = round(o["counts_only_ms"][0] / o["cigar_build_ms"][0], 3)
        o["counts_only_over_variants_counts_only"] = round(o["counts_only_ms"][0] / o["variants_counts_only_ms"][0], 3)
        out[leg] = o
        del d_offset, d_text
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 3 and sys.argv[3]:
        with open(sys.argv[3], "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
