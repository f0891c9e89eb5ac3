"""The variant calls (swg_variant_records_device) timed over resident columns of the benchmark's shape with the
input, the batch and the method of tools/diffs_bench.py: the first kept records (a random 30 % status) whose CIGAR text fits a
default batch, each with the synthetic CIGAR of tools/lift_exact_bench.py at diff_every = DIFF_EVERY.  The sequences are random
bases generated on the device, every sequence as long as its longest record needs: a quarter of the X columns are then `same`, and
the inserted and deleted bases are whatever lies there.
  (a) the call with counts and pairs only (no variant is built) and the call with variants and pool fetched to the host, under the
      capacity protocol's second call: a host clock around calls that end in a device synchronise, warmed up, median of REPS;
  (b) the HIP-event split per kernel of one more call with variants (memsets, read-backs and copies carry no events);
  (c) two yardsticks in the same run: cigar_build alone (swg_lift_exact_records_device without regions) and
      swg_diff_records_device without rows, timed as (a);
  (d) the M-only text -- every = and X run of the same CIGARs written as M, so that every aligned column is a candidate -- over the
      first entries whose columns stay below 2.4 * 10^9 (three quarters of them differ, and one call takes fewer than 2^31 variants): counts only, its rate in columns per second beside the
      2 bytes a column must read, and the event split of that call.

    python tools/variants_bench.py [n_records] [n_genomes] [out.json] [diff_every]     -> one JSON line on standard output (and into out.json)

The result is kept as profiles/variants_bench_100m.json.
"""
import json
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
import sweepga_amd as sw  # noqa: E402
from sweepga_amd.diffs import diff_records_device  # noqa: E402
from sweepga_amd.lift import lift_exact_records_device  # noqa: E402
from sweepga_amd.variants import variant_records_device  # noqa: E402
from tools.diffs_bench import DIFF_EVERY  # noqa: E402
from tools.lift_bench import REPS, timed  # noqa: E402
from tools.lift_exact_bench import CIGAR_OWN, DIFF_UNIT, synthetic_cigar  # noqa: E402

VARIANTS_OWN = ("variants_letters", "variants_entries", "variants_ops", "variants_columns", "variants_rows", "variants_alleles", "variants_collect")
RUN = re.compile(r"(\d+)([=XM])")


def m_only(text):
    """every run of = and X ops as one M op"""
    out, run = [], 0
    for part in re.findall(r"\d+[A-Z=]", text):
        m = RUN.fullmatch(part)
        if m:
            run += int(m.group(1))
            continue
        if run:
            out.append("%dM" % run)
            run = 0
        out.append(part)
    if run:
        out.append("%dM" % run)
    return "".join(out)


def device_set(texts, device):
    offset = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in texts], out=offset[1:])
    return torch.from_numpy(offset).to(device), torch.from_numpy(np.frombuffer(b"".join(texts) or b"\0", dtype=np.uint8).copy()).to(device), int(offset[-1])


def note(what):
    print("variants_bench: " + what, file=sys.stderr, flush=True)


def split(ctx, f):
    ctx.profile_reset()
    ctx.profile(True)
    f()
    ctx.profile(False)
    return {name: round(v[1], 3) for name, v in ctx.profile_table().items()}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    every = int(sys.argv[4]) if len(sys.argv) > 4 else DIFF_EVERY
    if not torch.cuda.is_available():
        raise SystemExit("variants_bench: no GPU (there is no CPU path to time)")
    device = torch.device("cuda:0")
    ctx = sw.Context(0)
    cols, _ = bench.gen_shard(torch, n, G, 2025, device)
    status = (torch.rand(n, device=device) < 0.3).to(torch.uint8)
    n_seq = int(cols["seq_genome_last"].numel())
    sync = lambda: (torch.cuda.synchronize(), ctx.synchronize())   # noqa: E731
    sync()
    batch = min(torch.cuda.mem_get_info()[0] // 64, 1 << 30)
    wide = lambda name: cols[name].long() & 0xffffffff   # noqa: E731
    lq, lt = wide("q_end") - wide("q_start"), wide("t_end") - wide("t_start")
    kept = torch.nonzero(status).flatten()
    unit = len(DIFF_UNIT) if every > 0 else 6
    bound = unit * (torch.minimum(lq, lt)[kept] // 200) + 16      # at least a record's text
    k = int(torch.searchsorted(torch.cumsum(bound, 0), batch).item())
    assert k > 0
    at = kept[:k]
    lq_h, lt_h = lq[at].cpu().numpy(), lt[at].cpu().numpy()
    note("%d entries: writing their CIGARs" % k)
    texts = [synthetic_cigar(int(a), int(b), every) for a, b in zip(lq_h, lt_h)]
    # the sequences: each as long as its longest record needs, random bases
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
    d_offset, d_text, cigar_bytes = device_set([t.encode() for t in texts], device)
    assert cigar_bytes <= batch
    common = dict(status=status, set="kept", max_indel=10_000)
    call = lambda cap, off=d_offset, text=d_text, kk=k: variant_records_device(ctx, cols, cols["strand"], n_seq, genome, n_genome, d_record, off, text, kk,   # noqa: E731
                                                                                seq_offset, bases, capacity=cap, **common)
    note("%d bases on the device: the first call" % total_bases)
    first = call((None, None, None))
    f = lambda: call((first.n_variants, first.pool_bytes, first.n_pairs))   # noqa: E731
    got = f()
    assert got.variants is not None and len(got.variants) == first.n_variants and len(got.pool) == first.pool_bytes
    sums = {name: int(got.pairs[name].sum()) for name in ("entries", "compared", "snvs", "same", "m_equal", "n_columns", "n_ins", "ins_bases", "n_del", "del_bases",
                                                          "long_indels", "unanchored")}
    out = {"n": n, "n_genomes": G, "n_seq": n_seq, "reps": REPS, "batch_bytes": int(batch), "diff_every": every, "entries": k, "cigar_bytes": cigar_bytes,
           "bases": total_bases, "ops": got.ops, "variants": got.n_variants, "pool_bytes": got.pool_bytes, "pairs": got.n_pairs, "usable": got.usable,
           "cigar_bad": got.cigar_bad, "columns": got.columns, "sums": sums}
    note("%d variants, %d pool bytes: timing" % (got.n_variants, got.pool_bytes))
    out["counts_only_ms"] = timed(lambda: call((None, None, first.n_pairs)), sync)
    out["call_ms"] = timed(f, sync)
    table = split(ctx, f)
    out["kernels_ms"] = table
    out["cigar_kernels_ms"] = round(sum(v for name, v in table.items() if name in CIGAR_OWN), 3)
    out["variants_kernels_ms"] = round(sum(v for name, v in table.items() if name in VARIANTS_OWN), 3)
    regs = torch.zeros((1, 4), dtype=torch.int32, device=device)
    g = lambda: lift_exact_records_device(ctx, cols, cols["strand"], n_seq, regs, 0, d_record, d_offset, d_text, k, status=status, set="kept",   # noqa: E731
                                          capacity=0)
    assert g().ops == got.ops
    out["cigar_build_ms"] = timed(g, sync)
    d = lambda: diff_records_device(ctx, cols, cols["strand"], n_seq, genome, n_genome, d_record, d_offset, d_text, k, status=status, set="kept",   # noqa: E731
                                    kinds=15, min_indel=1, capacity=(None, first.n_pairs))
    assert d().ops == got.ops
    out["diffs_counts_only_ms"] = timed(d, sync)
    for name in ("counts_only", "call"):
        out[name + "_over_cigar_build"] = round(out[name + "_ms"][0] / out["cigar_build_ms"][0], 3)
        out[name + "_over_diffs_counts_only"] = round(out[name + "_ms"][0] / out["diffs_counts_only_ms"][0], 3)
    # the M-only text over the first entries of the set
    note("the yardsticks are timed: the M-only text")
    aligned = np.minimum(lq_h, lt_h).astype(np.int64)
    km = int(np.searchsorted(np.cumsum(aligned), (1 << 31) + (1 << 28)))      # (three quarters of random columns differ: fewer than 2^31 variants)
    m_offset, m_text, m_bytes = device_set([m_only(t).encode() for t in texts[:km]], device)
    del texts
    fm = lambda: call((None, None, first.n_pairs), m_offset, m_text, km)   # noqa: E731
    gm = fm()
    out["m_only"] = {"entries": km, "cigar_bytes": m_bytes, "ops": gm.ops, "columns": gm.columns, "variants": gm.n_variants,
                     "m_equal": int(gm.pairs["m_equal"].sum()), "counts_only_ms": timed(fm, sync)}
    mt = split(ctx, fm)
    out["m_only"]["kernels_ms"] = mt
    col_ms = mt.get("variants_columns", 0.0)
    out["m_only"]["columns_per_s_call"] = round(gm.columns / (out["m_only"]["counts_only_ms"][0] * 1e-3))
    out["m_only"]["columns_per_s_kernel"] = round(gm.columns / (col_ms * 1e-3)) if col_ms else None
    out["m_only"]["kernel_read_GBps_at_2_bytes_per_column"] = round(2 * gm.columns / (col_ms * 1e-3) / 1e9, 1) if col_ms else None
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 3 and sys.argv[3]:
        with open(sys.argv[3], "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
