"""The base-exact lift (swg_lift_exact_records_device) timed over resident columns of the benchmark's shape --
bench.gen_shard: G single-chromosome genomes, every ordered pair, pair-major -- in the manner of tools/lift_bench.py.  10^4 random
regions of 1 - 100 kb on random sequences, resident too.  The records that are hit come from swg_lift_hit_records_device; each gets a
synthetic CIGAR of about one op per 100 bases that adds up to its two sides (runs of `=` with an `X` every 200 bases, and one `I` or `D`
for the difference of the sides), laid end to end and uploaded once:
  (a) the whole call, both axes, the rows of the kept set under the two-call capacity protocol's second call (rows, summary and states
      come back to the host): a host clock around calls that end in a device synchronise, warmed up, median of REPS;
  (b) the HIP-event split per kernel of one more such call (the library's per-launch profile; memsets, read-backs and copies carry
      no events, so the split sums to less than (a));
and once, as the yardstick, (c) one swg_lift_records_device call on the same columns and regions, timed as (a), and the hit-record call.

    python tools/lift_exact_bench.py [n_records] [n_genomes] [n_regions] [out.json]     -> one JSON line on standard output (and into out.json)

The result is kept as profiles/lift_exact_bench_100m.json.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
import sweepga_amd as sw  # noqa: E402
from sweepga_amd.lift import lift_exact_records_device, lift_hit_records_device, lift_records_device  # noqa: E402
from tools.lift_bench import OWN, REPS, timed  # noqa: E402

CIGAR_OWN = ("cigar_set_check", "cigar_count", "cigar_parse", "cigar_entries", "cigar_refine")


DIFF_UNIT = "99=1X48=2I50=2D"      # 200 bases on either side, as "198=2X": a mismatch, a 2-base insertion and a 2-base deletion


def synthetic_cigar(lq, lt, diff_every=0):
    """About one op per 100 bases, the sides' sums exact.  diff_every = N > 0: every N-th unit of 200 bases is DIFF_UNIT (for
    tools/diffs_bench.py, which needs indels inside the mappings); 0: the text as it always was."""
    both = min(lq, lt)
    units = both // 200
    if diff_every > 0:
        text = ("198=2X" * (diff_every - 1) + DIFF_UNIT) * (units // diff_every) + "198=2X" * (units % diff_every)
    else:
        text = "198=2X" * units
    if both % 200:
        text += "%d=" % (both % 200)
    if lq != lt:
        text += "%d%s" % (abs(lq - lt), "I" if lq > lt else "D")
    return text


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    m = int(sys.argv[3]) if len(sys.argv) > 3 and int(sys.argv[3]) else 10_000
    if not torch.cuda.is_available():
        raise SystemExit("lift_exact_bench: no GPU (there is no CPU path to time)")
    device = torch.device("cuda:0")
    ctx = sw.Context(0)
    cols, _ = bench.gen_shard(torch, n, G, 2025, device)
    status = (torch.rand(n, device=device) < 0.3).to(torch.uint8)
    n_seq = int(cols["seq_genome_last"].numel())
    top = int((cols["q_end"].long() & 0xffffffff).max().item())
    sync = lambda: (torch.cuda.synchronize(), ctx.synchronize())   # noqa: E731
    gen = torch.Generator(device=device)
    gen.manual_seed(7)
    start = torch.randint(0, max(top, 1), (m,), device=device, generator=gen)
    width = torch.randint(1_000, 100_001, (m,), device=device, generator=gen)
    regs = torch.stack([torch.randint(0, n_seq, (m,), device=device, generator=gen), start, start + width, torch.zeros_like(start)], 1)
    regs = regs.to(torch.int32).contiguous()   # (values below 2^31: the bits are those of the uint32 the library reads)
    kw = dict(status=status, set="kept", axes="both")
    sync()
    hit, k = lift_hit_records_device(ctx, cols, cols["strand"], n_seq, regs, m, **kw)
    at = torch.from_numpy(hit.astype(np.int64)).to(device)
    sides = [(cols[b].long()[at] & 0xffffffff) - (cols[a].long()[at] & 0xffffffff) for a, b in (("q_start", "q_end"), ("t_start", "t_end"))]
    lq, lt = (s.cpu().numpy() for s in sides)
    texts = [synthetic_cigar(int(a), int(b)).encode() for a, b in zip(lq, lt)]
    offset = np.zeros(k + 1, dtype=np.int64)
    np.cumsum([len(t) for t in texts], out=offset[1:])
    d_record = torch.from_numpy(hit.astype(np.int32)).to(device)
    d_offset = torch.from_numpy(offset).to(device)
    d_text = torch.from_numpy(np.frombuffer(b"".join(texts) or b"\0", dtype=np.uint8).copy()).to(device)
    call = lambda cap: lift_exact_records_device(ctx, cols, cols["strand"], n_seq, regs, m, d_record, d_offset, d_text, k, capacity=cap, **kw)   # noqa: E731
    first = call(0)
    f = lambda: call(first.n)   # noqa: E731
    got = f()
    out = {"n": n, "n_genomes": G, "n_seq": n_seq, "reps": REPS, "regions": m, "hit_records": k, "text_bytes": int(offset[-1]), "ops": got.ops,
           "rows": got.n, "exact_rows": got.exact_rows, "cigar_bad": got.cigar_bad, "aligned": int(got.rows["aligned"].astype(np.int64).sum()),
           "matches": int(got.rows["matches"].astype(np.int64).sum())}
    out["call_ms"] = timed(f, sync)
    ctx.profile_reset()
    ctx.profile(True)
    f()
    ctx.profile(False)
    table = {name: round(v[1], 3) for name, v in ctx.profile_table().items()}
    out["kernels_ms"] = table
    out["cigar_kernels_ms"] = round(sum(v for name, v in table.items() if name in CIGAR_OWN), 3)
    out["lift_kernels_ms"] = round(sum(v for name, v in table.items() if name in OWN), 3)
    g = lambda: lift_records_device(ctx, cols, cols["strand"], n_seq, regs, m, capacity=first.n, **kw)   # noqa: E731
    out["lift_ms"] = timed(g, sync)
    out["hit_records_ms"] = timed(lambda: lift_hit_records_device(ctx, cols, cols["strand"], n_seq, regs, m, capacity=k, **kw), sync)
    out["call_over_lift"] = round(out["call_ms"][0] / out["lift_ms"][0], 3)
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
