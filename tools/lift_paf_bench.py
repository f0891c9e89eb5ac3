"""The lift slices (swg_lift_slice_records_device) timed on the workload of tools/lift_exact_bench.py: resident
columns of the benchmark's shape, 10^4 random regions of 1 - 100 kb, the hit records' synthetic CIGARs uploaded once.  In one run:
  (a) the exact lift's call on the same set, rows fetched: the reference point (profiles/lift_exact_bench_100m.json);
  (b) the slice call with counts only (no slices, no text: the text kernel does not run), and (c) with slices and text fetched under
      the two-call protocol's second call: a host clock around calls that end in a device synchronise, warmed up, median of REPS;
  (d) the HIP-event split per kernel of one more call of (c), and from it slice_text's (bytes read + bytes written) / time -- the
      verbatim bytes, 24 bytes of plan and 8 of end per slice, the text -- beside a device-to-device hipMemcpyAsync of text_bytes timed
      in the same run, the bound the copy kernel is judged against; the same for the byte-per-lane form (SWG_SLICE_TEXT_FORM=1);
  (e) the unbalanced leg the tiling exists for: one region over a whole record of 10^8 bases whose CIGAR has megabytes, beside 4,000
      records of nine bytes under the same region; slice_text alone from the kernel split, both forms.

    python tools/lift_paf_bench.py [n_records] [n_genomes] [n_regions] [out.json]     -> one JSON line on standard output (and into out.json)

The result is kept as profiles/lift_paf_bench_100m.json.
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
import sweepga_amd as sw  # noqa: E402
from sweepga_amd.lift import lift_exact_records_device, lift_hit_records_device, lift_slice_records, lift_slice_records_device  # noqa: E402
from tools.lift_bench import REPS, timed  # noqa: E402
from tools.lift_exact_bench import synthetic_cigar  # noqa: E402

SLICE_OWN = ("slice_op_pos", "slice_rows", "slice_gather", "slice_first", "slice_text")


def kernel_split(ctx, f):
    ctx.profile_reset()
    ctx.profile(True)
    f()
    ctx.profile(False)
    return {name: round(v[1], 3) for name, v in ctx.profile_table().items()}


def text_rate(ms, got):
    """(bytes read + bytes written) / time of slice_text in GB/s: the text written, its bytes read, a plan and an end per slice"""
    moved = 2 * got.counts["text_bytes"] + 32 * got.counts["n_slices"]
    return round(moved / (ms * 1e-3) / 1e9, 1) if ms else None


def both_forms(ctx, f, got, out, prefix):
    for form, key in (("4", "dword"), ("1", "byte")):
        os.environ["SWG_SLICE_TEXT_FORM"] = form
        ms = [kernel_split(ctx, f)["slice_text"] for _ in range(5)]
        out["%sslice_text_%s_ms" % (prefix, key)] = [round(statistics.median(ms), 3), min(ms), max(ms)]
        out["%sslice_text_%s_gbs" % (prefix, key)] = text_rate(statistics.median(ms), got)
    del os.environ["SWG_SLICE_TEXT_FORM"]


def memcpy_ms(nbytes, sync):
    """A device-to-device hipMemcpyAsync of nbytes on the null stream, host clock, warmed up: median, min, max"""
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    src = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device="cuda:0")
    dst = torch.empty_like(src)
    copy = lambda: hip.hipMemcpyAsync(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), C.c_size_t(nbytes), 3, None)   # noqa: E731  (3: device to device)
    ts = []
    for k in range(REPS + 2):
        sync()
        t0 = time.perf_counter()
        if copy() != 0:
            raise SystemExit("hipMemcpyAsync failed")
        hip.hipDeviceSynchronize()
        if k >= 2:
            ts.append((time.perf_counter() - t0) * 1e3)
    return [round(x, 3) for x in (statistics.median(ts), min(ts), max(ts))]


def unbalanced_leg(ctx, out, sync):
    """One record of 10^8 bases (`50=1X` throughout: 9.8 MB of text) and 4,000 records of 20 bases (`9=1X10=`, nine bytes) on one query
    sequence, one region over all of it: a slice of megabytes beside thousands of nine bytes."""
    long_n, small = 100_000_000, 4_000
    unit = long_n // 51
    texts = [("50=1X" * unit + "%d=" % (long_n - 51 * unit)).encode()] + [b"9=1X10="] * small
    starts = np.concatenate([[0], long_n + 10 + 30 * np.arange(small)]).astype(np.uint32)
    lens = np.concatenate([[long_n], np.full(small, 20)]).astype(np.uint32)
    cols = {"q_id": np.zeros(small + 1, dtype=np.uint32), "t_id": np.ones(small + 1, dtype=np.uint32), "q_start": starts, "q_end": starts + lens,
            "t_start": starts, "t_end": starts + lens}
    strand = np.zeros(small + 1, dtype=np.uint8)
    f = lambda: lift_slice_records(ctx, cols, strand, 2, [(0, 0, 2**32 - 1)], list(range(small + 1)), texts, axes="query")   # noqa: E731
    got = f()
    assert got.counts["n_slices"] == small + 1 and got.text == b"".join(texts)
    out["unbalanced"] = {"slices": got.counts["n_slices"], "text_bytes": got.counts["text_bytes"], "longest": len(texts[0])}
    both_forms(ctx, f, got, out["unbalanced"], "")
    out["unbalanced"]["memcpy_ms"] = memcpy_ms(got.counts["text_bytes"], sync)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    m = int(sys.argv[3]) if len(sys.argv) > 3 and int(sys.argv[3]) else 10_000
    if not torch.cuda.is_available():
        raise SystemExit("lift_paf_bench: no GPU (there is no CPU path to time)")
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
    exact = lambda cap: lift_exact_records_device(ctx, cols, cols["strand"], n_seq, regs, m, d_record, d_offset, d_text, k, capacity=cap, **kw)   # noqa: E731
    first = exact(0)
    call = lambda **more: lift_slice_records_device(ctx, cols, cols["strand"], n_seq, regs, m, d_record, d_offset, d_text, k, **more, **kw)   # noqa: E731
    counts = call(slice_capacity=0, text_capacity=0, want_slices=False, want_text=False).counts
    f = lambda: call(slice_capacity=counts["n_slices"], text_capacity=counts["text_bytes"])   # noqa: E731
    got = f()
    out = {"n": n, "n_genomes": G, "n_seq": n_seq, "reps": REPS, "regions": m, "hit_records": k, "cigar_bytes": int(offset[-1]), **got.counts,
           "aligned": int(got.slices["aligned"].astype(np.int64).sum()), "longest_slice": int(got.slices["text_len"].max()) if len(got.slices) else 0}
    out["exact_call_ms"] = timed(lambda: exact(first.n), sync)
    out["counts_only_ms"] = timed(lambda: call(slice_capacity=0, text_capacity=0, want_slices=False, want_text=False), sync)
    out["call_ms"] = timed(f, sync)
    table = kernel_split(ctx, f)
    out["kernels_ms"] = table
    out["slice_kernels_ms"] = round(sum(v for name, v in table.items() if name in SLICE_OWN), 3)
    both_forms(ctx, f, got, out, "")
    out["memcpy_ms"] = memcpy_ms(got.counts["text_bytes"], sync)
    out["memcpy_gbs"] = round(2 * got.counts["text_bytes"] / (out["memcpy_ms"][0] * 1e-3) / 1e9, 1) if got.counts["text_bytes"] else None
    out["call_over_exact"] = round(out["call_ms"][0] / out["exact_call_ms"][0], 3)
    unbalanced_leg(ctx, out, sync)
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
