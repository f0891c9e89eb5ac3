"""Timing of the `--joblist` sketch path on synthetic PanSN pangenomes.

For each shape (haplotypes x bases per haplotype, several contigs each) it writes a FASTA, then prints one JSON line:
  - the sketch kernels on their own (bases/s and k-mers/s from device events: hash kernel, radix select, H2D copies);
  - the end-to-end swg_joblist wall time split into read, sketch (upload + hash + select), merge, distances, select;
  - the same pipeline through a CPU path in this tool (numpy SipHash over 16 worker processes), for context.
Usage: python tools/sketch_bench.py [--shapes 64x12000000,8x3100000000] [--k 15] [--s 1000] [--strategy tree:5:2:0.05]
       [--cpu-max-bases N] [--dir DIR]"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_pangenome(path, n_hap, hap_bases, contigs, seed=1):
    """one random ancestor, each haplotype a 1%-mutated copy with soft-masked stretches and N runs"""
    rng = np.random.default_rng(seed)
    clen = hap_bases // contigs
    anc = rng.integers(0, 4, clen, dtype=np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as f:
        for h in range(n_hap):
            for c in range(contigs):
                s = anc.copy()
                mut = rng.random(clen) < 0.01
                s[mut] = rng.integers(0, 4, int(mut.sum()), dtype=np.uint8)
                b = lut[s]
                b[1000:1500] += 32  # soft-masked
                b[5000:5100] = ord("N")
                f.write(f">S{h}#1#ctg{c}\n".encode())
                f.write(b.tobytes())
                f.write(b"\n")


def _cpu_sketch(args):
    from tests import mash_model as mm
    seq, k, s = args
    return mm.sketch(seq, k, s)


def cpu_pipeline(path, k, s, strategy, workers=16):
    from tests import mash_model as mm
    t0 = time.perf_counter()
    names, seqs = mm.read_fasta_bytes(open(path, "rb").read())
    t1 = time.perf_counter()
    with ProcessPoolExecutor(workers) as ex:
        sk = list(ex.map(_cpu_sketch, [(x, k, s) for x in seqs]))
    t2 = time.perf_counter()
    keys = sorted(set(mm.pansn_key(n) for n in names))
    groups = {h: [] for h in keys}
    for i, n in enumerate(names):
        groups[mm.pansn_key(n)].append(i)
    hs = [mm.merge([sk[i] for i in groups[h]], s) for h in keys]
    d = mm.distance_matrix(hs, k)
    t3 = time.perf_counter()
    mm.select(mm.parse_strategy(strategy), d, len(keys))
    t4 = time.perf_counter()
    return dict(read_ms=(t1 - t0) * 1e3, sketch_ms=(t2 - t1) * 1e3, merge_distances_ms=(t3 - t2) * 1e3, select_ms=(t4 - t3) * 1e3,
                total_ms=(t4 - t0) * 1e3, workers=workers)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64x12000000")
    ap.add_argument("--contigs", type=int, default=4)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--s", type=int, default=1000)
    ap.add_argument("--strategy", default="tree:5:2:0.05")
    ap.add_argument("--cpu-max-bases", type=float, default=2e8, help="skip the CPU path above this many bases")
    ap.add_argument("--dir", default=None, help="where the synthetic FASTA is written (default: a temporary directory)")
    a = ap.parse_args()
    from sweepga_amd import build, default_context, mash
    build.build()
    ctx = default_context(0)
    tmp = None
    if a.dir is None:
        a.dir = tmp = tempfile.mkdtemp(prefix="sketch_bench_")
    os.makedirs(a.dir, exist_ok=True)
    for shape in a.shapes.split(","):
        n_hap, hap_bases = (int(float(x)) for x in shape.split("x"))
        path = os.path.join(a.dir, f"pg_{n_hap}x{hap_bases}.fa")
        write_pangenome(path, n_hap, hap_bases, a.contigs)
        fa = mash.Fasta([path])
        bases = int(fa.offsets[-1])
        mash.sketch(ctx, [fa.sequence(0)[:100000]], a.k, a.s)  # warm-up (code objects, pinned buffers)
        _, tm = mash.sketch(ctx, None, a.k, a.s, bases=fa.bases, offsets=fa.offsets, timing=True)
        del fa
        text, jt = mash.joblist(ctx, [path], a.strategy, a.k, a.s, timing=True)
        rec = dict(shape=shape, haplotypes=n_hap, bases=bases, k=a.k, s=a.s, strategy=a.strategy, jobs=text.count("\n"),
                   sketch=dict(wall_ms=tm["wall_ms"], h2d_ms=tm["h2d_ms"], hash_ms=tm["hash_ms"], select_ms=tm["select_ms"],
                               kmers=tm["kmers"], hash_kmers_per_s=tm["kmers"] / (tm["hash_ms"] * 1e-3),
                               hash_bases_per_s=bases / (tm["hash_ms"] * 1e-3), h2d_bytes_per_s=bases / (tm["h2d_ms"] * 1e-3),
                               end_to_end_bases_per_s=bases / (tm["wall_ms"] * 1e-3)),
                   joblist=jt)
        if bases <= a.cpu_max_bases:
            rec["cpu16"] = cpu_pipeline(path, a.k, a.s, a.strategy)
        print(json.dumps(rec), flush=True)
        os.remove(path)
    if tmp:
        os.rmdir(tmp)


if __name__ == "__main__":
    main()
