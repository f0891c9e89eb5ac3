"""`--joblist` on the MI355X: device sketches, distances and random pairs against the numpy restatement
(tests/mash_model.py) value for value, and `sweepga-gpu --joblist` text byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from tests import mash_model as mm
from tests.test_mash_cpu import _bgzf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "B-3106.fa")


@pytest.fixture(scope="module")
def env():
    from sweepga_amd import build, default_context
    build.build()
    from sweepga_amd import mash
    return mash, default_context(0)


def _fixture_seqs():
    return mm.read_fasta_bytes(open(FIXTURE, "rb").read())


def _synthetic(rng):
    base = bytes(rng.choice(list(b"ACGT"), 3000).astype(np.uint8))
    soft = bytearray(base)
    for a in range(0, 3000, 500):
        soft[a:a + 120] = bytes(soft[a:a + 120]).lower()
    nrun = bytearray(base)
    nrun[100:400] = b"N" * 300
    nrun[1000:1003] = b"RYK"
    tandem = b"ACGTTGCA" * 300 + b"ACG" * 200  # few distinct k-mers: duplicates fill the bottom s
    return [bytes(soft), bytes(nrun), tandem, b"ACGT", b"", b"acgtn" * 3, base[:64]]


@pytest.mark.parametrize("k", [1, 7, 15, 21, 31, 32, 33, 64])
def test_sketch_equals_restatement(env, k):
    mash, ctx = env
    _, seqs = _fixture_seqs()
    seqs = seqs + _synthetic(np.random.default_rng(k))
    for s in (1, 10, 1000, 5000):
        got = mash.sketch(ctx, seqs, k, s)
        for i, x in enumerate(seqs):
            want = mm.sketch(x, k, s)
            assert got[i].dtype == np.uint64 and np.array_equal(got[i], want), (k, s, i, len(got[i]), len(want))


def test_sketch_longer_than_a_chunk(env):
    """contigs over several 2^22-window chunks (k - 1 bytes of overlap at every seam), with an N run across a seam"""
    mash, ctx = env
    rng = np.random.default_rng(5)
    long = bytearray(rng.choice(list(b"ACGTacgt"), (1 << 22) + 20000).astype(np.uint8))
    long[(1 << 22) - 40:(1 << 22) + 5] = b"N" * 45
    rep = b"ACGTACGGT" * ((1 << 22) // 9 + 500)
    for k, s in ((15, 1000), (33, 65536)):
        got = mash.sketch(ctx, [bytes(long), rep], k, s)
        assert np.array_equal(got[0], mm.sketch(bytes(long), k, s)), (k, s)
        assert np.array_equal(got[1], mm.sketch(rep, k, s)), (k, s)


def test_sketch_limits(env):
    from sweepga_amd import SwgError
    mash, ctx = env
    for k, s in ((0, 10), (65, 10), (15, 0), (15, 65537)):
        with pytest.raises(SwgError) as e:
            mash.sketch(ctx, [b"ACGTACGTACGTACGTACGT"], k, s)
        assert e.value.code == -6 and "k must be in 1..64" in str(e.value)


def test_distances_bit_equal(env):
    mash, ctx = env
    rng = np.random.default_rng(11)
    pool = rng.integers(0, 2**64 - 1, 3000, dtype=np.uint64, endpoint=True)
    for n, s in ((300, 200), (37, 5000)):
        sk = []
        for i in range(n):
            r = rng.random()
            if r < 0.05:
                sk.append(np.zeros(0, dtype=np.uint64))
            elif r < 0.1 and sk:
                sk.append(sk[-1].copy())  # J = 1: distance -0.0
            else:
                sk.append(np.sort(rng.choice(pool, rng.integers(1, min(s, len(pool)) + 1), replace=True)))  # repeats: sets
        for k in (15, 21):
            d, inter, union = mash.distances(ctx, sk, k, counts_too=True)
            sets = [set(int(x) for x in v) for v in sk]
            for i in range(n):
                for j in range(i + 1, n):
                    ci, cu = len(sets[i] & sets[j]), len(sets[i] | sets[j])
                    want = mm.distance_from_counts(ci, cu, k)
                    assert d[i, j].tobytes() == np.float64(want).tobytes() == d[j, i].tobytes(), (i, j, d[i, j], want)
                    assert (int(inter[i, j]), int(union[i, j])) == (ci, cu)
            assert np.all(np.diag(d) == 0.0)


def test_random_pairs_mask_at_2_16(env):
    mash, ctx = env
    n = 1 << 16
    wpr = n // 64
    for f in (0.05, 1.0, 0.5):
        thr = np.uint64(mm.random_threshold(f))
        for r0, r1 in ((0, 2), (777, 780), (n - 3, n)):
            m = mash.random_pairs_mask(ctx, n, f, r0, r1)
            assert m.shape == (r1 - r0, wpr)
            for i in range(r0, r1):
                bits = np.unpackbits(m[i - r0].view(np.uint8), bitorder="little").astype(bool)
                j = np.arange(n, dtype=np.uint64)
                want = (j > i) & (mm.sip13_pair(np.full(n, i, dtype=np.uint64), j) <= thr)
                assert np.array_equal(bits, want), (f, i)
    m = mash.random_pairs_mask(ctx, n, 1e-6)  # the whole mask (512 MiB), rows over several launches
    total = int(sum(bin(int(w)).count("1") for w in m[m != 0]))
    assert 0 < total < 10 * 2**31 * 1e-6


def _haplotypes(rng, n_hap, contigs=2, mut=0.02):
    _, seqs = _fixture_seqs()
    out = []
    for h in range(n_hap):
        for c in range(contigs):
            s = bytearray(seqs[c % len(seqs)])
            pos = rng.random(len(s)) < mut * (1 + h % 5)
            s = bytes(np.where(pos, rng.choice(list(b"ACGT"), len(s)), np.frombuffer(bytes(s), dtype=np.uint8)).astype(np.uint8))
            out.append((f"H{h:02d}#{h % 3}#c{c}", s))
    return out


def _write_fa(path, recs, gz=False):
    data = b"".join(b">" + n.encode() + b" desc\n" + s[:70] + b"\n" + s[70:] + b"\n" for n, s in recs)
    open(path, "wb").write(_bgzf(data) if gz else data)
    return data


def _model_reader(path):
    data = open(path, "rb").read()
    if data[:2] == b"\x1f\x8b":
        import gzip
        data = gzip.decompress(data)
    return data


@pytest.mark.parametrize("strategy", ["tree:2:1:0.2", "knn:3", "giant:0.9", "auto", "random:0.3", "none"])
def test_joblist_equals_restatement(env, tmp_path, strategy):
    mash, ctx = env
    rng = np.random.default_rng(17)
    recs = _haplotypes(rng, 12)
    one = tmp_path / "pg.fa"
    _write_fa(one, recs)
    a, b = tmp_path / "a.fa.gz", tmp_path / "b.fa"
    _write_fa(a, recs[:10], gz=True)
    _write_fa(b, recs[10:])
    for paths in ([str(one)], [str(a), str(b)]):
        for t, ll in ((8, 0), (2, 5000)):
            want = mm.joblist(paths, strategy, 15, 1000, t, ll, "jobs", reader=_model_reader)
            assert mash.joblist(ctx, paths, strategy, 15, 1000, t, ll, "jobs") == want
    # the command line: -t / --min-aln-length given and omitted
    cli = os.path.join(ROOT, "sweepga_amd", "bin", "sweepga-gpu")
    for extra, t, ll in (([], 8, 0), (["-t", "3", "--min-aln-length", "2k"], 3, 2000)):
        r = subprocess.run([cli, "--joblist", str(a), str(b), "--sparsify", strategy, "--joblist-output-dir", str(tmp_path / "o")] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert r.stdout == mm.joblist([str(a), str(b)], strategy, 15, 1000, t, ll, str(tmp_path / "o"), reader=_model_reader)


@pytest.mark.parametrize("n_hap", [10, 11, 50, 51])
def test_joblist_auto_ranges(env, tmp_path, n_hap):
    """auto: all pairs up to 10 haplotypes, giant:0.99 up to 50, tree:5:2:0.05 beyond (knn_graph.rs:507-527)"""
    mash, ctx = env
    recs = _haplotypes(np.random.default_rng(n_hap), n_hap, contigs=2, mut=0.01)
    p = tmp_path / "pg.fa"
    _write_fa(p, recs)
    for k, s in ((15, 1000), (21, 64)):
        assert mash.joblist(ctx, [str(p)], "auto", k, s) == mm.joblist([str(p)], "auto", k, s)


def test_cli_joblist_errors(env, tmp_path):
    cli = os.path.join(ROOT, "sweepga_amd", "bin", "sweepga-gpu")
    recs = _haplotypes(np.random.default_rng(2), 3)
    p = tmp_path / "pg.fa"
    _write_fa(p, recs)
    for extra in (["--mash-kmer-size", "0"], ["--mash-kmer-size", "65"], ["--mash-sketch-size", "0"], ["--mash-sketch-size", "70000"]):
        r = subprocess.run([cli, "--joblist", str(p), "--sparsify", "tree:1"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "k must be in 1..64" in r.stderr, (extra, r.stderr)
    plain = tmp_path / "plain.fa"
    plain.write_bytes(open(FIXTURE, "rb").read())
    r = subprocess.run([cli, "--joblist", str(plain), "--sparsify", "tree:1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "PanSN" in r.stderr
    paf = tmp_path / "a.paf"
    paf.write_text("a\t1\t0\t10\t+\tb\t1\t0\t10\t9\t10\t60\n")
    r = subprocess.run([cli, "--joblist", str(paf), "--sparsify", "tree:1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "FASTA" in r.stderr
