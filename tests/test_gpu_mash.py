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


HIGH_J_U = (18, 36, 72, 92, 200, 1000, 5000)
# the smallest (inter, union) whose ratio 2J / (1 + J) the integer-domain table logarithm got wrong in the last bit
HIGH_J_WITNESSES = ((17, 18), (34, 36), (70, 71), (79, 80), (89, 92))


def _nested(rng, U):
    """n = min(U, 128) sketches over a sorted pool of U distinct values: sketch i = the pool's first U - i values, so the
    pair i < j has inter = U - j and union = U - i by construction"""
    pool = np.unique(rng.integers(0, 2**64 - 1, U + 64, dtype=np.uint64, endpoint=True))[:U]
    assert len(pool) == U
    return [pool[:U - i].copy() for i in range(min(U, 128))]


def _check_nested(mash, ctx, sk, U, k):
    n = len(sk)
    d, inter, union = mash.distances(ctx, sk, k, counts_too=True)
    i, j = np.triu_indices(n, 1)
    ci, cu = U - j, U - i
    assert np.array_equal(inter[i, j], ci) and np.array_equal(inter[j, i], ci), (U, k)
    assert np.array_equal(union[i, j], cu) and np.array_equal(union[j, i], cu), (U, k)
    want = np.array([mm.distance_from_counts(int(a), int(b), k) for a, b in zip(ci, cu)], dtype=np.float64)
    for got in (d[i, j], d[j, i]):
        bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
        assert bad.size == 0, (U, k, bad.size, int(ci[bad[0]]), int(cu[bad[0]]), float(got[bad[0]]).hex(), float(want[bad[0]]).hex())
    assert np.all(np.diag(d) == 0.0)
    return ci, cu


def test_distances_bit_equal_at_high_jaccard(env):
    """Distance, intersection and union at J >= 15/17, where 2J / (1 + J) >= 0.9375 lies in the near-1 window of glibc's
    log: near-identical sketches with (inter, union) known by construction, bytes for bytes against the model in both
    triangles.  The table-only logarithm returned -0x1.daee8ab72e7e5p-6 for ln(34/35), the ratio of (17, 18); libm and
    the model give ...e4p-6."""
    import math
    mash, ctx = env
    rng = np.random.default_rng(29)
    seen = set()
    for U in HIGH_J_U:
        sk = _nested(rng, U)
        for k in (15, 21):
            ci, cu = _check_nested(mash, ctx, sk, U, k)
        j = ci / cu
        ratio = (2.0 * j) / (1.0 + j)
        seen.update((U, int(a), int(b)) for a, b in zip(ci[ratio >= 0.9375], cu[ratio >= 0.9375]))
    # not vacuous: enough pairs in the window, the known witnesses among them, and the model on libm's side of one
    assert len(seen) >= 10_000, len(seen)
    in_window = {(a, b) for _, a, b in seen}
    assert all(w in in_window for w in HIGH_J_WITNESSES), [w for w in HIGH_J_WITNESSES if w not in in_window]
    j = 17 / 18
    assert math.log((2.0 * j) / (1.0 + j)) != float.fromhex("-0x1.daee8ab72e7e5p-6")
    assert mm.distance_from_counts(17, 18, 15) == (-1.0 / 15) * float.fromhex("-0x1.daee8ab72e7e4p-6")
    print(f"high-J pairs in the window: {len(seen)} per k")


def test_distances_high_jaccard_with_repeats(env):
    """the nested sketches with every value repeated 1 to 3 times: sets are what counts, so the same counts and distances"""
    mash, ctx = env
    rng = np.random.default_rng(31)
    for U in (92, 1000):
        sk = [np.repeat(v, rng.integers(1, 4, len(v))) for v in _nested(rng, U)]
        assert all(len(v) > len(np.unique(v)) for v in sk[:-1]) and all(np.all(v[1:] >= v[:-1]) for v in sk)
        _check_nested(mash, ctx, sk, U, 15)


def test_distances_high_jaccard_unstaged(env):
    """second sketch longer than the kernel's LDS staging buffer (4096 values): two sketches of 40,000 values that share all
    but 100 (J = 39900 / 40100), and a short one before them so that a short first sketch meets a long second one"""
    mash, ctx = env
    rng = np.random.default_rng(37)
    pool = np.unique(rng.integers(0, 2**64 - 1, 40_300, dtype=np.uint64, endpoint=True))[:40_100]
    assert len(pool) == 40_100
    drop = rng.permutation(40_100)[:200]
    a = np.delete(pool, drop[:100])
    b = np.delete(pool, drop[100:])
    sk = [a[:3000].copy(), a, b]
    assert len(a) == len(b) == 40_000 and mm.jaccard_counts(a, b) == (39_900, 40_100)
    for k in (15, 21):
        d, inter, union = mash.distances(ctx, sk, k, counts_too=True)
        for i in range(3):
            for j in range(i + 1, 3):
                ci, cu = mm.jaccard_counts(sk[i], sk[j])
                want = mm.distance_from_counts(ci, cu, k)
                assert d[i, j].tobytes() == np.float64(want).tobytes() == d[j, i].tobytes(), (i, j, float(d[i, j]).hex(), want.hex())
                assert (int(inter[i, j]), int(union[i, j]), int(inter[j, i]), int(union[j, i])) == (ci, cu, ci, cu)


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


@pytest.mark.parametrize("strategy", ["knn:3", "tree:2:1:0.2", "giant:0.9"])
def test_joblist_near_identical_haplotypes(env, tmp_path, strategy):
    """The high-J route end to end: 12 haplotypes mutated at 0.1 %, so that at least half of the haplotype pairs have
    J >= 0.8824 and their distances come from the near-1 branch of the logarithm; the Python API and the command line
    against the model, text byte for byte.  A last-bit error in a distance rarely moves a selection, so this case is
    expected to pass with the table-only logarithm as well: test_distances_bit_equal_at_high_jaccard is the one that
    catches that.  This one is here so that sketches, merge, distances and selection are run together at such J."""
    mash, ctx = env
    recs = _haplotypes(np.random.default_rng(17), 12, mut=0.001)
    groups = {}
    for name, seq in recs:
        groups.setdefault(mm.pansn_key(name), []).append(mm.sketch(seq, 15, 1000))
    hs = [mm.merge(groups[h], 1000) for h in sorted(groups)]
    jac = [np.divide(*mm.jaccard_counts(hs[i], hs[j])) for i in range(len(hs)) for j in range(i + 1, len(hs))]
    assert len(jac) == 66 and sum(x >= 0.8824 for x in jac) >= 33, sorted(jac)
    a, b = tmp_path / "a.fa.gz", tmp_path / "b.fa"
    _write_fa(a, recs[:10], gz=True)
    _write_fa(b, recs[10:])
    paths = [str(a), str(b)]
    want = mm.joblist(paths, strategy, 15, 1000, 8, 0, str(tmp_path / "o"), reader=_model_reader)
    assert want and mash.joblist(ctx, paths, strategy, 15, 1000, 8, 0, str(tmp_path / "o")) == want
    cli = os.path.join(ROOT, "sweepga_amd", "bin", "sweepga-gpu")
    r = subprocess.run([cli, "--joblist", str(a), str(b), "--sparsify", strategy, "--joblist-output-dir", str(tmp_path / "o")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want


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
