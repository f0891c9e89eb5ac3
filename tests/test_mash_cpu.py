"""`--joblist` on the CPU: the numpy restatement (tests/mash_model.py) against the reference's own unit vectors and the
scalar SipHash of test_tree_filter_cpu.py; the library's host code (FASTA reader, merge, pair selection, job text) against
the restatement.  Nothing here needs a GPU: the strategies used draw no random pairs and read no sequence."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import mash_model as mm
from tests.test_tree_filter_cpu import siphash

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "B-3106.fa")


@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build
    build.build()
    from sweepga_amd import mash
    return mash


def test_vectorised_siphash_matches_scalar():
    rng = np.random.default_rng(1)
    for k in (1, 7, 8, 15, 16, 31, 33, 64):
        seq = bytes(rng.choice(list(b"ACGTacgt"), 80 + k).astype(np.uint8))
        arr = np.frombuffer(seq, dtype=np.uint8)
        st = np.arange(0, 80)
        h = mm._hash_windows(arr, st, k)
        for s in (0, 5, 79):
            assert int(h[s]) == siphash(1, 3, 0, 0, k.to_bytes(8, "little") + seq[s:s + k])
    i, j = np.array([0, 3, 70000]), np.array([1, 9, 65535])
    h = mm.sip13_pair(i, j)
    for a, b, x in zip(i, j, h):
        assert int(x) == siphash(1, 3, 0, 0, int(a).to_bytes(8, "little") + int(b).to_bytes(8, "little"))


def test_sketch_restatement_literal_quirks():
    # the forward hash keeps case, the reverse one is over the upper-cased complement
    lo, up = mm.sketch(b"acgta", 5, 10), mm.sketch(b"ACGTA", 5, 10)
    h_lo = siphash(1, 3, 0, 0, (5).to_bytes(8, "little") + b"acgta")
    h_rc = siphash(1, 3, 0, 0, (5).to_bytes(8, "little") + b"TACGT")
    assert int(lo[0]) == min(h_lo, h_rc) and len(up) == 1
    assert len(mm.sketch(b"ACG", 5, 10)) == 0                         # shorter than k
    assert len(mm.sketch(b"ACGTNACGT", 5, 10)) == 0                   # every window holds the N
    rep = mm.sketch(b"ACACACACACACAC", 4, 100)                        # tandem repeat: duplicates keep their slots
    assert len(rep) == 11 and len(np.unique(rep)) == 2


def test_reference_unit_vectors():
    # knn_graph.rs test_build_knn_graph
    d = [[0.0, 0.1, 0.9], [0.1, 0.0, 0.8], [0.9, 0.8, 0.0]]
    p = mm.build_knn_graph(d, 1, False)
    assert len(p) == 3 and (0, 1) in p and (1, 0) in p
    # knn_graph.rs test_estimate_pair_count and _larger
    assert mm.estimate_tree_pair_count(4, 1, 0, 0.0) == 4
    assert mm.estimate_tree_pair_count(4, 1, 1, 0.0) == 6
    assert [mm.estimate_tree_pair_count(10, *a) for a in ((0, 0, 0.0), (1, 0, 0.0), (2, 0, 0.0), (0, 0, 0.5), (10, 10, 1.0))] == \
        [0, 10, 20, 23, 45]
    # pansn.rs extract_pansn_key tests (Haplotype level)
    assert mm.pansn_key(">HG01106#1#CM087962.1") == "HG01106#1"
    assert mm.pansn_key(">HG01106#1#chr1 extra annotation") == "HG01106#1"
    assert mm.pansn_key("HG01106#1#chr1:29000000-29003000") == "HG01106#1"
    assert mm.pansn_key("chr1") == "chr1" and mm.pansn_key(">chr1 extra") == "chr1"
    # joblist.rs wfmash_pansn_* tests, strings verbatim
    jobs = [("HG01106#1", "HG00733#2", "/data/pangenome.fa", "/data/pangenome.fa"),
            ("SGDref#0", "HG01106#1", "/data/pangenome.fa", "/data/pangenome.fa")]
    assert mm.emit(jobs, "/out", 8, 0).splitlines() == [
        "wfmash -t 8 -T HG01106#1 -Q HG00733#2 /data/pangenome.fa > /out/HG01106_1_vs_HG00733_2.paf",
        "wfmash -t 8 -T SGDref#0 -Q HG01106#1 /data/pangenome.fa > /out/SGDref_0_vs_HG01106_1.paf"]
    assert mm.emit([("HG01106#1", "HG00733#2", "/data/hg01106.fa", "/data/hg00733.fa")], "/out", 4, 0).rstrip() == \
        "wfmash -t 4 -T HG01106#1 -Q HG00733#2 /data/hg01106.fa /data/hg00733.fa > /out/HG01106_1_vs_HG00733_2.paf"
    s = mm.emit([("A#0", "B#0", "pg.fa", "pg.fa")], ".", 4, 20000)
    assert "-l 20000" in s and "-T A#0 -Q B#0" in s


def _bgzf(data):
    """BGZF by hand: gzip members of <= 64 KiB with the BC extra field, then the empty EOF block."""
    import struct
    import zlib
    out = b""
    for o in range(0, len(data), 60000):
        chunk = data[o:o + 60000]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = c.compress(chunk) + c.flush()
        bsize = 18 + len(comp) + 8 - 1
        out += b"\x1f\x8b\x08\x04" + b"\0" * 4 + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize) + comp + \
            struct.pack("<II", zlib.crc32(chunk) & 0xffffffff, len(chunk))
    return out + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def test_fasta_reader_quirks(lib, tmp_path):
    text = (b"PREAMBLE acgt\n\n>A#1#c1 some words\r\nACGTNNac  \r\n\r\n  RYKM gt\n>A#1#c2\n>B#1#c1\tx\nTTTT\n"
            b">\n acg\n>B#1#c2 last-no-newline\nGGA")
    p = tmp_path / "x.fa"
    p.write_bytes(text)
    q = tmp_path / "y.fa.gz"
    q.write_bytes(_bgzf(b"junk\n>C#0#z\nAC\r\nGT\n" * 3000))
    f = lib.Fasta([str(p), str(q)])
    names, seqs = mm.read_fasta_bytes(text)
    n2, s2 = mm.read_fasta_bytes(b"junk\n>C#0#z\nAC\r\nGT\n" * 3000)
    assert f.names == names + n2
    assert [f.sequence(i) for i in range(len(f))] == seqs + s2
    assert seqs[0] == b"PREAMBLE acgtACGTNNacRYKM gt" and names[0] == "A#1#c1" and names[3] == ""
    assert list(f.file_index) == [0] * len(names) + [1] * len(n2)
    # no header at all: the preamble goes nowhere
    e = tmp_path / "e.fa"
    e.write_bytes(b"ACGT\nACGT\n")
    f = lib.Fasta([str(e), str(p)])
    assert f.names == names and f.sequence(0) == seqs[0]


def test_merge_is_sort_dedup_truncate(lib):
    a = np.array([5, 9, 9, 20], dtype=np.uint64)
    b = np.array([1, 9, 30], dtype=np.uint64)
    for s in (1, 3, 5, 10):
        assert list(lib.merge([a, b], s)) == list(mm.merge([a, b], s))
    assert list(lib.merge([a, b], 3)) == [1, 5, 9]


def _rand_dist(rng, n, ties=False):
    d = rng.random((n, n))
    if ties:
        d = np.round(d * 4) / 4
        d[d == 0.0] = -0.0
    d = (d + d.T) / 2 if not ties else np.triu(d, 1) + np.triu(d, 1).T
    np.fill_diagonal(d, 0.0)
    return d


@pytest.mark.parametrize("strategy", ["tree:1", "tree:2:1", "knn:3:2:0", "tree:0:1", "none", "all", "wfmash:auto", "wfmash:0.3"])
def test_select_matches_restatement(lib, strategy):
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 7, 20):
        for ties in (False, True):
            d = _rand_dist(rng, n, ties)
            assert lib.select_pairs(None, strategy, d) == sorted(set(mm.select(mm.parse_strategy(strategy), d, n))), (strategy, n, ties)


def test_select_ties_and_negative_zero(lib):
    # equal distances keep ascending j; -0.0 ranks with +0.0 (partial_cmp)
    d = np.array([[0.0, 0.5, 0.5, 0.5], [0.5, 0.0, -0.0, 0.0], [0.5, -0.0, 0.0, 0.5], [0.5, 0.0, 0.5, 0.0]])
    assert lib.select_pairs(None, "tree:1", d) == [(0, 1), (1, 2), (1, 3)]
    assert lib.select_pairs(None, "tree:0:1", d) == sorted(set(mm.select(("tree", 0, 1, 0.0), d, 4)))
    # knn_graph.rs test_build_knn_graph through the product: each row's nearest
    assert lib.select_pairs(None, "tree:1", [[0.0, 0.1, 0.9], [0.1, 0.0, 0.8], [0.9, 0.8, 0.0]]) == [(0, 1), (1, 2)]


def test_auto_small_is_all_pairs(lib):
    for n in (2, 10):
        assert lib.select_pairs(None, "auto", np.zeros((n, n))) == [(i, j) for i in range(n) for j in range(i + 1, n)]


def test_strategy_errors(lib):
    from sweepga_amd import SwgError
    for bad in ("bogus", "tree:0", "random:2", "giant:1", "tree:1:2:3:4", "1.5"):
        with pytest.raises(SwgError):
            lib.select_pairs(None, bad, np.zeros((3, 3)))
    with pytest.raises(SwgError):
        lib.select_pairs(None, "tree:1", None, n=3)  # needs distances


def _pangenome(tmp_path, n_hap=4, contigs=3, name="pg.fa"):
    names, seqs = mm.read_fasta_bytes(open(FIXTURE, "rb").read())
    out = b""
    for h in range(n_hap):
        for c in range(contigs):
            out += f">S{h}#{h % 2}#ctg{c}\n".encode() + seqs[(h + c) % len(seqs)] + b"\n"
    p = tmp_path / name
    p.write_bytes(out)
    return p


@pytest.mark.parametrize("strategy", ["none", "all", "wfmash:auto"])
def test_joblist_sketch_free_matches_restatement(lib, tmp_path, strategy):
    p = _pangenome(tmp_path)
    for threads, ll, od in ((8, 0, "."), (3, 20000, "out/"), (8, 0, "")):
        got = lib.joblist(None, [str(p)], strategy, threads=threads, min_aln_length=ll, output_dir=od)
        assert got == mm.joblist([str(p)], strategy, threads=threads, block_length=ll, output_dir=od)
    # several files: the haplotype's first contig's file, both files when they differ
    q = _pangenome(tmp_path, 3, 2, "other.fa")
    q.write_bytes(q.read_bytes().replace(b">S", b">T"))
    got = lib.joblist(None, [str(p), str(q)], strategy)
    assert got == mm.joblist([str(p), str(q)], strategy) and f" {p} {q} > " in got


def test_joblist_refusals(lib, tmp_path):
    from sweepga_amd import SwgError
    plain = tmp_path / "plain.fa"
    plain.write_bytes(open(FIXTURE, "rb").read())
    with pytest.raises(SwgError, match="no PanSN haplotype structure"):
        lib.joblist(None, [str(plain)], "none")
    paf = tmp_path / "a.paf"
    paf.write_text("a\t1\t0\t10\t+\tb\t1\t0\t10\t9\t10\t60\n")
    with pytest.raises(SwgError, match="requires FASTA"):
        lib.joblist(None, [str(paf)], "none")
    p = _pangenome(tmp_path)
    for k, s in ((0, 1000), (65, 1000), (15, 0), (15, 65537)):
        with pytest.raises(SwgError, match="k must be in 1..64") as e:
            lib.joblist(None, [str(p)], "tree:1", k=k, s=s)
        assert e.value.code == -6


def test_cli_joblist_without_gpu(tmp_path):
    """the flags, sketch-free strategies (no device needed), and the PAF path's refusals left as they were"""
    from sweepga_amd import build
    build.build()
    cli = build.CLI
    p = _pangenome(tmp_path)
    r = subprocess.run([cli, "--joblist", str(p), "--sparsify", "none", "-t", "4", "--min-aln-length", "5k",
                        "--joblist-output-dir", str(tmp_path / "jobs" / "x")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == mm.joblist([str(p)], "none", threads=4, block_length=5000, output_dir=str(tmp_path / "jobs" / "x"))
    assert os.path.isdir(tmp_path / "jobs" / "x")
    out = tmp_path / "jobs.txt"
    r = subprocess.run([cli, "--joblist", str(p), "--output-file", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and out.read_text() == mm.joblist([str(p)], "none")
    for extra in (["--mash-kmer-size", "65", "--sparsify", "tree:1"], ["--mash-sketch-size", "0", "--sparsify", "auto"]):
        r = subprocess.run([cli, "--joblist", str(p)] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "k must be in 1..64" in r.stderr
    plain = tmp_path / "plain.fa"
    plain.write_bytes(open(FIXTURE, "rb").read())
    r = subprocess.run([cli, "--joblist", str(plain)], capture_output=True, text=True)
    assert r.returncode == 1 and "PanSN" in r.stderr
    paf = tmp_path / "a.paf"
    paf.write_text("a\t1\t0\t10\t+\tb\t1\t0\t10\t9\t10\t60\n")
    r = subprocess.run([cli, "--joblist", str(paf)], capture_output=True, text=True)
    assert r.returncode == 1 and "FASTA" in r.stderr
    r = subprocess.run([cli, str(paf), "--sparsify", "giant:0.9"], capture_output=True, text=True)
    assert r.returncode == 1 and "not valid for post-alignment" in r.stderr
