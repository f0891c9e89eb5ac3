"""alnstats on the device (sweepga_amd/csrc/swg_alnstats.hip) against the host alnstats that tests/test_alnstats_cpu.py pins:
swg_paf_alnstats == swg_alnstats_open of the same text (ALL) and of the file swg_paf_write writes (KEPT), the two record seams
against a numpy restatement, the command line's --stats against bin/alnstats, and one case large enough for the
multi-work-group merges and the hashed genome-pair table.  Every comparison is exact: integers, bytes, f64 bit patterns."""
import ctypes as C
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import gen
from tests.test_gpu_wide import Hip
from sweepga_amd.alnstats import PAIR_DTYPE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMMARY_INTS = ("total_mappings", "total_bases", "total_matches", "self_mappings", "inter_chromosomal", "inter_genome",
                "chr_pair_count", "genome_pairs", "above_95_pct")
NONE64 = 2**64 - 1


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


def bits(x):
    return struct.pack("<d", x)


def assert_same(dev, host, what=""):
    """Every field of swg_alnstats_summary (doubles as bit patterns), every pair in order, the detailed report byte for byte."""
    for k in SUMMARY_INTS:
        assert int(getattr(dev.summary, k)) == int(getattr(host.summary, k)), (what, k)
    for k in ("avg_identity", "avg_coverage"):
        assert bits(getattr(dev.summary, k)) == bits(getattr(host.summary, k)), (what, k)
    dp, hp = dev.pairs, host.pairs
    assert len(dp) == len(hp), what
    for a, b in zip(dp, hp):
        assert a[:2] == b[:2] and bits(a[2]) == bits(b[2]) and a[3:] == b[3:], (what, a, b)
    assert dev.report("label.paf", True) == host.report("label.paf", True), what
    assert dev.report("label.paf", False) == host.report("label.paf", False), what


def line(q, ql, qs, qe, t, tl, m, extra=()):
    return "\t".join([q, str(ql), str(qs), str(qe), "+", t, str(tl), "0", str(qe - qs), str(m), str(max(qe - qs, 1)), "60", *extra])


def gen_text(seed, n, pansn=True, **kw):
    rng = np.random.default_rng(seed)
    rec = gen.random_records(rng, n, pansn=pansn, **kw)
    return gen.records_to_paf(rng, rec, junk_lines=False)   # (the junk lines of gen hold unparsable numbers: the host tool stops there)


def named_text(seed, n, names, lengths=None):
    """n lines over the given sequence names, every sequence with ONE length unless `lengths` says otherwise."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, len(names), n)
    t = rng.integers(0, len(names), n)
    qs = rng.integers(0, 50_000, n)
    ln = rng.integers(0, 5_000, n)
    m = (ln * rng.uniform(0.6, 1.0, n)).astype(np.int64)
    out = []
    for i in range(n):
        ql = lengths[i][0] if lengths else 100_000 + int(q[i])
        tl = lengths[i][1] if lengths else 100_000 + int(t[i])
        out.append(line(names[int(q[i])], ql, int(qs[i]), int(qs[i] + ln[i]), names[int(t[i])], tl, int(m[i])))
    return "\n".join(out) + "\n"


HAND = (
    # self, inter-chromosomal, inter-genome; a sequence whose length differs between lines (last writer wins)
    line("a#1#c1", 1000, 0, 500, "a#1#c1", 1000, 450) + "\n" +
    line("a#1#c1", 1000, 0, 300, "a#1#c2", 2000, 290) + "\n" +
    line("a#1#c1", 1111, 10, 400, "b#1#c1", 3000, 380) + "\n" +
    # query == target name with two different lengths on one line: the target's (column 7) has the last word
    line("b#1#c1", 3000, 0, 100, "b#1#c1", 3333, 99) + "\n" +
    # exactly 11 columns (no mapq), then lines with fewer than 11 (skipped by both), an empty one and a comment
    "\t".join(["b#1#c2", "700", "5", "105", "-", "a#1#c2", "2222", "0", "100", "90", "100"]) + "\n" +
    "too\tfew\tfields\n\n# comment\n" +
    "\t".join(["b#1#c2", "700", "5", "105", "-", "a#1#c2", "2222", "0", "100", "90"]) + "\n" +
    # zero-length mappings, '+' numbers, a CRLF line
    line("b#1#c2", 700, 50, 50, "a#1#c1", 999, 0) + "\n" +
    line("c#2#c1", "+4000", 7, 7, "a#1#c1", 999, 0) + "\n" +
    line("c#2#c1", 4000, 0, 3999, "b#1#c2", 701, 3900, ("tp:A:P", "cg:Z:3900=99X")) + "\r\n" +
    line("plain", 50, 0, 50, "other", 60, 50) + "\n" +
    line("one#x", 50, 0, 50, "one#y", 60, 50) + "\n" +
    line("p#q#r#s", 50, 0, 50, "p#q#r#t", 60, 50) + "\n" +
    line("p#q#r#s", 50, 0, 50, "p#q#z#t", 60, 50)   # no final newline
)
# one genome pair holding more than 2^32 bases in total (u64 sums), coordinates below 2^32
BIG = "".join(line("g1#1#c%d" % (i % 3), 4_000_000_000, 0, 3_900_000_000, "g2#1#c1", 4_100_000_000, 3_800_000_000) + "\n" for i in range(7))
# a cg:Z: tag whose '=' total is NOT column 10: the filter's matches column differs from what alnstats reads
CG_OVERRIDE = (line("a#1#c1", 1000, 0, 500, "b#1#c1", 1000, 450, ("cg:Z:400=100X",)) + "\n" +
               line("a#1#c1", 1000, 0, 300, "b#1#c2", 2000, 290) + "\n")


def shape_texts():
    out = {
        "pansn": gen_text(1, 6_000, n_genomes=5, chrs_per_genome=4),
        "pansn_selfheavy": gen_text(2, 3_000, n_genomes=2, chrs_per_genome=2, self_frac=0.3),
        "one_hash": named_text(3, 4_000, ["g%d#chr%d" % (g, c) for g in range(6) for c in range(3)]),
        "three_hashes": named_text(4, 4_000, ["s%d#%d#x%d#chr%d" % (g, g % 2, g % 3, c) for g in range(7) for c in range(3)]),
        "no_hash_20000_contigs": named_text(5, 60_000, ["ctg%05d" % i for i in range(20_000)]),
        "hand": HAND,
        "over_2_32_bases": BIG,
        "cg_override": CG_OVERRIDE,
        "single": line("q", 10, 0, 5, "t", 10, 5) + "\n",
    }
    rng = np.random.default_rng(6)
    out["lengths_vary"] = named_text(7, 3_000, ["v%d#1#c%d" % (g, c) for g in range(3) for c in range(2)],
                                     lengths=[(int(a), int(b)) for a, b in rng.integers(60_000, 70_000, (3_000, 2))])
    return out


SHAPES = shape_texts()


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_all_equals_the_host_tool(sw, shape):
    text = SHAPES[shape]
    host = sw.AlnStats(text=text)
    with sw.PafFile(text=text) as paf:
        dev, none = sw.AlnStats.from_paf(sw.default_context(), paf)
        assert none is None
        assert_same(dev, host, shape)
    if shape == "over_2_32_bases":
        assert int(dev.summary.total_bases) == 7 * 3_900_000_000 > 2**32 and dev.pairs[0][3] == 7 * 3_900_000_000
    if shape == "no_hash_20000_contigs":
        assert int(dev.summary.genome_pairs) > 50_000   # every contig its own genome: the hashed pair table


def test_three_orders_of_one_record_set(sw):
    """Pair-major, by query and shuffled: each equals the host tool on the same text; the integer results and the SET of pairs
    are those of the other orders (the pair ORDER is first appearance, which the host tool dictates equally)."""
    lines = SHAPES["pansn"].splitlines()
    rng = np.random.default_rng(11)
    key_pair = lambda l: (l.split("\t")[0].rsplit("#", 1)[0], l.split("\t")[5].rsplit("#", 1)[0])   # noqa: E731
    orders = {"pair_major": sorted(lines, key=key_pair), "by_query": sorted(lines, key=lambda l: l.split("\t")[0]),
              "shuffled": [lines[i] for i in rng.permutation(len(lines))]}
    seen = []
    for name, ls in orders.items():
        text = "\n".join(ls) + "\n"
        with sw.PafFile(text=text) as paf:
            dev, _ = sw.AlnStats.from_paf(sw.default_context(), paf)
            assert_same(dev, sw.AlnStats(text=text), name)
            seen.append(([int(getattr(dev.summary, k)) for k in SUMMARY_INTS], sorted((p[0], p[1], p[3], p[4]) for p in dev.pairs)))
    assert seen[0] == seen[1] == seen[2]
    # every sequence has one length in this text, so coverage per pair is order-independent too
    assert len(seen[0][1]) == int(seen[0][0][7])


def test_unparsable_lines_fail_like_the_host_tool(sw):
    text = line("a#1#c1", 1000, 0, 500, "b#1#c1", 1000, 450) + "\n" + "q\t1\tx\ty\t+\tt\t1\t0\t0\tz\t\t0\n"
    with pytest.raises(sw.SwgError) as host_err:
        sw.AlnStats(text=text)
    with sw.PafFile(text=text) as paf:
        with pytest.raises(sw.SwgError) as dev_err:
            sw.AlnStats.from_paf(sw.default_context(), paf)
    assert str(dev_err.value) == str(host_err.value) and "Invalid query start (line 2)" in str(dev_err.value)
    text = line("a#1#c1", "12x", 0, 500, "b#1#c1", 1000, 450) + "\n"   # a length the device path reads (the sequence's last line)
    with pytest.raises(sw.SwgError) as host_err:
        sw.AlnStats(text=text)
    with sw.PafFile(text=text) as paf:
        with pytest.raises(sw.SwgError) as dev_err:
            sw.AlnStats.from_paf(sw.default_context(), paf)
    assert str(dev_err.value) == str(host_err.value)


# ---- KEPT ------------------------------------------------------------------------------------------------------------------
def run_filter(sw, paf, cfg):
    from sweepga_amd._lib import SwgStats
    ctx = sw.default_context()
    n = paf.n
    status = np.zeros(max(n, 1), dtype=np.uint8)
    chain = np.zeros(max(n, 1), dtype=np.uint32)
    stats = SwgStats()
    cc = cfg.to_c(False, False)
    if n:
        ctx.check(ctx.lib.swg_filter(ctx.handle, C.byref(paf.records), C.byref(cc), status.ctypes.data, chain.ctypes.data, C.byref(stats)))
    return status[:n], chain[:n]


def filter_cfgs(sw):
    FM = sw.FilterMode
    return {
        "default": sw.FilterConfig(),
        "one_to_one": sw.FilterConfig(mapping_filter_mode=FM.OneToOne, mapping_max_per_query=1, mapping_max_per_target=1, scaffold_gap=0),
        "scaffold_rescue": sw.FilterConfig(mapping_filter_mode=FM.OneToOne, mapping_max_per_query=1, mapping_max_per_target=1,
                                           scaffold_filter_mode=FM.OneToOne, scaffold_max_per_query=1, scaffold_max_per_target=1,
                                           scaffold_gap=10_000, min_scaffold_length=2_000, scaffold_max_deviation=20_000),
    }


def check_kept(sw, text, status, chain, tmp_path, what):
    inp, outp = tmp_path / "in.paf", tmp_path / "out.paf"
    inp.write_text(text, newline="")
    with sw.PafFile(path=str(inp)) as paf:
        assert paf.n == len(status)
        paf.write(str(outp), status, chain)
        all_, kept = sw.AlnStats.from_paf(sw.default_context(), paf, status)
    host_in, host_out = sw.AlnStats(path=str(inp)), sw.AlnStats(path=str(outp))
    assert_same(all_, host_in, what + " all")
    assert_same(kept, host_out, what + " kept")
    assert all_.compare(kept, str(inp), str(outp)) == host_in.compare(host_out, str(inp), str(outp)), what
    return all_, kept


@pytest.mark.parametrize("cfg_name", ["default", "one_to_one", "scaffold_rescue"])
@pytest.mark.parametrize("shape", ["pansn", "lengths_vary", "hand"])
def test_kept_equals_the_host_tool_on_the_written_file(sw, tmp_path, shape, cfg_name):
    text = SHAPES[shape] if shape != "pansn" else gen_text(21, 20_000, n_genomes=4, chrs_per_genome=3, span=400_000)
    with sw.PafFile(text=text) as paf:
        status, chain = run_filter(sw, paf, filter_cfgs(sw)[cfg_name])
    all_, kept = check_kept(sw, text, status, chain, tmp_path, f"{shape}/{cfg_name}")
    assert int(kept.summary.total_mappings) == int((status != 0).sum())
    if shape == "pansn":
        assert 0 < int(kept.summary.total_mappings) <= int(all_.summary.total_mappings)
        if cfg_name == "one_to_one":
            assert int(kept.summary.total_mappings) < int(all_.summary.total_mappings)


def test_kept_a_sequence_only_in_dropped_records_and_nothing_kept(sw, tmp_path):
    text = (line("a#1#c1", 1000, 0, 500, "b#1#c1", 2000, 450) + "\n" +
            line("a#1#c2", 5000, 0, 500, "b#1#c1", 2000, 450) + "\n" +     # a#1#c2 appears only here
            line("a#1#c1", 1000, 600, 900, "b#1#c1", 2000, 250) + "\n" +
            line("a#1#c1", 1234, 0, 400, "b#1#c2", 2000, 350) + "\n")      # ... and a#1#c1's LAST length only here
    status = np.array([1, 0, 3, 0], dtype=np.uint8)
    chain = np.array([1, 0, 0, 0], dtype=np.uint32)
    all_, kept = check_kept(sw, text, status, chain, tmp_path, "vanishing sequence")
    # genome a#1#: 1234 + 5000 before, 1000 after; coverage of (a#1#, b#1#) = 100 * bases / that
    assert bits(all_.pairs[0][2]) == bits(100.0 * 1700 / 6234) and bits(kept.pairs[0][2]) == bits(100.0 * 800 / 1000)
    assert int(kept.summary.chr_pair_count) == 1 and int(all_.summary.chr_pair_count) == 3
    none = np.zeros(4, dtype=np.uint8)
    all_, kept = check_kept(sw, text, none, chain, tmp_path, "nothing kept")
    assert int(kept.summary.total_mappings) == 0 and int(kept.summary.genome_pairs) == 0 and kept.pairs == []


# ---- the record seams -------------------------------------------------------------------------------------------------------
def np_counts(q, t, qs, qe, m, seq_genome, sel=None):
    """The integer results of parse_paf (:103-161) over columns, restated."""
    n = len(q)
    idx = np.arange(n) if sel is None else np.flatnonzero(sel)
    q, t = q[idx].astype(np.int64), t[idx].astype(np.int64)
    ln = (qe[idx].astype(np.int64) - qs[idx].astype(np.int64))
    mm = m[idx].astype(np.int64)
    gq, gt = seq_genome[q].astype(np.int64), seq_genome[t].astype(np.int64)
    self_ = q == t
    inter = ~self_ & (gq != gt)
    out = dict(total_mappings=len(idx), total_bases=int(ln.sum()), total_matches=int(mm.sum()), self_mappings=int(self_.sum()),
               inter_genome=int(inter.sum()), inter_chromosomal=int((~self_ & ~inter).sum()),
               chr_pair_count=len(np.unique(q * (1 << 32) + t)))
    G = int(seq_genome.max()) + 1
    key = gq[inter] * G + gt[inter]
    uk, first, inv = np.unique(key, return_index=True, return_inverse=True)
    bases = np.zeros(len(uk), dtype=np.int64)
    matches = np.zeros(len(uk), dtype=np.int64)
    np.add.at(bases, inv, ln[inter])
    np.add.at(matches, inv, mm[inter])
    rec_first = idx[np.flatnonzero(inter)[first]] if len(uk) else np.zeros(0, dtype=np.int64)
    order = np.argsort(rec_first, kind="stable")      # first appearance
    pairs = np.zeros(len(uk), dtype=PAIR_DTYPE)
    pairs["q_genome"], pairs["t_genome"] = (uk // G)[order], (uk % G)[order]
    pairs["bases"], pairs["matches"], pairs["first_record"] = bases[order], matches[order], rec_first[order]
    out["pairs"] = pairs
    out["n_pairs"] = len(uk)
    # last line per sequence: 2 * record + side; assignments in ascending record order, so the last one written is the largest
    as_q = np.full(len(seq_genome), -1, dtype=np.int64)
    as_t = np.full(len(seq_genome), -1, dtype=np.int64)
    as_q[q] = 2 * idx
    as_t[t] = 2 * idx + 1
    last = np.maximum(as_q, as_t)
    out["seq_last"] = np.where(last < 0, np.uint64(NONE64), last.astype(np.uint64)).astype(np.uint64)
    return out


def assert_counts(got, want, what=""):
    for k, v in want.items():
        if k in ("seq_last", "pairs"):
            assert got[k] is not None and got[k].dtype == v.dtype and np.array_equal(got[k], v), (what, k)
        else:
            assert got[k] == v, (what, k, got[k] if k != "pairs" else len(got[k]))


def records_of(cols, n_seq, n=None):
    """SwgRecords over numpy columns (host) or device addresses (then n is given)."""
    from sweepga_amd._lib import SwgRecords
    r = SwgRecords()
    r.n = len(cols["q_id"]) if n is None else n
    for k, a in cols.items():
        setattr(r, k, a if isinstance(a, int) else a.ctypes.data)
    r.n_seq = n_seq
    return r


def synth_columns(rng, n, n_seq, per_genome, order):
    q = rng.integers(0, n_seq, n).astype(np.uint32)
    t = np.where(rng.random(n) < 0.05, q, rng.integers(0, n_seq, n)).astype(np.uint32)
    seq_genome = (np.arange(n_seq) // per_genome).astype(np.uint32)
    if order == "pair_major":
        G = int(seq_genome.max()) + 1
        o = np.argsort(seq_genome[q].astype(np.int64) * G + seq_genome[t], kind="stable")
        q, t = q[o], t[o]
    qs = rng.integers(0, 1_000_000, n).astype(np.uint32)
    qe = (qs + rng.integers(0, 20_000, n)).astype(np.uint32)
    m = rng.integers(0, 20_000, n).astype(np.uint32)
    return dict(q_id=q, t_id=t, q_start=qs, q_end=qe, matches=m), seq_genome


def test_record_seams_host_and_device_agree_with_numpy(sw):
    from sweepga_amd.alnstats import alnstats_counts
    ctx = sw.default_context()
    rng = np.random.default_rng(31)
    for n, n_seq, per_genome, order in ((1, 2, 1, "shuffled"), (70_000, 40, 4, "pair_major"), (70_000, 3_000, 1, "shuffled"),
                                        (50_000, 12, 12, "shuffled"), (1 << 20, 64, 1, "shuffled")):
        cols, seq_genome = synth_columns(rng, n, n_seq, per_genome, order)
        G = int(seq_genome.max()) + 1
        status = (rng.random(n) < 0.4).astype(np.uint8) * rng.integers(1, 4, n).astype(np.uint8)
        want_all = np_counts(*cols.values(), seq_genome)
        want_kept = np_counts(*cols.values(), seq_genome, status != 0)
        a, k = alnstats_counts(ctx, records_of(cols, n_seq), seq_genome, G, status)
        assert_counts(a, want_all, "host all")
        assert_counts(k, want_kept, "host kept")
        a1, none = alnstats_counts(ctx, records_of(cols, n_seq), seq_genome, G)
        assert none is None
        assert_counts(a1, want_all, "host, no status")
        hip = Hip()
        try:
            dcols = {name: hip.up(c) for name, c in cols.items()}
            a2, k2 = alnstats_counts(ctx, records_of(dcols, n_seq, n), hip.up(seq_genome), G, hip.up(status), device=True)
            assert_counts(a2, want_all, "device all")
            assert_counts(k2, want_kept, "device kept")
        finally:
            hip.free()
        # the capacity protocol: too small a pair array is left alone, n_pairs says how many there are
        a3, _ = alnstats_counts(ctx, records_of(cols, n_seq), seq_genome, G, pair_capacity=max(want_all["n_pairs"] - 1, 0) or 1)
        if want_all["n_pairs"] > 1:
            assert a3["n_pairs"] == want_all["n_pairs"] and a3["pairs"] is None


def test_device_seam_on_the_status_swg_filter_device_leaves(sw):
    from sweepga_amd._lib import SwgRecords, SwgStats
    from sweepga_amd.alnstats import alnstats_counts
    rng = np.random.default_rng(41)
    rec = gen.random_records(rng, 30_000, n_genomes=4, chrs_per_genome=3, span=500_000)
    packed = sw.pack_records(gen.records_to_meta(rec))
    assert not packed.wide
    n = packed.n
    ctx = sw.default_context()
    hip = Hip()
    try:
        r = SwgRecords()
        r.n = n
        for k in ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end", "identity", "matches", "block_len", "strand"):
            setattr(r, k, hip.up(packed.cols[k]))
        r.n_seq = packed.n_seq
        r.seq_genome_last = hip.up(packed.seq_genome_last)
        r.n_genome_last = packed.n_genome_last
        r.seq_genome_two = hip.up(packed.seq_genome_two)
        r.n_genome_two = packed.n_genome_two
        d_status, d_chain = hip.alloc(n), hip.alloc(4 * n)
        cc = sw.FilterConfig().to_c(False, False)
        stats = SwgStats()
        ctx.check(ctx.lib.swg_filter_device(ctx.handle, C.byref(r), C.byref(cc), C.c_void_p(d_status), C.c_void_p(d_chain), C.byref(stats)))
        a, k = alnstats_counts(ctx, r, r.seq_genome_last, packed.n_genome_last, d_status, device=True)
        status = hip.down(d_status, np.uint8, n)
    finally:
        hip.free()
    cols = [packed.cols[c] for c in ("q_id", "t_id", "q_start", "q_end", "matches")]
    assert_counts(a, np_counts(*cols, packed.seq_genome_last), "all")
    assert_counts(k, np_counts(*cols, packed.seq_genome_last, status != 0), "kept")
    assert k["total_mappings"] == stats.n_out > 0


def test_under_a_memory_limit_the_answer_is_the_same_or_a_clean_oom(sw):
    from sweepga_amd.alnstats import alnstats_counts
    ctx = sw.Context(0)
    try:
        rng = np.random.default_rng(51)
        n, n_seq = 400_000, 5_000
        cols, seq_genome = synth_columns(rng, n, n_seq, 1, "shuffled")     # G = 5000: hashed pair table
        status = (rng.random(n) < 0.5).astype(np.uint8)
        want_all, want_kept = np_counts(*cols.values(), seq_genome), np_counts(*cols.values(), seq_genome, status != 0)
        outcomes = []
        for limit in (1 << 20, 8 << 20, 24 << 20, 64 << 20, 1 << 30, 0):
            ctx.set_memory_limit(limit)
            try:
                a, k = alnstats_counts(ctx, records_of(cols, n_seq), seq_genome, n_seq, status)
            except sw.SwgError as e:
                assert e.code == -4, e     # SWG_ERR_OOM, nothing else
                outcomes.append("oom")
                continue
            assert_counts(a, want_all, f"limit {limit} all")
            assert_counts(k, want_kept, f"limit {limit} kept")
            outcomes.append("ok")
            if limit:
                assert ctx.memory_info()[0] <= limit
        # 21 bytes per record of staging alone are 8.4 MB: the smallest limits cannot hold the call, no limit can
        assert outcomes[0] == outcomes[1] == "oom" and outcomes[-1] == outcomes[-2] == "ok", outcomes
    finally:
        ctx.close()


def test_ids_out_of_range_are_refused(sw):
    from sweepga_amd.alnstats import alnstats_counts
    ctx = sw.default_context()
    rng = np.random.default_rng(61)
    cols, seq_genome = synth_columns(rng, 5_000, 30, 3, "shuffled")
    cols["t_id"][1234] = 30
    with pytest.raises(sw.SwgError) as e:
        alnstats_counts(ctx, records_of(cols, 30), seq_genome, 10)
    assert e.value.code == -1
    cols["t_id"][1234] = 3
    with pytest.raises(sw.SwgError) as e:
        alnstats_counts(ctx, records_of(cols, 30), seq_genome, 9)      # genome id 9 >= n_genome
    assert e.value.code == -1


# ---- command line ---------------------------------------------------------------------------------------------------------
def test_cli_stats(sw, tmp_path):
    from sweepga_amd import build
    text = gen_text(71, 15_000, n_genomes=4, chrs_per_genome=3, span=400_000)
    inp = tmp_path / "in.paf"
    inp.write_text(text, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-jump", "10k", "--scaffold-mass", "2k", "--quiet"]
    plain, out, rep = tmp_path / "plain.paf", tmp_path / "out.paf", tmp_path / "rep.txt"
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), *flags], capture_output=True)
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--stats", str(rep), *flags], capture_output=True)
    assert r0.returncode == r.returncode == 0, r.stderr
    assert out.read_bytes() == plain.read_bytes() and out.stat().st_size > 0 and r.stdout == r0.stdout == b""
    host = subprocess.run([build.STATS, str(inp), str(out)], capture_output=True)
    assert host.returncode == 0 and rep.read_bytes() == host.stdout and len(host.stdout) > 500
    # --stats-detailed: followed by the two -d reports
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--stats", str(rep), "--stats-detailed", *flags], capture_output=True)
    d_in = subprocess.run([build.STATS, str(inp), "-d"], capture_output=True).stdout
    d_out = subprocess.run([build.STATS, str(out), "-d"], capture_output=True).stdout
    assert r.returncode == 0 and rep.read_bytes() == host.stdout + d_in + d_out and out.read_bytes() == plain.read_bytes()
    # --stats - : the report on standard error, the PAF alone on standard output
    r1 = subprocess.run([build.CLI, str(inp), *flags], capture_output=True)
    r2 = subprocess.run([build.CLI, str(inp), "--stats", "-", *flags], capture_output=True)
    assert r1.returncode == r2.returncode == 0 and r2.stdout == r1.stdout == plain.read_bytes()
    host_dash = subprocess.run([build.STATS, str(inp), "-"], input=r1.stdout, capture_output=True)
    assert r2.stderr == host_dash.stdout
    # gzip input
    gz = tmp_path / "in.paf.gz"
    gz.write_bytes(gzip.compress(text.encode()))
    r = subprocess.run([build.CLI, str(gz), "--output-file", str(out), "--stats", str(rep), *flags], capture_output=True)
    host = subprocess.run([build.STATS, str(gz), str(out)], capture_output=True)
    assert r.returncode == 0 and out.read_bytes() == plain.read_bytes() and rep.read_bytes() == host.stdout
    # --no-filter: every line to standard output, the host report of the input against itself
    r = subprocess.run([build.CLI, str(inp), "--no-filter", "--stats", str(rep)], capture_output=True)
    host = subprocess.run([build.STATS, str(inp), "-"], input=r.stdout, capture_output=True)
    assert r.returncode == 0 and r.stdout == text.encode() and rep.read_bytes() == host.stdout


# ---- size -----------------------------------------------------------------------------------------------------------------
def test_twenty_million_records_pair_major_and_shuffled(sw):
    """2 * 10^7 records over 3000 genomes of one sequence each (G * G beyond the dense limit: the hashed genome-pair table),
    thousands of work-groups merging into it; device-resident columns, both orders, against the numpy restatement."""
    from sweepga_amd.alnstats import alnstats_counts
    ctx = sw.default_context()
    rng = np.random.default_rng(81)
    n, n_seq = 20_000_000, 3_000
    for order in ("pair_major", "shuffled"):
        cols, seq_genome = synth_columns(rng, n, n_seq, 1, order)
        status = (rng.random(n) < 0.3).astype(np.uint8)
        hip = Hip()
        try:
            dcols = {name: hip.up(c) for name, c in cols.items()}
            d_genome, d_status = hip.up(seq_genome), hip.up(status)
            ctx.profile(True)
            ctx.profile_reset()
            a, k = alnstats_counts(ctx, records_of(dcols, n_seq, n), d_genome, n_seq, d_status, device=True)
            table = ctx.profile_table()
            ctx.profile(False)
        finally:
            hip.free()
        for name in ("alnstats_seqpair", "alnstats_reduce", "alnstats_collect"):
            assert table[name][0] >= 1, (order, table)   # (twice when the first attempt outgrew the scratch arena)
        print(order, {name: round(table[name][1], 3) for name in table})
        want_all, want_kept = np_counts(*cols.values(), seq_genome), np_counts(*cols.values(), seq_genome, status != 0)
        assert want_all["n_pairs"] > 1 << 20
        assert_counts(a, want_all, order + " all")
        assert_counts(k, want_kept, order + " kept")
