"""Tree sparsification on records, on the device (sweepga_amd/csrc/swg_sparsify.hip): the mask of swg_paf_tree_select against the
lines the oracle's text pass keeps; the record seams against the handle; swg_filter_subset_device against swg_filter_device on
numpy-compacted columns; the command line against oracle/sweepga-ref byte for byte, with the route it reports; the .1aln twin.
Sequence ids are not renumbered after compaction (include/sweepga_gpu.h): test_ids_keep_the_full_inputs_numbering
builds the input where that could matter and compares with the oracle on the sparsified text."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import gen, orc
from tests.test_gpu_ranged import Hip, _reorder
from tests.test_tree_filter_cpu import oracle_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = [(1, 0, 0.0), (2, 1, 0.1), (0, 2, 0.0), (5, 2, 0.05), (0, 0, 0.3), (3, 0, 1.0)]
COLS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end", "identity", "matches", "block_len", "strand")


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


def genome_two(name):
    parts = name.split("#")
    return parts[0] + "#" + parts[1] + "#" if len(parts) >= 2 else name


def ordered(rec, how, rng):
    n = len(rec.qname)
    if how == "shuffled":
        return _reorder(rec, rng.permutation(n))
    gq = np.array([genome_two(s) for s in rec.qname])
    gt = np.array([genome_two(s) for s in rec.tname])
    if how == "by_query":
        return _reorder(rec, np.argsort(gq, kind="stable"))
    return _reorder(rec, np.lexsort((gt, gq)))      # pair-major


def plain_paf(rec):
    """One bare line per record (no tags: every handle column is what the text pass reads)."""
    return "".join(f"{rec.qname[i]}\t1000000\t{rec.qs[i]}\t{rec.qe[i]}\t{chr(rec.strand[i])}\t{rec.tname[i]}\t1000000\t{rec.ts[i]}\t{rec.te[i]}"
                   f"\t{rec.matches[i]}\t{rec.block_length[i]}\t60\n" for i in range(len(rec.qname)))


class Paf:
    def __init__(self, text):
        from sweepga_amd import _lib
        self.lib = _lib.load()
        raw = text.encode()
        self.h = C.c_void_p()
        assert self.lib.swg_paf_open_buffer(raw, len(raw), 8, C.byref(self.h)) == 0, self.lib.swg_paf_last_error()
        self.rec = self.lib.swg_paf_records(self.h).contents
        self.n = int(self.rec.n)
        self.ranks = np.ctypeslib.as_array(C.cast(self.lib.swg_paf_ranks(self.h), C.POINTER(C.c_uint64)), (max(self.n, 1),))[:self.n]

    def col(self, name, dtype):
        n = self.rec.n_seq if name.startswith("seq_") else self.n
        return np.ctypeslib.as_array(C.cast(getattr(self.rec, name), C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), (max(n, 1),))[:n]

    def close(self):
        self.lib.swg_paf_close(self.h)


def kept_text(lines, ranks, keep):
    return "".join(lines[int(ranks[i])] + "\n" for i in np.flatnonzero(keep))


CASES = [  # n, genomes, chromosomes, PanSN names, order, self fraction
    (1_000, 5, 2, True, "shuffled", 0.1),
    (50_000, 12, 3, True, "pair_major", 0.02),
    (200_000, 40, 2, True, "by_query", 0.02),
    (1_000_000, 40, 2, True, "shuffled", 0.02),
    (20_000, 30, 1, False, "shuffled", 0.05),        # names without '#': every contig its own genome
    (300_000, 1_500, 1, False, "shuffled", 0.01),    # G x G > 2^20: the open-addressing pair table and selected-pair set
    (300_000, 1_500, 1, False, "pair_major", 0.01),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_mask_equals_the_oracles_lines_and_the_record_seams_agree(sw, case):
    from sweepga_amd import sparsify
    n, ng, nc, pansn, how, self_frac = CASES[case]
    rng = np.random.default_rng(900 + case)
    rec = ordered(gen.random_records(rng, n, n_genomes=ng, chrs_per_genome=nc, pansn=pansn, self_frac=self_frac), how, rng)
    text = plain_paf(rec)
    lines = text.split("\n")
    ctx = sw.default_context()
    p = Paf(text)
    hip = Hip()
    try:
        assert p.n == n and p.lib.swg_paf_tree_needs_text(p.h) == 0
        pre = sparsify.handle_prefixes(p.h)
        assert (len(pre) > 1024) == (ng > 1024)
        g_two = p.col("seq_genome_two", np.uint32)
        d_rec = None
        for kn, kf, rf in GRID:
            keep, n_kept, route = sparsify.paf_tree_select(ctx, p.h, kn, kf, rf)
            assert route == sparsify.ROUTE_DEVICE and n_kept == int(keep.sum())
            assert set(np.unique(keep).tolist()) <= {0, 1}
            assert kept_text(lines, p.ranks, keep) == oracle_tree(text, kn, kf, rf), (case, kn, kf, rf)
            # record seam = handle: host columns ...
            k2, m2 = sparsify.tree_select(ctx, p.rec, g_two, pre, kn, kf, rf)
            assert m2 == n_kept and np.array_equal(k2, keep), (case, kn, kf, rf, "host seam")
            # ... and device columns (only the four columns the call reads exist on the device)
            if d_rec is None:
                from sweepga_amd._lib import SwgRecords
                d_rec = SwgRecords()
                d_rec.n, d_rec.n_seq = n, p.rec.n_seq
                for c in ("q_id", "t_id", "matches", "block_len"):
                    setattr(d_rec, c, hip.up(p.col(c, np.uint32)))
                d_genome, d_keep = hip.up(g_two), hip.alloc(n)
            _, m3 = sparsify.tree_select(ctx, d_rec, d_genome, pre, kn, kf, rf, device=True, keep=d_keep)
            assert m3 == n_kept and np.array_equal(hip.down(d_keep, np.uint8, n), keep), (case, kn, kf, rf, "device seam")
    finally:
        hip.free()
        p.close()


def test_select_errors(sw):
    from sweepga_amd import _lib, sparsify
    ctx = sw.default_context()
    q = np.array([0, 1, 0], dtype=np.uint32)
    t = np.array([1, 0, 1], dtype=np.uint32)
    big = np.full(3, 0xffffffff, dtype=np.uint32)
    r = _lib.SwgRecords()
    r.n, r.n_seq = 3, 2
    r.q_id, r.t_id, r.matches, r.block_len = q.ctypes.data, t.ctypes.data, big.ctypes.data, big.ctypes.data
    keep, m = sparsify.tree_select(ctx, r, np.array([0, 1], dtype=np.uint32), ["a#1#", "b#1#"], 1)
    assert keep.tolist() == [1, 1, 1] and m == 3
    with pytest.raises(_lib.SwgError) as e:    # a genome id out of range
        sparsify.tree_select(ctx, r, np.array([0, 2], dtype=np.uint32), ["a#1#", "b#1#"], 1)
    assert e.value.code == -1
    # a pair's sum of 2^53 or more: 2^21 + 1 records of 2^32 - 1
    n = (1 << 21) + 1
    z = np.zeros(n, dtype=np.uint32)
    o = np.ones(n, dtype=np.uint32)
    f = np.full(n, 0xffffffff, dtype=np.uint32)
    r.n = n
    r.q_id, r.t_id, r.matches, r.block_len = z.ctypes.data, o.ctypes.data, f.ctypes.data, f.ctypes.data
    with pytest.raises(_lib.SwgError) as e:
        sparsify.tree_select(ctx, r, np.array([0, 1], dtype=np.uint32), ["a#1#", "b#1#"], 1)
    assert e.value.code == -5
    r.n = n - 2                                 # (2^21 - 1) * (2^32 - 1) < 2^53
    keep, m = sparsify.tree_select(ctx, r, np.array([0, 1], dtype=np.uint32), ["a#1#", "b#1#"], 1)
    assert m == n - 2


# ---- the subset filter ---------------------------------------------------------------------------------------------------------
CONFIGS = [
    ("default", dict()),
    ("sweep", dict(mapping_filter_mode="OneToOne", scaffold_gap=0)),
    ("c5", dict(scaffold_filter_mode="OneToOne", scaffold_max_deviation=20_000)),
    ("full", dict(mapping_filter_mode="OneToOne", scaffold_filter_mode="OneToOne", scaffold_max_deviation=20_000)),
]


def make_cfg(sw, kw):
    kw = dict(kw)
    for k in ("mapping_filter_mode", "scaffold_filter_mode"):
        if k in kw:
            kw[k] = getattr(sw.FilterMode, kw[k])
    return sw.FilterConfig(**kw).to_c(False, False)


def device_records(hip, packed, cols=None, n=None):
    from sweepga_amd._lib import SwgRecords
    r = SwgRecords()
    cols = packed.cols if cols is None else cols
    r.n = packed.n if n is None else n
    for k in COLS:
        setattr(r, k, hip.up(cols[k]) if cols[k] is not None else None)
    r.n_seq = packed.n_seq
    r.seq_genome_last = hip.up(packed.seq_genome_last)
    r.n_genome_last = packed.n_genome_last
    r.seq_genome_two = hip.up(packed.seq_genome_two)
    r.n_genome_two = packed.n_genome_two
    return r


def reference_subset(sw, ctx, hip, packed, keep, cc):
    """swg_filter_device on numpy-compacted columns, scattered back in numpy"""
    from sweepga_amd._lib import SwgStats
    n, sel = packed.n, np.flatnonzero(keep)
    status, chain = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32)
    if len(sel):
        sub = {k: np.ascontiguousarray(packed.cols[k][sel]) for k in COLS}
        r = device_records(hip, packed, sub, len(sel))
        d_s, d_c = hip.alloc(len(sel)), hip.alloc(4 * len(sel))
        ctx.check(ctx.lib.swg_filter_device(ctx.handle, C.byref(r), C.byref(cc), C.c_void_p(d_s), C.c_void_p(d_c), C.byref(SwgStats())))
        status[sel] = hip.down(d_s, np.uint8, len(sel))
        chain[sel] = hip.down(d_c, np.uint32, len(sel))
    return status, chain


def check_subset(sw, packed, keep, cfgs, what):
    from sweepga_amd import sparsify
    ctx = sw.default_context()
    n = packed.n
    for name, kw in cfgs:
        cc = make_cfg(sw, kw)
        hip = Hip()
        try:
            want_s, want_c = reference_subset(sw, ctx, hip, packed, keep, cc)
            r = device_records(hip, packed)
            # poisoned outputs: no entry may be left unwritten
            d_s, d_c, d_k = hip.up(np.full(n, 0xff, dtype=np.uint8)), hip.up(np.full(n, 0xffffffff, dtype=np.uint32)), hip.up(keep)
            _, _, st = sparsify.filter_subset(ctx, r, d_k, cc, device=True, status=d_s, chain=d_c)
            got_s, got_c = hip.down(d_s, np.uint8, n), hip.down(d_c, np.uint32, n)
            assert np.array_equal(got_s, want_s) and np.array_equal(got_c, want_c), (what, name, "device")
            assert st.n_in == n and st.n_out == int((want_s != 0).sum())
        finally:
            hip.free()
        hs, hc, _ = sparsify.filter_subset(ctx, packed.to_c(), keep, cc)     # host columns; outputs start as 0xff in the mirror
        assert np.array_equal(hs, want_s) and np.array_equal(hc, want_c), (what, name, "host")
        assert not (want_s[keep == 0] != 0).any() and not (want_c[keep == 0] != 0).any()


def packed_records(sw, rng, n, **kw):
    rec = gen.random_records(rng, n, **kw)
    packed = sw.pack_records(gen.records_to_meta(rec))
    assert not packed.wide and packed.n == n
    return rec, packed


def test_subset_filter_equals_filter_on_compacted_columns(sw):
    rng = np.random.default_rng(77)
    _, packed = packed_records(sw, rng, 60_000, n_genomes=6, chrs_per_genome=3, span=600_000)
    n = packed.n
    one = np.zeros(n, dtype=np.uint8)
    one[n // 3] = 1
    masks = {"random 0.5": (rng.random(n) < 0.5).astype(np.uint8), "random 0.03": (rng.random(n) < 0.03).astype(np.uint8),
             "all ones": np.ones(n, dtype=np.uint8), "all zeros": np.zeros(n, dtype=np.uint8), "one kept": one,
             "any non-zero byte counts": (rng.random(n) < 0.5).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)}
    for what, keep in masks.items():
        check_subset(sw, packed, keep, CONFIGS, what)


@pytest.mark.parametrize("n", [63, 64, 65, 1023, 1025, (1 << 20) + 1])
def test_subset_filter_sizes(sw, n):
    rng = np.random.default_rng(n)
    _, packed = packed_records(sw, rng, n, n_genomes=4, chrs_per_genome=2, span=max(200_000, n))
    keep = (rng.random(n) < 0.6).astype(np.uint8)
    keep[[0, n - 1]] = (1, 1)
    check_subset(sw, packed, keep, CONFIGS if n < 100_000 else CONFIGS[:1] + CONFIGS[3:], f"n={n}")
    keep[[0, n - 1]] = (0, 0)
    check_subset(sw, packed, keep, CONFIGS[:1], f"n={n}, ends dropped")


def test_keep_null_is_the_plain_filter(sw):
    from sweepga_amd import sparsify
    rng = np.random.default_rng(5)
    _, packed = packed_records(sw, rng, 20_000, n_genomes=3, chrs_per_genome=2)
    ctx = sw.default_context()
    cc = make_cfg(sw, {})
    s0, c0 = sw.PafFilter(sw.FilterConfig()).filter_columns(packed)
    s1, c1, _ = sparsify.filter_subset(ctx, packed.to_c(), None, cc)
    assert np.array_equal(s0, s1) and np.array_equal(c0, c1)


def test_subset_filter_under_a_memory_limit(sw):
    from sweepga_amd import _lib, sparsify
    rng = np.random.default_rng(6)
    _, packed = packed_records(sw, rng, 50_000, n_genomes=5, chrs_per_genome=2, span=500_000)
    keep = (rng.random(packed.n) < 0.5).astype(np.uint8)
    cc = make_cfg(sw, {})
    hip = Hip()
    ctx = sw.Context(0)
    try:
        want_s, want_c = reference_subset(sw, sw.default_context(), hip, packed, keep, cc)
        r = device_records(hip, packed)
        d_s, d_c, d_k = hip.alloc(packed.n), hip.alloc(4 * packed.n), hip.up(keep)
        ctx.set_memory_limit(1 << 30)
        sparsify.filter_subset(ctx, r, d_k, cc, device=True, status=d_s, chain=d_c)
        assert np.array_equal(hip.down(d_s, np.uint8, packed.n), want_s) and np.array_equal(hip.down(d_c, np.uint32, packed.n), want_c)
        assert ctx.memory_limit() == 1 << 30
        ctx.set_memory_limit(256 << 10)       # does not hold the compacted columns: a clean SWG_ERR_OOM
        with pytest.raises(_lib.SwgError) as e:
            sparsify.filter_subset(ctx, r, d_k, cc, device=True, status=d_s, chain=d_c)
        assert e.value.code == -4 and ctx.memory_limit() == 256 << 10
    finally:
        ctx.close()
        hip.free()


def test_ids_keep_the_full_inputs_numbering(sw):
    """A sequence first seen in a DROPPED line and next seen after a later sequence's kept line: parsed afresh, the sparsified text
    numbers the two sequences the other way round.  The subset filter on the full input's ids must still give what the oracle
    gives on the sparsified text -- status and chain number of every kept line -- for every flag set."""
    from sweepga_amd import sparsify
    rng = np.random.default_rng(12)
    rec = gen.random_records(rng, 40_000, n_genomes=6, chrs_per_genome=3, span=400_000)
    # pair-major by DESCENDING genome of the query: dropped pairs come first and introduce most sequences
    order = np.lexsort((np.array(rec.tname), np.array(rec.qname)))[::-1]
    rec = _reorder(rec, np.ascontiguousarray(order))
    text = plain_paf(rec)
    lines = text.split("\n")
    ctx = sw.default_context()
    p = Paf(text)
    try:
        keep, n_kept, route = sparsify.paf_tree_select(ctx, p.h, 1, 1, 0.0)
        assert route == sparsify.ROUTE_DEVICE and 0 < n_kept < p.n
        sparse_text = oracle_tree(text, 1, 1, 0.0)
        assert kept_text(lines, p.ranks, keep) == sparse_text
        # the situation in question does occur: the first-appearance order of the sequences differs between the two numberings
        q_id, t_id = p.col("q_id", np.uint32), p.col("t_id", np.uint32)
        seen = []
        for i in np.flatnonzero(keep):
            for s in (int(q_id[i]), int(t_id[i])):
                if s not in seen:
                    seen.append(s)
        assert seen != sorted(seen)
        orec = orc.parse_paf_text(sparse_text)
        sel = np.flatnonzero(keep)
        for name, kw in CONFIGS:
            okw = {k: (orc.ONE_TO_ONE if v == "OneToOne" else v) for k, v in kw.items()}
            ost, och = orc.apply_filters(orc.Config(**okw), orec)
            s, c, _ = sparsify.filter_subset(ctx, p.rec, keep, make_cfg(sw, kw))
            assert np.array_equal(s[sel], ost) and np.array_equal(c[sel], och), name
            assert not s[keep == 0].any() and not c[keep == 0].any()
    finally:
        p.close()


# ---- the command line ----------------------------------------------------------------------------------------------------------
FLAG_SETS = [[], ["--num-mappings", "1:1", "--scaffold-jump", "0"],
             ["--num-mappings", "1:1", "--scaffold-filter", "1:1", "--scaffold-dist", "20000"]]


@pytest.fixture(scope="module")
def bins():
    from sweepga_amd import build
    return build.CLI, os.path.join(ROOT, "oracle", "sweepga-ref"), build.STATS


@pytest.mark.parametrize("irregular", [False, True])
def test_cli_is_byte_identical_and_names_its_route(bins, tmp_path, irregular):
    cli, ref, stats_bin = bins
    rng = np.random.default_rng(31 + irregular)
    rec = ordered(gen.random_records(rng, 30_000, n_genomes=7, chrs_per_genome=3, span=500_000), "by_query", rng)
    # irregular: cg:Z: / dv:f: tags and junk lines, among them a 12-field line whose columns 10 and 11 do not parse
    text = gen.records_to_paf(rng, rec) if irregular else plain_paf(rec)
    if irregular:
        assert "\tz\t\t0" in text
    paf = tmp_path / "in.paf"
    paf.write_text(text)
    for k, flags in enumerate(FLAG_SETS):
        o1, o2, rep = tmp_path / f"gpu{k}.paf", tmp_path / f"ref{k}.paf", tmp_path / f"stats{k}.txt"
        args = [str(paf), "--sparsify", "tree:2:1:0.1", *flags]
        # (SWG_DEBUG: the command line poisons its result columns and checks that every entry was written)
        r = subprocess.run([cli, *args, "--output-file", str(o1)] + ([] if irregular else ["--stats", str(rep)]), capture_output=True,
                           text=True, env=dict(os.environ, SWG_DEBUG="1"))
        assert r.returncode == 0, r.stderr[-2000:]
        subprocess.check_call([ref, *args, "--output-file", str(o2)])
        assert o1.read_bytes() == o2.read_bytes(), flags
        assert os.path.getsize(o1) > 0
        route = [ln for ln in r.stderr.splitlines() if "--sparsify tree:2:1:0.1:" in ln]
        assert len(route) == 1 and ("text fall-back" if irregular else "device mask") in route[0], r.stderr[-2000:]
        if not irregular:
            assert "30000 records" in route[0]
        # --stats with --sparsify: what `alnstats <input> <output>` prints, byte for byte
        if not irregular:
            want = subprocess.run([stats_bin, str(paf), str(o1)], capture_output=True)
            assert want.returncode == 0 and rep.read_bytes() == want.stdout, flags


# ---- .1aln ----------------------------------------------------------------------------------------------------------------------
def test_aln_twin_equals_the_oracle_on_the_same_alignments(sw):
    """apply_tree_filter_to_1aln sums aln.matches over aln.query_end - aln.query_start (src/tree_filter.rs:314-317): the PAF lines
    the oracle reads carry that span as column 11, the names as the handle cuts them."""
    from sweepga_amd import sparsify
    rng = np.random.default_rng(3)
    n = 40_000
    heads = [f"g{g}#1#chr{c}" + str(rng.choice(["", " len=12345 circular", "\tdesc"])) for g in range(9) for c in range(3)]
    heads += ["plain" + str(rng.choice(["", " x"])), "other"]
    qi = rng.integers(0, len(heads), n)
    ti = rng.integers(0, len(heads), n)
    qn, tn = [heads[i] for i in qi], [heads[i] for i in ti]
    qs = rng.integers(0, 400_000, n)
    ql = np.minimum(np.exp(rng.normal(7.5, 1.0, n)).astype(np.int64) + 50, 20_000)
    ts = rng.integers(0, 400_000, n)
    tl = np.maximum(ql + rng.integers(-30, 30, n), 1)
    matches = (ql * rng.uniform(0.5, 1.0, n)).astype(np.int64)
    strand = "".join(rng.choice(["+", "-"], n))
    ctx = sw.default_context()
    with sw.AlnRecords(qn, tn, qs, qs + ql, ts, ts + tl, matches, strand) as a:
        names = a.names
        r = a.records
        q_id = np.ctypeslib.as_array(C.cast(r.q_id, C.POINTER(C.c_uint32)), (n,))
        t_id = np.ctypeslib.as_array(C.cast(r.t_id, C.POINTER(C.c_uint32)), (n,))
        text = "".join(f"{names[q_id[i]]}\t1\t{qs[i]}\t{qs[i] + ql[i]}\t{strand[i]}\t{names[t_id[i]]}\t1\t{ts[i]}\t{ts[i] + tl[i]}\t{matches[i]}\t{ql[i]}\t60\n"
                       for i in range(n))
        lines = text.split("\n")
        pre = sparsify.handle_prefixes(a.handle, aln=True)
        assert sorted(pre) == sorted({genome_two(s) for s in names})
        for kn, kf, rf in GRID:
            keep, n_kept = sparsify.aln_tree_select(ctx, a.handle, kn, kf, rf)
            assert n_kept == int(keep.sum())
            assert kept_text(lines, np.arange(n), keep) == oracle_tree(text, kn, kf, rf), (kn, kf, rf)
