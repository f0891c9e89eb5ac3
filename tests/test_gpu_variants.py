"""The variant calls on the device (sweepga_amd/csrc/swg_variants.hip) against tests/variants_model.py: in every case the host seam
against the model and the device seam against the host seam -- variants, pool, pairs and counts, byte for byte.  The shapes are the
smallest at which each part can go wrong: the column pass's tile of 1,024 candidates with a mismatch on the first and last column of
every tile and of every op, the compaction's tile of 4,096 flags, entries of one op, indels at a contig's first base, one thread's
allele loop over 70,000 bases, the LDS genome-pair table's 256 slots; the capacity protocol; random cases with lower case, IUPAC
codes and X ops over equal bases.  Every comparison is exact: integers and bytes.  The model's own assertions (the consensus
property among them) run where the entries are short; tests/test_variants_cpu.py runs them on 3,000 random entries."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import lift_model as lm
from tests import variants_model as vm
from tests.test_gpu_alnstats import filter_cfgs, run_filter
from tests.test_gpu_lift import Dev
from tests.test_gpu_wide import Hip

pytestmark = pytest.mark.gpu
COLS = lm.COLS
FIELDS = vm.FIELDS
SNP, INS, DEL = vm.SNP, vm.INS, vm.DEL


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


def same(a, b):
    return (a.variants.tobytes() == b.variants.tobytes() and a.pool.tobytes() == b.pool.tobytes() and a.pairs.tobytes() == b.pairs.tobytes()
            and all(getattr(a, f) == getattr(b, f) for f in FIELDS))


def both_seams(sw, cols, strand, genome, G_, cig, seqs, status=None, set_=0, ref=None, query=None, max_indel=0, ctx=None, shift=0):
    """The result of the host seam, after checking that the device seam gives the same.  shift: the device text and the device bases
    start that many bytes behind a 16-byte boundary."""
    from sweepga_amd.lift import cigar_set
    from sweepga_amd.variants import sequence_set, variant_records, variant_records_device
    ctx = ctx or sw.default_context()
    recs = sorted(cig)
    n_seq = len(genome)
    kw = dict(status=status, set=set_, ref=ref, query=query, max_indel=max_indel)
    s_off, s_bases = sequence_set(seqs)
    got = variant_records(ctx, cols, strand, n_seq, genome, G_, recs, [cig[i] for i in recs], (s_off, s_bases), **kw)
    record, offset, text = cigar_set(recs, [cig[i] for i in recs])
    hip = Hip()
    try:
        dcols = {k: Dev(hip, cols[k], np.uint32) for k in COLS}
        dtext = Dev(hip, np.concatenate([np.zeros(shift, dtype=np.uint8), text]))
        dbases = Dev(hip, np.concatenate([np.zeros(shift, dtype=np.uint8), s_bases]))
        dtext.ptr += shift
        dbases.ptr += shift
        kw["status"] = Dev(hip, status, np.uint8) if status is not None else None
        dev = variant_records_device(ctx, dcols, Dev(hip, strand, np.uint8), n_seq, Dev(hip, genome, np.uint32), G_, Dev(hip, record), Dev(hip, offset), dtext,
                                     len(recs), Dev(hip, s_off), dbases, **kw)
    finally:
        hip.free()
    assert same(dev, got)
    return got


def compare(got, want, what=""):
    assert {f: getattr(got, f) for f in FIELDS} == {f: want[f] for f in FIELDS}, what
    rows = vm.variants_array(want["variants"])
    if got.variants.tobytes() != rows.tobytes():
        bad = [k for k in range(len(rows)) if got.variants[k].tobytes() != rows[k].tobytes()]
        raise AssertionError((what, len(bad), [(k, tuple(int(v) for v in got.variants[k]), want["variants"][k]) for k in bad[:5]]))
    if got.pool.tobytes() != want["pool"]:
        k = next(k for k in range(len(want["pool"])) if got.pool[k] != want["pool"][k])
        raise AssertionError((what, "pool byte", k, got.pool[max(k - 8, 0):k + 8].tobytes(), want["pool"][max(k - 8, 0):k + 8]))
    assert [tuple(int(v) for v in p) for p in got.pairs] == want["pairs"], what
    assert got.pairs.tobytes() == vm.pairs_array(want["pairs"]).tobytes(), what


def check(sw, cols, strand, genome, G_, cig, seqs, status=None, set_=0, ref=None, query=None, max_indel=0, what="", ctx=None, shift=0, model_checks=True):
    """Both seams against the model."""
    cols = {k: np.asarray(cols[k]).astype(np.uint32) for k in COLS}
    strand = np.asarray(strand).astype(np.uint8)
    genome = np.asarray(genome).astype(np.uint32)
    got = both_seams(sw, cols, strand, genome, G_, cig, seqs, status, set_, ref, query, max_indel, ctx, shift)
    compare(got, vm.variant_records(cols, strand, genome, G_, cig, seqs, None if status is None else np.asarray(status) != 0, set_, ref, query, max_indel,
                                    check=model_checks), what)
    return got


def build_case(rng, specs, gap=3, lead=2, lower=0.0, iupac=0.0):
    """One record per spec (edits, minus, fuse, fake), target on sequence 1 and query on sequence 0, one behind the other from base
    `lead` on.  -> (cols, strand, cigars, seqs)"""
    need = [sum(l for l, ch in s[0] if ch in "=XD") for s in specs]
    T = vm.plant(rng, vm.random_bases(rng, lead + sum(need) + gap * len(specs) + 1), lower, iupac)
    cols = {k: np.zeros(len(specs), dtype=np.int64) for k in COLS}
    cols["t_id"][:] = 1
    t, q, parts, cigars = lead, 0, [], {}
    for i, (edits, minus, fuse, fake) in enumerate(specs):
        cigars[i], walk, t_end = vm.derive(rng, T, t, edits, minus, fuse, fake)
        flank = vm.random_bases(rng, lead if i == 0 else gap)
        cols["q_start"][i], cols["q_end"][i], cols["t_start"][i], cols["t_end"][i] = q + len(flank), q + len(flank) + len(walk), t, t_end
        parts += [flank, vm.plant(rng, walk, lower, 0.0)]
        q, t = q + len(flank) + len(walk), t_end + gap
    strand = np.array([s[1] for s in specs], dtype=np.uint8)
    return {k: v.astype(np.uint32) for k, v in cols.items()}, strand, cigars, [b"".join(parts) + b"A", T]


def check_specs(sw, rng, specs, what="", lower=0.0, iupac=0.0, **kw):
    cols, strand, cig, seqs = build_case(rng, specs, lower=lower, iupac=iupac)
    return check(sw, cols, strand, [0, 1], 2, cig, seqs, what=what, **kw)


# ---- the column pass -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", [False, True])
def test_mismatches_on_the_first_and_last_column_of_every_tile_and_op(sw, fuse):
    """X (and, fused, M) ops of 1, 1,023, 1,024, 1,025 and 5,000 columns, one entry each, on alternating strands: the entries end on
    candidates 1, 1,024, 2,048, ... so entry borders lie on tile borders.  Every other column is an X over equal bases."""
    rng = np.random.default_rng(3 + fuse)
    lengths, specs, base = [1, 1023, 1024, 1025, 5000, 1, 1], [], 0
    for i, l in enumerate(lengths):
        hit = lambda k, base=base, l=l: not (k in (0, l - 1) or (base + k) % 1024 in (0, 1023))   # noqa: E731
        specs.append(([(l, "X")], i % 2, fuse, hit))
        base += l
    for shift in (0, 7):
        got = check_specs(sw, rng, specs, "tiles", shift=shift, model_checks=False)
        assert got.columns == sum(lengths) and got.usable == len(lengths) and got.n_variants == got.pool_bytes // 2
        assert int(got.pairs["m_equal" if fuse else "same"][0]) == got.columns - got.n_variants and 20 <= got.n_variants <= 30
        per_record = np.bincount(got.variants["record"], minlength=len(lengths)).tolist()
        assert per_record[0] == per_record[-1] == 1 and per_record[1] == 2 and per_record[4] >= 10


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_ops_and_variants_around_4096(sw, n):
    rng = np.random.default_rng(n)
    specs = [([(2, "=")], 0, False, 0.0), ([(1, "X")] * n, 1, False, 0.0), ([(3, "=")], 0, False, 0.0), ([(1, "X"), (1, "I")] * (n // 2) + [(1, "D")], 0, False, 0.0)]
    got = check_specs(sw, rng, specs, "n = %d" % n, model_checks=False)
    assert np.bincount(got.variants["record"]).tolist() == [0, n, 0, 2 * (n // 2) + 1] and got.ops == 2 + n + 2 * (n // 2) + 1
    assert (np.diff(got.variants["allele_offset"].astype(np.int64)) == (got.variants["ref_len"] + got.variants["alt_len"])[:-1]).all()


def test_entries_of_one_op_and_empty_and_unusable_entries_between(sw):
    rng = np.random.default_rng(5)
    ops = [(1, "="), (2, "X"), (3, "X"), (4, "I"), (5, "D"), (1, "X")]
    specs = [([ops[k % 6]], k % 2, k % 6 == 2, 0.3) for k in range(3_000)]
    for shift in (0, 9):
        got = check_specs(sw, rng, specs, "3000 entries", shift=shift, lower=0.3)
        assert got.usable == 3_000 and int(got.pairs["n_ins"][0]) == int(got.pairs["n_del"][0]) == 500
    cols, strand, cig, seqs = build_case(rng, [([(2, "X"), (1, "I"), (2, "=")], k % 2, False, 0.0) for k in range(9)])
    for i in (0, 3, 4, 8):
        cig[i] = ""                                    # empty entries
    cig[6] = cig[6] + "1="                             # the target sum is wrong
    status = np.array([1, 1, 0, 1, 1, 1, 1, 1, 1], dtype=np.uint8)
    got = check(sw, cols, strand, [0, 1], 2, cig, seqs, status=status, set_=1, what="between")
    assert sorted(set(got.variants["record"].tolist())) == [1, 5, 7] and got.usable == 3 and got.cigar_bad == 1 and got.n_variants == 9


def test_lower_case_iupac_and_n_on_either_side(sw):
    rng = np.random.default_rng(6)
    specs = [(vm.random_edits(rng, 30), k % 2, k % 3 == 0, 0.2) for k in range(200)]
    got = check_specs(sw, rng, specs, "iupac", lower=0.4, iupac=0.1, shift=3)
    p = got.pairs[0]
    assert int(p["n_columns"]) > 50 and int(p["same"]) > 50 and int(p["m_equal"]) > 50 and int(p["snvs"]) > 200 and all(int(p[s]) > 0 for s in vm.SUBS)
    assert set(got.pool.tobytes()) == set(b"ACGTN")


# ---- indels ----------------------------------------------------------------------------------------------------------------------------
def first_base_case():
    """Indels at a contig's first base, a deletion of a whole target and a target of one base, on both strands."""
    seqs = [b"acGTTGCAAT", b"ACGTA", b"G", b"TTACG"]       # the query, three targets
    recs = [("2I3=", 0, 0, 5, 1, 0, 3), ("2I3=", 1, 5, 10, 1, 0, 3), ("2D3=", 0, 2, 5, 1, 0, 5), ("2D1=", 1, 0, 1, 3, 0, 3), ("5D", 0, 4, 4, 1, 0, 5),
            ("1D", 1, 4, 4, 2, 0, 1), ("1X", 0, 0, 1, 2, 0, 1), ("1X", 1, 3, 4, 2, 0, 1), ("1I1D", 0, 7, 8, 2, 0, 1), ("1I4D", 1, 7, 8, 3, 0, 4),
            ("1D1X", 0, 1, 2, 3, 0, 2), ("2I1X", 1, 2, 5, 3, 0, 1), ("4D1I", 0, 3, 4, 3, 0, 4), ("1X1I", 0, 3, 5, 2, 0, 1)]
    cols = {k: np.array([r[j] for r in recs], dtype=np.uint32) for k, j in (("q_start", 2), ("q_end", 3), ("t_id", 4), ("t_start", 5), ("t_end", 6))}
    cols["q_id"] = np.zeros(len(recs), dtype=np.uint32)
    return cols, np.array([r[1] for r in recs], dtype=np.uint8), {i: r[0] for i, r in enumerate(recs)}, seqs


def test_indels_at_the_first_base_unanchored_and_a_target_of_one_base(sw):
    cols, strand, cig, seqs = first_base_case()
    for max_indel in (0, 1, 2, 4):
        got = check(sw, cols, strand, [0, 1, 1, 2], 3, cig, seqs, max_indel=max_indel, what="first base, max_indel %d" % max_indel, shift=1,
                    model_checks=False)      # (the = ops of these hand-made records lie over unequal bases)
        assert got.usable == len(cig) and int(got.pairs["unanchored"].sum()) == 3
    assert got.alleles(0) == (b"A", b"ACA") and tuple(int(v) for v in got.variants[0])[:6] == (0, INS, 0, 1, 3, 0)
    long = check(sw, cols, strand, [0, 1, 1, 2], 3, cig, seqs, max_indel=1, what="max_indel 1", model_checks=False)
    assert int(long.pairs["long_indels"].sum()) == 7 and long.n_variants < got.n_variants


def test_max_indel_around_each_length(sw):
    rng = np.random.default_rng(8)
    specs = [([(3, "="), (5, "I"), (2, "="), (7, "D"), (1, "X")], k % 2, False, 0.0) for k in range(6)]
    cols, strand, cig, seqs = build_case(rng, specs)
    base = check(sw, cols, strand, [0, 1], 2, cig, seqs, what="no limit")
    for max_indel, n_long in ((4, 2), (5, 1), (6, 1), (7, 0), (2**32 - 1, 0)):
        got = check(sw, cols, strand, [0, 1], 2, cig, seqs, max_indel=max_indel, what="max_indel %d" % max_indel)
        assert int(got.pairs["long_indels"][0]) == 6 * n_long and got.n_variants == base.n_variants - 6 * n_long
        assert all(int(got.pairs[k][0]) == int(base.pairs[k][0]) for k in vm.SUMS if k != "long_indels")


def test_an_insertion_of_70000_bases_and_a_deletion_as_long(sw):
    rng = np.random.default_rng(9)
    specs = [([(3, "="), (70_000, "I"), (2, "=")], 0, False, 0.0), ([(1, "X"), (70_000, "D"), (1, "X")], 1, False, 0.0), ([(2, "X"), (70_000, "I")], 1, False, 0.0)]
    got = check_specs(sw, rng, specs, "70000", shift=5, model_checks=False)
    assert got.n_variants == 7 and got.pool_bytes == 3 * 70_002 + 4 * 2 and sorted(got.variants["alt_len"].tolist())[-2:] == [70_001, 70_001]
    cut = check_specs(sw, np.random.default_rng(9), specs, "70000, cut", max_indel=69_999, model_checks=False)
    assert cut.n_variants == 4 and cut.pool_bytes == 8 and int(cut.pairs["long_indels"][0]) == 3


# ---- the summary -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G_, hashed", [(1, False), (2, False), (60, False), (300, False), (60, True)])
def test_genome_pairs_dense_hashed_and_beyond_the_lds_table(sw, monkeypatch, G_, hashed):
    """2,000 entries of one or two ops whose genome pair changes from entry to entry: with 60 and 300 genomes a tile of 1,024 candidate
    columns meets more pairs than the 256 slots of the work-group's LDS table (dense global table below 4,096 slots, hashed beyond
    or by the knob)."""
    if hashed:
        monkeypatch.setenv("SWG_VARIANTS_HASH", "1")
    rng = np.random.default_rng(G_)
    n = 2_000
    ops = [[(1, "X")], [(2, "I"), (1, "X")], [(1, "="), (1, "X")], [(3, "D")], [(2, "X")], [(1, "X"), (1, "=")]]
    cols, strand, cig, seqs = build_case(rng, [(ops[k % 6], k % 2, k % 6 == 4, 0.2) for k in range(n)])
    n_seq = max(G_, 2) + 3
    q_id, t_id = rng.integers(0, n_seq, n).astype(np.uint32), rng.integers(0, n_seq, n).astype(np.uint32)
    Q, T = seqs
    seqs = [Q if s % 2 == 0 else T for s in range(n_seq)]       # a record's sequences must hold its sides: queries on even ids
    cols["q_id"], cols["t_id"] = q_id - q_id % 2, t_id | 1
    cols["t_id"][cols["t_id"] >= n_seq] = 1
    genome = np.arange(n_seq) % G_
    got = check(sw, cols, strand, genome, G_, cig, seqs, what="G = %d" % G_)
    assert got.n_pairs == len(set(zip((genome[cols["q_id"]]).tolist(), (genome[cols["t_id"]]).tolist()))) and got.n_pairs >= min(G_ * G_ // 4, 500)
    assert int(got.pairs["entries"].sum()) == n


# ---- the filters -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(7)
    cols, strand, genome, cig, seqs = vm.random_case(rng, 600, n_targets=3, n_queries=3, genomes=3)
    seqs[1] = b""                                          # an absent target
    cols["t_end"][cols["t_id"] == 2] += (rng.random(int((cols["t_id"] == 2).sum())) < 0.01).astype(np.uint32)      # a target sum off by one: bad
    last = int(np.flatnonzero(cols["t_id"] == 0)[-1])
    seqs[0] = seqs[0][:int(cols["t_end"][last]) - 1]       # t_end one past the sequence
    return cols, strand, genome, cig, seqs, (rng.random(600) < 0.6).astype(np.uint8)


def test_each_genome_filter_both_sets_and_a_status_that_keeps_nothing(sw, small):
    cols, strand, genome, cig, seqs, status = small
    base = check(sw, cols, strand, genome, 3, cig, seqs, what="any")
    assert base.n_pairs == 6 and base.no_sequence > 100 and base.out_of_sequence == 1 and base.usable + base.no_sequence + base.out_of_sequence + base.cigar_bad == 600
    total = 0
    for g in range(3):
        by_ref = check(sw, cols, strand, genome, 3, cig, seqs, ref=g, what="ref %d" % g, model_checks=False)
        by_query = check(sw, cols, strand, genome, 3, cig, seqs, query=g, what="query %d" % g, model_checks=False)
        assert set(by_ref.pairs["t_genome"].tolist()) <= {g} and set(by_query.pairs["q_genome"].tolist()) == {g}
        total += by_ref.n_variants
        both = check(sw, cols, strand, genome, 3, cig, seqs, ref=g, query=(g + 1) % 3, what="both", model_checks=False)
        assert both.n_pairs <= 1
    assert total == base.n_variants
    kept = check(sw, cols, strand, genome, 3, cig, seqs, status=status, set_=1, what="kept")
    assert 0 < kept.n_variants < base.n_variants and 0 < kept.usable < base.usable
    check(sw, cols, strand, genome, 3, cig, seqs, status=status, set_=0, what="all, with a status")
    none = check(sw, cols, strand, genome, 3, cig, seqs, status=np.zeros(600, dtype=np.uint8), set_=1, what="never in status")
    assert (none.n_variants, none.pool_bytes, none.n_pairs, none.usable, none.no_sequence, none.columns, none.ops) == (0, 0, 0, 0, 0, 0, base.ops)


# ---- the protocol --------------------------------------------------------------------------------------------------------------------------
def raw_call(sw, fn, cols, strand, genome, G_, cig, seqs, caps, set_=0, status=None, ctx=None, null=(), ref=vm.ANY, query=vm.ANY, reserved=0, seq_set=True):
    """The host seam with caller arrays full of 0xAB -> (rc, request, variants, pool, pairs bytes)"""
    from sweepga_amd import _lib
    from sweepga_amd.lift import cigar_set
    from sweepga_amd.variants import sequence_set
    ctx = ctx or sw.default_context()
    rec = _lib.SwgRecords()
    rec.n = len(strand)
    keep = {k: np.ascontiguousarray(cols[k], dtype=np.uint32) for k in COLS}
    for k, a in keep.items():
        setattr(rec, k, a.ctypes.data)
    rec.strand, rec.n_seq = strand.ctypes.data, len(genome) if genome is not None else 6
    record, offset, text = cig if isinstance(cig, tuple) else cigar_set(sorted(cig), [cig[i] for i in sorted(cig)])
    cs = _lib.SwgCigarSet()
    cs.record, cs.offset, cs.text, cs.k = record.ctypes.data, offset.ctypes.data, text.ctypes.data, len(record)
    s_off, s_bases = seqs if isinstance(seqs, tuple) else sequence_set(seqs)
    ss = _lib.SwgSeqSet()
    ss.offset, ss.bases, ss.n_seq = s_off.ctypes.data if s_off is not None else None, s_bases.ctypes.data if s_bases is not None else None, rec.n_seq
    arrays = [np.full(size * max(c, 1), 0xab, dtype=np.uint8) for size, c in zip((32, 1, 200), caps)]
    req = _lib.SwgVariantRequest()
    req.set, req.t_genome, req.q_genome, req.reserved, req.n_variants = set_, ref, query, reserved, 99
    req.variant_capacity, req.pool_capacity, req.pair_capacity = caps
    req.variants, req.pool, req.pairs = (None if k in null else a.ctypes.data for k, a in enumerate(arrays))
    rc = fn(ctx.handle, C.byref(rec), genome.ctypes.data if genome is not None else None, G_, status.ctypes.data if status is not None else None,
            C.byref(cs), C.byref(ss) if seq_set else None, C.byref(req))
    return (rc, req) + tuple(a.tobytes() for a in arrays)


def test_capacities_with_poisoned_arrays(sw, small):
    cols, strand, genome, cig, seqs, _ = small
    lib = sw.default_context().lib
    want = vm.variant_records(cols, strand, genome, 3, cig, seqs, check=False)
    counts = (want["n_variants"], want["pool_bytes"], want["n_pairs"])
    full = (vm.variants_array(want["variants"]).tobytes(), want["pool"], vm.pairs_array(want["pairs"]).tobytes())
    assert counts[0] > 300 and counts[1] > 2 * counts[0] and counts[2] == 6
    for which in range(3):
        for cap in (0, counts[which] - 1, counts[which]):
            caps = tuple(cap if k == which else counts[k] for k in range(3))
            rc, req, *arrays = raw_call(sw, lib.swg_variant_records, cols, strand, genome, 3, cig, seqs, caps)
            assert rc == 0 and (req.n_variants, req.pool_bytes, req.n_pairs, req.usable) == counts + (want["usable"],)
            fits = [caps[k] >= counts[k] for k in range(3)]
            fits[0] = fits[1] = fits[0] and fits[1]      # a variant array that fits with a pool that does not leaves both untouched
            for k in range(3):
                if fits[k]:
                    assert arrays[k] == full[k], (which, cap, k)
                else:
                    assert set(arrays[k]) == {0xab}, (which, cap, k)
    for null in ((0,), (1,), (0, 1, 2)):
        rc, req, *arrays = raw_call(sw, lib.swg_variant_records, cols, strand, genome, 3, cig, seqs, counts, null=null)
        assert rc == 0 and req.n_variants == counts[0] and req.pool_bytes == counts[1] and set(arrays[0]) == set(arrays[1]) == {0xab}
        assert (arrays[2] == full[2]) == (2 not in null)


def test_no_entries_a_partial_set_and_records_permuted(sw, small):
    from sweepga_amd.variants import variant_records
    cols, strand, genome, cig, seqs, status = small
    ctx = sw.default_context()
    got = variant_records(ctx, cols, strand, 6, genome, 3, [], [], seqs)
    assert all(getattr(got, f) == 0 for f in FIELDS) and len(got.variants) == len(got.pool) == len(got.pairs) == 0
    got = variant_records(ctx, cols, strand, 6, genome, 3, [], [], None)      # k = 0 asks for no sequences
    assert got.n_variants == 0
    part = check(sw, cols, strand, genome, 3, {i: cig[i] for i in range(0, 600, 3)}, seqs, status=status, set_=1, what="a partial set")
    assert 0 < part.usable < 200
    perm = np.random.default_rng(3).permutation(600)
    pcols = {k: v[perm] for k, v in cols.items()}
    every = check(sw, cols, strand, genome, 3, cig, seqs, what="in order", model_checks=False)
    moved = check(sw, pcols, strand[perm], genome, 3, {j: cig[i] for j, i in enumerate(perm)}, seqs, what="permuted", model_checks=False)
    assert moved.pairs.tobytes() == every.pairs.tobytes() and moved.n_variants == every.n_variants and moved.pool_bytes == every.pool_bytes

    def keyed(r):
        return sorted((int(perm[v["record"]]) if r is moved else int(v["record"]), int(v["kind_flags"]), int(v["pos"]), int(v["q_pos"])) + r.alleles(k)
                      for k, v in enumerate(r.variants))
    assert keyed(moved) == keyed(every)


def test_refusals(sw, small):
    from sweepga_amd.lift import cigar_set
    from sweepga_amd.variants import sequence_set, variant_records, variant_records_device
    cols, strand, genome, cig, seqs, status = small
    ctx = sw.default_context()
    lib = ctx.lib
    good = cigar_set([3, 5, 9], ["1=", "2=", ""])
    s_off, s_bases = sequence_set(seqs)
    down = s_off.copy()
    down[3] = down[2] - 1
    for kw, word in (({"set": 2}, "set"), ({"set": 1}, "status"), ({"ref": 3}, "genome filter"), ({"query": 2**32 - 2}, "genome filter")):
        with pytest.raises(sw.SwgError) as e:
            variant_records(ctx, cols, strand, 6, genome, 3, None, good, seqs, **kw)
        assert e.value.code == -1 and word in str(e.value)
    for bad_seqs, word in ((None, "NULL sequences"), ((down, s_bases), "descend"), ((s_off[:-1], s_bases), "n_seq")):
        with pytest.raises(sw.SwgError) as e:
            variant_records(ctx, cols, strand, 6, genome, 3, None, good, bad_seqs)
        assert e.value.code == -1 and word in str(e.value), word
    rc, req, variants, pool, prs = raw_call(sw, lib.swg_variant_records, cols, strand, genome, 3, good, seqs, (4, 40, 4), reserved=1)
    assert rc == -1 and set(variants) == set(pool) == set(prs) == {0xab} and req.n_variants == 99 and b"reserved" in lib.swg_last_error(ctx.handle)
    rc, *_ = raw_call(sw, lib.swg_variant_records, cols, strand, None, 3, good, seqs, (4, 40, 4))
    assert rc == -1 and b"seq_genome" in lib.swg_last_error(ctx.handle)
    rc, *_ = raw_call(sw, lib.swg_variant_records, cols, strand, genome, 3, good, (None, s_bases), (4, 40, 4))
    assert rc == -1 and b"NULL sequences" in lib.swg_last_error(ctx.handle)
    twos = np.full(6, 2, dtype=np.uint32)
    rc, *_ = raw_call(sw, lib.swg_variant_records, cols, strand, twos, 2, good, seqs, (4, 40, 4))
    assert rc == -1 and b"genome" in lib.swg_last_error(ctx.handle)
    bad_set = (np.array([5, 3, 9], dtype=np.uint32), good[1], good[2])
    rc, *_ = raw_call(sw, lib.swg_variant_records, cols, strand, genome, 3, bad_set, seqs, (4, 40, 4))
    assert rc == -1
    hip = Hip()
    try:
        dcols = {k: Dev(hip, cols[k], np.uint32) for k in COLS}
        args = (dcols, Dev(hip, strand, np.uint8), 6, Dev(hip, genome, np.uint32), 3, *(Dev(hip, a) for a in good), 3)
        with pytest.raises(sw.SwgError) as e:      # descending offsets in device memory: refused before a base is read
            variant_records_device(ctx, *args, Dev(hip, down), Dev(hip, s_bases))
        assert e.value.code == -1 and "descend" in str(e.value)
        with pytest.raises(sw.SwgError) as e:
            variant_records_device(ctx, *args, None, None)
        assert e.value.code == -1 and "NULL sequences" in str(e.value)
        with pytest.raises(sw.SwgError) as e:
            variant_records_device(ctx, *args, Dev(hip, s_off), Dev(hip, s_bases), ref=7)
        assert e.value.code == -1
        ok = variant_records_device(ctx, *args, Dev(hip, s_off), Dev(hip, s_bases))
        assert ok.ops == 2
    finally:
        hip.free()
    after = check(sw, cols, strand, genome, 3, {3: cig[3]}, seqs, what="after the refusals")      # the context is as usable as before
    assert after.usable + after.no_sequence == 1


def test_a_memory_limit_that_does_not_hold_the_call_and_one_that_does(sw, small):
    from sweepga_amd.variants import variant_records
    cols, strand, genome, cig, seqs, _ = small
    ctx = sw.Context(0)
    try:
        n = 100_000      # 2 * 10^5 ops: 32 bytes of prefix sums and 17 of this report each
        T = vm.random_bases(np.random.default_rng(1), n)
        c1 = {"q_id": [0], "t_id": [1], "q_start": [0], "q_end": [2 * n], "t_start": [0], "t_end": [n]}
        c1 = {k: np.array(v, dtype=np.uint32) for k, v in c1.items()}
        Qs = bytes(np.repeat(np.frombuffer(T, dtype=np.uint8), 2))
        ctx.set_memory_limit(4 << 20)
        with pytest.raises(sw.SwgError) as e:
            variant_records(ctx, c1, np.zeros(1, dtype=np.uint8), 2, [0, 1], 2, [0], ["1M1I" * n], [Qs, T])
        assert e.value.code == -4
        got = variant_records(ctx, cols, strand, 6, genome, 3, sorted(cig), [cig[i] for i in sorted(cig)], seqs)      # the same context, a call that fits
        compare(got, vm.variant_records(cols, strand, genome, 3, cig, seqs, check=False), "under the limit")
        ctx.set_memory_limit(0)
        got = variant_records(ctx, c1, np.zeros(1, dtype=np.uint8), 2, [0, 1], 2, [0], ["1M1I" * n], [Qs, T])
        assert got.n_variants == n and got.pool_bytes == 3 * n and int(got.pairs["m_equal"][0]) == n and got.alleles(n - 1) == (T[-1:], T[-1:] * 2)
    finally:
        ctx.close()


def test_smallest_shapes_on_a_fresh_context(sw):
    """The seams around the kernels at the smallest shapes -- one record; three records -- with and without a status, on a context of
    its own: its first call sizes the arena from the input, the later ones find it sized."""
    rng = np.random.default_rng(2)
    cols, strand, cig, seqs = build_case(rng, [([(2, "="), (1, "X"), (2, "I"), (3, "="), (1, "D"), (1, "X")], k, k == 2, 0.0) for k in (0, 1, 0)])
    ctx = sw.Context(0)
    try:
        for n in (1, 3, 1, 3):
            part = {k: v[:n] for k, v in cols.items()}
            for status in (None, np.array([1, 0, 1], dtype=np.uint8)[:n]):
                got = check(sw, part, strand[:n], [0, 1], 2, {i: cig[i] for i in range(n)}, seqs, status=status, set_=0 if status is None else 1, what=f"n = {n}",
                            ctx=ctx)
                assert got.usable == (n if status is None else (n + 1) // 2) and got.variants["record"].tolist()[:4] == [0, 0, 0, 0]
    finally:
        ctx.close()


# ---- the whole path ------------------------------------------------------------------------------------------------------------------------
def test_20000_generated_records_under_a_real_one_to_one_status(sw):
    rng = np.random.default_rng(11)
    n = 20_000
    cols, strand, genome, cig, seqs = vm.random_case(rng, n, n_targets=6, n_queries=6, n_ops=8, max_len=4, genomes=4)
    lines = []
    for i in range(n):
        lines.append("\t".join(["s%d" % cols["q_id"][i], "400000", str(cols["q_start"][i]), str(cols["q_end"][i]), "-" if strand[i] else "+",
                                "s%d" % cols["t_id"][i], "400000", str(cols["t_start"][i]), str(cols["t_end"][i]), "50", "60", "60"]))
    with sw.PafFile(text="\n".join(lines) + "\n") as paf:
        status, _ = run_filter(sw, paf, filter_cfgs(sw)["one_to_one"])
    assert 0 < int((status != 0).sum()) < n
    roll = rng.random(n)
    part = {i: (cig[i] + "1=" if roll[i] < 0.05 else cig[i]) for i in range(n) if roll[i] >= 0.10 or roll[i] < 0.05}
    usable = []
    for set_ in (0, 1):
        got = check(sw, cols, strand, genome, 4, part, seqs, status=status, set_=set_, what="random, set %d" % set_, model_checks=set_ == 1, shift=set_)
        assert got.cigar_bad > 0.03 * len(part) and got.n_pairs == 16 and got.n_variants > got.usable > 0
        usable.append(got.usable)
    assert usable[0] > 15_000 and 0 < usable[1] < usable[0]


# ---- the PAF seam, the Python class and the command line ---------------------------------------------------------------------------------
def vcf_paf():
    """The mixed PAF of tests/test_ucsc_chain_cpu.py (=/X and M CIGARs on both strands, a line without a tag, one with two, an empty and
    a broken tag, a record beyond its sequence) with three more records: a copy of the first one -- two records with a variant at the
    same pos -- and two whose target is the sequence that appeared first, so that the targets' ids DESCEND along the file.  The FASTA
    lacks g3#1#s, holds g2#1#t twice (the first counts) and a sequence nobody names.  -> (text, kept, fasta records)"""
    from tests.test_ucsc_chain_cpu import G, QS, TS, mixed_paf, tagged
    text, kept = mixed_paf()
    q, t = "g1#1#q", "g2#1#t"
    more = [tagged([q, QS, 100, 120, "+", t, TS, 1000, 1022, 13, 22, 60], "cg:Z:" + G), tagged([t, TS, 50, 60, "-", q, QS, 30, 40, 9, 10, 60], "cg:Z:4=1X5="),
            tagged([t, TS, 0, 12, "+", q, QS, 0, 9, 9, 12, 60], "cg:Z:3I2M3D4M")]
    rng = np.random.default_rng(21)
    fasta = [(q, vm.plant(rng, vm.random_bases(rng, QS), 0.3, 0.02)), (t, vm.plant(rng, vm.random_bases(rng, TS), 0.3, 0.02)), (t, b"A" * TS),
             ("nobody", b"ACGT")]
    return text + "\n".join(more) + "\n", np.concatenate([kept, [True, True, True]]), fasta


def write_fasta(path, records, width=61):
    with open(path, "wb") as f:
        for name, seq in records:
            f.write(b">" + name.encode() + b" a description\n")
            for at in range(0, len(seq), width):
                f.write(seq[at:at + width] + b"\n")


def test_write_the_python_class_and_the_command_line_for_every_batch_size(sw, tmp_path):
    from sweepga_amd import build
    from tests.test_gpu_intervals import kept_mask
    text, kept, fasta = vcf_paf()
    st = kept.astype(np.uint8)
    fa, fa2 = tmp_path / "a.fa", tmp_path / "b.fa"
    write_fasta(fa, fasta[:1])
    write_fasta(fa2, fasta[1:], width=80)
    files = [str(fa), str(fa2)]
    out, summ = tmp_path / "v.vcf", tmp_path / "s.tsv"
    one_record = len("5=2I6=4D5X2=")
    with sw.PafFile(text=text) as paf:
        for set_, status in ((0, None), (1, st), (0, st)):
            n_records = 17 if set_ == 0 else int(kept.sum())
            for kw in (dict(), dict(max_indel=2), dict(ref="g2#1"), dict(query="g1#1#", max_indel=0), dict(ref="g1#1", query="g2#1")):
                want = vm.paf_texts(text, kept, fasta, set_, kw.get("ref"), kw.get("query"), kw.get("max_indel", 10000))
                assert want[2]["variants"] >= 1 and ("ref" in kw or "query" in kw or want[2]["no_sequence"] == 1 + (set_ == 0))
                for batch in (1, one_record, 40, 0):
                    got = sw.Variants.from_paf(paf, status, fasta=files, set=set_, batch_bytes=batch, **kw)
                    assert (got.text, got.summary_text) == want[:2], (set_, kw, batch)
                    assert {k: v for k, v in got.counts.items() if k != "batches"} == want[2]
                    assert sw.Variants.write_paf(paf, status, out, summ, fasta=files, set=set_, batch_bytes=batch, **kw) == got.counts
                    assert out.read_text() == want[0] and summ.read_text() == want[1]
                    assert 1 <= got.counts["batches"] <= n_records and (batch != 1 or got.counts["batches"] == n_records) and (batch or got.counts["batches"] == 1)
                assert len(got.variants) == want[2]["variants"] and len(got.pool) >= 2 * len(got.variants)
        every = sw.Variants.from_paf(paf, st, fasta=files)
        chroms = [v[0] for v in every.variants]
        assert chroms == sorted(chroms) and set(chroms) == {"g1#1#q", "g2#1#t"} and "##contig=<ID=g1#1#q,length=700>\n##contig=<ID=g2#1#t,length=9000>\n" in every.text
        twice = [v for v in every.variants if v[4]["REC"] in ("0", "14")]
        assert len(twice) >= 6 and [v[:4] for v in twice[0::2]] == [v[:4] for v in twice[1::2]] and [v[4]["REC"] for v in twice[:2]] == ["0", "14"]
        summary_only = sw.Variants.write_paf(paf, st, None, summ, fasta=files)                    # the variants are counted and not built
        assert summary_only["variants"] == every.counts["variants"] and summ.read_text() == every.summary_text
        short = sw.Variants.from_paf(paf, st, fasta=[str(fa)])                                    # the second file is missing: its sequences are absent
        assert short.counts["usable"] == 0 and short.counts["no_sequence"] > 5 and short.text == vm.vcf_header([])
        write_fasta(fa2, [(fasta[1][0], fasta[1][1][:-1])])
        off = sw.Variants.from_paf(paf, st, fasta=files)
        assert off.counts["length_mismatch"] == 1 and off.counts == dict(short.counts, length_mismatch=1)
        write_fasta(fa2, fasta[1:], width=80)
    # the command line: a real 1:1 filter over generated records; the output PAF and the --diffs file do not change
    rng = np.random.default_rng(12)
    cols, strand, genome, cig, seqs = vm.random_case(rng, 2_000, n_targets=4, n_queries=4, n_ops=10, genomes=3)
    name = ["g%d#1#c%d" % (genome[s], s) for s in range(8)]
    lines = []
    for i in range(2_000):
        q, t = int(cols["q_id"][i]), int(cols["t_id"][i])
        f = [name[q], str(len(seqs[q])), str(cols["q_start"][i]), str(cols["q_end"][i]), "-" if strand[i] else "+",
             name[t], str(len(seqs[t])), str(cols["t_start"][i]), str(cols["t_end"][i]), "50", "60", "60"]
        tags = (["tp:A:P", "cg:Z:" + cig[i]], ["cg:Z:" + cig[i], "nm:i:3"], ["tp:A:P"], ["cg:Z:1M", "cg:Z:" + cig[i]], ["cg:Z:"], ["cg:Z:" + cig[i] + "9"])[i % 6]
        lines.append("\t".join(f + tags))
    big = "\n".join(lines) + "\n"
    records = list(zip(name, seqs))
    big_fa = tmp_path / "big.fa"
    write_fasta(big_fa, records)
    inp, plain, outp, d0, d1 = (tmp_path / nm for nm in ("in.paf", "plain.paf", "out.paf", "plain.diffs", "out.diffs"))
    inp.write_text(big, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-jump", "10k", "--scaffold-mass", "2k"]
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), "--diffs", str(d0), *flags, "--quiet"], capture_output=True)
    assert r0.returncode == 0 and plain.stat().st_size > 0 and d0.stat().st_size > 0, r0.stderr
    kept = kept_mask(big, plain.read_bytes().decode())
    with sw.PafFile(text=big) as paf:      # every batch size gives the same bytes
        for set_ in (1, 0):
            want = vm.paf_texts(big, kept, records, set_)
            got = [sw.Variants.from_paf(paf, kept.astype(np.uint8), fasta=[str(big_fa)], set=set_, batch_bytes=b) for b in (1, 100, 4096, 0)]
            assert all((g.text, g.summary_text) == want[:2] for g in got) and all({k: v for k, v in g.counts.items() if k != "batches"} == want[2] for g in got)
            batches = [g.counts["batches"] for g in got]
            assert batches[0] > batches[1] > batches[2] >= batches[3] == 1
    for extra, set_, kw in (([], 1, {}), (["--vcf-set", "all", "--vcf-ref", "g1#1", "--vcf-query", "g0#1#", "--vcf-max-indel", "3", "--vcf-batch", "2k"], 0,
                                       dict(ref="g1#1", query="g0#1#", max_indel=3))):
        want = vm.paf_texts(big, kept, records, set_, **kw)
        r = subprocess.run([build.CLI, str(inp), "--output-file", str(outp), "--diffs", str(d1), "--vcf", str(out), "--vcf-summary", str(summ),
                            "--vcf-fasta", str(big_fa), *extra, *flags], capture_output=True)
        assert r.returncode == 0 and r.stdout == b"" and outp.read_bytes() == plain.read_bytes() and d1.read_bytes() == d0.read_bytes(), r.stderr
        c = want[2]
        assert out.read_text() == want[0] and summ.read_text() == want[1] and c["records"] > 100 and c["variants"] > 100 and c["usable"] > (30 if kw else c["records"] // 3)      # (the genome filters leave one pair of three genomes)
        assert ("--vcf: %d variants (%d SNVs, %d insertions, %d deletions), %d same, %d N columns, %d equal under M ops, %d long, %d unanchored, "
                "%d entries without sequence, %d out of sequence, %d bad, %d without a cg:Z: tag\n"
                % (c["variants"], c["snvs"], c["n_ins"], c["n_del"], c["same"], c["n_columns"], c["m_equal"], c["long_indels"], c["unanchored"], c["no_sequence"],
                   c["out_of_sequence"], c["bad"], c["untagged"])) in r.stderr.decode()
    out.unlink()
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(outp), "--vcf-summary", str(summ), "--vcf-fasta", str(big_fa), "--no-filter", "--quiet"],
                       capture_output=True)
    assert r.returncode == 0 and summ.read_text() == vm.paf_texts(big, None, records, 0)[1] and not out.exists(), r.stderr
    outp.unlink(), d1.unlink()
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(outp), "--diffs", str(d1), "--vcf", str(out), "--vcf-fasta", str(big_fa), "--vcf-ref", "g7#1",
                        *flags, "--quiet"], capture_output=True)
    assert r.returncode == 2 and b"--vcf-ref: unknown genome 'g7#1'" in r.stderr      # a usage error, found before the filter: nothing is written
    assert not out.exists() and not outp.exists() and not d1.exists()
