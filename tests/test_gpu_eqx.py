"""The resolved CIGARs on the device (sweepga_amd/csrc/swg_eqx.hip) against tests/eqx_model.py: in every case the host seam against
the model and the device seam against the host seam -- entries, text and counts, byte for byte.  The shapes are the smallest at
which each part can go wrong: the column pass's tile of 4,096 columns with a mismatch on the first and last column of every tile and
of every op, eq alternating on every column, runs across tile borders, the compaction's tile of 4,096 flags, the text kernel's tile of
4,096 bytes with an item across every border, entries of one op, a target of one base, one op of 2 * 10^6 columns; the capacity
protocol; the variant calls and the difference list as cross-checks on the device; the PAF seam, the Python class and --eqx.  Every
comparison is exact: integers and bytes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import eqx_model as xm
from tests import lift_model as lm
from tests import variants_model as vm
from tests.test_gpu_alnstats import filter_cfgs, run_filter
from tests.test_gpu_lift import Dev
from tests.test_gpu_variants import build_case, vcf_paf, write_fasta
from tests.test_gpu_wide import Hip

pytestmark = pytest.mark.gpu
COLS = lm.COLS
FIELDS = xm.FIELDS
CT = TT = 4096      # the column pass's tile and the text kernel's


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


def same(a, b):
    return a.entries.tobytes() == b.entries.tobytes() and a.text.tobytes() == b.text.tobytes() and all(getattr(a, f) == getattr(b, f) for f in FIELDS)


def both_seams(sw, cols, strand, n_seq, cig, seqs, status=None, set_=0, ctx=None, shift=0):
    """The result of the host seam, after checking that the device seam gives the same.  shift: the device text and the device bases
    start that many bytes behind a 16-byte boundary."""
    from sweepga_amd.eqx import eqx_records, eqx_records_device
    from sweepga_amd.lift import cigar_set
    from sweepga_amd.variants import sequence_set
    ctx = ctx or sw.default_context()
    recs = sorted(cig)
    s_off, s_bases = sequence_set(seqs)
    got = eqx_records(ctx, cols, strand, n_seq, recs, [cig[i] for i in recs], (s_off, s_bases), status=status, set=set_)
    record, offset, text = cigar_set(recs, [cig[i] for i in recs])
    hip = Hip()
    try:
        dcols = {k: Dev(hip, cols[k], np.uint32) for k in COLS}
        dtext = Dev(hip, np.concatenate([np.zeros(shift, dtype=np.uint8), text]))
        dbases = Dev(hip, np.concatenate([np.zeros(shift, dtype=np.uint8), s_bases]))
        dtext.ptr += shift
        dbases.ptr += shift
        dev = eqx_records_device(ctx, dcols, Dev(hip, strand, np.uint8), n_seq, Dev(hip, record), Dev(hip, offset), dtext, len(recs), Dev(hip, s_off), dbases,
                                 status=Dev(hip, status, np.uint8) if status is not None else None, set=set_)
    finally:
        hip.free()
    assert same(dev, got)
    return got


def compare(got, want, what=""):
    assert {f: getattr(got, f) for f in FIELDS} == {f: want[f] for f in FIELDS}, what
    rows = xm.entries_array(want["entries"])
    if got.entries.tobytes() != rows.tobytes():
        bad = [k for k in range(len(rows)) if got.entries[k].tobytes() != rows[k].tobytes()]
        raise AssertionError((what, len(bad), [(k, tuple(int(v) for v in got.entries[k]), want["entries"][k]) for k in bad[:5]]))
    text = got.text.tobytes().decode("latin-1")
    if text != want["text"]:
        k = next((k for k in range(min(len(text), len(want["text"]))) if text[k] != want["text"][k]), min(len(text), len(want["text"])))
        raise AssertionError((what, "text byte", k, text[max(k - 20, 0):k + 20], want["text"][max(k - 20, 0):k + 20]))


def check(sw, cols, strand, n_seq, cig, seqs, status=None, set_=0, what="", ctx=None, shift=0):
    """Both seams against the model."""
    cols = {k: np.asarray(cols[k]).astype(np.uint32) for k in COLS}
    strand = np.asarray(strand).astype(np.uint8)
    got = both_seams(sw, cols, strand, n_seq, cig, seqs, status, set_, ctx, shift)
    compare(got, xm.eqx_records(cols, strand, cig, seqs, None if status is None else np.asarray(status) != 0, set_), what)
    return got


def check_specs(sw, rng, specs, what="", lower=0.0, iupac=0.0, **kw):
    cols, strand, cig, seqs = build_case(rng, specs, lower=lower, iupac=iupac)
    return check(sw, cols, strand, 2, cig, seqs, what=what, **kw), cig


def edits_with_mismatches(l, at):
    """l columns as = and X ops with a mismatch on every column of `at`"""
    out = []
    for k in range(l):
        ch = "X" if k in at else "="
        if out and out[-1][1] == ch:
            out[-1] = (out[-1][0] + 1, ch)
        else:
            out.append((1, ch))
    return out


# ---- the column pass -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["M", "=X", "X"])
def test_mismatches_on_the_first_and_last_column_of_every_tile_and_op(sw, form):
    """Ops of 1, T - 1, T, T + 1 and 5,000 columns, one entry each, on alternating strands: the entries end on columns 1, T, 2 T, ...
    so entry borders lie on tile borders.  As one M op, as the = and X ops that say the same, and as one X op over mostly equal
    bases."""
    rng = np.random.default_rng(3)
    lengths, specs, base = [1, CT - 1, CT, CT + 1, 5000, 1, 1], [], 0
    want_text, n_mis = [], 0
    for i, l in enumerate(lengths):
        at = {k for k in range(l) if k in (0, l - 1) or (base + k) % CT in (0, CT - 1)}
        n_mis += len(at)
        if form == "X":
            specs.append(([(l, "X")], i % 2, False, lambda k, at=at: k not in at))
        else:
            specs.append((edits_with_mismatches(l, at), i % 2, form == "M", 0.0))
        want_text.append("".join("%d%s" % op for op in edits_with_mismatches(l, at)))
        base += l
    for shift in (0, 7):
        got, cig = check_specs(sw, rng, specs, "tiles, " + form, shift=shift)
        assert got.columns == sum(lengths) and got.usable == len(lengths) and [got.cigar(j).decode() for j in range(len(lengths))] == want_text
        assert got.changed == (0 if form == "=X" else len(lengths) - (3 if form == "X" else 0)) and got.mismatches == n_mis >= 12
        assert (got.m_columns, got.x_wrong) == {"M": (got.columns, 0), "=X": (0, 0), "X": (0, got.matches)}[form] and got.eq_wrong == 0


def test_eq_alternating_on_every_column_across_two_tiles(sw):
    """The densest output: two bytes per column."""
    rng = np.random.default_rng(4)
    n = 2 * CT + 10
    got, _ = check_specs(sw, rng, [([(1, "="), (1, "X")] * (n // 2), 0, True, 0.0), ([(1, "X"), (1, "=")] * (n // 2), 1, True, 0.0)], "alternating", shift=7)
    assert got.cigar(0) == b"1=1X" * (n // 2) and got.cigar(1) == b"1X1=" * (n // 2) and got.text_bytes == 4 * n and got.out_ops == 2 * n


def test_runs_across_tile_borders_give_one_op(sw):
    """A constant stretch across a tile border, and a run of three ops whose borders fall on tile borders (X ops over equal bases:
    the three merge)."""
    rng = np.random.default_rng(5)
    specs = [([(CT, "="), (CT, "X"), (CT, "=")], 0, False, 1.0), ([(3000, "=")], 1, True, 0.0), ([(5000, "=")], 0, True, 0.0), ([(2 * CT, "X")], 1, False, 0.0),
             ([(CT - 904, "="), (CT, "X"), (1, "I"), (CT, "=")], 0, False, 0.0)]
    got, _ = check_specs(sw, rng, specs, "runs")
    assert [got.cigar(j) for j in range(5)] == [b"%d=" % (3 * CT), b"3000=", b"5000=", b"%dX" % (2 * CT), b"%d=%dX1I%d=" % (CT - 904, CT, CT)]
    assert got.x_wrong == CT and got.changed == 3 and int(got.entries["out_ops"][4]) == 4


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_items_and_boundaries_around_4096(sw, n):
    rng = np.random.default_rng(n)
    specs = [([(2, "=")], 0, False, 0.0), ([(1, "X"), (1, "=")] * (n // 2) + [(1, "X")] * (n % 2), 1, n % 2 == 0, 0.0), ([(3, "=")], 0, False, 0.0),
             ([(1, "I"), (1, "D")] * (n // 2) + [(1, "=")], 0, False, 0.0)]
    got, _ = check_specs(sw, rng, specs, "n = %d" % n)
    assert got.entries["out_ops"].tolist() == [1, n, 1, 2 * (n // 2) + 1] and got.out_ops == n + 2 * (n // 2) + 3
    alone, _ = check_specs(sw, rng, specs[1:2], "boundaries alone, n = %d" % n)      # n boundaries and n items in all
    assert alone.out_ops == n and alone.text_bytes == 2 * n
    verbatim, _ = check_specs(sw, rng, [([(1, "I"), (1, "D")] * (n // 2) + [(1, "I")] * (n % 2), 1, False, 0.0)], "verbatim alone, n = %d" % n)
    assert verbatim.out_ops == n and verbatim.columns == 0 and verbatim.changed == 0


def test_an_item_across_every_border_of_the_text_tile(sw):
    """Clips with up to ten digits between short column ops: items of 2 to 11 bytes over five tiles of text; the output is searched for
    an item across each border, and for every way an item of 11 bytes can be cut."""
    rng = np.random.default_rng(6)
    T = vm.random_bases(rng, 3000)
    for shift, seed in ((0, 1), (7, 2)):
        r = np.random.default_rng(seed)
        parts, n_cols, size = [], 0, 0
        while size < 5 * TT + 100:
            if r.random() < 0.35 and n_cols < 2990 and parts and parts[-1] != "1M" and (size + 2) % TT:
                parts.append("1M")
                n_cols += 1
            else:
                width = int(r.integers(1, 11))
                width += -1 if (size + width + 1) % TT == 0 and width > 1 else (size + width + 1) % TT == 0      # no item ends on a border
                parts.append("%0*d%s" % (width, int(r.integers(0, 10)), "SHP"[int(r.integers(3))]))
            size += len(parts[-1])
        text = "".join(parts)
        cols = {"q_id": [0], "t_id": [1], "q_start": [5], "q_end": [5 + n_cols], "t_start": [2], "t_end": [2 + n_cols]}
        got = check(sw, cols, [0], 2, {0: text}, [b"ACGTA" + T[2:2 + n_cols] + b"A", T], what="text tiles", shift=shift)
        assert got.cigar(0).decode() == text.replace("M", "=") and got.text_bytes > 5 * TT
        at, cuts = 0, set()
        for d, ch in xm.raw_ops(text):
            for border in range(TT, got.text_bytes, TT):
                if at < border < at + len(d) + 1:
                    cuts.add(border)
            at += len(d) + 1
        assert cuts == set(range(TT, got.text_bytes, TT)) and len(cuts) == 5
    # an item of 11 bytes cut at each of its ten places by the first border
    for cut in range(1, 11):
        pad = TT - cut
        text = "0S" * ((pad - 3 * (pad % 2)) // 2) + "00S" * (pad % 2) + "1234567890H" + "3M"
        cols = {"q_id": [0], "t_id": [1], "q_start": [0], "q_end": [3], "t_start": [0], "t_end": [3]}
        got = check(sw, cols, [1], 2, {0: text}, [b"CGT", b"ACG"], what="cut %d" % cut)
        assert got.cigar(0).decode() == text[:-2] + "3=" and got.text_bytes == pad + 13


def test_entries_of_one_op_and_empty_and_unusable_entries_between(sw):
    rng = np.random.default_rng(7)
    ops = [(1, "="), (2, "X"), (3, "X"), (4, "I"), (5, "D"), (1, "X")]
    specs = [([ops[k % 6]], k % 2, k % 6 == 2, 0.3) for k in range(3_000)]
    for shift in (0, 9):
        got, _ = check_specs(sw, rng, specs, "3000 entries", shift=shift, lower=0.3)
        assert got.usable == 3_000 and int(got.entries["inserted"].sum()) == 4 * 500 and int(got.entries["deleted"].sum()) == 5 * 500 and got.x_wrong > 100
    cols, strand, cig, seqs = build_case(rng, [([(2, "X"), (1, "I"), (2, "=")], k % 2, k % 3 == 0, 0.0) for k in range(9)])
    for i in (0, 3, 4, 8):
        cig[i] = ""                                    # empty entries
    cig[6] = cig[6] + "1="                             # the target sum is wrong
    status = np.array([1, 1, 0, 1, 1, 1, 1, 1, 1], dtype=np.uint8)
    got = check(sw, cols, strand, 2, cig, seqs, status=status, set_=1, what="between")
    assert np.flatnonzero(got.entries["flags"]).tolist() == [1, 5, 7] and (got.usable, got.cigar_bad, got.empty) == (3, 1, 4) and got.text_bytes == 3 * 6


def test_lower_case_iupac_and_n_on_either_side(sw):
    rng = np.random.default_rng(8)
    specs = [(vm.random_edits(rng, 30), k % 2, k % 3 == 0, 0.2) for k in range(200)]
    got, _ = check_specs(sw, rng, specs, "iupac", lower=0.4, iupac=0.1, shift=3)
    assert got.n_columns > 50 and got.eq_wrong > 20 and got.x_wrong > 50 and got.m_columns > 500 and got.matches > got.mismatches > got.n_columns


def test_a_target_of_one_base_and_hand_made_records(sw):
    seqs = [b"acGTTGCAAT", b"ACGTA", b"G", b"TTACG"]       # the query, three targets
    recs = [("1M", 0, 2, 3, 2, 0, 1), ("1M", 1, 6, 7, 2, 0, 1), ("1X", 0, 0, 1, 2, 0, 1), ("1=", 1, 3, 4, 2, 0, 1), ("1I1D", 0, 7, 8, 2, 0, 1), ("1D", 1, 4, 4, 2, 0, 1),
            ("2I3M", 0, 0, 5, 1, 0, 3), ("0M2S3M0=0X2N", 1, 0, 3, 1, 0, 5), ("5M", 0, 5, 10, 3, 0, 5), ("001M2D02M", 1, 7, 10, 3, 0, 5)]
    cols = {k: np.array([r[j] for r in recs], dtype=np.uint32) for k, j in (("q_start", 2), ("q_end", 3), ("t_id", 4), ("t_start", 5), ("t_end", 6))}
    cols["q_id"] = np.zeros(len(recs), dtype=np.uint32)
    got = check(sw, cols, np.array([r[1] for r in recs], dtype=np.uint8), 4, {i: r[0] for i, r in enumerate(recs)}, seqs, what="one base", shift=1)
    assert got.usable == len(recs) and [got.cigar(j) for j in range(3)] == [b"1=", b"1=", b"1X"] and got.cigar(5) == b"1D"


def test_one_op_of_two_million_columns_beside_a_thousand_of_one(sw):
    """The long op's expectation comes from numpy (the model walks column by column); the short entries' from the model."""
    from sweepga_amd.eqx import eqx_records
    rng = np.random.default_rng(9)
    L = 2_000_000
    T = np.frombuffer(vm.random_bases(rng, L + 1000), dtype=np.uint8).copy()
    Q = T.copy()
    hit = np.flatnonzero(rng.random(L) < 0.01)
    Q[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), Q[hit]) + 1) % 4]
    n = 1000
    cols = {"q_id": np.zeros(n + 1), "t_id": np.ones(n + 1), "q_start": np.r_[np.arange(L, L + 500), 0, np.arange(L + 500, L + 1000)],
            "q_end": np.r_[np.arange(L, L + 500) + 1, L, np.arange(L + 500, L + 1000) + 1]}
    cols["t_start"], cols["t_end"] = cols["q_start"], cols["q_end"]
    cig = {i: "1M" for i in range(n + 1)}
    cig[500] = "%dM" % L
    ctx = sw.default_context()
    got = eqx_records(ctx, {k: v.astype(np.uint32) for k, v in cols.items()}, np.zeros(n + 1, dtype=np.uint8), 2, sorted(cig), [cig[i] for i in sorted(cig)],
                      [Q.tobytes(), T.tobytes()])
    eq = Q[:L] == T[:L]
    starts = np.r_[0, np.flatnonzero(eq[1:] != eq[:-1]) + 1]
    want = "".join("%d%s" % (b - a, "=" if eq[a] else "X") for a, b in zip(starts, np.r_[starts[1:], L]))
    assert got.cigar(500).decode() == want and got.text.tobytes().decode() == "1=" * 500 + want + "1=" * 500
    assert (got.columns, got.matches, got.mismatches, got.out_ops) == (L + n, int(eq.sum()) + n, L - int(eq.sum()), len(starts) + n)
    assert int(got.entries["text_first"][501]) == 1000 + len(want) and got.changed == n + 1 and got.m_columns == L + n


# ---- sets, protocol, refusals ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(7)
    cols, strand, genome, cig, seqs = vm.random_case(rng, 600, n_targets=3, n_queries=3, genomes=3)
    seqs[1] = b""                                          # an absent target
    cols["t_end"][cols["t_id"] == 2] += (rng.random(int((cols["t_id"] == 2).sum())) < 0.01).astype(np.uint32)      # a target sum off by one: bad
    last = int(np.flatnonzero(cols["t_id"] == 0)[-1])
    seqs[0] = seqs[0][:int(cols["t_end"][last]) - 1]       # t_end one past the sequence
    return cols, strand, genome, cig, seqs, (rng.random(600) < 0.6).astype(np.uint8)


def test_both_sets_and_a_status_that_keeps_nothing(sw, small):
    cols, strand, _, cig, seqs, status = small
    base = check(sw, cols, strand, 6, cig, seqs, what="all")
    assert base.no_sequence > 100 and base.out_of_sequence == 1 and base.cigar_bad >= 1 and base.usable + base.no_sequence + base.out_of_sequence + base.cigar_bad == 600
    kept = check(sw, cols, strand, 6, cig, seqs, status=status, set_=1, what="kept", shift=7)
    assert 0 < kept.usable < base.usable and 0 < kept.text_bytes < base.text_bytes and kept.cigar_bad == base.cigar_bad
    check(sw, cols, strand, 6, cig, seqs, status=status, set_=0, what="all, with a status")
    none = check(sw, cols, strand, 6, cig, seqs, status=np.zeros(600, dtype=np.uint8), set_=1, what="never in status")
    assert (none.usable, none.no_sequence, none.columns, none.out_ops, none.text_bytes, none.ops) == (0, 0, 0, 0, 0, base.ops)
    assert none.entries["record"].tolist() == list(range(600)) and not none.entries["flags"].any()


def raw_call(sw, fn, cols, strand, n_seq, cig, seqs, caps, set_=0, status=None, null=(), reserved=0, seq_set=True):
    """The host seam with caller arrays full of 0xAB -> (rc, request, entries, text bytes)"""
    from sweepga_amd import _lib
    from sweepga_amd.lift import cigar_set
    from sweepga_amd.variants import sequence_set
    ctx = sw.default_context()
    rec = _lib.SwgRecords()
    rec.n = len(strand)
    keep = {k: np.ascontiguousarray(cols[k], dtype=np.uint32) for k in COLS}
    for k, a in keep.items():
        setattr(rec, k, a.ctypes.data)
    rec.strand, rec.n_seq = strand.ctypes.data, n_seq
    record, offset, text = cig if isinstance(cig, tuple) else cigar_set(sorted(cig), [cig[i] for i in sorted(cig)])
    cs = _lib.SwgCigarSet()
    cs.record, cs.offset, cs.text, cs.k = record.ctypes.data, offset.ctypes.data, text.ctypes.data, len(record)
    s_off, s_bases = seqs if isinstance(seqs, tuple) else sequence_set(seqs)
    ss = _lib.SwgSeqSet()
    ss.offset, ss.bases, ss.n_seq = s_off.ctypes.data if s_off is not None else None, s_bases.ctypes.data if s_bases is not None else None, n_seq
    arrays = [np.full(size * max(c, 1), 0xab, dtype=np.uint8) for size, c in zip((64, 1), caps)]
    req = _lib.SwgEqxRequest()
    req.set, req.reserved, req.usable = set_, reserved, 99
    req.entry_capacity, req.text_capacity = caps
    req.entries, req.text = (None if k in null else a.ctypes.data for k, a in enumerate(arrays))
    rc = fn(ctx.handle, C.byref(rec), status.ctypes.data if status is not None else None, C.byref(cs), C.byref(ss) if seq_set else None, C.byref(req))
    return (rc, req) + tuple(a.tobytes() for a in arrays)


def test_capacities_with_poisoned_arrays(sw, small):
    cols, strand, _, cig, seqs, _ = small
    lib = sw.default_context().lib
    want = xm.eqx_records(cols, strand, cig, seqs)
    counts = (600, want["text_bytes"])
    full = (xm.entries_array(want["entries"]).tobytes(), want["text"].encode())
    assert counts[1] > 3000
    for which in range(2):
        for cap in (0, counts[which] - 1, counts[which]):
            caps = tuple(cap if k == which else counts[k] for k in range(2))
            rc, req, *arrays = raw_call(sw, lib.swg_eqx_records, cols, strand, 6, cig, seqs, caps)
            assert rc == 0 and (req.text_bytes, req.usable, req.out_ops, req.changed) == (counts[1], want["usable"], want["out_ops"], want["changed"])
            for k in range(2):
                if caps[k] >= counts[k]:
                    assert arrays[k] == full[k], (which, cap, k)
                else:
                    assert set(arrays[k]) == {0xab}, (which, cap, k)
    for null in ((0,), (1,), (0, 1)):
        rc, req, *arrays = raw_call(sw, lib.swg_eqx_records, cols, strand, 6, cig, seqs, counts, null=null)
        assert rc == 0 and req.text_bytes == counts[1] and req.matches == want["matches"]
        for k in range(2):
            assert arrays[k] == full[k] if k not in null else set(arrays[k]) == {0xab}


def test_no_entries_a_partial_set_and_records_permuted(sw, small):
    from sweepga_amd.eqx import eqx_records
    cols, strand, _, cig, seqs, status = small
    ctx = sw.default_context()
    got = eqx_records(ctx, cols, strand, 6, [], [], seqs)
    assert all(getattr(got, f) == 0 for f in FIELDS) and len(got.entries) == len(got.text) == 0
    got = eqx_records(ctx, cols, strand, 6, [], [], None)      # k = 0 asks for no sequences
    assert got.usable == 0
    part = check(sw, cols, strand, 6, {i: cig[i] for i in range(0, 600, 3)}, seqs, status=status, set_=1, what="a partial set")
    assert 0 < part.usable < 200 and len(part.entries) == 200
    perm = np.random.default_rng(3).permutation(600)
    pcols = {k: v[perm] for k, v in cols.items()}
    every = check(sw, cols, strand, 6, cig, seqs, what="in order")
    moved = check(sw, pcols, strand[perm], 6, {j: cig[i] for j, i in enumerate(perm)}, seqs, what="permuted")
    assert all(getattr(moved, f) == getattr(every, f) for f in FIELDS)
    assert all(moved.cigar(j) == every.cigar(int(perm[j])) for j in range(600))
    names = [f for f in xm.ENTRY_FIELDS if f not in ("record", "text_first")]
    assert all(moved.entries[f][j] == every.entries[f][perm[j]] for f in names for j in range(0, 600, 7))


def test_refusals(sw, small):
    from sweepga_amd.eqx import eqx_records, eqx_records_device
    from sweepga_amd.lift import cigar_set
    from sweepga_amd.variants import sequence_set
    cols, strand, _, cig, seqs, status = small
    ctx = sw.default_context()
    lib = ctx.lib
    good = cigar_set([3, 5, 9], ["1=", "2=", ""])
    s_off, s_bases = sequence_set(seqs)
    down = s_off.copy()
    down[3] = down[2] - 1
    for kw, word in (({"set": 2}, "set"), ({"set": 1}, "status")):
        with pytest.raises(sw.SwgError) as e:
            eqx_records(ctx, cols, strand, 6, None, good, seqs, **kw)
        assert e.value.code == -1 and word in str(e.value)
    for bad_seqs, word in ((None, "NULL sequences"), ((down, s_bases), "descend"), ((s_off[:-1], s_bases), "n_seq")):
        with pytest.raises(sw.SwgError) as e:
            eqx_records(ctx, cols, strand, 6, None, good, bad_seqs)
        assert e.value.code == -1 and word in str(e.value), word
    rc, req, entries, text = raw_call(sw, lib.swg_eqx_records, cols, strand, 6, good, seqs, (4, 40), reserved=1)
    assert rc == -1 and set(entries) == set(text) == {0xab} and req.usable == 99 and b"reserved" in lib.swg_last_error(ctx.handle)
    rc, *_ = raw_call(sw, lib.swg_eqx_records, cols, strand, 6, good, (None, s_bases), (4, 40))
    assert rc == -1 and b"NULL sequences" in lib.swg_last_error(ctx.handle)
    high = dict(cols, q_id=np.full(600, 6, dtype=np.uint32))
    rc, *_ = raw_call(sw, lib.swg_eqx_records, high, strand, 6, good, seqs, (4, 40))
    assert rc == -1 and b"sequence id" in lib.swg_last_error(ctx.handle)
    bad_set = (np.array([5, 3, 9], dtype=np.uint32), good[1], good[2])
    rc, *_ = raw_call(sw, lib.swg_eqx_records, cols, strand, 6, bad_set, seqs, (4, 40))
    assert rc == -1
    hip = Hip()
    try:
        dcols = {k: Dev(hip, cols[k], np.uint32) for k in COLS}
        args = (dcols, Dev(hip, strand, np.uint8), 6, *(Dev(hip, a) for a in good), 3)
        with pytest.raises(sw.SwgError) as e:      # descending offsets in device memory: refused before a base is read
            eqx_records_device(ctx, *args, Dev(hip, down), Dev(hip, s_bases))
        assert e.value.code == -1 and "descend" in str(e.value)
        with pytest.raises(sw.SwgError) as e:
            eqx_records_device(ctx, *args, None, None)
        assert e.value.code == -1 and "NULL sequences" in str(e.value)
        with pytest.raises(sw.SwgError) as e:
            eqx_records_device(ctx, *args, Dev(hip, s_off), Dev(hip, s_bases), set=1)
        assert e.value.code == -1 and "status" in str(e.value)
        ok = eqx_records_device(ctx, *args, Dev(hip, s_off), Dev(hip, s_bases))
        assert ok.ops == 2 and ok.empty == 1
    finally:
        hip.free()
    after = check(sw, cols, strand, 6, {3: cig[3]}, seqs, what="after the refusals")      # the context is as usable as before
    assert after.usable + after.no_sequence == 1


def test_a_memory_limit_that_does_not_hold_the_call_and_one_that_does(sw, small):
    from sweepga_amd.eqx import eqx_records
    cols, strand, _, cig, seqs, _ = small
    ctx = sw.Context(0)
    try:
        n = 100_000      # 2 * 10^5 ops: 32 bytes of prefix sums and 22 of this report each, 20 per output op
        T = vm.random_bases(np.random.default_rng(1), n)
        c1 = {"q_id": [0], "t_id": [1], "q_start": [0], "q_end": [2 * n], "t_start": [0], "t_end": [n]}
        c1 = {k: np.array(v, dtype=np.uint32) for k, v in c1.items()}
        Qs = bytes(np.repeat(np.frombuffer(T, dtype=np.uint8), 2))
        ctx.set_memory_limit(4 << 20)
        with pytest.raises(sw.SwgError) as e:
            eqx_records(ctx, c1, np.zeros(1, dtype=np.uint8), 2, [0], ["1M1I" * n], [Qs, T])
        assert e.value.code == -4
        got = eqx_records(ctx, cols, strand, 6, sorted(cig), [cig[i] for i in sorted(cig)], seqs)      # the same context, a call that fits
        compare(got, xm.eqx_records(cols, strand, cig, seqs), "under the limit")
        ctx.set_memory_limit(0)
        got = eqx_records(ctx, c1, np.zeros(1, dtype=np.uint8), 2, [0], ["1M1I" * n], [Qs, T])
        assert got.text.tobytes() == b"1=1I" * n and (got.matches, got.out_ops, int(got.entries["inserted"][0]), int(got.entries["block"][0])) == (n, 2 * n, n, 2 * n)
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
                got = check(sw, part, strand[:n], 2, {i: cig[i] for i in range(n)}, seqs, status=status, set_=0 if status is None else 1, what=f"n = {n}", ctx=ctx)
                assert got.usable == (n if status is None else (n + 1) // 2) and got.cigar(0) == b"2=1X2I3=1D1X"
    finally:
        ctx.close()


# ---- the whole path and the cross-checks on the device ------------------------------------------------------------------------------------
def test_20000_generated_records_idempotence_variants_and_diffs(sw):
    """2 * 10^4 generated records under a real 1:1 status.  The output set fed back gives the same bytes; swg_variant_records' pair sums
    agree with the entries' sums (see tests/test_eqx_cpu.py on the columns under =); swg_diff_records on the output text gives no M
    column and the aligned, inserted and deleted bases of the input."""
    from sweepga_amd.diffs import diff_records
    from sweepga_amd.variants import variant_records
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
        got = check(sw, cols, strand, 12, part, seqs, status=status, set_=set_, what="random, set %d" % set_, shift=7 * set_)
        assert got.cigar_bad > 0.03 * len(part) and got.usable > 0 and got.changed > got.usable // 4
        usable.append(got.usable)
    assert usable[0] > 15_000 and 0 < usable[1] < usable[0]
    ctx = sw.default_context()
    recs = sorted(part)
    ok = np.flatnonzero(got.entries["flags"] & xm.USABLE)
    out = {recs[j]: got.cigar(j).decode() for j in ok}
    again = check(sw, cols, strand, 12, out, seqs, what="fed back")
    assert again.text.tobytes() == got.text.tobytes() and (again.eq_wrong, again.x_wrong, again.m_columns, again.changed) == (0, 0, 0, 0)
    assert again.usable == got.usable and (again.matches, again.mismatches, again.n_columns) == (got.matches, got.mismatches, got.n_columns)
    # the variant calls over the same entries with every = written as M: their columns are all the columns
    as_m = {i: part[i].replace("=", "M") for i in out}
    var = variant_records(ctx, cols, strand, 12, genome, 4, sorted(as_m), [as_m[i] for i in sorted(as_m)], seqs)
    key = genome[cols["q_id"][[recs[j] for j in ok]]].astype(np.int64) * 4 + genome[cols["t_id"][[recs[j] for j in ok]]]
    for p in var.pairs:
        mine = key == int(p["q_genome"]) * 4 + int(p["t_genome"])
        assert int(got.entries["matches"][ok][mine].sum()) == int(p["same"]) + int(p["m_equal"])
        assert int(got.entries["mismatches"][ok][mine].sum()) == int(p["snvs"]) + int(p["n_columns"])
    assert var.usable == got.usable and var.columns == got.columns and int(var.pairs["n_columns"].sum()) == got.n_columns
    d_in = diff_records(ctx, cols, strand, 12, genome, 4, sorted(out), [part[i] for i in sorted(out)], kinds=15)
    d_out = diff_records(ctx, cols, strand, 12, genome, 4, sorted(out), [out[i] for i in sorted(out)], kinds=15)
    assert d_in.usable == d_out.usable == got.usable and int(d_out.pairs["m_columns"].sum()) == 0 and int(d_in.pairs["m_columns"].sum()) == got.m_columns
    for f in ("aligned", "n_ins", "ins_bases", "n_del", "del_bases", "n_skip", "skip_bases"):
        assert d_in.pairs[f].tolist() == d_out.pairs[f].tolist(), f
    assert int(d_out.pairs["eq"].sum()) == got.matches and int(d_out.pairs["snp_bases"].sum()) == got.mismatches


# ---- the PAF seam, the Python class and the command line ---------------------------------------------------------------------------------
def test_write_the_python_class_and_the_command_line_for_every_batch_size(sw, tmp_path):
    from sweepga_amd import build
    from tests.test_gpu_intervals import kept_mask
    text, kept, fasta = vcf_paf()
    st = kept.astype(np.uint8)
    fa, fa2 = tmp_path / "a.fa", tmp_path / "b.fa"
    write_fasta(fa, fasta[:1])
    write_fasta(fa2, fasta[1:], width=80)
    files = [str(fa), str(fa2)]
    out = tmp_path / "e.paf"
    one_record = max(xm.batch_costs(text, None, 0))
    with sw.PafFile(text=text) as paf:
        for set_, status in ((0, None), (1, st), (0, st)):
            n_records = 17 if set_ == 0 else int(kept.sum())
            for unresolved in ("keep", "drop"):
                want = xm.paf_text(text, kept, fasta, set_, unresolved)
                assert want[1]["usable"] >= 5 and want[1]["untagged"] == 1 and want[1]["bad"] >= 1 and want[1]["no_sequence"] == 1 + (set_ == 0)
                assert want[1]["lines"] == (n_records if unresolved == "keep" else want[1]["usable"]) and want[1]["changed"] >= 3
                for batch in (1, one_record, 40, 0):
                    got = sw.Eqx.from_paf(paf, status, fasta=files, set=set_, unresolved=unresolved, batch_bytes=batch)
                    assert got.text == want[0], (set_, unresolved, batch)
                    assert {k: v for k, v in got.counts.items() if k != "batches"} == want[1]
                    assert sw.Eqx.write_paf(paf, status, out, fasta=files, set=set_, unresolved=unresolved, batch_bytes=batch) == got.counts
                    assert out.read_text() == want[0]
                    assert 1 <= got.counts["batches"] <= n_records and (batch != 1 or got.counts["batches"] == n_records) and (batch or got.counts["batches"] == 1)
        short = sw.Eqx.from_paf(paf, st, fasta=[str(fa)])                                    # the second file is missing: its sequences are absent
        assert short.counts["usable"] == 0 and short.counts["no_sequence"] > 5 and short.text == "".join(ln + "\n" for ln, k in zip(text.split("\n"), kept) if k)
        write_fasta(fa2, [(fasta[1][0], fasta[1][1][:-1])])
        off = sw.Eqx.from_paf(paf, st, fasta=files)
        assert off.counts["length_mismatch"] == 1 and off.counts == dict(short.counts, length_mismatch=1) and off.text == short.text
        write_fasta(fa2, fasta[1:], width=80)
        # the resolved PAF is a PAF like any other: read back, every usable record resolves to itself
        keep_text = xm.paf_text(text, kept, fasta, 1, "drop")[0]
    with sw.PafFile(text=keep_text) as paf2:
        back = sw.Eqx.from_paf(paf2, None, fasta=files, set="all")
        assert back.text == keep_text and back.counts["changed"] == 0 and back.counts["eq_wrong"] == back.counts["x_wrong"] == back.counts["m_columns"] == 0
    # the command line: a real 1:1 filter over generated records; the output PAF, the --diffs file and the --vcf file do not change
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
    inp, plain, outp, d0, d1, v0, v1 = (tmp_path / nm for nm in ("in.paf", "plain.paf", "out.paf", "plain.diffs", "out.diffs", "plain.vcf", "out.vcf"))
    inp.write_text(big, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-jump", "10k", "--scaffold-mass", "2k"]
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), "--diffs", str(d0), "--vcf", str(v0), "--vcf-fasta", str(big_fa), *flags, "--quiet"],
                        capture_output=True)
    assert r0.returncode == 0 and plain.stat().st_size > 0 and d0.stat().st_size > 0 and v0.stat().st_size > 0, r0.stderr
    kept = kept_mask(big, plain.read_bytes().decode())
    with sw.PafFile(text=big) as paf:      # every batch size gives the same bytes
        for set_ in (1, 0):
            want = xm.paf_text(big, kept, records, set_)
            got = [sw.Eqx.from_paf(paf, kept.astype(np.uint8), fasta=[str(big_fa)], set=set_, batch_bytes=b) for b in (1, 100, 4096, 0)]
            assert all(g.text == want[0] for g in got) and all({k: v for k, v in g.counts.items() if k != "batches"} == want[1] for g in got)
            batches = [g.counts["batches"] for g in got]
            assert batches[0] > batches[1] > batches[2] >= batches[3] == 1
    for extra, set_, unresolved in (([], 1, "keep"), (["--eqx-set", "all", "--eqx-unresolved", "drop", "--eqx-batch", "2k"], 0, "drop")):
        want, c = xm.paf_text(big, kept, records, set_, unresolved)
        r = subprocess.run([build.CLI, str(inp), "--output-file", str(outp), "--diffs", str(d1), "--vcf", str(v1), "--vcf-fasta", str(big_fa), "--eqx", str(out),
                            "--eqx-fasta", str(big_fa), *extra, *flags], capture_output=True)
        assert r.returncode == 0 and r.stdout == b"" and outp.read_bytes() == plain.read_bytes() and d1.read_bytes() == d0.read_bytes(), r.stderr
        assert v1.read_bytes() == v0.read_bytes() and out.read_text() == want and c["records"] > 100 and c["usable"] > c["records"] // 3 and c["x_wrong"] > 0
        assert ("--eqx: %d lines, %d resolved (%d changed): %d columns, %d matches, %d mismatches, %d under M ops; %d entries without sequence, %d out of sequence, "
                "%d bad, %d without a cg:Z: tag, %d sequences of another length; eq_wrong %d, x_wrong %d"
                % (c["lines"], c["usable"], c["changed"], c["columns"], c["matches"], c["mismatches"], c["m_columns"], c["no_sequence"], c["out_of_sequence"],
                   c["bad"], c["untagged"], c["length_mismatch"], c["eq_wrong"], c["x_wrong"])) in r.stderr.decode()
    # the resolved file through the other reports: --diffs reads it like any PAF and meets no M column
    r = subprocess.run([build.CLI, str(out), "--output-file", str(outp), "--diffs", str(d1), "--no-filter"], capture_output=True)
    assert r.returncode == 0 and b" 0 columns under M ops" in r.stderr, r.stderr
    out.unlink()
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(outp), "--eqx", str(out), "--eqx-fasta", str(big_fa), "--no-filter", "--quiet"], capture_output=True)
    assert r.returncode == 0 and out.read_text() == xm.paf_text(big, None, records, 0)[0], r.stderr
