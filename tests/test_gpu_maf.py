"""The alignment blocks on the device (sweepga_amd/csrc/swg_maf.hip) against tests/maf_model.py: in every case the host seam against
the model and the device seam against the host seam -- blocks, text and counts, byte for byte.  The shapes are the smallest at which
each part can go wrong: blocks whose borders and whose border between the two rows fall on, before and behind the text kernel's tile
of 4,096 bytes; as many one-column blocks as fill the LDS list of block ends and cross the compactions' tile of 4,096; an entry
whose every column lies in another op; one op of 2 * 10^6 columns; sequences that touch both edges of the bases; gaps across a whole
tile; the split at every place; the capacity protocol; the resolved CIGARs as a cross-check on the device; the PAF seam, the Python
class and --maf.  Every comparison is exact: integers and bytes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import lift_model as lm
from tests import maf_model as mm
from tests import variants_model as vm
from tests.test_eqx_cpu import widen
from tests.test_gpu_lift import Dev
from tests.test_gpu_variants import build_case, vcf_paf, write_fasta
from tests.test_gpu_wide import Hip

pytestmark = pytest.mark.gpu
COLS = lm.COLS
FIELDS = mm.FIELDS
TT = 4096      # the text kernel's tile


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


def same(a, b):
    return a.blocks.tobytes() == b.blocks.tobytes() and a.text.tobytes() == b.text.tobytes() and all(getattr(a, f) == getattr(b, f) for f in FIELDS)


def both_seams(sw, cols, strand, n_seq, cig, seqs, status=None, set_=0, g=0, shift=0):
    """The result of the host seam, after checking that the device seam gives the same.  shift: the device text and the device bases
    start that many bytes behind a 16-byte boundary."""
    from sweepga_amd.lift import cigar_set
    from sweepga_amd.maf import maf_records, maf_records_device
    from sweepga_amd.variants import sequence_set
    ctx = sw.default_context()
    recs = sorted(cig)
    s_off, s_bases = sequence_set(seqs)
    got = maf_records(ctx, cols, strand, n_seq, recs, [cig[i] for i in recs], (s_off, s_bases), status=status, set=set_, split_gap=g)
    record, offset, text = cigar_set(recs, [cig[i] for i in recs])
    hip = Hip()
    try:
        dcols = {k: Dev(hip, cols[k], np.uint32) for k in COLS}
        dtext = Dev(hip, np.concatenate([np.zeros(shift, dtype=np.uint8), text]))
        dbases = Dev(hip, np.concatenate([np.zeros(shift, dtype=np.uint8), s_bases]))
        dtext.ptr += shift
        dbases.ptr += shift
        dev = maf_records_device(ctx, dcols, Dev(hip, strand, np.uint8), n_seq, Dev(hip, record), Dev(hip, offset), dtext, len(recs), Dev(hip, s_off), dbases,
                                 status=Dev(hip, status, np.uint8) if status is not None else None, set=set_, split_gap=g)
    finally:
        hip.free()
    assert same(dev, got)
    return got


def compare(got, want, what=""):
    assert {f: getattr(got, f) for f in FIELDS} == {f: want[f] for f in FIELDS}, what
    rows = mm.blocks_array(want["blocks"])
    if got.blocks.tobytes() != rows.tobytes():
        bad = [k for k in range(len(rows)) if got.blocks[k].tobytes() != rows[k].tobytes()]
        raise AssertionError((what, len(bad), [(k, tuple(int(v) for v in got.blocks[k]), want["blocks"][k]) for k in bad[:5]]))
    text = got.text.tobytes()
    if text != want["text"]:
        a, b = np.frombuffer(text, dtype=np.uint8), np.frombuffer(want["text"], dtype=np.uint8)
        k = int(np.flatnonzero(a[:min(a.size, b.size)] != b[:min(a.size, b.size)])[0]) if a.size == b.size else min(a.size, b.size)
        raise AssertionError((what, "text byte", k, text[max(k - 20, 0):k + 20], want["text"][max(k - 20, 0):k + 20]))


def check(sw, cols, strand, n_seq, cig, seqs, status=None, set_=0, g=0, what="", shift=0):
    """Both seams against the model."""
    cols = {k: np.asarray(cols[k]).astype(np.uint32) for k in COLS}
    strand = np.asarray(strand).astype(np.uint8)
    got = both_seams(sw, cols, strand, n_seq, cig, seqs, status, set_, g, shift)
    compare(got, mm.maf_records(cols, strand, cig, seqs, None if status is None else np.asarray(status) != 0, set_, g), what)
    return got


def check_specs(sw, rng, specs, what="", lower=0.0, iupac=0.0, **kw):
    cols, strand, cig, seqs = build_case(rng, specs, lower=lower, iupac=iupac)
    return check(sw, cols, strand, 2, cig, seqs, what=what, **kw)


# ---- the text kernel's tiles -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("minus", [0, 1])
def test_block_and_row_borders_on_before_and_behind_tile_borders(sw, minus):
    """Blocks of 2,047, 2,048 and 2,049 columns (4,094 / 4,096 / 4,098 bytes), each with an insertion and a deletion inside, in every
    order that puts a block border and the border between its two rows on, before and behind a tile border."""
    rng = np.random.default_rng(3 + minus)
    edits = lambda n: [(n - 12, "="), (3, "I"), (2, "X"), (4, "D"), (3, "=")]      # noqa: E731  (n columns)
    for order in ((2048, 2047, 2049, 2048), (2047, 2049, 2048), (2049, 2049, 2047, 2047)):
        for shift in (0, 7):
            got = check_specs(sw, rng, [(edits(n), minus, k % 2 == 1, 0.0) for k, n in enumerate(order)], "tiles %s" % (order,), lower=0.2, shift=shift)
            assert got.blocks["columns"].tolist() == list(order) and got.text_bytes == 2 * sum(order) and got.n_blocks == len(order)


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_one_column_blocks_around_4096(sw, n):
    """n blocks of one column, two bytes each: 2,048 blocks in every full tile -- the LDS list of block ends at its bound -- and the
    compactions' tile of 4,096 candidates crossed.  Every third entry is a gap-only candidate, which takes no place in the text."""
    rng = np.random.default_rng(n)
    specs = []
    for k in range(n):
        specs.append(([(1, "=" if k % 2 else "X")], k % 3 == 0, False, 0.0))
        if k % 3 == 1:
            specs.append(([(1, "I")], 0, False, 0.0))
    got = check_specs(sw, rng, specs, "one-column blocks", shift=7)
    assert (got.n_blocks, got.text_bytes, got.columns, got.aligned) == (n, 2 * n, n, n) and got.gap_only == len(specs) - n
    assert got.blocks["text_first"].tolist() == list(range(0, 2 * n, 2))


@pytest.mark.parametrize("minus", [0, 1])
def test_every_column_in_another_op_and_the_same_columns_under_one_op(sw, minus):
    """One entry of 1=1I1D repeated 1,500 times: 4,500 columns, 9,000 bytes across three tiles, and every lane searches its op.  A
    second entry holds the first one's aligned columns under ONE M op (one search per wavefront): its rows must be the first
    one's rows at every third column."""
    rng = np.random.default_rng(5 + minus)
    reps = 1500
    cols, strand, cig, seqs = build_case(rng, [([(1, "="), (1, "I"), (1, "D")] * reps, minus, False, 0.0)], lower=0.2)
    first = mm.maf_records(cols, strand, cig, seqs)
    rows = np.frombuffer(first["text"], dtype=np.uint8)
    t_row, q_row = rows[:3 * reps:3], rows[3 * reps::3]
    assert first["columns"] == 3 * reps and t_row.size == q_row.size == reps
    q2 = mm.COMP_RAW[q_row[::-1]] if minus else q_row      # the query whose walk gives q_row
    seqs = seqs + [b"a" + q2.tobytes() + b"c", b"gg" + t_row.tobytes()]
    cols = {k: np.r_[cols[k], {"q_id": 2, "t_id": 3, "q_start": 1, "q_end": 1 + reps, "t_start": 2, "t_end": 2 + reps}[k]] for k in COLS}
    strand = np.r_[strand, minus].astype(np.uint8)
    cig[1] = "%dM" % reps
    for shift in (0, 7):
        got = check(sw, cols, strand, 4, cig, seqs, what="every column another op", shift=shift)
        a, b = got.rows(0), got.rows(1)
        assert (a[0][::3], a[1][::3]) == b and len(b[0]) == reps and got.n_blocks == 2 and b"-" not in b[0] + b[1]
        assert a[0][1::3] == b"-" * reps and a[1][2::3] == b"-" * reps


def test_one_op_of_two_million_columns(sw):
    """One block across about 1,000 tiles, between two short ones; '-' on the long one."""
    rng = np.random.default_rng(9)
    L = 2_000_000
    got = check_specs(sw, rng, [([(3, "="), (1, "I")], 0, False, 0.0), ([(L, "X")], 1, True, 0.3), ([(2, "D"), (5, "=")], 1, False, 0.0)], "2e6", lower=0.1, shift=7)
    assert got.blocks["columns"].tolist() == [4, L, 7] and got.text_bytes == 2 * (L + 11) and int(got.blocks["text_first"][2]) == 8 + 2 * L


def test_gaps_across_a_whole_tile(sw):
    """I ops and D ops of 5,000 columns inside a block: more gap bytes than a tile holds, in either row, on both strands."""
    rng = np.random.default_rng(10)
    edits = [(7, "="), (5000, "I"), (3, "X"), (5000, "D"), (1, "="), (5000, "D"), (5000, "I"), (2, "=")]
    for shift in (0, 7):
        got = check_specs(sw, rng, [(edits, 0, False, 0.0), (edits, 1, True, 0.0)], "long gaps", shift=shift)
        assert got.blocks["columns"].tolist() == [20013, 20013] and got.aligned == 26 and got.rows(0)[0][7:5007] == b"-" * 5000


def test_sequences_that_touch_both_edges_of_the_bases(sw):
    """A target of one base; a query that is the first sequence of the set from its first base on; a target that is the last
    sequence up to its last base -- lengths that are no multiple of four, on both strands, at every alignment of the bases: the
    32-bit loads meet the first and the last dword of the bases."""
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 5, 13, 14, 15, 16, 17):
        q = vm.plant(rng, vm.random_bases(rng, n), 0.3, 0.0)
        t = vm.plant(rng, vm.random_bases(rng, n), 0.3, 0.0)
        seqs = [q, b"G", t]                                 # the query first, a target of one base, the other target last
        recs = [("%dM" % n, 0, 0, n, 2, 0, n), ("%dM" % n, 1, 0, n, 2, 0, n), ("1M", 0, 0, 1, 1, 0, 1), ("1X", 1, n - 1, n, 1, 0, 1)]
        if n >= 5:
            recs += [("2=1I%dM" % (n - 4), 1, 0, n - 1, 2, 2, n), ("%dM1D2=" % (n - 3), 0, 0, n - 1, 2, 0, n), ("%dM" % (n - 1), 1, 1, n, 2, 1, n)]
        cols = {k: np.array([r[j] for r in recs], dtype=np.uint32) for k, j in (("q_start", 2), ("q_end", 3), ("t_id", 4), ("t_start", 5), ("t_end", 6))}
        cols["q_id"] = np.zeros(len(recs), dtype=np.uint32)
        for shift in (0, 1, 2, 3, 7):
            got = check(sw, cols, np.array([r[1] for r in recs], dtype=np.uint8), 3, {i: r[0] for i, r in enumerate(recs)}, seqs, what="edges %d" % n, shift=shift)
            assert got.usable == len(recs) == got.n_blocks and got.rows(0) == (t, q) and got.rows(2) == (b"G", q[:1])


# ---- the split --------------------------------------------------------------------------------------------------------------------------
HAND = [("2=2I8=", 0, b"ACGTACGTAC", b"ACttGTACGTAC"), ("2=2I8=", 1, b"ACGTACGTAC", b"GTACGTACaaGT"), ("3D2=1S0I2N", 0, b"ACGTACGTAC", b"TA"),
        ("2=3I3D2=", 0, b"ACGTACGTAC", b"ACgggTA"), ("2=3D1I3D2=", 0, b"ACGTACGTAC", b"ACgGT"), ("3D0M3D", 0, b"ACGTACGTAC", b"A"),
        ("1I3D2I", 1, b"ACGTACGTAC", b"ggg"), ("5I", 0, b"ACGTACGTAC", b"ggggg"), ("3=2I2=1D2=", 1, b"ACGTACGTAC", b"ACTAaaCGT")]


@pytest.mark.parametrize("g", [0, 1, 2, 3, 5])
def test_the_hand_cases_of_the_cpu_test(sw, g):
    """The entries of tests/test_maf_cpu.py's breaker cases, one call: breakers with l = g - 1 and l = g, first and last, adjacent,
    gap-only candidates, an entry without a block."""
    seqs, cig, rows = [], {}, []
    for i, (text, minus, t, q) in enumerate(HAND):
        seqs += [t, q]
        qn = sum(int(d) for d, ch in mm.xm.raw_ops(text) if ch in "M=XI")
        tn = sum(int(d) for d, ch in mm.xm.raw_ops(text) if ch in "M=XDN")
        rows.append((2 * i + 1, 2 * i, 0, qn, 0, tn))
        cig[i] = text
    cols = {k: np.array([r[j] for r in rows], dtype=np.uint32) for j, k in enumerate(("q_id", "t_id", "q_start", "q_end", "t_start", "t_end"))}
    got = check(sw, cols, np.array([h[1] for h in HAND], dtype=np.uint8), len(seqs), cig, seqs, g=g, what="hand, g = %d" % g, shift=7)
    assert got.usable == len(HAND)
    if g == 2:
        assert got.rows(0) == (b"AC", b"AC") and got.rows(1) == (b"GTACGTAC", b"GTACGTAC") and got.gap_only == 1 + 1 + 1
    if g == 3:
        assert (got.breakers, got.gap_only) == (1 + 2 + 2 + 2 + 1 + 1, 1 + 1 + 2)


@pytest.fixture(scope="module")
def random_entries():
    rng = np.random.default_rng(13)
    cols, strand, _, cig, seqs = vm.random_case(rng, 3000, n_targets=3, n_queries=3, n_ops=14, max_len=6, iupac=0.03)
    return cols, strand, {i: widen(rng, t) for i, t in cig.items()}, seqs


@pytest.mark.parametrize("g", [0, 1, 3, 50])
def test_3000_random_entries(sw, random_entries, g):
    cols, strand, cig, seqs = random_entries
    got = check(sw, cols, strand, 6, cig, seqs, g=g, what="random, g = %d" % g, shift=7 if g else 0)
    assert got.usable == 3000 and (got.breakers > 3000) == (g in (1, 3)) and (g in (0, 50)) == (got.n_blocks == 3000 - got.gap_only)


def test_5000_alternating_breakers_and_one_column_ops(sw):
    """One entry of 5,000 one-column = ops with a breaker behind each -- I and D in turn -- so the candidates cross the compactions'
    tile of 4,096; with split_gap one above the breakers' length it is one block of 15,000 columns."""
    rng = np.random.default_rng(14)
    edits = []
    for k in range(5000):
        edits += [(1, "="), (2, "I" if k % 2 else "D")]
    for g, n_blocks in ((2, 5000), (3, 1)):
        got = check_specs(sw, rng, [([(2, "=")], 1, False, 0.0), (edits, 0, False, 0.0), (edits, 1, False, 0.0)], "alternating", g=g, shift=7)
        assert got.n_blocks == 1 + 2 * n_blocks and got.breakers == (2 * 5000 if g == 2 else 0) and got.skipped_t == got.skipped_q == (10000 if g == 2 else 0)
        assert got.columns == (2 + 2 * 5000 if g == 2 else 2 + 2 * 15000)


# ---- sets, protocol, cross-checks ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(7)
    cols, strand, genome, cig, seqs = vm.random_case(rng, 600, n_targets=3, n_queries=3, genomes=3)
    seqs[1] = b""                                          # an absent target
    cols["t_end"][cols["t_id"] == 2] += (rng.random(int((cols["t_id"] == 2).sum())) < 0.01).astype(np.uint32)      # a target sum off by one: bad
    last = int(np.flatnonzero(cols["t_id"] == 0)[-1])
    seqs[0] = seqs[0][:int(cols["t_end"][last]) - 1]       # t_end one past the sequence
    cig = dict(cig)
    cig[5] = ""
    return cols, strand, genome, cig, seqs, (rng.random(600) < 0.6).astype(np.uint8)


def test_both_sets_and_every_unusable_reason(sw, small):
    cols, strand, _, cig, seqs, status = small
    base = check(sw, cols, strand, 6, cig, seqs, g=4, what="all")
    assert base.no_sequence > 100 and base.out_of_sequence == 1 and base.cigar_bad >= 1 and base.empty == 1
    assert base.usable + base.no_sequence + base.out_of_sequence + base.cigar_bad + base.empty == 600
    kept = check(sw, cols, strand, 6, cig, seqs, status=status, set_=1, g=4, what="kept", shift=7)
    assert 0 < kept.usable < base.usable and 0 < kept.text_bytes < base.text_bytes and kept.cigar_bad == base.cigar_bad
    none = check(sw, cols, strand, 6, cig, seqs, status=np.zeros(600, dtype=np.uint8), set_=1, what="never in status")
    assert (none.usable, none.no_sequence, none.columns, none.n_blocks, none.text_bytes, none.ops) == (0, 0, 0, 0, 0, base.ops)
    from sweepga_amd.maf import maf_records
    got = maf_records(sw.default_context(), cols, strand, 6, [], [], None)      # k = 0 asks for no sequences
    assert all(getattr(got, f) == 0 for f in FIELDS) and len(got.blocks) == len(got.text) == 0


def raw_call(sw, fn, cols, strand, n_seq, cig, seqs, caps, g=0, null=(), device=False):
    """One seam (device: the columns, the set's arrays and the sequences in device memory) with caller arrays full of 0xAB ->
    (rc, request, blocks, text bytes)"""
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
    record, offset, text = cigar_set(sorted(cig), [cig[i] for i in sorted(cig)])
    cs = _lib.SwgCigarSet()
    cs.record, cs.offset, cs.text, cs.k = record.ctypes.data, offset.ctypes.data, text.ctypes.data, len(record)
    s_off, s_bases = sequence_set(seqs)
    ss = _lib.SwgSeqSet()
    ss.offset, ss.bases, ss.n_seq = s_off.ctypes.data, s_bases.ctypes.data, n_seq
    hip = Hip() if device else None
    if device:
        dev = {k: Dev(hip, a, np.uint32) for k, a in keep.items()}
        for k, d in dev.items():
            setattr(rec, k, d.ptr)
        d_strand, d_record, d_offset, d_text, d_off, d_bases = (Dev(hip, a) for a in (strand, record, offset, text, s_off, s_bases))
        rec.strand = d_strand.ptr
        cs.record, cs.offset, cs.text = d_record.ptr, d_offset.ptr, d_text.ptr
        ss.offset, ss.bases = d_off.ptr, d_bases.ptr
    arrays = [np.full(size * max(c, 1), 0xab, dtype=np.uint8) for size, c in zip((64, 1), caps)]
    req = _lib.SwgMafRequest()
    req.set, req.split_gap, req.usable = 0, g, 99
    req.block_capacity, req.text_capacity = caps
    req.blocks, req.text = (None if k in null else a.ctypes.data for k, a in enumerate(arrays))
    try:
        rc = fn(ctx.handle, C.byref(rec), None, C.byref(cs), C.byref(ss), C.byref(req))
    finally:
        if hip is not None:
            hip.free()
    return (rc, req) + tuple(a.tobytes() for a in arrays)


def test_capacities_with_poisoned_arrays(sw, small):
    """Each array too small by one, NULL, or exact, on the host seam and on the device seam: what must not be written stays untouched,
    the counts come always."""
    cols, strand, _, cig, seqs, _ = small
    lib = sw.default_context().lib
    seams = ((lib.swg_maf_records, False), (lib.swg_maf_records_device, True))
    want = mm.maf_records(cols, strand, cig, seqs, g=3)
    counts = (want["n_blocks"], want["text_bytes"])
    full = (mm.blocks_array(want["blocks"]).tobytes(), want["text"])
    assert counts[0] > 500 and counts[1] > 3000
    for fn, device in seams:
        for which in range(2):
            for cap in (0, counts[which] - 1, counts[which]):
                caps = tuple(cap if k == which else counts[k] for k in range(2))
                rc, req, *arrays = raw_call(sw, fn, cols, strand, 6, cig, seqs, caps, g=3, device=device)
                assert rc == 0 and {f: getattr(req, f) for f in FIELDS} == {f: want[f] for f in FIELDS}, (device, which, cap)
                for k in range(2):
                    if caps[k] >= counts[k]:
                        assert arrays[k] == full[k], (device, which, cap, k)
                    else:
                        assert set(arrays[k]) == {0xab}, (device, which, cap, k)
        for null in ((0,), (1,), (0, 1)):
            rc, req, *arrays = raw_call(sw, fn, cols, strand, 6, cig, seqs, counts, g=3, null=null, device=device)
            assert rc == 0 and {f: getattr(req, f) for f in FIELDS} == {f: want[f] for f in FIELDS}, (device, null)
            for k in range(2):
                assert arrays[k] == full[k] if k not in null else set(arrays[k]) == {0xab}, (device, null, k)


def test_the_rows_against_the_resolved_cigars_on_the_device(sw, random_entries):
    """split_gap = 0: the columns whose two row bytes are equal after norm and are no N number exactly swg_eqx_records' matches on the
    same set, and `aligned` is its `columns`."""
    from sweepga_amd.eqx import eqx_records
    from sweepga_amd.maf import maf_records
    cols, strand, cig, seqs = random_entries
    ctx = sw.default_context()
    recs = sorted(cig)
    got = maf_records(ctx, cols, strand, 6, recs, [cig[i] for i in recs], seqs)
    eqx = eqx_records(ctx, cols, strand, 6, recs, [cig[i] for i in recs], seqs)
    code = np.full(256, 4, dtype=np.uint8)
    for k, ch in enumerate(b"ACGT"):
        code[ch] = code[ch | 0x20] = k
    matches = 0
    for b in range(len(got.blocks)):
        t_row, q_row = (np.frombuffer(r, dtype=np.uint8) for r in got.rows(b))
        # ('-' in a row is a gap or a '-' of the sequence itself: norm makes both N, and neither is a match)
        matches += int(((code[t_row] == code[q_row]) & (code[t_row] != 4)).sum())
    assert matches == eqx.matches > 10_000 and got.aligned == eqx.columns and got.usable == eqx.usable == 3000


# ---- the PAF seam, the Python class and the command line ---------------------------------------------------------------------------------
def reparse(text):
    """The blocks of a MAF text, each `s` line's size held against its row without the gaps (the sequences hold no '-' of their own),
    the score against the columns without a gap in either row -> the number of blocks"""
    assert text.startswith(mm.HEADER)
    blocks = text[len(mm.HEADER):].split("\n\n")
    assert blocks[-1] == ""
    for blk in blocks[:-1]:
        a, t, q = blk.split("\n")
        assert a.startswith("a score=") and int(a[8:]) >= 1
        for ln in (t, q):
            f = ln.split(" ")
            assert len(f) == 7 and f[0] == "s" and f[4] in "+-" and int(f[2]) + int(f[3]) <= int(f[5])
            assert int(f[3]) == len(f[6]) - f[6].count("-"), ln[:80]
        ft, fq = t.split(" "), q.split(" ")
        assert len(ft[6]) == len(fq[6]) and ft[4] == "+"
        assert int(a[8:]) == sum(x != "-" and y != "-" for x, y in zip(ft[6], fq[6])) and not any(x == y == "-" for x, y in zip(ft[6], fq[6]))
    return len(blocks) - 1


def test_write_the_python_class_and_the_command_line_for_every_batch_size(sw, tmp_path):
    from sweepga_amd import build
    text, kept, fasta = vcf_paf()
    fasta = [(nm, seq.replace(b"-", b"N")) for nm, seq in fasta]      # (no '-' of the sequences' own: reparse tells bases from gaps by it)
    assert any(ch in seq for _, seq in fasta for ch in b"RYKMBDHV") and any(seq != seq.upper() for _, seq in fasta)
    st = kept.astype(np.uint8)
    fa, fa2 = tmp_path / "a.fa", tmp_path / "b.fa"
    write_fasta(fa, fasta[:1])
    write_fasta(fa2, fasta[1:], width=80)
    files = [str(fa), str(fa2)]
    out = tmp_path / "e.maf"
    one_record = max(mm.batch_costs(text, None, 0))
    with sw.PafFile(text=text) as paf:
        for set_, status in ((0, None), (1, st), (0, st)):
            n_records = 17 if set_ == 0 else int(kept.sum())
            for g in (0, 2):
                want = mm.paf_text(text, kept, fasta, set_, g)
                assert want[1]["usable"] >= 5 and want[1]["untagged"] == 1 and want[1]["bad"] >= 1 and want[1]["no_sequence"] == 1 + (set_ == 0)
                assert want[1]["blocks"] >= want[1]["usable"] - 1 and (g == 0 or want[1]["breakers"] >= 3) and reparse(want[0]) == want[1]["blocks"]
                for batch in (1, one_record, 40, 0):
                    got = sw.Maf.from_paf(paf, status, fasta=files, set=set_, split_gap=g, batch_bytes=batch)
                    assert reparse(got.text) == got.counts["blocks"], (set_, g, batch)      # the library's own text, whatever the model says
                    assert got.text == want[0], (set_, g, batch)
                    assert {k: v for k, v in got.counts.items() if k != "batches"} == want[1]
                    assert sw.Maf.write_paf(paf, status, out, fasta=files, set=set_, split_gap=g, batch_bytes=batch) == got.counts
                    assert reparse(out.read_text()) == got.counts["blocks"] and out.read_text() == want[0]
                    assert 1 <= got.counts["batches"] <= n_records and (batch != 1 or got.counts["batches"] == n_records) and (batch or got.counts["batches"] == 1)
        short = sw.Maf.from_paf(paf, st, fasta=[str(fa)])                                    # the second file is missing: its sequences are absent
        assert short.counts["usable"] == 0 and short.counts["no_sequence"] > 5 and short.text == mm.HEADER
        write_fasta(fa2, [(fasta[1][0], fasta[1][1][:-1])])
        off = sw.Maf.from_paf(paf, st, fasta=files)
        assert off.counts["length_mismatch"] == 1 and off.counts == dict(short.counts, length_mismatch=1) and off.text == short.text
    # the command line over generated records: the output PAF does not change, the MAF is the model's
    rng = np.random.default_rng(12)
    cols, strand, genome, cig, seqs = vm.random_case(rng, 2_000, n_targets=4, n_queries=4, n_ops=10, genomes=3, iupac=0.0)
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
    inp, plain, outp = (tmp_path / nm for nm in ("in.paf", "plain.paf", "out.paf"))
    inp.write_text(big, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-jump", "10k", "--scaffold-mass", "2k"]
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), *flags, "--quiet"], capture_output=True)
    assert r0.returncode == 0 and plain.stat().st_size > 0, r0.stderr
    from tests.test_gpu_intervals import kept_mask
    kept = kept_mask(big, plain.read_bytes().decode())
    for extra, set_, g in (([], 1, 0), (["--maf-set", "all", "--maf-split-gap", "3", "--maf-batch", "2k"], 0, 3)):
        want, c = mm.paf_text(big, kept, records, set_, g)
        r = subprocess.run([build.CLI, str(inp), "--output-file", str(outp), "--maf", str(out), "--maf-fasta", str(big_fa), *extra, *flags], capture_output=True)
        assert r.returncode == 0 and r.stdout == b"" and outp.read_bytes() == plain.read_bytes(), r.stderr
        assert reparse(out.read_text()) == c["blocks"] > 100      # the command line's own file
        assert out.read_text() == want and c["records"] > 100 and c["usable"] > c["records"] // 3
        assert ("--maf: %d blocks of %d records (%d usable): %d columns, %d aligned; %d breakers over %d target and %d query bases, %d runs of gaps only; "
                "%d entries without sequence, %d out of sequence, %d bad, %d without a cg:Z: tag, %d sequences of another length"
                % (c["blocks"], c["records"], c["usable"], c["columns"], c["aligned"], c["breakers"], c["skipped_t"], c["skipped_q"], c["gap_only"],
                   c["no_sequence"], c["out_of_sequence"], c["bad"], c["untagged"], c["length_mismatch"])) in r.stderr.decode()
    out.unlink()
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(outp), "--maf", str(out), "--maf-fasta", str(big_fa), "--no-filter", "--quiet"], capture_output=True)
    assert r.returncode == 0 and reparse(out.read_text()) > 500 and out.read_text() == mm.paf_text(big, None, records, 0)[0], r.stderr
