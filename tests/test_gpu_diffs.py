"""The difference list on the device (sweepga_amd/csrc/swg_diffs.hip) against tests/diffs_model.py: in every case the host seam
against the model and the device seam against the host seam -- rows, pairs, spectrum, counts and states, byte for byte.  The shapes
are the smallest at which each part can go wrong: the letter pass's chunk of 16 text bytes at every alignment, the op pass's
work-group of 256 ops and the compaction's tile of 4,096 flags, entries of one op, the LDS genome-pair table's 256 slots, every
spectrum bin; the capacity protocol; a random case; the texts of swg_paf_diffs_write / Diffs.from_paf / --diffs for every batch
size.  Every comparison is exact: integers and bytes.  The model's own assertions (a one-base exact lift per mismatched base) run
where the entries are short; tests/test_diffs_cpu.py runs them on 3,000 random CIGARs."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import diffs_model as dm
from tests import lift_model as lm
from tests.test_gpu_alnstats import filter_cfgs, run_filter
from tests.test_gpu_intervals import kept_mask
from tests.test_gpu_lift import Dev
from tests.test_gpu_lift_exact import corrupt, random_case
from tests.test_gpu_ucsc_chain import pairs, records_of
from tests.test_gpu_wide import Hip
from tests.test_ucsc_chain_cpu import G, H, mixed_paf

pytestmark = pytest.mark.gpu
COLS = lm.COLS
FIELDS = ("n_rows", "n_pairs", "ops", "cigar_bad", "usable")
SNP, INS, DEL, SKIP = dm.SNP, dm.INS, dm.DEL, dm.SKIP


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


def same(a, b):
    return (a.rows.tobytes() == b.rows.tobytes() and a.pairs.tobytes() == b.pairs.tobytes() and a.spectrum.tobytes() == b.spectrum.tobytes()
            and a.state.tobytes() == b.state.tobytes() and all(getattr(a, f) == getattr(b, f) for f in FIELDS))


def both_seams(sw, cols, strand, genome, G_, cig, status=None, set_=0, kinds=15, min_indel=1, ctx=None, shift=0):
    """The result of the host seam, after checking that the device seam gives the same.  shift: the device text starts that many
    bytes behind a 16-byte boundary."""
    from sweepga_amd.diffs import diff_records, diff_records_device
    from sweepga_amd.lift import cigar_set
    ctx = ctx or sw.default_context()
    recs = sorted(cig)
    n_seq = len(genome)
    got = diff_records(ctx, cols, strand, n_seq, genome, G_, recs, [cig[i] for i in recs], status=status, set=set_, kinds=kinds, min_indel=min_indel)
    record, offset, text = cigar_set(recs, [cig[i] for i in recs])
    hip = Hip()
    try:
        dcols = {k: Dev(hip, cols[k], np.uint32) for k in COLS}
        dtext = Dev(hip, np.concatenate([np.zeros(shift, dtype=np.uint8), text]))
        dtext.ptr += shift
        dev = diff_records_device(ctx, dcols, Dev(hip, strand, np.uint8), n_seq, Dev(hip, genome, np.uint32), G_, Dev(hip, record), Dev(hip, offset), dtext,
                                  len(recs), status=Dev(hip, status, np.uint8) if status is not None else None, set=set_, kinds=kinds, min_indel=min_indel)
    finally:
        hip.free()
    assert same(dev, got)
    return got


def compare(got, want, what=""):
    assert got.state.tolist() == want["state"], (what, [(k, a, b) for k, (a, b) in enumerate(zip(got.state.tolist(), want["state"])) if a != b][:8])
    assert {f: getattr(got, f) for f in FIELDS} == {f: want[f] for f in FIELDS}, what
    rows = dm.rows_array(want["rows"])
    if got.rows.tobytes() != rows.tobytes():
        bad = [k for k in range(len(rows)) if got.rows[k].tobytes() != rows[k].tobytes()]
        raise AssertionError((what, len(bad), [(k, tuple(int(v) for v in got.rows[k]), want["rows"][k]) for k in bad[:5]]))
    assert [tuple(int(v) for v in p) for p in got.pairs] == want["pairs"], what
    assert got.pairs.tobytes() == dm.pairs_array(want["pairs"]).tobytes(), what
    assert (got.spectrum == want["spectrum"]).all(), (what, np.argwhere(got.spectrum != want["spectrum"])[:8])


def check(sw, cols, strand, genome, G_, cig, status=None, set_=0, kinds=15, min_indel=1, what="", ctx=None, shift=0, model_checks=True):
    """Both seams against the model."""
    cols = {k: np.asarray(cols[k]).astype(np.uint32) for k in COLS}
    strand = np.asarray(strand).astype(np.uint8)
    genome = np.asarray(genome).astype(np.uint32)
    got = both_seams(sw, cols, strand, genome, G_, cig, status, set_, kinds, min_indel, ctx, shift)
    compare(got, dm.diff_records(cols, strand, genome, G_, cig, None if status is None else np.asarray(status) != 0, set_, kinds, min_indel,
                                 check=model_checks), what)
    return got


def check_texts(sw, texts, what="", strands=None, **kw):
    """One record per CIGAR text, query on sequence 0 (genome 0) and target on sequence 1 (genome 1)."""
    cols, strand, _ = records_of(texts, strands)
    return check(sw, cols, strand, [0, 1], 2, dict(enumerate(texts)), what=what, **kw)


UNITS = ("1X", "2=", "1I", "1=", "1D", "3=", "1N", "1M", "2X", "1=")


def text_of(nbytes, first=0):
    """A CIGAR of exactly nbytes bytes (2 or more) that mixes every letter; an odd length starts with a three-byte op."""
    out, k = ("10D" if nbytes % 2 else ""), first
    while len(out) < nbytes:
        out += UNITS[k % len(UNITS)]
        k += 1
    assert len(out) == nbytes
    return out


# ---- the letter pass -----------------------------------------------------------------------------------------------------------------
def test_hand_cases(sw):
    texts = [G, G, "10M", H, H, "1X3=2X", "2D4=1N", "3N2=2D", "1X1X", "3=0=1X0I2=", "3=0X2=0D0N0I", "2S1H1X3=1X0P4S", "5I3D", "3M1X2M"]
    got = check_texts(sw, texts, "hand", strands=[0, 1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 0, 1, 0])
    q0, t0 = 5, 7                    # records_of: the first record starts there
    assert [tuple(int(v) for v in r) for r in got.rows[:3]] == [(0, INS, t0 + 5, t0 + 5, q0 + 5, q0 + 7, 5, 6), (0, DEL, t0 + 11, t0 + 15, q0 + 13, q0 + 13, 6, 0),
                                                                (0, SNP, t0 + 15, t0 + 20, q0 + 13, q0 + 18, 0, 2)]
    assert [int(r["kind_flags"]) for r in got.rows[3:6]] == [INS | 256, DEL | 256, SNP | 256]
    per_record = np.bincount(got.rows["record"], minlength=len(texts)).tolist()
    assert per_record == [3, 3, 0, 4, 4, 2, 2, 2, 2, 1, 0, 2, 2, 1] and got.usable == len(texts) and got.n_pairs == 1
    assert int(got.pairs["m_columns"][0]) == 15 and int(got.pairs["n_skip"][0]) == 2


def test_an_op_letter_at_every_byte_of_a_chunk_and_chunks_of_digits(sw):
    """The text behind a first entry of 16 .. 31 bytes: every op letter of it lies once on each byte of a 16-byte chunk, the first and
    the last included.  Numbers of 10 digits leave chunks with a single letter; D against N and M against X at equal lengths, which
    the prefix sums cannot tell apart.  (A chunk of digits ONLY cannot lie inside a 10-digit number, 16 digits are a syntax error:
    that chunk is the bad entry's here, beside intact neighbours.)"""
    body = "0000000004X5=0000000003N2=7D1M1X0000000003D0000000004M3I3N"
    for lead in range(16, 32):
        texts = [text_of(lead), body, "00000000000000000000000000000000000000004X", body, "3=3X3M"]
        got = check_texts(sw, texts, "lead %d" % lead, strands=[0, 1, 0, 0, 1])
        assert got.state.tolist() == [0, 0, 1, 0, 0] and got.cigar_bad == 1
        kinds = [int(r["kind_flags"]) & 255 for r in got.rows if r["record"] == 3]
        assert kinds == [SNP, SKIP, DEL, SNP, DEL, INS, SKIP]
        assert int(got.pairs["m_columns"][0]) >= 2 * 5 + 3 and int(got.pairs["snp_bases"][0]) >= 2 * 5 + 3


@pytest.mark.parametrize("nbytes", [15, 16, 17, 4095, 4096, 4097])
def test_texts_around_a_chunk_and_a_tile_on_and_off_a_boundary(sw, nbytes):
    for shift in (0, 5):
        check_texts(sw, [text_of(nbytes)], "one entry", strands=[shift & 1], shift=shift)
        got = check_texts(sw, [text_of(16), text_of(16, 3), text_of(nbytes, 1), text_of(32, 5), text_of(15)], "entry borders on chunk borders", shift=shift)
        assert got.usable == 5 and got.n_rows > 10


# ---- the op pass and the compaction --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_entries_and_row_counts_around_4096(sw, n):
    got = check_texts(sw, [pairs(n, "1=", "1X"), "2=", pairs(n, "1D", "3X"), "1X"], "entries of %d ops" % n, model_checks=False)
    assert got.ops == 2 * n + 2 and np.bincount(got.rows["record"]).tolist() == [n // 2, 0, n, 1]
    got = check_texts(sw, ["3=", "1X" * n, "4="], "%d rows" % n, strands=[0, 1, 0], model_checks=False)      # adjacent runs are not merged
    assert got.n_rows == n and got.rows["left"].max() == 0 and (np.diff(got.rows["t_start"].astype(np.int64)) == 1).all()
    got = check_texts(sw, ["3=", "1X" * n, "4="], "kinds without rows", strands=[0, 1, 0], kinds=INS | DEL, model_checks=False)
    assert got.n_rows == 0 and len(got.rows) == 0 and int(got.pairs["snp_runs"][0]) == n


def test_entries_of_one_op_5000_entries_and_empty_entries(sw):
    texts = [("1=", "2X", "3M", "4I", "5D", "6N", "0X", "7S")[k % 8] for k in range(5_000)]
    for shift in (0, 9):
        got = check_texts(sw, texts, "5000 entries", shift=shift)
        assert got.n_rows == 4 * 625 and got.usable == 5_000 and not got.rows["left"].any() and not got.rows["right"].any()
    got = check_texts(sw, ["", "1X", "", "", "2I1=", "", "5=1D"], "empty entries between")
    assert got.rows["record"].tolist() == [1, 4, 6] and got.usable == 3 and got.state.tolist() == [16, 0, 16, 16, 0, 16, 0]


def test_flanks_never_reach_into_the_neighbouring_entry(sw):
    got = check_texts(sw, ["5=", "1X", "7=", "2I", "9=", "3D", "4=", "1X2=", "2=1X"], "flanks", strands=[0, 0, 0, 1, 1, 1, 0, 0, 0])
    assert got.rows["left"].tolist() == [0, 0, 0, 0, 2] and got.rows["right"].tolist() == [0, 0, 0, 2, 0]


def test_every_state_beside_intact_neighbours(sw):
    good = "4=1X3=1D2=1I2="
    bad = ["5=x5=", "4294967296D10=", "9=1I", "9=1D", "", "7", "X3=", "3=3", "3=\t2=", "1X" * 40 + "y"]
    texts = []
    for b in bad:
        texts += [good, b]
    texts.append(good)
    cols, strand, _ = records_of(texts)
    cols["q_end"][5] = cols["q_start"][5] + 11           # "9=1I": x = 10, the record says 11 -> 4
    cols["t_end"][5] = cols["t_start"][5] + 9
    cols["q_end"][7] = cols["q_start"][7] + 9            # "9=1D": y = 10, the record says 11 -> 8
    cols["t_end"][7] = cols["t_start"][7] + 11
    got = check(sw, cols, strand, [0, 1], 2, dict(enumerate(texts)), what="states")
    assert got.state.tolist()[1::2] == [1, 2, 4, 8, 16, 1, 1, 1, 1, 1] and set(got.state.tolist()[0::2]) == {0}
    assert got.usable == len(bad) + 1 and got.cigar_bad == 9 and got.n_rows == 3 * got.usable
    assert tuple(int(v) for v in got.pairs[0])[2:] == tuple(got.usable * v for v in (1, 12, 11, 0, 1, 1, 1, 1, 1, 1, 0, 0))
    assert set(got.rows["record"].tolist()) == set(range(0, len(texts), 2))


# ---- coordinates -----------------------------------------------------------------------------------------------------------------------
def test_one_cigar_of_100000_ops_on_both_strands(sw):
    """One genome pair whose ops lie across 400 work-groups of the op pass."""
    long = "".join(("2=", "1X", "3=", "2I", "1=", "3D", "1M", "1N")[k % 8] for k in range(100_000))
    got = check_texts(sw, ["2=", long, long, "1X"], "10^5", strands=[0, 0, 1, 1], model_checks=False)
    assert got.ops == 200_002 and got.n_rows == 4 * 25_000 + 1 and got.n_pairs == 1 and int(got.pairs["entries"][0]) == 4
    minus = got.rows[got.rows["record"] == 2]
    assert (np.diff(minus["q_start"].astype(np.int64)) <= 0).all() and (np.diff(minus["t_start"].astype(np.int64)) >= 0).all()


def test_the_largest_op_in_a_sum_that_fits(sw):
    top = 2**32 - 1
    texts = ["4294967295D", "3=4294967290D2=", "4294967295N", "1X4294967294I", "4294967295X"]
    cols = {"q_id": [0] * 5, "t_id": [1] * 5, "q_start": [5, 9, 0, 0, 0], "q_end": [5, 14, 0, top, top], "t_start": [0] * 5, "t_end": [top, top, top, 1, top]}
    for strands in ([0] * 5, [1] * 5):
        got = check(sw, cols, strands, [0, 1], 2, dict(enumerate(texts)), what="2^32 - 1", model_checks=False)      # (no 2^32 columns expanded)
        assert got.state.tolist() == [0] * 5 and got.n_rows == 6
        assert tuple(int(v) for v in got.rows[0])[2:6] == (0, top, 5, 5) and tuple(int(v) for v in got.rows[1])[2:4] == (3, top - 2)
        assert int(got.spectrum[2][32]) == 2 and int(got.spectrum[3][32]) == 1 and int(got.spectrum[1][32]) == 1 and int(got.spectrum[0][32]) == 1


# ---- the summary -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G_, hashed", [(1, False), (2, False), (60, False), (300, False), (60, True)])
def test_genome_pairs_dense_hashed_and_beyond_the_lds_table(sw, monkeypatch, G_, hashed):
    """5,000 entries of one or two ops whose genome pair changes from entry to entry: with 60 and 300 genomes a work-group meets more
    pairs than the 256 slots of its LDS table (dense global table below 4,096 slots, hashed beyond or by the knob)."""
    if hashed:
        monkeypatch.setenv("SWG_DIFFS_HASH", "1")
    rng = np.random.default_rng(G_)
    texts = [("1X", "2I", "1=1X", "3D", "2M", "1N1=")[k % 6] for k in range(5_000)]
    cols, strand, _ = records_of(texts)
    n_seq = max(G_, 2) + 3
    cols["q_id"], cols["t_id"] = rng.integers(0, n_seq, 5_000).astype(np.uint32), rng.integers(0, n_seq, 5_000).astype(np.uint32)
    genome = np.arange(n_seq) % G_
    got = check(sw, cols, strand, genome, G_, dict(enumerate(texts)), what="G = %d" % G_)
    assert got.n_pairs == len(set(zip((genome[cols["q_id"]]).tolist(), (genome[cols["t_id"]]).tolist()))) and got.n_pairs >= min(G_ * G_, 2_000)
    assert int(got.pairs["entries"].sum()) == 5_000


def test_all_four_kinds_in_every_spectrum_bin(sw):
    """Single ops of length 2^(b-1) and 2^b - 1 for b = 1 .. 32: two counts in every bin of every kind, none in bin 0."""
    texts, q_end, t_end = [], [], []
    for letter in "XIDN":
        for b in range(1, 33):
            for l in (1 << (b - 1), (1 << b) - 1):
                texts.append("%d%s" % (l, letter))
                q_end.append(l if letter in "XI" else 0)
                t_end.append(l if letter in "XDN" else 0)
    n = len(texts)
    cols = {"q_id": [0] * n, "t_id": [1] * n, "q_start": [0] * n, "q_end": q_end, "t_start": [0] * n, "t_end": t_end}
    got = check(sw, cols, np.arange(n) % 2, [0, 1], 2, dict(enumerate(texts)), what="spectrum", model_checks=False)
    assert (got.spectrum[:, 1:] == 2).all() and not got.spectrum[:, 0].any() and got.n_rows == n


# ---- the filters ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(7)
    cols, strand, texts = random_case(rng, 600, 4)
    return cols, strand, texts, np.array([0, 1, 1, 2], dtype=np.uint32), (rng.random(600) < 0.6).astype(np.uint8)


def test_every_kinds_mask_min_indel_and_both_sets(sw, small):
    cols, strand, texts, genome, status = small
    every = dict(enumerate(texts))
    base = check(sw, cols, strand, genome, 3, every, what="all kinds")
    assert base.n_pairs == 9 and all(base.spectrum[k].any() for k in range(4))
    for kinds in range(1, 15):
        got = check(sw, cols, strand, genome, 3, every, kinds=kinds, what="kinds %d" % kinds, model_checks=False)
        assert got.n_rows == int(sum(((base.rows["kind_flags"] & 255) == k).sum() for k in (1, 2, 4, 8) if k & kinds))
        assert got.pairs.tobytes() == base.pairs.tobytes() and got.spectrum.tobytes() == base.spectrum.tobytes()
    length = 17
    for min_indel in (0, 1, length, length + 1, 2**32 - 1):
        got = check(sw, cols, strand, genome, 3, every, min_indel=min_indel, what="min_indel %d" % min_indel, model_checks=False)
        lens = np.maximum(got.rows["t_end"] - got.rows["t_start"], got.rows["q_end"] - got.rows["q_start"])
        indel = (got.rows["kind_flags"] & 255) != SNP
        assert int((~indel).sum()) == int(((base.rows["kind_flags"] & 255) == SNP).sum()) and (lens[indel] >= min_indel).all()
        assert (min_indel <= 1) == (got.n_rows == base.n_rows) and (min_indel != length + 1 or (lens[indel] > length).all())
    kept = check(sw, cols, strand, genome, 3, every, status=status, set_=1, what="kept")
    assert kept.usable == int(status.sum()) and 0 < kept.n_rows < base.n_rows
    check(sw, cols, strand, genome, 3, every, status=status, set_=0, what="all, with a status")
    none = check(sw, cols, strand, genome, 3, every, status=np.zeros(600, dtype=np.uint8), set_=1, what="never in status")
    assert (none.n_rows, none.n_pairs, none.usable, none.ops) == (0, 0, 0, base.ops) and not none.spectrum.any() and set(none.state.tolist()) == {0}


# ---- the protocol --------------------------------------------------------------------------------------------------------------------------
def raw_call(sw, fn, cols, strand, genome, G_, cig, caps, set_=0, kinds=15, status=None, ctx=None, null=()):
    """A record seam with caller arrays full of 0xAB -> (rc, request, rows, pairs, spectrum, state bytes)"""
    from sweepga_amd import _lib
    from sweepga_amd.lift import cigar_set
    ctx = ctx or sw.default_context()
    rec = _lib.SwgRecords()
    rec.n = len(strand)
    keep = {k: np.ascontiguousarray(cols[k], dtype=np.uint32) for k in COLS}
    for k, a in keep.items():
        setattr(rec, k, a.ctypes.data)
    rec.strand, rec.n_seq = strand.ctypes.data, len(genome) if genome is not None else 4
    record, offset, text = cig if isinstance(cig, tuple) else cigar_set(sorted(cig), [cig[i] for i in sorted(cig)])
    cs = _lib.SwgCigarSet()
    cs.record, cs.offset, cs.text, cs.k = record.ctypes.data, offset.ctypes.data, text.ctypes.data, len(record)
    arrays = [np.full(size * max(c, 1), 0xab, dtype=np.uint8) for size, c in zip((32, 104), caps)]
    state = np.full(max(len(record), 1), 0xab, dtype=np.uint8)
    spectrum = np.full(4 * 33 * 8, 0xab, dtype=np.uint8)
    req = _lib.SwgDiffRequest()
    req.set, req.kinds, req.min_indel, req.state, req.spectrum, req.n_rows = set_, kinds, 1, state.ctypes.data, spectrum.ctypes.data, 99
    req.row_capacity, req.pair_capacity = caps
    req.rows, req.pairs = (None if k in null else a.ctypes.data for k, a in enumerate(arrays))
    rc = fn(ctx.handle, C.byref(rec), genome.ctypes.data if genome is not None else None, G_, status.ctypes.data if status is not None else None,
            C.byref(cs), C.byref(req))
    return (rc, req) + tuple(a.tobytes() for a in arrays) + (spectrum.tobytes(), state.tobytes())


def test_capacities_with_poisoned_arrays(sw, small):
    cols, strand, texts, genome, _ = small
    lib = sw.default_context().lib
    cig = dict(enumerate(texts))
    want = dm.diff_records(cols, strand, genome, 3, cig, kinds=15, check=False)
    counts = (want["n_rows"], want["n_pairs"])
    full = (dm.rows_array(want["rows"]).tobytes(), dm.pairs_array(want["pairs"]).tobytes())
    assert counts[0] > 600 and counts[1] == 9
    for which in range(2):
        for cap in (0, counts[which] - 1, counts[which]):
            caps = tuple(cap if k == which else counts[k] for k in range(2))
            rc, req, *arrays, spectrum, state = raw_call(sw, lib.swg_diff_records, cols, strand, genome, 3, cig, caps)
            assert rc == 0 and (req.n_rows, req.n_pairs, req.usable) == (counts[0], counts[1], 600) and list(state) == want["state"]
            assert spectrum == want["spectrum"].tobytes()          # written whenever the call succeeds
            for k in range(2):
                if caps[k] < counts[k]:
                    assert set(arrays[k]) == {0xab}, (which, cap, k)      # an array that does not hold its count is left alone
                else:
                    assert arrays[k] == full[k], (which, cap, k)
    rc, req, *arrays, spectrum, state = raw_call(sw, lib.swg_diff_records, cols, strand, genome, 3, cig, counts, null=(0, 1))
    assert rc == 0 and req.n_rows == counts[0] and all(set(a) == {0xab} for a in arrays)


def test_no_entries_a_partial_set_and_records_permuted(sw, small):
    from sweepga_amd.diffs import diff_records
    cols, strand, texts, genome, status = small
    ctx = sw.default_context()
    got = diff_records(ctx, cols, strand, 4, genome, 3, [], [])
    assert (got.n_rows, got.n_pairs, got.ops, got.usable, len(got.rows), len(got.pairs)) == (0, 0, 0, 0, 0, 0) and not got.spectrum.any()
    part = check(sw, cols, strand, genome, 3, {i: texts[i] for i in range(0, 600, 3)}, status=status, set_=1, what="a partial set")
    assert 0 < part.usable < 200
    perm = np.random.default_rng(3).permutation(600)
    pcols = {k: v[perm] for k, v in cols.items()}
    every = check(sw, cols, strand, genome, 3, dict(enumerate(texts)), what="in order", model_checks=False)
    moved = check(sw, pcols, strand[perm], genome, 3, {j: texts[i] for j, i in enumerate(perm)}, what="permuted", model_checks=False)
    assert moved.pairs.tobytes() == every.pairs.tobytes() and moved.spectrum.tobytes() == every.spectrum.tobytes() and moved.n_rows == every.n_rows
    back = moved.rows.copy()
    back["record"] = perm[back["record"]]
    assert sorted(map(bytes, back)) == sorted(map(bytes, every.rows))


def test_refusals(sw, small):
    from sweepga_amd import _lib
    from sweepga_amd.diffs import diff_records, diff_records_device
    from sweepga_amd.lift import cigar_set
    cols, strand, texts, genome, status = small
    ctx = sw.default_context()
    lib = ctx.lib
    good = cigar_set([3, 5, 9], ["1=", "2=", ""])
    bad_sets = [(np.array([3, 3, 9], dtype=np.uint32), good[1], good[2]), (np.array([5, 3, 9], dtype=np.uint32), good[1], good[2]),
                (np.array([3, 5, 600], dtype=np.uint32), good[1], good[2]), (good[0], np.array([0, 4, 2, 4], dtype=np.uint64), good[2]),
                (good[0], np.array([1, 2, 4, 4], dtype=np.uint64), good[2])]
    hip = Hip()
    try:
        dcols = {k: Dev(hip, cols[k], np.uint32) for k in COLS}
        dstrand, dgenome = Dev(hip, strand, np.uint8), Dev(hip, genome, np.uint32)
        for record, offset, text in bad_sets:
            rc, req, rows, prs, spectrum, state = raw_call(sw, lib.swg_diff_records, cols, strand, genome, 3, (record, offset, text), (4, 4))
            assert rc == -1 and set(rows) == set(state) == set(spectrum) == {0xab} and req.n_rows == 99, (record, offset)
            with pytest.raises(sw.SwgError) as e:
                diff_records_device(ctx, dcols, dstrand, 4, dgenome, 3, Dev(hip, record), Dev(hip, offset), Dev(hip, text), 3)
            assert e.value.code == -1, (record, offset)
        dset = [Dev(hip, a) for a in good]
        for kw, word in (({"kinds": 0}, "kinds"), ({"kinds": 16}, "kinds"), ({"set": 2}, "set"), ({"set": 1}, "status")):      # (set 1: KEPT without a status)
            with pytest.raises(sw.SwgError) as e:
                diff_records_device(ctx, dcols, dstrand, 4, dgenome, 3, *dset, 3, **kw)
            assert e.value.code == -1 and word in str(e.value)
            with pytest.raises(sw.SwgError) as e:
                diff_records(ctx, cols, strand, 4, genome, 3, None, good, **kw)
            assert e.value.code == -1 and word in str(e.value)
        with pytest.raises(sw.SwgError) as e:      # a NULL seq_genome
            diff_records_device(ctx, dcols, dstrand, 4, None, 3, *dset, 3)
        assert e.value.code == -1 and "seq_genome" in str(e.value)
        twos = np.full(4, 2, dtype=np.uint32)
        for n_genome in (2, 0):                    # a genome id >= n_genome, on both seams
            with pytest.raises(sw.SwgError) as e:
                diff_records_device(ctx, dcols, dstrand, 4, Dev(hip, twos), n_genome, *dset, 3)
            assert e.value.code == -1 and "genome" in str(e.value)
            rc, req, rows, *_ = raw_call(sw, lib.swg_diff_records, cols, strand, twos, n_genome, good, (4, 4))
            assert rc == -1 and set(rows) == {0xab} and b"genome" in lib.swg_last_error(ctx.handle)
    finally:
        hip.free()
    for fn in (lib.swg_diff_records, lib.swg_diff_records_device):      # k is looked at before any array
        cs = _lib.SwgCigarSet()
        cs.record, cs.offset, cs.text, cs.k = good[0].ctypes.data, good[1].ctypes.data, good[2].ctypes.data, 2**31
        rec = _lib.SwgRecords()
        rec.n, rec.n_seq = 600, 4
        req = _lib.SwgDiffRequest()
        req.kinds = 7
        assert fn(ctx.handle, C.byref(rec), genome.ctypes.data, 3, None, C.byref(cs), C.byref(req)) == -5
    rc, req, rows, *_ = raw_call(sw, lib.swg_diff_records, cols, strand, None, 3, good, (4, 4))
    assert rc == -1 and set(rows) == {0xab} and b"seq_genome" in lib.swg_last_error(ctx.handle)
    with pytest.raises(sw.SwgError) as e:      # a set for no records
        diff_records(ctx, {k: np.zeros(0, dtype=np.uint32) for k in COLS}, np.zeros(0, dtype=np.uint8), 4, genome, 3, [0], ["1="])
    assert e.value.code == -1
    after = check(sw, cols, strand, genome, 3, {3: texts[3]}, what="after the refusals")      # the context is as usable as before
    assert after.usable == 1


def test_a_memory_limit_too_small_is_a_clean_oom(sw, small):
    from sweepga_amd.diffs import diff_records
    cols, strand, texts, genome, _ = small
    ctx = sw.Context(0)
    try:
        long = "1=1I" * 100_000      # 400 kB of text, 2 * 10^5 ops: 32 bytes of prefix sums each, 6.4 MB
        c1 = {"q_id": [0], "t_id": [1], "q_start": [0], "q_end": [200_000], "t_start": [0], "t_end": [100_000]}
        c1 = {k: np.array(v, dtype=np.uint32) for k, v in c1.items()}
        ctx.set_memory_limit(4 << 20)
        with pytest.raises(sw.SwgError) as e:
            diff_records(ctx, c1, np.zeros(1, dtype=np.uint8), 2, [0, 1], 2, [0], [long])
        assert e.value.code == -4
        got = diff_records(ctx, cols, strand, 4, genome, 3, list(range(600)), texts, kinds=15)      # the same context, a call that fits
        compare(got, dm.diff_records(cols, strand, genome, 3, dict(enumerate(texts)), kinds=15, check=False), "under the limit")
        ctx.set_memory_limit(0)
        got = diff_records(ctx, c1, np.zeros(1, dtype=np.uint8), 2, [0, 1], 2, [0], [long])
        assert got.n_rows == 100_000 and tuple(int(v) for v in got.rows[-1]) == (0, INS, 100_000, 100_000, 199_999, 200_000, 1, 0)
        assert tuple(int(v) for v in got.pairs[0]) == (0, 1, 1, 100_000, 100_000, 0, 0, 0, 100_000, 100_000, 0, 0, 0, 0)
    finally:
        ctx.close()


def test_smallest_shapes_on_a_fresh_context(sw):
    """The seams around the kernels at the smallest shapes -- one record; three records -- with and without a status, on a context of
    its own: its first call sizes the arena from the input, the later ones find it sized."""
    texts = [G, "10M", H]
    cols, strand, _ = records_of(texts)
    ctx = sw.Context(0)
    try:
        for n in (1, 3, 1, 3):
            part = {k: v[:n] for k, v in cols.items()}
            for status in (None, np.array([1, 0, 1], dtype=np.uint8)[:n]):
                got = check(sw, part, strand[:n], [0, 1], 2, dict(enumerate(texts[:n])), status=status, set_=0 if status is None else 1, what=f"n = {n}", ctx=ctx)
                assert got.usable == (n if status is None else (n + 1) // 2) and got.rows["record"].tolist()[:3] == [0, 0, 0]
    finally:
        ctx.close()


# ---- the whole path ------------------------------------------------------------------------------------------------------------------------
def test_write_the_python_class_and_the_command_line_for_every_batch_size(sw, tmp_path):
    from sweepga_amd import build
    text, kept = mixed_paf()
    st = kept.astype(np.uint8)
    out, summ = tmp_path / "d.tsv", tmp_path / "s.tsv"
    one_record = len("5=2I6=4D5X2=")
    with sw.PafFile(text=text) as paf:
        for set_, status in ((0, None), (1, st), (0, st)):
            n_records = 14 if set_ == 0 else int(kept.sum())
            for kinds, min_indel in ((("snp", "ins", "del"), 1), (("ins", "del", "skip"), 3), ("snp", 0)):
                want = dm.paf_texts(text, kept, set_, sw.diffs.kinds_mask(kinds), min_indel)
                assert want[2]["rows"] >= 3
                for batch in (1, one_record, 40, 0):
                    got = sw.Diffs.from_paf(paf, status, set=set_, kinds=kinds, min_indel=min_indel, batch_bytes=batch)
                    assert (got.text, got.summary_text) == want[:2], (set_, kinds, batch)
                    assert {k: v for k, v in got.counts.items() if k != "batches"} == want[2]
                    assert sw.Diffs.write_paf(paf, status, out, summ, set=set_, kinds=kinds, min_indel=min_indel, batch_bytes=batch) == got.counts
                    assert out.read_text() == want[0] and summ.read_text() == want[1]
                    assert 1 <= got.counts["batches"] <= n_records and (batch != 1 or got.counts["batches"] == n_records) and (batch or got.counts["batches"] == 1)
                assert len(got.rows) == want[2]["rows"] and len(got.pairs) == (4 if set_ == 0 else 3)
        summary_only = sw.Diffs.write_paf(paf, st, None, summ)                    # the rows are counted and not built
        assert summary_only["rows"] == 20 and summ.read_text() == dm.paf_texts(text, kept, 1)[1]
    # the command line: a real 1:1 filter, the differences of what it keeps; the output PAF and the chain file do not change
    rng = np.random.default_rng(12)
    cols, strand, texts = random_case(rng, 2_000, 6)
    lines = []
    for i in range(2_000):
        f = ["g%d#1#c" % cols["q_id"][i], "400000", str(cols["q_start"][i]), str(cols["q_end"][i]), "-" if strand[i] else "+",
             "g%d#1#c" % cols["t_id"][i], "400000", str(cols["t_start"][i]), str(cols["t_end"][i]), "50", "60", "60"]
        tags = (["tp:A:P", "cg:Z:" + texts[i]], ["cg:Z:" + texts[i], "nm:i:3"], ["tp:A:P"], ["cg:Z:1M", "cg:Z:" + texts[i]], ["cg:Z:"], ["cg:Z:" + texts[i] + "9"])[i % 6]
        lines.append("\t".join(f + tags))
    big = "\n".join(lines) + "\n"
    inp, plain, outp, chain0, chain1 = (tmp_path / nm for nm in ("in.paf", "plain.paf", "out.paf", "plain.chain", "out.chain"))
    inp.write_text(big, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-jump", "10k", "--scaffold-mass", "2k"]
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), "--ucsc-chain", str(chain0), *flags, "--quiet"], capture_output=True)
    assert r0.returncode == 0 and plain.stat().st_size > 0 and chain0.stat().st_size > 0, r0.stderr
    kept = kept_mask(big, plain.read_bytes().decode())
    with sw.PafFile(text=big) as paf:      # every batch size gives the same bytes
        for set_ in (1, 0):
            want = dm.paf_texts(big, kept, set_)
            got = [sw.Diffs.from_paf(paf, kept.astype(np.uint8), set=set_, batch_bytes=b) for b in (1, 100, 4096, 0)]
            assert all((g.text, g.summary_text) == want[:2] for g in got) and all({k: v for k, v in g.counts.items() if k != "batches"} == want[2] for g in got)
            batches = [g.counts["batches"] for g in got]
            assert batches[0] > batches[1] > batches[2] >= batches[3] == 1
    for extra, set_, kinds, min_indel in (([], 1, 7, 1), (["--diffs-set", "all", "--diffs-kinds", "ins,skip,del", "--diffs-min-indel", "10", "--diffs-batch", "2k"], 0, 14, 10)):
        want = dm.paf_texts(big, kept, set_, kinds, min_indel)
        r = subprocess.run([build.CLI, str(inp), "--output-file", str(outp), "--ucsc-chain", str(chain1), "--diffs", str(out), "--diffs-summary", str(summ),
                            *extra, *flags], capture_output=True)
        assert r.returncode == 0 and r.stdout == b"" and outp.read_bytes() == plain.read_bytes() and chain1.read_bytes() == chain0.read_bytes(), r.stderr
        c = want[2]
        assert out.read_text() == want[0] and summ.read_text() == want[1] and c["records"] > 100 and c["rows"] > 100 and c["usable"] > c["records"] // 3
        assert ("--diffs: %d rows of %d usable entries in %d records, %d mismatched, %d inserted, %d deleted bases, %d columns under M ops, %d bad, "
                "%d without a cg:Z: tag\n" % (c["rows"], c["usable"], c["records"], c["snp_bases"], c["ins_bases"], c["del_bases"] + c["skip_bases"],
                                              c["m_columns"], c["bad"], c["untagged"])) in r.stderr.decode()
    out.unlink()
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(outp), "--diffs-summary", str(summ), "--no-filter", "--quiet"], capture_output=True)
    assert r.returncode == 0 and summ.read_text() == dm.paf_texts(big, None, 0)[1] and not out.exists(), r.stderr


def test_20000_records_built_from_random_cigars(sw):
    """5 % of the entries are corrupted, 5 % of the records are left out of the set, a real 1:1 status picks the kept set."""
    rng = np.random.default_rng(9)
    n, n_seq = 20_000, 12
    cols, strand, texts = random_case(rng, n, n_seq)
    lines = []
    for i in range(n):
        lines.append("\t".join(["g%d#1#c" % cols["q_id"][i], "400000", str(cols["q_start"][i]), str(cols["q_end"][i]), "-" if strand[i] else "+",
                                "g%d#1#c" % cols["t_id"][i], "400000", str(cols["t_start"][i]), str(cols["t_end"][i]), "50", "60", "60"]))
    with sw.PafFile(text="\n".join(lines) + "\n") as paf:
        status, _ = run_filter(sw, paf, filter_cfgs(sw)["one_to_one"])
        pcols = {c: paf.column(c).copy() for c in COLS}      # (the handle's ids: names in order of first appearance)
        pstrand, p_seq = paf.column("strand").copy(), int(paf.records.n_seq)
    assert 0 < int((status != 0).sum()) < n
    roll = rng.random(n)
    cig = {i: (corrupt(texts[i], rng) if roll[i] < 0.05 else texts[i]) for i in range(n) if roll[i] >= 0.10 or roll[i] < 0.05}
    genome = np.arange(p_seq) // 2
    usable = []
    for set_ in (0, 1):
        got = check(sw, pcols, pstrand, genome, (p_seq + 1) // 2, cig, status=status, set_=set_, what="random, set %d" % set_, model_checks=set_ == 1)
        assert int((got.state == 0).sum()) >= 0.85 * len(cig) and got.cigar_bad > 0.03 * len(cig)
        assert got.n_pairs == 36 and got.n_rows > got.usable > 0
        usable.append(got.usable)
    assert usable[0] > 15_000 and 0 < usable[1] < usable[0]      # (the entries of records the filter dropped are not usable in the kept set)
