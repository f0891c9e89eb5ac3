"""The divergence track without a GPU: the model of tests/divergence_model.py against windows worked out by hand on both axes and
both strands, its four invariants on random inputs (the overlap per entry and window, the windows report, the difference list's
sums, the base-exact lift of every window), and the host side of the feature -- header, ctypes mirrors, exported symbols, the
no-device paths and refusals of swg_paf_divergence and of the record seams, the usage errors of --divergence, and the formatters
and the batch merge under the host sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import divergence_model as vm
from tests import lift_exact_model as em
from tests import lift_model as lm
from tests.test_lift_cpu import REBASED
from tests.test_ucsc_chain_cpu import mixed_paf, random_cigar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 100
OTHER = 5000      # where the side that is not the axis starts, on the other sequence


def hand_record(text, axis, a):
    """(q_start, q_end, t_start, t_end) of a record whose axis side starts at a and whose sides are what the ops add up to."""
    Lq, Lt = em.advances(em.parse(text)[1])
    return (OTHER, OTHER + Lq, a, a + Lt) if axis else (a, a + Lq, OTHER, OTHER + Lt)


def cells(**kw):
    return kw


# (what, CIGAR, axis, minus, where the axis side starts, {window: the non-zero fields}) -- every number below is worked out by hand
HAND = [
    # X: wholly inside a window, cut by a border, ending exactly on a border, starting exactly on one
    ("X inside", "50=3X47=", 1, 0, 100, {1: cells(aligned=100, matches=97, mismatches=3, mismatch_runs=1)}),
    ("X cut", "48=4X48=", 1, 0, 150, {1: cells(aligned=50, matches=48, mismatches=2, mismatch_runs=1), 2: cells(aligned=50, matches=48, mismatches=2)}),
    ("X ends on a border", "46=4X50=", 1, 1, 150, {1: cells(aligned=50, matches=46, mismatches=4, mismatch_runs=1), 2: cells(aligned=50, matches=50)}),
    ("X starts on a border", "50=4X46=", 1, 0, 150, {1: cells(aligned=50, matches=50), 2: cells(aligned=50, matches=46, mismatches=4, mismatch_runs=1)}),
    # on the query axis a '-' record walks downwards: 48= lies on 249 .. 202, the X on 201 .. 198 (its lowest base in window 1)
    ("X cut, query -", "48=4X48=", 0, 1, 150, {1: cells(aligned=50, matches=48, mismatches=2, mismatch_runs=1), 2: cells(aligned=50, matches=48, mismatches=2)}),
    ("X cut, query - uneven", "10=4X86=", 0, 1, 112, {2: cells(aligned=12, matches=10, mismatches=2), 1: cells(aligned=88, matches=86, mismatches=2, mismatch_runs=1)}),
    # D and N on the target axis consume axis bases against a gap
    ("D inside", "10=5D10=", 1, 0, 310, {3: cells(aligned=20, matches=20, unaligned=5, indels=1)}),
    ("D cut", "40=20D40=", 1, 0, 150, {1: cells(aligned=40, matches=40, unaligned=10, indels=1), 2: cells(aligned=40, matches=40, unaligned=10)}),
    ("D ends on a border", "30=20D50=", 1, 0, 150, {1: cells(aligned=30, matches=30, unaligned=20, indels=1), 2: cells(aligned=50, matches=50)}),
    ("N inside", "10=5N10=", 1, 0, 410, {4: cells(aligned=20, matches=20, unaligned=5, indels=1)}),
    ("N ends on a border", "30=20N50=", 1, 1, 150, {1: cells(aligned=30, matches=30, unaligned=20, indels=1), 2: cells(aligned=50, matches=50)}),
    ("N over three windows", "10=230N10=", 1, 0, 160, {1: cells(aligned=10, matches=10, unaligned=30, indels=1), 2: cells(unaligned=100),
                                                      3: cells(unaligned=100), 4: cells(aligned=10, matches=10)}),
    # ... and are a point on the query axis: p = q_start + x on '+', q_end - x on '-'
    ("D point, query +", "30=20D50=", 0, 0, 150, {1: cells(aligned=50, matches=50, inserted=20, indels=1), 2: cells(aligned=30, matches=30)}),
    ("D point, query -", "30=20D50=", 0, 1, 150, {1: cells(aligned=50, matches=50), 2: cells(aligned=30, matches=30, inserted=20, indels=1)}),
    ("N point inside, query +", "10=5N10=", 0, 0, 610, {6: cells(aligned=20, matches=20, inserted=5, indels=1)}),
    # '-': 50= on 249 .. 200, the D at p = q_end - 50 = 200 (the first base of window 2), 50= on 199 .. 150
    ("D point on a border, query -", "50=6D50=", 0, 1, 150, {1: cells(aligned=50, matches=50), 2: cells(aligned=50, matches=50, inserted=6, indels=1)}),
    # I on the target axis is a point, on the query axis an extent
    ("I point on a border", "50=7I50=", 1, 0, 150, {1: cells(aligned=50, matches=50), 2: cells(aligned=50, matches=50, inserted=7, indels=1)}),
    ("I inside, query +", "10=4I10=", 0, 0, 510, {5: cells(aligned=20, matches=20, unaligned=4, indels=1)}),
    ("I cut, query +", "48=4I48=", 0, 0, 150, {1: cells(aligned=48, matches=48, unaligned=2, indels=1), 2: cells(aligned=48, matches=48, unaligned=2)}),
    ("I ends on a border, query +", "46=4I50=", 0, 0, 150, {1: cells(aligned=46, matches=46, unaligned=4, indels=1), 2: cells(aligned=50, matches=50)}),
    # '-': 40= on 249 .. 210, the I on 209 .. 206, 56= on 205 .. 150
    ("I inside, query -", "40=4I56=", 0, 1, 150, {1: cells(aligned=50, matches=50), 2: cells(aligned=46, matches=46, unaligned=4, indels=1)}),
    # = and M over three windows
    ("= over three windows", "250=", 1, 0, 150, {1: cells(aligned=50, matches=50), 2: cells(aligned=100, matches=100), 3: cells(aligned=100, matches=100)}),
    ("M over three windows", "250M", 0, 1, 150, {1: cells(aligned=50, m_columns=50), 2: cells(aligned=100, m_columns=100), 3: cells(aligned=100, m_columns=100)}),
    # a CIGAR that begins with I (p = a) and one that ends with I (p = b: the window of b - 1)
    ("begins with I", "5I100=", 1, 0, 200, {2: cells(aligned=100, matches=100, inserted=5, indels=1)}),
    ("ends with I", "100=5I", 1, 0, 100, {1: cells(aligned=100, matches=100, inserted=5, indels=1)}),
    ("ends with D, query +", "100=5D", 0, 0, 100, {1: cells(aligned=100, matches=100, inserted=5, indels=1)}),
    ("begins with D, query -", "5D100=", 0, 1, 100, {1: cells(aligned=100, matches=100, inserted=5, indels=1)}),      # p = q_end = b
    # an I directly followed by a D, on a border
    ("I then D on a border", "50=3I4D46=", 1, 0, 150, {1: cells(aligned=50, matches=50), 2: cells(aligned=46, matches=46, unaligned=4, inserted=3, indels=2)}),
    ("I then D, query +", "50=3I4D46=", 0, 0, 150, {1: cells(aligned=50, matches=50), 2: cells(aligned=46, matches=46, unaligned=3, inserted=4, indels=2)}),
    # S / H / P and zero-length ops add nothing
    ("S H P", "5S2H50=3P0X0I0D4S", 1, 0, 700, {7: cells(aligned=50, matches=50)}),
    ("mixed", "2X3M1=2X", 1, 0, 896, {8: cells(aligned=4, mismatches=2, m_columns=2, mismatch_runs=1), 9: cells(aligned=4, matches=1, mismatches=2, m_columns=1, mismatch_runs=1)}),
]


def nonzero(table):
    return {k: {f: v for f, v in c.items() if v} for k, c in table.items() if any(c.values())}


def test_model_against_windows_worked_out_by_hand():
    for what, text, axis, minus, a, want in HAND:
        rec = hand_record(text, axis, a)
        got = vm.entry_table(text, axis, minus, *rec, W)
        assert nonzero(got) == want, what
        b = rec[3] if axis else rec[1]
        vm.check_entry(got, a, b, W)
        if axis:      # the target axis does not look at the strand
            assert nonzero(vm.entry_table(text, axis, 1 - minus, *rec, W)) == want, what
    # p = b = seq_len in a partial last window: the window of b - 1
    got = vm.entry_table("50=5I", 1, 0, OTHER, OTHER + 55, 1000, 1050, W)
    assert nonzero(got) == {10: cells(aligned=50, matches=50, inserted=5, indels=1)}


def hand_inputs(axis, seq_len=1000, second=False):
    """The hand cases of one axis as records of sequence 0 (genome 0) against sequence 1 (genome 1), then -- `second` -- the same on
    sequence 2 (genome 2, 20 bases longer): (cols, strand, seq_len, genome, cigars, the summed expectation per (seq, window))."""
    cases = [h for h in HAND if h[2] == axis]
    cols, strand, cig, want = {k: [] for k in lm.COLS}, [], {}, {}
    for s in ((0, 2) if second else (0,)):
        for what, text, _, minus, a, cells_ in cases:
            rec = hand_record(text, axis, a)
            ids = (1, s) if axis else (s, 1)
            for k, v in zip(lm.COLS, ids + rec):
                cols[k].append(v)
            cig[len(strand)] = text
            strand.append(minus)
            for k, c in cells_.items():
                acc = want.setdefault((s, k), dict.fromkeys(vm.FIELDS, 0))
                for f, v in c.items():
                    acc[f] += v
        # p = b = seq_len: the window of b - 1, a partial one when seq_len is no multiple of W
        length = seq_len + (20 if s else 0)
        rec = hand_record("20=5I" if axis else "20=5D", axis, length - 20)
        for k, v in zip(lm.COLS, ((1, s) if axis else (s, 1)) + rec):
            cols[k].append(v)
        cig[len(strand)] = "20=5I" if axis else "20=5D"
        strand.append(0)
        acc = want.setdefault((s, (length - 1) // W), dict.fromkeys(vm.FIELDS, 0))
        for f, v in cells(aligned=20, matches=20, inserted=5, indels=1).items():
            acc[f] += v
    lens = [seq_len, 10_000, seq_len + 20]
    return {k: np.array(v, dtype=np.uint32) for k, v in cols.items()}, np.array(strand, dtype=np.uint8), lens, [0, 1, 2], cig, want


def check_hand_rows(rows, want, W_=W):
    seen = set()
    for r in rows:
        key = (int(r["seq"]), int(r["start"]) // W_)
        cell = want.get(key, dict.fromkeys(vm.FIELDS, 0))
        assert {f: int(r[f]) for f in vm.FIELDS} == cell, key
        seen.add(key)
    assert set(want) <= seen


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("seq_len", [1000, 1050])
def test_hand_cases_as_one_table(axis, seq_len):
    for second in (False, True):
        cols, strand, lens, genome, cig, want = hand_inputs(axis, seq_len, second)
        got = vm.divergence(cols, strand, lens, genome, cig, axis=axis, window=W)
        assert len(got["rows"]) == (seq_len + W - 1) // W + ((seq_len + 20 + W - 1) // W if second else 0)
        check_hand_rows(got["rows"], want)
        assert got["usable"] == len(cig) and got["seqs"]["entries"].tolist() == [len(cig) // (1 + second)] * (1 + second)
        assert (got["rows"]["end"][got["rows"]["seq"] == 0][-1]) == seq_len
        vm.check_windows(got, cols, lens, genome, None, 0, axis, W)
        vm.check_diffs(got, cols, strand, genome, 3, cig)
        assert vm.check_lift(got, cols, strand, cig, axis, W) >= len(cig)


def one(text, rec, strand=0, genome=(0, 1), seq_len=(1000, 10_000), **kw):
    cols = {k: np.array([v], dtype=np.uint32) for k, v in zip(lm.COLS, (0, 1) + tuple(rec))}
    return vm.divergence(cols, np.array([strand], dtype=np.uint8), list(seq_len), list(genome), {0: text} if text is not None else {}, **kw)


def test_states_sets_and_who_takes_part():
    zero = dict.fromkeys(vm.FIELDS, 0)
    # each of the five states: the sequence is listed, its rows are all zero, records > entries = 0
    for text, rec, state in (("5=x5=", (600, 610, 6000, 6010), 1), ("4294967296D10=", (620, 630, 6020, 6030), 2), ("9=1X", (640, 651, 6040, 6050), 4),
                             ("9=1X", (660, 670, 6060, 6071), 8), ("", (680, 690, 6080, 6090), 16), (None, (680, 690, 6080, 6090), None)):
        got = one(text, rec, window=W)
        assert got["state"] == ([state] if state is not None else []) and got["usable"] == 0 and got["cigar_bad"] == (state in (1, 2, 4, 8))
        assert len(got["rows"]) == 10 and not any(got["rows"][f].any() for f in vm.FIELDS + ("n",))
        assert [tuple(int(v) for v in e) for e in got["seqs"]] == [(0, 10, 1, 0) + (0,) * 8]
    good, rec = "4=1X5=", (95, 105, 6000, 6010)
    base = one(good, rec, window=W)
    assert base["usable"] == 1 and base["rows"]["n"].tolist() == [1, 1] + [0] * 8
    assert {f: base["rows"][f][:2].tolist() for f in ("aligned", "matches", "mismatches", "mismatch_runs")} == dict(
        aligned=[5, 5], matches=[4, 5], mismatches=[1, 0], mismatch_runs=[1, 0])
    assert tuple(int(v) for v in base["seqs"][0]) == (0, 10, 1, 1, 10, 9, 1, 0, 0, 0, 1, 0)
    # a record outside the set lists nothing; inside the set with status it does
    assert len(one(good, rec, window=W, kept=[0], set_=1)["rows"]) == 0 and one(good, rec, window=W, kept=[0], set_=1)["state"] == [0]
    assert one(good, rec, window=W, kept=[1], set_=1)["rows"].tobytes() == base["rows"].tobytes()
    assert one(good, rec, window=W, kept=[0], set_=0)["rows"].tobytes() == base["rows"].tobytes()
    # intra-genome, and excluded by other_genome
    assert len(one(good, rec, genome=(3, 3), window=W)["rows"]) == 0
    assert len(one(good, rec, genome=(0, 1), window=W, other_genome=0)["rows"]) == 0
    assert one(good, rec, genome=(0, 1), window=W, other_genome=1)["rows"].tobytes() == base["rows"].tobytes()
    # the target axis lists the target's sequence
    t = one(good, rec, window=W, axis=1)
    assert set(t["rows"]["seq"].tolist()) == {1} and len(t["rows"]) == 100 and int(t["rows"]["aligned"][60]) == 10
    with pytest.raises(ValueError, match="record 0"):
        one(good, (995, 1005, 6000, 6010), window=W)
    assert zero == dict.fromkeys(vm.FIELDS, 0)


def random_inputs(rng, n, n_seq=6, max_start=3_000):
    texts = []
    for _ in range(n):
        t = random_cigar(rng)
        if rng.random() < 0.6:
            t = "%d=" % rng.integers(1, 300) + t + "%d%s" % (rng.integers(1, 9_000 if rng.random() < 0.05 else 200), "=XMDN"[int(rng.integers(0, 5))])
        texts.append(t)
    adv = np.array([em.advances(em.parse(t)[1]) for t in texts], dtype=np.int64)
    qs, ts = rng.integers(0, max_start, n), rng.integers(0, max_start, n)
    cols = {"q_id": rng.integers(0, n_seq, n), "t_id": rng.integers(0, n_seq, n), "q_start": qs, "q_end": qs + adv[:, 0], "t_start": ts, "t_end": ts + adv[:, 1]}
    return {k: np.asarray(v).astype(np.uint32) for k, v in cols.items()}, rng.integers(0, 2, n).astype(np.uint8), texts


@pytest.mark.parametrize("window", [1, 7, 64, 5_000])
def test_the_four_invariants_on_random_inputs(window):
    rng = np.random.default_rng(window)
    n = 150 if window == 1 else 400
    cols, strand, texts = random_inputs(rng, n)
    seq_len = [int(max(cols["q_end"].max(), cols["t_end"].max())) + 3] * 6
    genome = [0, 0, 1, 1, 2, 2]
    kept = rng.random(n) < 0.6
    cig = dict(enumerate(texts))
    lifted = 0
    for axis in (0, 1):
        for set_, other in ((0, None), (1, None), (0, 2)):
            got = vm.divergence(cols, strand, seq_len, genome, cig, kept, set_, axis, window, other)      # (check_entry on every entry)
            assert 0 < got["usable"] <= len(got["takes"]) and (got["rows"]["aligned"] == got["rows"]["matches"] + got["rows"]["mismatches"] + got["rows"]["m_columns"]).all()
            vm.check_diffs(got, cols, strand, genome, 3, cig)
            usable = {i: texts[i] for i in got["takes"] if em.entry_state(texts[i], *(int(v) for v in (cols["q_end"][i] - cols["q_start"][i], cols["t_end"][i] - cols["t_start"][i]))) == 0}
            full = vm.divergence(cols, strand, seq_len, genome, usable, kept, set_, axis, window, other, check=False)
            assert full["usable"] == got["usable"]
            if len(usable) == len(got["takes"]):
                vm.check_windows(full, cols, seq_len, genome, kept, set_, axis, window, other)
            if set_ == 0 and other is None and window > 1:
                lifted += vm.check_lift(got, cols, strand, cig, axis, window)
    assert window == 1 or lifted > 300


def test_the_windows_invariant_on_a_set_whose_entries_are_all_usable():
    rng = np.random.default_rng(5)
    cols, strand, texts = random_inputs(rng, 300)
    texts = [t if em.entry_state(t, int(cols["q_end"][i] - cols["q_start"][i]), int(cols["t_end"][i] - cols["t_start"][i])) == 0 else "" for i, t in enumerate(texts)]
    good = [i for i, t in enumerate(texts) if t]
    part = {k: v[good] for k, v in cols.items()}
    seq_len = [int(max(cols["q_end"].max(), cols["t_end"].max())) + 3] * 6
    kept = rng.random(len(good)) < 0.5
    for axis in (0, 1):
        for set_ in (0, 1):
            for window in (7, 64, 5_000):
                got = vm.divergence(part, strand[good], seq_len, [0, 0, 1, 1, 2, 2], {j: texts[i] for j, i in enumerate(good)}, kept, set_, axis, window)
                vm.check_windows(got, part, seq_len, [0, 0, 1, 1, 2, 2], kept, set_, axis, window)


def test_paf_texts_of_the_model():
    text, kept = mixed_paf()
    # record 9 of the mixed PAF ends beyond its sequence on the query axis: refused, with its number
    with pytest.raises(ValueError, match="record 9"):
        vm.paf_texts(text, kept, 0, 0, 100)
    rows, summary, counts = vm.paf_texts(text, kept, 1, 1, 1000)
    assert counts == dict(records=11, usable=8, bad=1, untagged=1, windows=10, seqs=2)
    # the target axis lists g1#1#q too (the last record's target); per window of g2#1#t: the gaps-only record, G on '+', G on '-', the
    # dropped 10M, H on both strands (a record without a tag beside the second), the last tag 49=1X (a broken tag beside it), 15=
    assert rows == vm.ROWS_HEADER + "".join("\t".join(str(v) for v in r) + "\n" for r in (
        ("g1#1#q", 0, 700, 1, 80, 80, 0, 0, 0, 10, 0, 2), ("g2#1#t", 0, 1000, 1, 0, 0, 0, 0, 3, 5, 0, 2), ("g2#1#t", 1000, 2000, 1, 18, 13, 5, 0, 4, 2, 1, 2),
        ("g2#1#t", 2000, 3000, 1, 18, 13, 5, 0, 4, 2, 1, 2), ("g2#1#t", 3000, 4000) + (0,) * 9, ("g2#1#t", 4000, 5000, 1, 6, 6, 0, 0, 3, 6, 0, 4),
        ("g2#1#t", 5000, 6000, 1, 6, 6, 0, 0, 3, 6, 0, 4), ("g2#1#t", 6000, 7000, 1, 50, 49, 1, 0, 0, 0, 1, 0), ("g2#1#t", 7000, 8000, 1, 15, 15) + (0,) * 6,
        ("g2#1#t", 8000, 9000) + (0,) * 9))
    assert summary == (vm.SUMMARY_HEADER + "g1#1#q\t700\t1\t1\t1\t80\t80\t0\t0\t0\t10\t0\t2\n" + "g2#1#t\t9000\t9\t9\t7\t113\t102\t11\t0\t17\t21\t3\t14\n")
    assert vm.paf_texts("", None, 0) == (vm.ROWS_HEADER, vm.SUMMARY_HEADER, dict(records=0, usable=0, bad=0, untagged=0, windows=0, seqs=0))
    assert vm.paf_texts(text, np.zeros(14, dtype=bool), 1)[:2] == (vm.ROWS_HEADER, vm.SUMMARY_HEADER)
    only = vm.paf_texts(text, kept, 1, 1, 1000, "g3#1")      # only the mappings whose other side is g3#1#: the last record
    assert only[2] == dict(records=11, usable=1, bad=1, untagged=1, windows=1, seqs=1)
    assert only[1] == vm.SUMMARY_HEADER + "g1#1#q\t700\t1\t1\t1\t80\t80\t0\t0\t0\t10\t0\t2\n" and only == vm.paf_texts(text, kept, 1, 1, 1000, "g3#1#")


@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib, divergence
    structs = (("swg_divergence_row", _lib.SwgDivergenceRow), ("swg_divergence_seq", _lib.SwgDivergenceSeq),
               ("swg_divergence_request", _lib.SwgDivergenceRequest), ("swg_divergence_counts", _lib.SwgDivergenceCounts))
    prints = ['printf("%%zu\\n", sizeof(%s));' % name for name, _ in structs]
    prints += ['printf("%%zu\\n", offsetof(%s, %s));' % (name, f) for name, cls in structs for f, _ in cls._fields_]
    prints += ['printf("%u %u %d\\n", SWG_DIVERGENCE_ROWS, SWG_DIVERGENCE_SUMMARY, SWG_ABI_VERSION);']
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(cls) for _, cls in structs] + [getattr(cls, f).offset for _, cls in structs for f, _ in cls._fields_] + [1, 2, 1]
    assert got == want and got[:4] == [80, 88, 104, 56]
    for _, cls in structs:      # no implicit padding
        assert sum(C.sizeof(t) for _, t in cls._fields_) == C.sizeof(cls)
    assert divergence.ROW_DTYPE == vm.ROW_DTYPE and divergence.SEQ_DTYPE == vm.SEQ_DTYPE and divergence.ROW_DTYPE.itemsize == 80
    for dt, cls in ((divergence.ROW_DTYPE, _lib.SwgDivergenceRow), (divergence.SEQ_DTYPE, _lib.SwgDivergenceSeq)):
        assert [dt.fields[f][1] for f, _ in cls._fields_] == [getattr(cls, f).offset for f, _ in cls._fields_]
    assert _lib.DIVERGENCE_SUMS == vm.FIELDS and tuple(f for f, _ in _lib.SwgDivergenceCounts._fields_) == divergence.COUNTS
    assert (divergence.ROWS, divergence.SUMMARY, divergence.ANY) == (1, 2, 2**32 - 1)


def test_symbols_are_exported_and_declared(lib):
    import sweepga_amd
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_divergence_records", "swg_divergence_records_device", "swg_paf_divergence"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    assert lib.swg_abi_version() == 1
    for name in ("Divergence", "DivergenceResult", "divergence_records", "divergence_records_device"):
        assert hasattr(sweepga_amd, name)
    assert os.path.join("host", "divergence_text.cpp") in sweepga_amd.build.SOURCES and "swg_divergence.hip" in sweepga_amd.build.SOURCES


def paf_divergence(lib, paf, status, set_=0, axis=0, window=100, genome=None, batch=0, ctx=None, want=(True, True)):
    """swg_paf_divergence -> (rc, rows text or None, summary text or None, counts)"""
    from sweepga_amd import _lib
    from sweepga_amd._marshal import take_texts, text_slots
    counts = _lib.SwgDivergenceCounts()
    p, n = text_slots(want)
    rc = lib.swg_paf_divergence(ctx, paf.handle, status.ctypes.data if status is not None else None, set_, axis, window, genome, batch, p, n, C.byref(counts))
    if rc != 0:
        assert not p[0] and not p[1] and n[0] == n[1] == 0
        return rc, None, None, None
    texts = [t.decode() if t is not None else None for t in take_texts(lib, p, n, want)]
    return rc, texts[0], texts[1], {k: int(getattr(counts, k)) for k in ("records", "usable", "bad", "untagged", "windows", "seqs", "batches")}


def test_paf_seam_without_a_device(lib):
    """A PAF without records of the set gives the header-only texts and needs no device; the refusals come before a context is looked
    at."""
    from sweepga_amd import Divergence, PafFile, SwgError
    zero = dict.fromkeys(("records", "usable", "bad", "untagged", "windows", "seqs", "batches"), 0)
    for text in ("", "# nothing\nfew\tfields\n"):
        with PafFile(text=text) as paf:
            for st in (None, np.zeros(1, dtype=np.uint8)):
                assert paf_divergence(lib, paf, st) == (0, vm.ROWS_HEADER, vm.SUMMARY_HEADER, zero)
                assert paf_divergence(lib, paf, st, axis=1, window=2**32 - 1, genome=b"no such genome", batch=5) == (0, vm.ROWS_HEADER, vm.SUMMARY_HEADER, zero)
                assert paf_divergence(lib, paf, st, want=(False, True)) == (0, None, vm.SUMMARY_HEADER, zero)
                assert paf_divergence(lib, paf, st, want=(True, False)) == (0, vm.ROWS_HEADER, None, zero)
            got = Divergence.from_paf(paf, None, set="all")
            assert (got.text, got.summary_text, got.counts, got.rows, got.summary) == (vm.ROWS_HEADER, vm.SUMMARY_HEADER, zero, [], [])
    text, kept = mixed_paf()
    with PafFile(text=text) as paf:
        none = np.zeros(paf.n, dtype=np.uint8)
        assert paf_divergence(lib, paf, none, set_=1) == (0, vm.ROWS_HEADER, vm.SUMMARY_HEADER, zero)      # a set that is never in status: no device
        assert Divergence.from_paf(paf, none).text == vm.ROWS_HEADER
        st = kept.astype(np.uint8)
        assert paf_divergence(lib, paf, st, set_=1)[0] == -1 and b"swg_paf_divergence: NULL context" in lib.swg_alnstats_last_error()
        for kw, word in ((dict(set_=2), b"set"), (dict(axis=2), b"axis"), (dict(window=0), b"window size"), (dict(set_=1, genome=b"g9#1"), b"unknown genome 'g9#1'")):
            assert paf_divergence(lib, paf, st, **kw)[0] == -1 and word in lib.swg_alnstats_last_error(), kw
        assert paf_divergence(lib, paf, None, set_=1)[0] == -1 and b"status" in lib.swg_alnstats_last_error()
        assert paf_divergence(lib, paf, st, want=(False, False))[0] == -1 and b"neither text" in lib.swg_alnstats_last_error()
        assert lib.swg_paf_divergence(None, None, None, 0, 0, 100, None, 0, None, None, None) == -1
        with pytest.raises(SwgError):
            Divergence.from_paf(paf, st, set=2)
        with pytest.raises(SwgError):
            Divergence.from_paf(paf, st, window=0)
        with pytest.raises(ValueError):
            Divergence.from_paf(paf, st, axis="sideways")
        with pytest.raises(ValueError):
            Divergence.from_paf(paf, st, window=2**32)
    with PafFile(text=REBASED) as paf:
        with pytest.raises(SwgError) as e:
            Divergence.from_paf(paf, np.ones(1, dtype=np.uint8))
        assert e.value.code == -6 and "2^32" in str(e.value)


def test_record_seams_refuse_without_a_device(lib):
    """A NULL context: there is no CPU path, and nothing the caller owns is touched."""
    from sweepga_amd import _lib
    from sweepga_amd.lift import cigar_set
    cols, strand, _ = lm.parse_paf(mixed_paf()[0])
    rec = _lib.SwgRecords()
    rec.n = len(strand)
    for k, a in cols.items():
        setattr(rec, k, a.ctypes.data)
    rec.strand, rec.n_seq = strand.ctypes.data, 3
    genome, seq_len = np.array([0, 1, 2], dtype=np.uint32), np.array([700, 9000, 95], dtype=np.uint32)
    record, offset, text = cigar_set([0, 2], ["5=2I6=4D5X2=", "10M"])
    cs = _lib.SwgCigarSet()
    cs.record, cs.offset, cs.text, cs.k = record.ctypes.data, offset.ctypes.data, text.ctypes.data, 2
    poison = np.full(80 * 4, 0xab, dtype=np.uint8)
    for fn in (lib.swg_divergence_records, lib.swg_divergence_records_device):
        req = _lib.SwgDivergenceRequest()
        req.want, req.window, req.other_genome, req.capacity, req.rows, req.n_rows, req.usable = 3, 100, 2**32 - 1, 4, poison.ctypes.data, 12345, 77
        assert fn(None, C.byref(rec), seq_len.ctypes.data, genome.ctypes.data, 3, None, C.byref(cs), C.byref(req)) == -1
        assert (poison == 0xab).all() and req.n_rows == 12345 and req.usable == 77


def test_command_line_usage_errors(lib, tmp_path):
    from sweepga_amd import build
    paf = tmp_path / "in.paf"
    paf.write_text(mixed_paf()[0])
    out, rows, summ = tmp_path / "out.paf", tmp_path / "d.tsv", tmp_path / "s.tsv"
    run = lambda *a: subprocess.run([build.CLI, str(paf), "--output-file", str(out), *a], capture_output=True, text=True)      # noqa: E731
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(w in r.stdout for w in ("--divergence FILE", "--divergence-summary FILE", "--divergence-window N",
                                                              "--divergence-axis query|target", "--divergence-genome NAME", "--divergence-set kept|all",
                                                              "--divergence-batch BYTES"))
    need = "need --divergence or --divergence-summary"
    cases = [(["--divergence-window", "1k"], need), (["--divergence-axis", "target"], need), (["--divergence-genome", "g1#1"], need),
             (["--divergence-set", "all"], need), (["--divergence-batch", "4k"], need),
             (["--divergence", str(rows), "--divergence-axis", "both"], "--divergence-axis: query or target"),
             (["--divergence", str(rows), "--divergence-set", "lost"], "--divergence-set: kept or all"),
             (["--divergence", str(rows), "--divergence-window", "0"], "--divergence-window"),
             (["--divergence", str(rows), "--divergence-window", "4294967296"], "--divergence-window"),
             (["--divergence-summary", str(summ), "--divergence-window", "wide"], "--divergence-window"),
             (["--divergence", str(rows), "--divergence-batch", "0"], "--divergence-batch"),
             (["--divergence-summary", str(summ), "--divergence-batch", "many"], "--divergence-batch"),
             (["--divergence", str(rows), "--divergence-genome", ""], "empty value for --divergence-genome"),
             (["--divergence", ""], "empty value for --divergence"), (["--divergence-summary", ""], "empty value for --divergence-summary")]
    for extra, word in cases:
        r = run(*extra)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)
        assert r.stdout == "" and not out.exists() and not rows.exists() and not summ.exists(), extra
    # no record at all: the headers, without a device, after --no-filter
    empty = tmp_path / "empty.paf"
    empty.write_text("")
    r = subprocess.run([build.CLI, str(empty), "--no-filter", "--divergence", str(rows), "--divergence-summary", "-"], capture_output=True, text=True)
    assert r.returncode == 0 and rows.read_text() == vm.ROWS_HEADER and vm.SUMMARY_HEADER in r.stderr, r.stderr
    assert "--divergence: 0 windows on 0 sequences from 0 usable entries of 0 records, 0 bad, 0 without a cg:Z: tag\n" in r.stderr


def test_text_helpers_under_the_host_sanitizers(tmp_path):
    """tests/native/divergence_text_check.cpp: a stand-alone program over csrc/host/divergence_text.cpp, built with the address and
    undefined-behaviour sanitizers; its answers must be the model's byte for byte."""
    exe = str(tmp_path / "divergence_text_check")
    host = os.path.join(ROOT, "sweepga_amd", "csrc", "host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "divergence_text_check.cpp"), os.path.join(host, "divergence_text.cpp"),
                           os.path.join(host, "ucsc_text.cpp"), os.path.join(host, "cigar_text.cpp"), "-lpthread"])
    top32, top64 = 2**32 - 1, 2**64 - 1
    feed, want = [], []
    # rows and summary entries at the ends of every field's range; empty and very long names
    for name, row in (("g1#1#q", (0, 0, 100, 1, 90, 80, 5, 5, 10, 3, 2, 4)), ("", (top32,) * 4 + (top64,) * 8), ("x" * 5000, (0,) * 12), ("a b", (7, top32 - 1, top32, 0) + (top64, 0) * 4)):
        feed += ["R", name, " ".join(str(v) for v in row)]
        r = np.zeros(1, dtype=vm.ROW_DTYPE)
        r[0] = row
        want.append(vm.rows_text(r, {int(row[0]): name}))
    assert want[1] == vm.ROWS_HEADER + "\t" + "\t".join(["4294967295"] * 3 + ["18446744073709551615"] * 8) + "\n"
    for name, length, e in (("g2#1#t", 9000, (1, 90, 9, 7, 82, 76, 6, 0, 17, 15, 2, 10)), ("", top32, (top32, top32) + (top64,) * 10), ("y" * 3000, 0, (0,) * 12)):
        feed += ["S", name, " ".join(str(v) for v in (length,) + e)]
        s = np.zeros(1, dtype=vm.SEQ_DTYPE)
        s[0] = e
        want.append(vm.summary_text(s, {int(e[0]): name}, {int(e[0]): length}))
    assert want[4].endswith("g2#1#t\t9000\t90\t9\t7\t82\t76\t6\t0\t17\t15\t2\t10\n")
    # the merge: three batches against the one-batch result (the entry-derived fields add, the keys stay); sums beyond 2^32
    rng = np.random.default_rng(33)
    keys = [(s, k * 100, min((k + 1) * 100, 250)) for s in (0, 3) for k in range(3)]
    parts = [[key + tuple(int(v) for v in rng.integers(0, 2**40, 9)) for key in keys] for _ in range(3)]
    for p in parts:
        for j in range(len(p)):
            p[j] = p[j][:3] + (p[j][3] % 1000,) + p[j][4:]
    total = [keys[j] + tuple(sum(p[j][f] for p in parts) for f in range(3, 12)) for j in range(len(keys))]
    lines = lambda rows: [" ".join(str(v) for v in r) for r in rows]      # noqa: E731
    feed += ["M", "3"] + sum(([str(len(p))] + lines(p) for p in parts), [])
    want.append("\n".join(lines(total)) + "\n--\n")
    feed += ["M", "1", str(len(total))] + lines(total)
    want.append("\n".join(lines(total)) + "\n--\n")
    feed += ["M", "2", "0", "0"]                                               # no window at all
    want.append("--\n")
    for wrong in ([(0, 0, 100) + (1,) * 9, (0, 100, 201) + (1,) * 9], [(0, 0, 100) + (1,) * 9, (1, 100, 200) + (1,) * 9], [(0, 0, 100) + (1,) * 9],
                  [(0, 0, 100) + (1,) * 9, (0, 100, 200) + (1,) * 9, (0, 200, 300) + (1,) * 9]):      # an end, a sequence, a count that disagree
        first = [(0, 0, 100) + (1,) * 9, (0, 100, 200) + (1,) * 9]
        feed += ["M", "2", "2"] + lines(first) + [str(len(wrong))] + lines(wrong)
        want.append("refused\n--\n")
    sparts = [[(s, 3, 5) + tuple(int(v) for v in rng.integers(0, 2**40, 9)) for s in (0, 3)] for _ in range(3)]
    stotal = [(s, 3, 5) + tuple(sum(p[j][f] for p in sparts) for f in range(3, 12)) for j, s in enumerate((0, 3))]
    feed += ["Q", "3"] + sum(([str(len(p))] + lines(p) for p in sparts), [])
    want.append("\n".join(lines(stotal)) + "\n--\n")
    for wrong in ((0, 3, 6), (0, 4, 5), (1, 3, 5)):                              # records, windows, the sequence disagree
        feed += ["Q", "2", "1", " ".join(str(v) for v in (0, 3, 5) + (1,) * 9), "1", " ".join(str(v) for v in wrong + (1,) * 9)]
        want.append("refused\n--\n")
    r = subprocess.run([exe], input="\n".join(feed) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert r.stdout == "".join(want)


def test_the_rules_of_the_walk_header_on_a_cpu(tmp_path):
    """tests/native/divergence_walk_check.cpp: csrc/swg_divergence_walk.h as a host compiler takes it, under the sanitizers, against
    the model: the hand cases and random CIGARs on both axes and strands, behind earlier ops so that the prefix sums do not start at 0,
    and near 2^32 so that the origin's arithmetic wraps."""
    exe = str(tmp_path / "divergence_walk_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "divergence_walk_check.cpp")])
    rng = np.random.default_rng(44)
    cases = [(text, axis, minus, hand_record(text, axis, a), W, 0) for _, text, axis, minus, a, _ in HAND]
    for _ in range(600):
        text = "%d=" % rng.integers(1, 300) + random_cigar(rng) + "%d%s" % (rng.integers(1, 400), "=XMIDN"[int(rng.integers(0, 6))])
        axis, minus = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        a = int(rng.integers(0, 3_000)) if rng.random() < 0.8 else 2**32 - 1 - max(em.advances(em.parse(text)[1])) - int(rng.integers(0, 9))
        cases.append((text, axis, minus, hand_record(text, axis, a) if a < 2**31 else ((a, a + em.advances(em.parse(text)[1])[0], 7, 7 + em.advances(em.parse(text)[1])[1])
                                                                                       if axis == 0 else (7, 7 + em.advances(em.parse(text)[1])[0], a, a + em.advances(em.parse(text)[1])[1])),
                      int(rng.choice([1, 7, 64, 100, 5_000])), int(rng.integers(0, 50))))
    feed, want = [], []
    fields = ("mismatches", "m_columns", "unaligned", "inserted", "mismatch_runs", "indels")
    for text, axis, minus, rec, window, first in cases:
        ops = em.parse(text)[1]
        feed.append(" ".join(str(v) for v in (axis, minus, rec[0], rec[1], rec[2], window, first, len(ops))) + " " + " ".join("%d %s" % op for op in ops))
        table = vm.entry_table(text, axis, minus, *rec, window)
        lines = ["%d " % k + " ".join(str(table[k][f]) for f in fields) for k in sorted(table) if any(table[k][f] for f in fields)]
        want.append("\n".join(lines + ["--"]) + "\n")
    r = subprocess.run([exe], input="\n".join(feed) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    got = [part + "--\n" for part in r.stdout.split("--\n")[:-1]]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g = "".join(ln + "\n" for ln in g.split("\n") if ln and (ln == "--" or any(int(v) for v in ln.split()[1:])))
        assert g == w, (cases[k], g, w)
