"""The difference list without a GPU: the brute-force model of tests/diffs_model.py against rows worked out by hand and against
the consequences of its definitions on random CIGARs, and the host side of the feature -- header, ctypes mirrors, exported
symbols, the no-device paths and refusals of swg_paf_diffs_write / _text and of the record seams, the usage errors of --diffs,
and the row formatter, the merge of pair sums and the summary text under the host sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import diffs_model as dm
from tests import lift_exact_model as em
from tests import lift_model as lm
from tests.test_lift_cpu import REBASED
from tests.test_ucsc_chain_cpu import G, H, mixed_paf, random_cigar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNP, INS, DEL, SKIP, MINUS = dm.SNP, dm.INS, dm.DEL, dm.SKIP, dm.MINUS


def rows_of(text, minus, qs, qe, ts, te, record=0):
    return [r for r, _ in dm.entry_diffs(text, minus, qs, qe, ts, te, record)[0]]


def test_model_against_rows_worked_out_by_hand():
    #   G = 5=2I6=4D5X2=:  I at x 5 y 5, D at x 13 y 11, X at x 13 y 15
    assert rows_of(G, 0, 100, 120, 1000, 1022) == [(0, INS, 1005, 1005, 105, 107, 5, 6), (0, DEL, 1011, 1015, 113, 113, 6, 0),
                                                    (0, SNP, 1015, 1020, 113, 118, 0, 2)]
    # '-': the query interval of length L at x is [q_end - x - L, q_end - x); rows stay in text order = descending along the query
    assert rows_of(G, 1, 200, 220, 2000, 2022, 7) == [(7, INS | MINUS, 2005, 2005, 213, 215, 5, 6), (7, DEL | MINUS, 2011, 2015, 207, 207, 6, 0),
                                                       (7, SNP | MINUS, 2015, 2020, 202, 207, 0, 2)]
    assert dm.entry_diffs(G, 0, 100, 120, 1000, 1022)[1] == dict(aligned=18, eq=13, m_columns=0, snp_runs=1, snp_bases=5, n_ins=1, ins_bases=2, n_del=1,
                                                                 del_bases=4, n_skip=0, skip_bases=0)
    #   H = 3I4=2I3D2=1I:  I at the first and the last op, an I directly followed by a D (two rows at one target point)
    assert rows_of(H, 0, 400, 412, 4000, 4009) == [(0, INS, 4000, 4000, 400, 403, 0, 4), (0, INS, 4004, 4004, 407, 409, 4, 0),
                                                    (0, DEL, 4004, 4007, 409, 409, 0, 2), (0, INS, 4009, 4009, 411, 412, 2, 0)]
    assert rows_of(H, 1, 500, 512, 5000, 5009) == [(0, INS | MINUS, 5000, 5000, 509, 512, 0, 4), (0, INS | MINUS, 5004, 5004, 503, 505, 4, 0),
                                                    (0, DEL | MINUS, 5004, 5007, 503, 503, 0, 2), (0, INS | MINUS, 5009, 5009, 500, 501, 2, 0)]
    # X, D and N at the first and the last op
    assert rows_of("1X3=2X", 0, 10, 16, 20, 26) == [(0, SNP, 20, 21, 10, 11, 0, 3), (0, SNP, 24, 26, 14, 16, 3, 0)]
    assert rows_of("1X3=2X", 1, 10, 16, 20, 26) == [(0, SNP | MINUS, 20, 21, 15, 16, 0, 3), (0, SNP | MINUS, 24, 26, 10, 12, 3, 0)]
    assert rows_of("2D4=1N", 0, 0, 4, 10, 17) == [(0, DEL, 10, 12, 0, 0, 0, 4), (0, SKIP, 16, 17, 4, 4, 4, 0)]
    assert rows_of("3N2=2D", 1, 0, 2, 10, 17) == [(0, SKIP | MINUS, 10, 13, 2, 2, 0, 2), (0, DEL | MINUS, 15, 17, 0, 0, 2, 0)]
    # adjacent ops of one kind are not merged
    assert rows_of("1X1X", 0, 0, 2, 0, 2) == [(0, SNP, 0, 1, 0, 1, 0, 0), (0, SNP, 1, 2, 1, 2, 0, 0)]
    assert rows_of("2I3I", 0, 0, 5, 9, 9) == [(0, INS, 9, 9, 0, 2, 0, 0), (0, INS, 9, 9, 2, 5, 0, 0)]
    # zero-length ops: no row of their own, and beside a row the flank is 0 (the op DIRECTLY beside it counts)
    assert rows_of("3=0=1X0I2=", 0, 0, 6, 0, 6) == [(0, SNP, 3, 4, 3, 4, 0, 0)]
    assert rows_of("3=0X2=0D0N0I", 0, 0, 5, 0, 5) == []
    # M only: no mismatch is knowable
    assert dm.entry_diffs("10M", 0, 300, 310, 3000, 3010) == ([], dict(aligned=10, eq=0, m_columns=10, snp_runs=0, snp_bases=0, n_ins=0, ins_bases=0,
                                                                       n_del=0, del_bases=0, n_skip=0, skip_bases=0))
    assert rows_of("3M1X2M", 0, 0, 6, 0, 6) == [(0, SNP, 3, 4, 3, 4, 0, 0)]          # an M beside a row is no flank
    # S / H / P at the ends advance nothing and are no flank
    assert rows_of("2S1H1X3=1X0P4S", 0, 10, 15, 20, 25) == [(0, SNP, 20, 21, 10, 11, 0, 3), (0, SNP, 24, 25, 14, 15, 3, 0)]
    # the largest op
    assert rows_of("4294967295D", 0, 5, 5, 0, 2**32 - 1) == [(0, DEL, 0, 2**32 - 1, 5, 5, 0, 0)]


def one_record(text, minus=0, qs=600, qe=610, ts=6000, te=6010):
    cols = {k: np.array([v], dtype=np.uint32) for k, v in zip(lm.COLS, (0, 1, qs, qe, ts, te))}
    return cols, np.array([minus], dtype=np.uint8), {0: text}


def test_model_states_sets_and_filters():
    empty = dict(rows=[], pairs=[], n_rows=0, n_pairs=0, usable=0)
    for text, (qs, qe, ts, te), state in (("5=x5=", (600, 610, 6000, 6010), 1), ("4294967296D10=", (620, 630, 6020, 6030), 2),
                                           ("9=1X", (640, 651, 6040, 6050), 4), ("9=1X", (660, 670, 6060, 6071), 8), ("", (680, 690, 6080, 6090), 16),
                                           ("5=1X9", (0, 6, 0, 6), 1), ("X5=", (0, 6, 0, 6), 1), ("12345678901X", (0, 6, 0, 6), 1),
                                           ("3=1X", (0, 5, 0, 5), 12)):
        cols, strand, cig = one_record(text, 0, qs, qe, ts, te)
        got = dm.diff_records(cols, strand, [0, 1], 2, cig)
        assert got["state"] == [state] and got["cigar_bad"] == (state != 16) and {k: got[k] for k in empty} == empty, text
        assert not got["spectrum"].any()
    cols, strand, cig = one_record("4=1X5=")
    for kept, set_, n in (([1], 1, 1), ([0], 1, 0), ([0], 0, 1)):          # a record outside the set gives nothing
        got = dm.diff_records(cols, strand, [0, 1], 2, cig, np.array(kept), set_)
        assert (got["n_rows"], got["usable"], got["n_pairs"], got["state"]) == (n, n, n, [0])
    assert dm.diff_records(cols, strand, [0, 1], 2, cig)["pairs"] == [(0, 1, 1, 10, 9, 0, 1, 1, 0, 0, 0, 0, 0, 0)]
    # the filters choose rows; the summary and the spectrum count every op
    cols, strand, cig = one_record("1X2=3I2=4D1=8N1=2X", 0, 0, 12, 0, 21)
    want = {SNP: 2, INS: 1, DEL: 1, SKIP: 1}
    base = dm.diff_records(cols, strand, [0, 0], 1, cig, kinds=15)
    assert base["pairs"] == [(0, 0, 1, 9, 6, 0, 2, 3, 1, 3, 1, 4, 1, 8)]
    assert [tuple(np.flatnonzero(base["spectrum"][k])) for k in range(4)] == [(1, 2), (2,), (3,), (4,)]
    for kinds in range(1, 16):
        got = dm.diff_records(cols, strand, [0, 0], 1, cig, kinds=kinds)
        assert got["n_rows"] == sum(n for k, n in want.items() if k & kinds)
        assert got["pairs"] == base["pairs"] and (got["spectrum"] == base["spectrum"]).all()
    for min_indel, n in ((0, 5), (1, 5), (3, 5), (4, 4), (5, 3), (8, 3), (9, 2), (2**32 - 1, 2)):      # never applied to SNP
        assert dm.diff_records(cols, strand, [0, 0], 1, cig, kinds=15, min_indel=min_indel)["n_rows"] == n


def test_the_definitions_hold_on_random_cigars():
    """entry_diffs asserts on every entry: the invariant of the sums, the walked lengths, every mismatched base as a one-base exact
    lift, a match just outside every flank, and the chain file's gaps as the inner indels."""
    rng = np.random.default_rng(32)
    rows = flanked = 0
    for _ in range(3000):
        text = random_cigar(rng)
        if rng.random() < 0.5:
            text = "%d=" % rng.integers(1, 9) + text + "%d=" % rng.integers(1, 9)
        Lq, Lt = em.advances(em.parse(text)[1])
        qs, ts = int(rng.integers(0, 50)), int(rng.integers(0, 50))
        for minus in (0, 1):
            got, sums = dm.entry_diffs(text, minus, qs, qs + Lq, ts, ts + Lt)
            rows += len(got)
            flanked += sum(1 for r, _ in got if r[6] or r[7])
            assert len(got) == sums["snp_runs"] + sums["n_ins"] + sums["n_del"] + sums["n_skip"]
    assert rows > 10000 and flanked > 2000


@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib, diffs
    structs = (("swg_diff_row", _lib.SwgDiffRow), ("swg_diff_pair", _lib.SwgDiffPair), ("swg_diff_request", _lib.SwgDiffRequest),
               ("swg_diff_counts", _lib.SwgDiffCounts))
    prints = ['printf("%%zu\\n", sizeof(%s));' % name for name, _ in structs]
    prints += ['printf("%%zu\\n", offsetof(%s, %s));' % (name, f) for name, cls in structs for f, _ in cls._fields_]
    prints += ['printf("%u %u %u %u %u %d %d\\n", SWG_DIFF_SNP, SWG_DIFF_INS, SWG_DIFF_DEL, SWG_DIFF_SKIP, SWG_DIFF_MINUS, SWG_DIFF_BINS, SWG_ABI_VERSION);']
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(cls) for _, cls in structs] + [getattr(cls, f).offset for _, cls in structs for f, _ in cls._fields_]
    want += [1, 2, 4, 8, 256, 33, 1]
    assert got == want
    assert got[:4] == [32, 104, 104, 120]
    for _, cls in structs:      # no implicit padding
        assert sum(C.sizeof(t) for _, t in cls._fields_) == C.sizeof(cls)
    assert diffs.ROW_DTYPE.itemsize == 32 and diffs.PAIR_DTYPE.itemsize == 104
    for dt, cls in ((diffs.ROW_DTYPE, _lib.SwgDiffRow), (diffs.PAIR_DTYPE, _lib.SwgDiffPair)):
        assert [dt.fields[f][1] for f, _ in cls._fields_] == [getattr(cls, f).offset for f, _ in cls._fields_]
    assert (diffs.SNP, diffs.INS, diffs.DEL, diffs.SKIP, diffs.MINUS, diffs.BINS) == (SNP, INS, DEL, SKIP, MINUS, dm.BINS)
    assert tuple(f for f, _ in _lib.SwgDiffCounts._fields_) == diffs.COUNTS == dm.COUNTS
    assert tuple(f for f, _ in _lib.SwgDiffRow._fields_) == dm.ROW_FIELDS and _lib.DIFF_SUMS == dm.SUMS


def test_symbols_are_exported_and_declared(lib):
    import sweepga_amd
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_diff_records", "swg_diff_records_device", "swg_paf_diffs_write", "swg_paf_diffs_text"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    assert lib.swg_abi_version() == 1
    for name in ("Diffs", "DiffsResult", "diff_records", "diff_records_device"):
        assert hasattr(sweepga_amd, name)
    assert sweepga_amd.diffs.kinds_mask(("snp", "ins", "del")) == 7 and sweepga_amd.diffs.kinds_mask("skip,snp") == 9
    with pytest.raises(ValueError):
        sweepga_amd.diffs.kinds_mask(("snp", "inv"))


def test_the_mixed_paf_of_the_model():
    """Counts worked out by hand: of the 14 records 11 are usable (a missing and an empty tag, one broken CIGAR), G gives an INS, a DEL
    and a SNP row on either strand, H three INS and a DEL, `5I3D` two rows, three CIGARs one row each, `40=5I40=5I` two."""
    text, kept = mixed_paf()
    rows, summary, counts = dm.paf_texts(text, None, 0)
    assert counts == dict(records=14, usable=11, bad=1, untagged=1, rows=21, snp_runs=4, snp_bases=12, n_ins=11, ins_bases=31, n_del=6, del_bases=19,
                          n_skip=0, skip_bases=0, m_columns=10)
    assert rows.startswith(dm.ROWS_HEADER + "g2#1#t\t1005\t1005\tg1#1#q\t105\t107\t+\tINS\t2\t5\t6\t0\n"
                           "g2#1#t\t1011\t1015\tg1#1#q\t113\t113\t+\tDEL\t4\t6\t0\t0\ng2#1#t\t1015\t1020\tg1#1#q\t113\t118\t+\tSNP\t5\t0\t2\t0\n"
                           "g2#1#t\t2005\t2005\tg1#1#q\t213\t215\t-\tINS\t2\t5\t6\t1\n")
    assert "g2#1#t\t6049\t6050\tg1#1#q\t649\t650\t+\tSNP\t1\t49\t0\t6\n" in rows                       # the LAST tag of the line counts
    assert "g2#1#t\t204\t206\tg2#1#t\t106\t106\t-\tDEL\t2\t4\t6\t10\n" in rows                          # the intra-sequence record
    assert rows.endswith("g1#1#q\t40\t40\tg3#1#s\t50\t55\t-\tINS\t5\t40\t40\t13\ng1#1#q\t80\t80\tg3#1#s\t5\t10\t-\tINS\t5\t40\t0\t13\n")
    assert summary == (dm.SUMMARY_HEADER + "g1#1#\tg2#1#\t8\t123\t102\t10\t3\t11\t9\t21\t5\t17\t0\t0\ng2#1#\tg2#1#\t1\t10\t10\t0\t0\t0\t0\t0\t1\t2\t0\t0\n"
                       "g3#1#\tg1#1#\t1\t80\t80\t0\t0\t0\t2\t10\t0\t0\t0\t0\ng3#1#\tg2#1#\t1\t9\t8\t0\t1\t1\t0\t0\t0\t0\t0\t0\n"
                       "#spectrum\tSNP\t1\t1\t2\n#spectrum\tSNP\t4\t7\t2\n#spectrum\tINS\t1\t1\t2\n#spectrum\tINS\t2\t3\t6\n#spectrum\tINS\t4\t7\t3\n"
                       "#spectrum\tDEL\t2\t3\t4\n#spectrum\tDEL\t4\t7\t2\n")
    _, _, c2 = dm.paf_texts(text, kept, 1)
    assert c2 == dict(records=11, usable=9, bad=1, untagged=1, rows=20, snp_runs=3, snp_bases=11, n_ins=11, ins_bases=31, n_del=6, del_bases=19,
                      n_skip=0, skip_bases=0, m_columns=0)
    assert dm.paf_texts(text, kept, 1, SNP)[2]["rows"] == 3 and dm.paf_texts(text, kept, 1, INS | DEL, 3)[2]["rows"] == 1 + 1 + 2 + 2 + 2 + 2
    assert dm.paf_texts("", None, 0) == ("", "", dict.fromkeys(dm.COUNTS[:-1], 0))
    assert dm.paf_texts(text, np.zeros(14, dtype=bool), 1)[:2] == ("", "")


def diffs_text(lib, paf, status, set_=0, kinds=7, min_indel=1, batch=0, ctx=None, want=(True, True)):
    """swg_paf_diffs_text -> (rc, rows text or None, summary text or None, counts)"""
    from sweepga_amd import _lib
    counts = _lib.SwgDiffCounts()
    p, n = (C.c_void_p(77), C.c_void_p(77)), (C.c_uint64(77), C.c_uint64(77))
    rc = lib.swg_paf_diffs_text(ctx, paf.handle, status.ctypes.data if status is not None else None, set_, kinds, min_indel, batch, C.byref(counts),
                                C.byref(p[0]) if want[0] else None, C.byref(n[0]) if want[0] else None, C.byref(p[1]) if want[1] else None,
                                C.byref(n[1]) if want[1] else None)
    texts = []
    for q, m, w in zip(p, n, want):
        if w and q.value:
            texts.append(C.string_at(q.value, m.value).decode())
            lib.swg_free(q)
        else:
            assert not w or m.value == 0
            texts.append(None)
    return rc, texts[0], texts[1], {k: int(getattr(counts, k)) for k in dm.COUNTS}


def test_paf_seams_without_a_device(lib, tmp_path):
    """A PAF without records of the set gives empty outputs and needs no device; the refusals come before a context is looked at, and
    before a file is touched."""
    from sweepga_amd import Diffs, PafFile, SwgError, _lib
    zero = {k: 0 for k in dm.COUNTS}
    out, summ = tmp_path / "x.tsv", tmp_path / "s.tsv"
    for text in ("", "# nothing\nfew\tfields\n"):
        with PafFile(text=text) as paf:
            for st in (None, np.zeros(1, dtype=np.uint8)):
                assert diffs_text(lib, paf, st) == (0, "", "", zero)
                assert diffs_text(lib, paf, st, kinds=15, min_indel=9, batch=5) == (0, "", "", zero)
                assert diffs_text(lib, paf, st, want=(False, True)) == (0, None, "", zero)
            out.write_text("stale"), summ.write_text("stale")
            counts = _lib.SwgDiffCounts()
            assert lib.swg_paf_diffs_write(None, paf.handle, None, 0, 7, 1, 0, str(out).encode(), str(summ).encode(), C.byref(counts)) == 0
            assert out.read_bytes() == b"" and summ.read_bytes() == b"" and counts.records == 0 and counts.batches == 0
            assert lib.swg_paf_diffs_write(None, paf.handle, None, 0, 7, 1, 0, None, str(summ).encode(), None) == 0      # counts may be NULL
            got = Diffs.from_paf(paf, None, set="all")
            assert (got.text, got.summary_text, got.counts, got.rows, got.pairs, got.spectrum) == ("", "", zero, [], [], {})
    text, kept = mixed_paf()
    with PafFile(text=text) as paf:
        none = np.zeros(paf.n, dtype=np.uint8)
        assert diffs_text(lib, paf, none, set_=1) == (0, "", "", zero)                    # a set that is never in status: no device
        assert Diffs.from_paf(paf, none).text == "" and Diffs.write_paf(paf, none, out, summ) == zero
        assert out.read_bytes() == b"" and summ.read_bytes() == b""
        st = kept.astype(np.uint8)
        out.write_text("stale"), summ.write_text("stale")
        rc, t, s, _ = diffs_text(lib, paf, st, set_=1)
        assert rc == -1 and t is None and s is None and b"swg_paf_diffs_text: NULL context" in lib.swg_alnstats_last_error()
        for set_, kinds, word in ((2, 7, b"set"), (0, 0, b"kinds"), (1, 16, b"kinds"), (0, 2**32 - 1, b"kinds")):
            rc, t, s, _ = diffs_text(lib, paf, st, set_=set_, kinds=kinds)
            assert rc == -1 and t is None and s is None and word in lib.swg_alnstats_last_error()
            assert lib.swg_paf_diffs_write(None, paf.handle, st.ctypes.data, set_, kinds, 1, 0, str(out).encode(), str(summ).encode(), None) == -1
            assert out.read_text() == "stale" and summ.read_text() == "stale"
        assert diffs_text(lib, paf, None, set_=1)[0] == -1 and b"status" in lib.swg_alnstats_last_error()
        assert lib.swg_paf_diffs_write(None, paf.handle, None, 1, 7, 1, 0, str(out).encode(), None, None) == -1 and out.read_text() == "stale"
        assert lib.swg_paf_diffs_write(None, paf.handle, none.ctypes.data, 1, 7, 1, 0, str(tmp_path / "no" / "dir.tsv").encode(), None, None) == -1
        assert b"cannot open" in lib.swg_alnstats_last_error()
        assert lib.swg_paf_diffs_write(None, paf.handle, none.ctypes.data, 1, 7, 1, 0, str(out).encode(), str(tmp_path / "no" / "s.tsv").encode(), None) == -1
        p, n = C.c_void_p(), C.c_uint64()
        assert lib.swg_paf_diffs_text(None, None, None, 0, 7, 1, 0, None, C.byref(p), C.byref(n), None, None) == -1
        assert lib.swg_paf_diffs_text(None, paf.handle, None, 0, 7, 1, 0, None, None, None, None, None) == -1           # neither text
        assert lib.swg_paf_diffs_text(None, paf.handle, None, 0, 7, 1, 0, None, C.byref(p), None, None, None) == -1     # a text without its length
        assert lib.swg_paf_diffs_write(None, paf.handle, None, 0, 7, 1, 0, None, None, None) == -1                      # neither file
        with pytest.raises(SwgError):
            Diffs.from_paf(paf, st, set=2)
        with pytest.raises(SwgError):
            Diffs.from_paf(paf, st, kinds=0)
    with PafFile(text=REBASED) as paf:
        with pytest.raises(SwgError) as e:
            Diffs.from_paf(paf, np.ones(1, dtype=np.uint8))
        assert e.value.code == -6 and "2^32" in str(e.value)
        out.write_text("stale")
        with pytest.raises(SwgError):
            Diffs.write_paf(paf, np.ones(1, dtype=np.uint8), out)
        assert out.read_text() == "stale"


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
    genome = np.array([0, 1, 2], dtype=np.uint32)
    record, offset, text = cigar_set([0, 2], [G, "10M"])
    cs = _lib.SwgCigarSet()
    cs.record, cs.offset, cs.text, cs.k = record.ctypes.data, offset.ctypes.data, text.ctypes.data, 2
    poison = np.full(32 * 4, 0xab, dtype=np.uint8)
    spectrum = np.full(4 * 33, 7, dtype=np.uint64)
    for fn in (lib.swg_diff_records, lib.swg_diff_records_device):
        req = _lib.SwgDiffRequest()
        req.kinds, req.row_capacity, req.rows, req.n_rows, req.usable, req.spectrum = 7, 4, poison.ctypes.data, 12345, 77, spectrum.ctypes.data
        assert fn(None, C.byref(rec), genome.ctypes.data, 3, None, C.byref(cs), C.byref(req)) == -1
        assert (poison == 0xab).all() and req.n_rows == 12345 and req.usable == 77 and (spectrum == 7).all()


def test_command_line_usage_errors(lib, tmp_path):
    from sweepga_amd import build
    paf = tmp_path / "in.paf"
    paf.write_text(mixed_paf()[0])
    out, rows, summ = tmp_path / "out.paf", tmp_path / "d.tsv", tmp_path / "s.tsv"
    run = lambda *a: subprocess.run([build.CLI, str(paf), "--output-file", str(out), *a], capture_output=True, text=True)      # noqa: E731
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(w in r.stdout for w in ("--diffs FILE", "--diffs-summary FILE", "--diffs-set kept|all", "--diffs-kinds LIST",
                                                              "--diffs-kinds snp,ins,del,skip", "--diffs-min-indel N", "--diffs-batch BYTES"))
    need = "need --diffs or --diffs-summary"
    cases = [(["--diffs-set", "all"], need), (["--diffs-kinds", "snp"], need), (["--diffs-min-indel", "5"], need), (["--diffs-batch", "4k"], need),
             (["--diffs", str(rows), "--diffs-set", "lost"], "--diffs-set: kept or all"),
             (["--diffs", str(rows), "--diffs-kinds", "snp,inv"], "--diffs-kinds"),
             (["--diffs", str(rows), "--diffs-kinds", "SNP"], "--diffs-kinds"),
             (["--diffs", str(rows), "--diffs-kinds", ""], "the list is empty"),
             (["--diffs-summary", str(summ), "--diffs-kinds", ",,"], "the list is empty"),
             (["--diffs", str(rows), "--diffs-min-indel", "few"], "--diffs-min-indel"),
             (["--diffs", str(rows), "--diffs-min-indel", "4294967296"], "--diffs-min-indel"),
             (["--diffs", str(rows), "--diffs-batch", "0"], "--diffs-batch"),
             (["--diffs-summary", str(summ), "--diffs-batch", "many"], "--diffs-batch"),
             (["--diffs", "-"], "not a standard error report"), (["--diffs-summary", "-"], "not a standard error report"),
             (["--diffs", ""], "empty value for --diffs"), (["--diffs-summary", ""], "empty value for --diffs-summary")]
    for extra, word in cases:
        r = run(*extra)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)
        assert r.stdout == "" and not out.exists() and not rows.exists() and not summ.exists(), extra


def test_text_helpers_under_the_host_sanitizers(tmp_path):
    """tests/native/diffs_text_check.cpp: a stand-alone program over csrc/host/diffs_text.cpp, built with the address and
    undefined-behaviour sanitizers; its answers must be the model's byte for byte."""
    exe = str(tmp_path / "diffs_text_check")
    host = os.path.join(ROOT, "sweepga_amd", "csrc", "host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "diffs_text_check.cpp"), os.path.join(host, "diffs_text.cpp"),
                           os.path.join(host, "ucsc_text.cpp"), os.path.join(host, "cigar_text.cpp"), "-lpthread"])
    top = 2**32 - 1
    feed, want = [], []
    # rows at every field's extreme: 10-digit values, empty intervals on either side, empty and very long names
    for row, t_name, q_name in (((0, INS, 1005, 1005, 105, 107, 5, 6), "g2#1#t", "g1#1#q"), ((top, SNP | MINUS, top - 1, top, top - 1, top, top, top), "", ""),
                                ((7, DEL | MINUS, 0, top, top, top, 0, 0), "x" * 5000, "y"), ((1, SKIP, 9, 10, 0, 0, 0, 1), "a b", "c d"),
                                ((2, INS | MINUS, 0, 0, 0, top, 0, 0), "t", "q" * 3000)):
        feed += ["R", " ".join(str(v) for v in row), t_name, q_name]
        want.append(dm.ROWS_HEADER + dm.row_text(t_name, q_name, row))
    assert want[1] == dm.ROWS_HEADER + "\t4294967294\t4294967295\t\t4294967294\t4294967295\t-\tSNP\t1\t4294967295\t4294967295\t4294967295\n"
    assert want[2].endswith("\t0\t4294967295\ty\t4294967295\t4294967295\t-\tDEL\t4294967295\t0\t0\t7\n")
    # the merge of pair sums across batches, in both orders: disjoint, interleaved, equal and empty lists; sums beyond 2^32
    big = 2**40
    a = [(0, 1) + tuple(range(1, 13)), (1, 1) + (big,) * 12, (2, 0) + (1,) + (0,) * 11]
    b = [(0, 0) + (5,) * 12, (1, 1) + tuple(range(12)), (2, 0) + (0,) * 11 + (9,), (2, 5) + (3,) * 12]

    def merged(x, y):
        acc = {}
        for p in x + y:
            acc[p[:2]] = tuple(u + v for u, v in zip(acc.get(p[:2], (0,) * 12), p[2:]))
        return "".join(" ".join(str(v) for v in k + acc[k]) + "\n" for k in sorted(acc)) + "--\n"
    for x, y in ((a, b), (b, a), (a, a), (a, []), ([], b), ([], [])):
        feed += ["M", "%d %d" % (len(x), len(y))] + [" ".join(str(v) for v in p) for p in x + y]
        want.append(merged(x, y))
    assert merged(a, b) == merged(b, a) and merged(a, b).startswith("0 0 5 5") and "1 1 %d %d" % (big, big + 1) in merged(a, b)
    # the summary: names empty and long, every kind's first and last bin, no pair at all
    names = ["g1#1#", "", "z" * 4000]
    spectrum = np.zeros((4, dm.BINS), dtype=np.uint64)
    for kind in range(4):
        spectrum[kind][1], spectrum[kind][32], spectrum[kind][kind + 5] = kind + 1, 2**63, 7
    for pairs in (a, []):
        sparse = [(int(i), int(v)) for i, v in enumerate(spectrum.ravel()) if v]
        feed += ["Y", "%d %d %d" % (len(names), len(pairs), len(sparse))] + names + [" ".join(str(v) for v in p) for p in pairs] + ["%d %d" % s for s in sparse]
        want.append(dm.summary_text(names, pairs, spectrum))
    assert "#spectrum\tSKIP\t2147483648\t4294967295\t9223372036854775808\n" in want[-1] and "#spectrum\tSNP\t1\t1\t1\n" in want[-1]
    r = subprocess.run([exe], input=("\n".join(feed) + "\n").encode(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.decode() == "".join(want)
