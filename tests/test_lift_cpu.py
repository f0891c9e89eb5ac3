"""The lift without a GPU: the model of tests/lift_model.py against rows worked out by hand, and the host side of the feature --
header, ctypes mirrors, exported symbols, the BED parser through swg_paf_lift on a record-free PAF, the refusals that need no
device, the command line's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import lift_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, CC = 0, 1, 2
U = lm.UNKNOWN
NAMES = ["g1#1#a", "g2#1#b", "g3#1#c"]


def hand_case():
    """Eight records on three sequences, eight regions.  Records: (q, t, qs, qe, ts, te, strand, kept)
      0  A B 100 200 1000 1100 + kept     D = L
      1  A B 150 250 2000 2030 - dropped  D / L = 30 / 100 does not divide
      2  A C 400 500   50   50 + kept     D = 0
      3  A A   0  50  600  650 + kept     a self record: a hit on both axes
      4  A B 100 120 3000 3010 + dropped  the start of record 0
      5  B A   0  10  200  210 - kept     A as the target
      6  C B   5   5    0   10 + kept     no length on the query
      7  B C  10  20   10   20 + kept
    Regions and their rows (region, record, ca, cb, dst_seq, dst_start, dst_end, flags), flags = strand | axis << 1:
      0  A 200 260   record 0 ends at 200 = a: no hit.  Record 1: o = 50 .. 100 of L = 100, D = 30: f = 15, c = 30, '-': [2030 - 30,
                     2030 - 15).  On the target axis record 5 whole: [0, 10) of B.
      1  A  90 101   records 0 and 4 start at 100 = b - 1: hits, in record order; o = 0 .. 1: c(1) = ceil(100 / 100) = 1 and
                     ceil(10 / 20) = 1.
      2  A   0 1000  every record of A whole, by start: 3, 0, 4, 1, 2 (D = 0: the empty interval at 50); then the target axis: 5, 3
      3  A 160 170   inside records 0 (o = 60 .. 70: [1060, 1070)) and 1 (o = 10 .. 20: f = floor(3.0) = 3, c = ceil(6.0) = 6: [2024, 2027))
      4  B   5   5   empty: nothing
      5  a name the input does not have
      6  C   0 100   record 6 has no length on C, record 2 none on its target side C; record 7 whole on the target axis: [10, 20) of B
      7  A 210 240   record 1 alone (o = 60 .. 90: f = 18, c = 27: [2003, 2012)), which the filter dropped: lost
    -> (cols, strand, kept, regions, rows, summary)"""
    recs = [(A, B, 100, 200, 1000, 1100, 0, 1), (A, B, 150, 250, 2000, 2030, 1, 0), (A, CC, 400, 500, 50, 50, 0, 1), (A, A, 0, 50, 600, 650, 0, 1),
            (A, B, 100, 120, 3000, 3010, 0, 0), (B, A, 0, 10, 200, 210, 1, 1), (CC, B, 5, 5, 0, 10, 0, 1), (B, CC, 10, 20, 10, 20, 0, 1)]
    arr = np.array(recs, dtype=np.int64)
    cols = {k: arr[:, i].astype(np.uint32) for i, k in enumerate(lm.COLS)}
    regions = [(A, 200, 260), (A, 90, 101), (A, 0, 1000), (A, 160, 170), (B, 5, 5), (U, 0, 10), (CC, 0, 100), (A, 210, 240)]
    rows = [(0, 1, 200, 250, B, 2000, 2015, 1), (0, 5, 200, 210, B, 0, 10, 3),
            (1, 0, 100, 101, B, 1000, 1001, 0), (1, 4, 100, 101, B, 3000, 3001, 0),
            (2, 3, 0, 50, A, 600, 650, 0), (2, 0, 100, 200, B, 1000, 1100, 0), (2, 4, 100, 120, B, 3000, 3010, 0), (2, 1, 150, 250, B, 2000, 2030, 1),
            (2, 2, 400, 500, CC, 50, 50, 0), (2, 5, 200, 210, B, 0, 10, 3), (2, 3, 600, 650, A, 0, 50, 2),
            (3, 0, 160, 170, B, 1060, 1070, 0), (3, 1, 160, 170, B, 2024, 2027, 1),
            (6, 7, 10, 20, B, 10, 20, 2),
            (7, 1, 210, 240, B, 2003, 2012, 1)]
    #          all q, all t, kept q, kept t
    summary = [(1, 1, 0, 1), (2, 0, 1, 0), (5, 2, 3, 2), (2, 0, 1, 0), (0, 0, 0, 0), (0, 0, 0, 0), (0, 1, 0, 1), (1, 0, 0, 0)]
    summary = np.array(summary, dtype=np.uint32).reshape(-1, 2, 2)
    return cols, arr[:, 6].astype(np.uint8), arr[:, 7].astype(bool), regions, rows, summary


def hand_paf():
    cols, strand, kept, _, _, _ = hand_case()
    lines = []
    for k in range(len(strand)):
        lines.append("\t".join([NAMES[cols["q_id"][k]], "5000", str(cols["q_start"][k]), str(cols["q_end"][k]), "-" if strand[k] else "+",
                                NAMES[cols["t_id"][k]], "5000", str(cols["t_start"][k]), str(cols["t_end"][k]), "10", "20", "60"]))
    return "\n".join(lines) + "\n", kept


HAND_BED = ("# a comment\ntrack name=x\n" + "g1#1#a\t200\t260\tgeneA\n" + "g1#1#a\t90\t101\n" + "\n" + "g1#1#a\t0\t1000\twhole\t0\t+\n" +
            "browser position\n" + "g1#1#a\t160\t170\t\n" + "g2#1#b\t5\t5\tempty\r\n" + "nowhere\t0\t10\n" + "g3#1#c\t0\t100\tc\n" + "g1#1#a\t210\t240\tgone")
HAND_SUMMARY = (lm.SUMMARY_HEADER + "geneA\tg1#1#a\t200\t260\t1\t1\t0\t1\tkept\n" + "g1#1#a:90-101\tg1#1#a\t90\t101\t2\t0\t1\t0\tkept\n" +
                "whole\tg1#1#a\t0\t1000\t5\t2\t3\t2\tkept\n" + "g1#1#a:160-170\tg1#1#a\t160\t170\t2\t0\t1\t0\tkept\n" + "empty\tg2#1#b\t5\t5\t0\t0\t0\t0\tnone\n" +
                "nowhere:0-10\tnowhere\t0\t10\t0\t0\t0\t0\tunknown\n" + "c\tg3#1#c\t0\t100\t0\t1\t0\t1\tkept\n" + "gone\tg1#1#a\t210\t240\t1\t0\t0\t0\tlost\n")


def test_model_against_rows_worked_out_by_hand():
    cols, strand, kept, regions, rows, summary = hand_case()
    got, got_summary = lm.lift(cols, strand, kept, regions, 0, 3)
    assert got == rows and np.array_equal(got_summary, summary)
    got_kept, s2 = lm.lift(cols, strand, kept, regions, 1, 3)
    assert got_kept == [r for r in rows if kept[r[1]]] and np.array_equal(s2, summary)
    for axes in (1, 2):
        got, s = lm.lift(cols, strand, kept, regions, 0, axes)
        assert got == [r for r in rows if (r[7] >> 1) == axes - 1]
        assert np.array_equal(s[:, :, axes - 1], summary[:, :, axes - 1]) and not s[:, :, 2 - axes].any()
    none, s = lm.lift(cols, strand, None, regions, 0, 3)
    assert none == rows and np.array_equal(s[:, 0], summary[:, 0]) and not s[:, 1].any()
    # the regions alone, and in another order: the rows of a region do not depend on the others
    for r, g in enumerate(regions):
        assert [row[1:] for row in lm.lift(cols, strand, kept, [g], 0, 3)[0]] == [row[1:] for row in rows if row[0] == r]
    # the prune: what hi - p0 comes to on A's query axis, sorted 3 (0, 50) 0 (100, 200) 4 (100, 120) 1 (150, 250) 2 (400, 500)
    assert lm.candidates(cols, [(A, 200, 260)], 1) == [1, 0]      # prefix maxima 50 200 200 250 500: p0 = 3, hi = 4
    assert lm.candidates(cols, [(A, 160, 170)], 1) == [3, 0]      # p0 = 1 (200 > 160), hi = 4: record 4 is looked at and is no hit
    assert lm.candidates(cols, [(B, 5, 5), (U, 0, 9)], 3) == [0, 0]
    # the texts
    text, kept = hand_paf()
    rows_text, summary_text = lm.paf_texts(text, kept, HAND_BED, 0, 3)
    assert summary_text == HAND_SUMMARY
    assert rows_text.split("\n")[0] == "g2#1#b\t2000\t2015\tgeneA\tg1#1#a\t200\t250\t-\tq\t1" and rows_text.count("\n") == len(rows)
    assert lm.paf_texts(text, None, HAND_BED, 0, 3)[1].split("\n")[1] == "geneA\tg1#1#a\t200\t260\t1\t1\t-\t-\tall"


def test_projection_rounds_outward_at_the_largest_values():
    top = 2**32 - 1
    assert lm.project(1, top - 1, 0, top, 1, top, 0) == (1, top - 1, 1, top)      # f(1) = 0, c(L - 1) = D: L = 2^32 - 1, D = 2^32 - 2
    assert lm.project(1, 2, 0, top, 1, top, 1) == (1, 2, top - 2, top)            # '-': [d1 - c(2), d1 - f(1)) = [d1 - 2, d1)


@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib, lift
    structs = (("swg_lift_region", _lib.SwgLiftRegion), ("swg_lift_row", _lib.SwgLiftRow), ("swg_lift_summary", _lib.SwgLiftSummary),
               ("swg_lift_request", _lib.SwgLiftRequest))
    prints = ['printf("%%zu\\n", sizeof(%s));' % name for name, _ in structs]
    prints += ['printf("%%zu\\n", offsetof(%s, %s));' % (name, f) for name, cls in structs for f, _ in cls._fields_]
    prints += ['printf("%u %u %u %u %d %d\\n", SWG_LIFT_AXIS_QUERY, SWG_LIFT_AXIS_TARGET, SWG_LIFT_MINUS, SWG_LIFT_ON_TARGET, SWG_IV_ALL, SWG_IV_KEPT);']
    prints += ['printf("%%zu\\n", sizeof(%s));' % s for s in ("swg_records", "swg_dot_request")]
    prints.append('printf("%d\\n", SWG_ABI_VERSION);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(cls) for _, cls in structs] + [getattr(cls, f).offset for _, cls in structs for f, _ in cls._fields_]
    want += [1, 2, 1, 2, 0, 1, 128, 88, 1]      # the structures that existed before keep their sizes
    assert got == want
    assert got[:4] == [16, 32, 16, 56]
    for _, cls in structs:      # no implicit padding
        assert sum(C.sizeof(t) for _, t in cls._fields_) == C.sizeof(cls)
    assert lift.ROW_DTYPE.itemsize == 32 and lift.REGION_DTYPE.itemsize == 16
    assert [lift.ROW_DTYPE.fields[f][1] for f, _ in _lib.SwgLiftRow._fields_] == [getattr(_lib.SwgLiftRow, f).offset for f, _ in _lib.SwgLiftRow._fields_]


def test_symbols_are_exported_and_declared(lib):
    import sweepga_amd
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_lift_records", "swg_lift_records_device", "swg_paf_lift"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    assert lib.swg_abi_version() == 1
    for name in ("Lift", "LiftResult", "lift_records", "lift_records_device"):
        assert hasattr(sweepga_amd, name)


def slots(rows=True, summary=True):
    marker = C.create_string_buffer(1)
    p = (C.c_void_p * 2)()
    p[0], p[1] = (C.addressof(marker) if rows else None), (C.addressof(marker) if summary else None)
    return p, (C.c_uint64 * 2)(7, 7), marker


def paf_lift(lib, paf, status, bed, set_=0, axes=3, ctx=None, rows=True, summary=True):
    """-> (rc, rows text, summary text)"""
    p, n, _m = slots(rows, summary)
    bed = bed.encode()
    rc = lib.swg_paf_lift(ctx, paf.handle, status.ctypes.data if status is not None else None, bed, len(bed), set_, axes, p, n)
    text = [None, None]
    for k in range(2):
        if p[k]:
            text[k] = C.string_at(p[k], n[k]).decode()
            lib.swg_free(C.c_void_p(p[k]))
        else:
            assert n[k] == 0
    return rc, text[0], text[1]


MALFORMED = [("a\t1\n", 1), ("a\t1\t5\nb 1 5\n", 2), ("#x\n\na\t5\t1\n", 3), ("a\t1\t4294967296\n", 1), ("a\t-1\t5\n", 1), ("a\t1e3\t5000\n", 1),
             ("a\t\t5\n", 1), ("\t1\t5\n", 1), ("track\na\t1\t2\na\t1\tx\n", 3), ("a\t1\t2\r\na\t 1\t2\r\n", 2), ("a\t1\t99999999999\n", 1),
             ("ok\t0\t4294967295\nok\t4294967295\t4294967295\nbad\t7", 3)]


def test_bed_parser_on_a_record_free_paf_without_a_device(lib):
    from sweepga_amd import Lift, PafFile, SwgError
    for text in ("", "# nothing\nfew\tfields\n"):
        with PafFile(text=text) as paf:
            assert paf.n == 0
            for st in (None, np.zeros(1, dtype=np.uint8)):
                assert paf_lift(lib, paf, st, HAND_BED) == (0, "", lm.SUMMARY_HEADER)
                assert paf_lift(lib, paf, st, "") == (0, "", lm.SUMMARY_HEADER)
            assert paf_lift(lib, paf, None, HAND_BED, rows=False) == (0, None, lm.SUMMARY_HEADER)
            assert paf_lift(lib, paf, None, HAND_BED, summary=False) == (0, "", None)
            got = Lift.from_paf(paf, None, HAND_BED, set="all")
            assert (got.text, got.summary_text) == ("", lm.SUMMARY_HEADER) == lm.paf_texts(text, None, HAND_BED, 0, 3)
            assert len(got.rows) == 0 and len(got.summary) == 0
            for bed, line in MALFORMED:
                rc, r, s = paf_lift(lib, paf, None, bed)
                assert rc == -1 and r is None and s is None, bed
                assert ("BED line %d:" % line).encode() in lib.swg_alnstats_last_error(), (bed, lib.swg_alnstats_last_error())
                with pytest.raises(lm.BedError) as e:
                    lm.parse_bed(bed, {})
                assert e.value.line == line, bed
                with pytest.raises(SwgError) as e2:
                    Lift.from_paf(paf, None, bed, set="all")
                assert e2.value.code == -1 and "line %d" % line in str(e2.value)
    # the model's parser on the hand BED: skipped lines, labels, an unknown name, a trailing line without a newline
    ids = {nm: i for i, nm in enumerate(NAMES)}
    assert lm.parse_bed(HAND_BED, ids) == [(A, 200, 260, "geneA", NAMES[0]), (A, 90, 101, "g1#1#a:90-101", NAMES[0]), (A, 0, 1000, "whole", NAMES[0]),
                                           (A, 160, 170, "g1#1#a:160-170", NAMES[0]), (B, 5, 5, "empty", NAMES[1]), (U, 0, 10, "nowhere:0-10", "nowhere"),
                                           (CC, 0, 100, "c", NAMES[2]), (A, 210, 240, "gone", NAMES[0])]


REBASED = "\t".join(["a#1#x", str(2**33), str(2**32), str(2**32 + 50), "+", "b#1#y", "900", "10", "60", "50", "50", "60"]) + "\n"


def test_refusals_that_need_no_device(lib):
    from sweepga_amd import Lift, PafFile, SwgError, _lib
    from sweepga_amd.lift import REGION_DTYPE, ROW_DTYPE
    cols, strand, kept, regions, _, _ = hand_case()
    rec = _lib.SwgRecords()
    rec.n = len(strand)
    for k, a in cols.items():
        setattr(rec, k, a.ctypes.data)
    rec.strand = strand.ctypes.data
    rec.n_seq = 3
    regs = np.array([(s, a, b, 0) for s, a, b in regions], dtype=REGION_DTYPE)
    status = kept.astype(np.uint8)
    poison = np.frombuffer(bytearray(b"\xab" * 32 * 4), dtype=ROW_DTYPE)
    for fn in (lib.swg_lift_records, lib.swg_lift_records_device):     # a NULL context: there is no CPU path
        req = _lib.SwgLiftRequest()
        req.set, req.axes, req.n, req.capacity, req.rows = 0, 3, 12345, 4, poison.ctypes.data
        assert fn(None, C.byref(rec), status.ctypes.data, regs.ctypes.data, len(regs), C.byref(req)) == -1
        assert poison.tobytes() == b"\xab" * 128 and req.n == 12345
    text, kept = hand_paf()
    st = kept.astype(np.uint8)
    with PafFile(text=text) as paf:
        assert paf_lift(lib, paf, st, HAND_BED)[0] == -1 and b"NULL context" in lib.swg_alnstats_last_error()
        assert paf_lift(lib, paf, st, "")[1:] == ("", lm.SUMMARY_HEADER)                         # no region: no device
        assert paf_lift(lib, paf, None, HAND_BED, set_=1)[0] == -1 and b"status" in lib.swg_alnstats_last_error()
        for set_, axes in ((2, 3), (0, 0), (0, 4), (1, 7)):
            assert paf_lift(lib, paf, st, HAND_BED, set_=set_, axes=axes)[0] == -1
        assert paf_lift(lib, paf, st, HAND_BED, rows=False, summary=False)[0] == -1
        assert paf_lift(lib, paf, st, "a\t5\t1\n")[0] == -1 and b"line 1" in lib.swg_alnstats_last_error()      # the BED before the context
        p, n, _m = slots()
        assert lib.swg_paf_lift(None, None, st.ctypes.data, b"", 0, 0, 3, p, n) == -1
        assert lib.swg_paf_lift(None, paf.handle, st.ctypes.data, b"", 0, 0, 3, None, n) == -1
        assert lib.swg_paf_lift(None, paf.handle, st.ctypes.data, None, 5, 0, 3, p, n) == -1
    with PafFile(text=REBASED) as paf:       # rebased columns: refused before the BED or a context is looked at
        with pytest.raises(SwgError) as e:
            Lift.from_paf(paf, np.ones(1, dtype=np.uint8), "a\t5\t1\n")
        assert e.value.code == -6 and "2^32" in str(e.value)


def test_command_line_usage_errors(lib, tmp_path):
    from sweepga_amd import build
    bed, bad, paf = tmp_path / "r.bed", tmp_path / "bad.bed", tmp_path / "in.paf"
    bed.write_text(HAND_BED)
    bad.write_text("g1#1#a\t1\t2\ng1#1#a\t9\t2\n")
    paf.write_text(hand_paf()[0])
    run = lambda *a: subprocess.run([build.CLI, str(paf), *a], capture_output=True, text=True)      # noqa: E731
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--lift-regions BED", "--lift FILE", "--lift-summary FILE", "--lift-set kept|all", "--lift-axis query|target|both"):
        assert flag in r.stdout, flag
    for flag in ("--lift-regions", "--lift", "--lift-summary"):
        r = run(flag + "=")
        assert r.returncode == 2 and "empty value for " + flag in r.stderr, (flag, r.stderr)
    for flag in ("--lift-regions", "--lift", "--lift-summary", "--lift-set", "--lift-axis"):
        r = run(flag)
        assert r.returncode == 2 and flag in r.stderr
    for extra in (["--lift", "x.tsv"], ["--lift-summary", "x.tsv"], ["--lift-set", "all"], ["--lift-axis", "query"]):
        r = run(*extra)
        assert r.returncode == 2 and "need --lift-regions" in r.stderr, (extra, r.stderr)
    r = run("--lift-regions", str(bed))
    assert r.returncode == 2 and "needs --lift or --lift-summary" in r.stderr
    r = run("--lift-regions", str(tmp_path / "missing.bed"), "--lift", "x.tsv")
    assert r.returncode == 2 and "cannot open" in r.stderr
    r = run("--lift-regions", str(bad), "--lift", str(tmp_path / "x.tsv"))
    assert r.returncode == 2 and "BED line 2" in r.stderr and "start > end" in r.stderr and not (tmp_path / "x.tsv").exists()
    for flag, v in (("--lift-set", "lost"), ("--lift-set", ""), ("--lift-axis", "q"), ("--lift-axis", "3")):
        r = run("--lift-regions", str(bed), "--lift", "x.tsv", flag + "=" + v)
        assert r.returncode == 2 and "invalid value for " + flag in r.stderr, (flag, v, r.stderr)
    assert r.stdout == ""


def test_command_line_refuses_64_bit_columns_before_it_filters(lib, tmp_path):
    from sweepga_amd import build
    inp, out, rep, bed = tmp_path / "in.paf", tmp_path / "out.paf", tmp_path / "lift.out", tmp_path / "r.bed"
    inp.write_text(REBASED)
    bed.write_text("a#1#x\t0\t10\n")
    for flag in ("--lift", "--lift-summary"):
        for extra in ([], ["--no-filter"]):
            r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--lift-regions", str(bed), flag, str(rep), *extra], capture_output=True, text=True)
            assert r.returncode == 3 and "--lift" in r.stderr and "2^32" in r.stderr, r.stderr
            assert r.stdout == "" and not out.exists() and not rep.exists()
