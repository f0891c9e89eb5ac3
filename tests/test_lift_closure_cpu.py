"""The transitive lift without a GPU: the model of tests/lift_closure_model.py against a walk worked out by hand, and the host side
of the feature -- header, ctypes and numpy mirrors, exported symbols, swg_paf_lift_closure on a record-free PAF, the refusals that
need no device, the command line's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import lift_closure_model as cm
from tests import lift_model as lm
from tests.test_lift_cpu import MALFORMED, REBASED, slots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, CC = 0, 1, 2
U = lm.UNKNOWN
NAMES = ["gA#1#x", "gB#1#y", "gC#1#z"]


def hand_case():
    """Three genomes, mappings A-B and B-C only.  Records (q, t, qs, qe, ts, te, strand, kept):
      0  A B  100  400 1000 1200 +  kept     L = 300, D = 200 on the query axis: D / L = 2 / 3 does not divide
      1  B C 1050 1250 5000 5200 -  dropped  L = D = 200
    Region 0 = A [200, 251), both axes, the set ALL:
      hop 1  record 0 on its query: o = 100 .. 151: f = floor(66.7) = 66, c = ceil(100.7) = 101: B [1066, 1101)         (35 bases)
      hop 2  from B [1066, 1101): record 1 on its query, o = 16 .. 51, '-': C [5200 - 51, 5200 - 16) = [5149, 5184)       (35 bases);
             record 0 on its target (L = 200, D = 300), o = 66 .. 101: f = floor(99.0) = 99, c = ceil(151.5) = 152: A [199, 252), of
             which [200, 251) is visited: the slivers A [199, 200) and A [251, 252) that outward rounding makes beside the region
      hop 3  min_len = 10: the slivers are not walked; C [5149, 5184) through record 1 on its target, o = 149 .. 184, '-': B [1250 -
             184, 1250 - 149) = [1066, 1101), visited: F_3 is empty, the walk is closed after 3 hops and 4 projections
             min_len = 1: A [199, 200) gives o = 99 .. 100: B [1066, 1067), visited; A [251, 252) gives o = 151 .. 152: f =
             floor(100.7) = 100, c = ceil(101.3) = 102: B [1100, 1102), new: B [1101, 1102) at hop 3 -- why min_len exists
    Region 1 is empty, region 2 an unknown name.  Region 3 = C [5100, 5150): record 1 on its target, o = 100 .. 150, '-': B [1100, 1150)
    at hop 1; from there record 1 on its query gives C [5100, 5150) back, record 0 on its target o = 100 .. 150: f = 150, c = 225:
    A [250, 325) at hop 2; hop 3 returns to B [1100, 1150): closed.
    -> (cols, strand, kept, regions)"""
    recs = [(A, B, 100, 400, 1000, 1200, 0, 1), (B, CC, 1050, 1250, 5000, 5200, 1, 0)]
    arr = np.array(recs, dtype=np.int64)
    cols = {k: arr[:, i].astype(np.uint32) for i, k in enumerate(lm.COLS)}
    regions = [(A, 200, 251), (B, 7, 7), (U, 0, 10), (CC, 5100, 5150)]
    return cols, arr[:, 6].astype(np.uint8), arr[:, 7].astype(bool), regions


# region 0 with max_hops = 3, min_len = 10: rows in (region, seq, start) order
HAND_ROWS = [(0, A, 199, 200, 2, 0), (0, A, 200, 251, 0, 0), (0, A, 251, 252, 2, 0), (0, B, 1066, 1101, 1, 0), (0, CC, 5149, 5184, 2, 0)]
HAND_SUMMARY = (1 + 51 + 1 + 35 + 35, 5, 3, 2, 0)


def hand_paf():
    cols, strand, kept, _ = hand_case()
    lines = []
    for k in range(len(strand)):
        lines.append("\t".join([NAMES[cols["q_id"][k]], "9000", str(cols["q_start"][k]), str(cols["q_end"][k]), "-" if strand[k] else "+",
                                NAMES[cols["t_id"][k]], "9000", str(cols["t_start"][k]), str(cols["t_end"][k]), "10", "20", "60"]))
    return "\n".join(lines) + "\n", kept


HAND_BED = "gA#1#x\t200\t251\tgene\n" + "gB#1#y\t7\t7\n" + "nowhere\t0\t10\n" + "gC#1#z\t5100\t5150\tback"


def test_model_against_a_walk_worked_out_by_hand():
    cols, strand, kept, regions = hand_case()
    one = regions[:1]
    rows, summary, info = cm.closure(cols, strand, kept, one, 1, 10)
    assert rows == [(0, A, 200, 251, 0, 0), (0, B, 1066, 1101, 1, 0)]                       # one hop reaches B only
    assert summary == [(51 + 35, 2, 2, 1, cm.CUT)] and info == {"hops_run": 1, "projections": 1, "candidates": [1, 0]}
    rows, summary, info = cm.closure(cols, strand, kept, one, 2, 10)
    assert rows == HAND_ROWS and summary == [HAND_SUMMARY[:4] + (cm.CUT,)]                  # two reach C; the piece on C is long: cut
    assert info == {"hops_run": 2, "projections": 3, "candidates": [2, 1]}
    for hops in (3, 4, 100):
        rows, summary, info = cm.closure(cols, strand, kept, one, hops, 10)
        assert rows == HAND_ROWS and summary == [HAND_SUMMARY]                              # hop 3 finds nothing new: closed
        assert info == {"hops_run": 3, "projections": 4, "candidates": [2, 2]}
    rows, summary, info = cm.closure(cols, strand, kept, one, 3, 36)                        # B's 35 bases are reported and not walked on
    assert rows == [HAND_ROWS[1], HAND_ROWS[3]] and summary == [(86, 2, 2, 1, 0)] and info == {"hops_run": 2, "projections": 1, "candidates": [1, 0]}
    rows, summary, info = cm.closure(cols, strand, kept, one, 3, 35)                        # ... with min_len = 35 they are, and so are C's
    assert rows == HAND_ROWS and summary == [HAND_SUMMARY] and info["projections"] == 4
    for min_len in (0, 1):                                                                  # the slivers walked on: a sliver of B at hop 3
        rows, summary, info = cm.closure(cols, strand, kept, one, 3, min_len)
        assert rows == HAND_ROWS[:4] + [(0, B, 1101, 1102, 3, 0)] + HAND_ROWS[4:]
        assert summary == [(124, 6, 3, 3, cm.CUT)] and info["projections"] == 6
    # the set KEPT has record 0 alone: C is out of reach, the slivers are still there
    rows, summary, _ = cm.closure(cols, strand, kept, one, 5, 10, set_=1)
    assert rows == HAND_ROWS[:4] and summary == [(88, 4, 2, 2, 0)]
    # the query axis alone makes the walk directional: A -> B -> C and never back
    rows, _, info = cm.closure(cols, strand, kept, one, 5, 10, axes=1)
    assert rows == [HAND_ROWS[1], HAND_ROWS[3], HAND_ROWS[4]] and info["hops_run"] == 3
    assert cm.closure(cols, strand, kept, one, 5, 10, axes=2)[0] == [HAND_ROWS[1]]
    # all four regions; the regions never influence each other
    rows, summary, info = cm.closure(cols, strand, kept, regions, 3, 10)
    back = [(3, A, 250, 325, 2, 0), (3, B, 1100, 1150, 1, 0), (3, CC, 5100, 5150, 0, 0)]
    assert rows == HAND_ROWS + back and summary == [HAND_SUMMARY, (0, 0, 0, 0, 0), (0, 0, 0, 0, 0), (75 + 50 + 50, 3, 3, 2, 0)]
    for r, g in enumerate(regions):
        assert [w[1:] for w in cm.closure(cols, strand, kept, [g], 3, 10)[0]] == [w[1:] for w in rows if w[0] == r]
    # without records hop 0 is all there is
    none = {k: np.zeros(0, dtype=np.uint32) for k in lm.COLS}
    rows, summary, info = cm.closure(none, np.zeros(0, dtype=np.uint8), None, regions, 3, 10)
    assert rows == [(0, A, 200, 251, 0, 0), (3, CC, 5100, 5150, 0, 0)] and summary[0] == (51, 1, 1, 0, 0) and info["hops_run"] == 0


HAND_TEXT = ("gA#1#x\t199\t200\tgene\t2\n" + "gA#1#x\t200\t251\tgene\t0\n" + "gA#1#x\t251\t252\tgene\t2\n" + "gB#1#y\t1066\t1101\tgene\t1\n" +
             "gC#1#z\t5149\t5184\tgene\t2\n" + "gA#1#x\t250\t325\tback\t2\n" + "gB#1#y\t1100\t1150\tback\t1\n" + "gC#1#z\t5100\t5150\tback\t0\n")
HAND_SUMMARY_TEXT = (cm.SUMMARY_HEADER + "gene\tgA#1#x\t200\t251\t5\t3\t3\t123\t2\tclosed\n" + "gB#1#y:7-7\tgB#1#y\t7\t7\t0\t0\t0\t0\t0\tnone\n" +
                     "nowhere:0-10\tnowhere\t0\t10\t0\t0\t0\t0\t0\tunknown\n" + "back\tgC#1#z\t5100\t5150\t3\t3\t3\t175\t2\tclosed\n")


def test_model_texts_of_the_hand_walk():
    text, kept = hand_paf()
    assert cm.paf_texts(text, kept, HAND_BED, 3, 10, 0, 3) == (HAND_TEXT, HAND_SUMMARY_TEXT)
    cut = cm.paf_texts(text, kept, HAND_BED, 2, 10, 0, 3)[1].split("\n")
    assert cut[1].endswith("\t2\tcut") and cut[4].endswith("\t2\tcut")
    kept_only = cm.paf_texts(text, kept, HAND_BED, 3, 10, 1, 3)[1].split("\n")
    assert kept_only[1] == "gene\tgA#1#x\t200\t251\t4\t2\t2\t88\t2\tclosed" and kept_only[4] == "back\tgC#1#z\t5100\t5150\t1\t1\t1\t50\t0\tnone"
    assert cm.paf_texts(text, kept, "", 3) == ("", cm.SUMMARY_HEADER)
    assert cm.genome_of("g#1#chr") == "g#1#" and cm.genome_of("plain") == "plain"


def test_interval_helpers_of_the_model():
    assert cm.merged([(0, 10), (10, 20)]) == [(0, 20)] and cm.merged([(0, 10), (11, 20)]) == [(0, 10), (11, 20)]
    assert cm.minus([(0, 100)], [(0, 5), (40, 60), (95, 100)]) == [(5, 40), (60, 95)]
    assert cm.minus([(0, 10), (20, 30)], [(5, 25)]) == [(0, 5), (25, 30)] and cm.minus([(3, 4)], []) == [(3, 4)]


@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib, lift
    structs = (("swg_closure_row", _lib.SwgClosureRow), ("swg_closure_summary", _lib.SwgClosureSummary), ("swg_closure_request", _lib.SwgClosureRequest))
    prints = ['printf("%%zu\\n", sizeof(%s));' % name for name, _ in structs]
    prints += ['printf("%%zu\\n", offsetof(%s, %s));' % (name, f) for name, cls in structs for f, _ in cls._fields_]
    prints += ['printf("%u\\n", SWG_CLOSURE_CUT);']
    prints += ['printf("%%zu\\n", sizeof(%s));' % s for s in ("swg_lift_request", "swg_lift_row", "swg_records")]
    prints.append('printf("%d\\n", SWG_ABI_VERSION);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(cls) for _, cls in structs] + [getattr(cls, f).offset for _, cls in structs for f, _ in cls._fields_]
    want += [cm.CUT, 56, 32, 128, 1]      # the structures that existed before keep their sizes
    assert got == want
    assert got[:3] == [24, 24, 80]
    for _, cls in structs:      # no implicit padding
        assert sum(C.sizeof(t) for _, t in cls._fields_) == C.sizeof(cls)
    for dtype, cls in ((lift.CLOSURE_ROW_DTYPE, _lib.SwgClosureRow), (lift.CLOSURE_SUMMARY_DTYPE, _lib.SwgClosureSummary)):
        assert dtype.itemsize == C.sizeof(cls)
        assert [dtype.fields[f][1] for f, _ in cls._fields_] == [getattr(cls, f).offset for f, _ in cls._fields_]
    assert lift.CLOSURE_CUT == cm.CUT


def test_symbols_are_exported_and_declared(lib):
    import sweepga_amd
    from sweepga_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_lift_closure_records", "swg_lift_closure_records_device", "swg_paf_lift_closure"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    assert lib.swg_abi_version() == 1
    for name in ("LiftClosure", "LiftClosureResult", "lift_closure_records", "lift_closure_records_device"):
        assert hasattr(sweepga_amd, name)
    assert "swg_lift_closure.hip" in build.SOURCES


def paf_closure(lib, paf, status, bed, hops=3, min_len=10, set_=0, axes=3, ctx=None, rows=True, summary=True):
    """-> (rc, rows text, summary text)"""
    p, n, _m = slots(rows, summary)
    bed = bed.encode()
    rc = lib.swg_paf_lift_closure(ctx, paf.handle, status.ctypes.data if status is not None else None, bed, len(bed), set_, axes, hops, min_len, p, n)
    text = [None, None]
    for k in range(2):
        if p[k]:
            text[k] = C.string_at(p[k], n[k]).decode()
            lib.swg_free(C.c_void_p(p[k]))
        else:
            assert n[k] == 0
    return rc, text[0], text[1]


def test_bed_path_on_a_record_free_paf_without_a_device(lib):
    """A PAF without records knows no name: every region is `unknown`, there are no rows, and no device is needed."""
    from sweepga_amd import LiftClosure, PafFile, SwgError
    for text in ("", "# nothing\nfew\tfields\n"):
        with PafFile(text=text) as paf:
            assert paf.n == 0
            want = cm.paf_texts(text, None, HAND_BED, 3, 10, 0, 3)
            assert want[0] == "" and want[1].count("\tunknown\n") == 4 and want[1].count("\n") == 5
            for st in (None, np.zeros(1, dtype=np.uint8)):
                assert paf_closure(lib, paf, st, HAND_BED) == (0,) + want
                assert paf_closure(lib, paf, st, "") == (0, "", cm.SUMMARY_HEADER)
            assert paf_closure(lib, paf, None, HAND_BED, rows=False) == (0, None, want[1])
            assert paf_closure(lib, paf, None, HAND_BED, summary=False) == (0, "", None)
            got = LiftClosure.from_paf(paf, None, HAND_BED, 3, 10, set="all")
            assert (got.text, got.summary_text) == want and len(got.rows) == 0 and list(got.summary["state"]) == ["unknown"] * 4
            for bed, line in MALFORMED:
                rc, r, s = paf_closure(lib, paf, None, bed)
                assert rc == -1 and r is None and s is None, bed
                assert ("swg_paf_lift_closure: BED line %d:" % line).encode() in lib.swg_alnstats_last_error(), (bed, lib.swg_alnstats_last_error())
                with pytest.raises(SwgError) as e2:
                    LiftClosure.from_paf(paf, None, bed, 2, set="all")
                assert e2.value.code == -1 and "line %d" % line in str(e2.value)


def records_of(cols, strand, n_seq):
    from sweepga_amd import _lib
    rec = _lib.SwgRecords()
    rec.n = len(strand)
    for k, a in cols.items():
        setattr(rec, k, a.ctypes.data if a.size else None)
    rec.strand = strand.ctypes.data if strand.size else None
    rec.n_seq = n_seq
    return rec


def test_refusals_that_need_no_device(lib):
    from sweepga_amd import LiftClosure, PafFile, SwgError, _lib
    from sweepga_amd.lift import CLOSURE_ROW_DTYPE, REGION_DTYPE
    cols, strand, kept, regions = hand_case()
    rec = records_of(cols, strand, 3)
    regs = np.array([(s, a, b, 0) for s, a, b in regions], dtype=REGION_DTYPE)
    status = kept.astype(np.uint8)
    poison = np.frombuffer(bytearray(b"\xab" * 24 * 4), dtype=CLOSURE_ROW_DTYPE)
    for fn in (lib.swg_lift_closure_records, lib.swg_lift_closure_records_device):     # a NULL context: there is no CPU path
        req = _lib.SwgClosureRequest()
        req.set, req.axes, req.max_hops, req.min_len, req.n, req.capacity, req.rows = 0, 3, 2, 10, 12345, 4, poison.ctypes.data
        assert fn(None, C.byref(rec), status.ctypes.data, regs.ctypes.data, len(regs), C.byref(req)) == -1
        assert poison.tobytes() == b"\xab" * 96 and req.n == 12345
    text, kept = hand_paf()
    st = kept.astype(np.uint8)
    with PafFile(text=text) as paf:
        assert paf_closure(lib, paf, st, HAND_BED)[0] == -1 and b"NULL context" in lib.swg_alnstats_last_error()
        assert paf_closure(lib, paf, st, "")[1:] == ("", cm.SUMMARY_HEADER)                         # no region: no device
        assert paf_closure(lib, paf, None, HAND_BED, set_=1)[0] == -1 and b"status" in lib.swg_alnstats_last_error()
        for set_, axes in ((2, 3), (0, 0), (0, 4), (1, 7)):
            assert paf_closure(lib, paf, st, HAND_BED, set_=set_, axes=axes)[0] == -1
        for hops in (0, 65536, 2**32 - 1):
            assert paf_closure(lib, paf, st, HAND_BED, hops=hops)[0] == -1 and b"max_hops" in lib.swg_alnstats_last_error()
            with pytest.raises(SwgError) as e:
                LiftClosure.from_paf(paf, st, HAND_BED, hops)
            assert e.value.code == -1
        assert paf_closure(lib, paf, st, HAND_BED, rows=False, summary=False)[0] == -1
        assert paf_closure(lib, paf, st, "a\t5\t1\n")[0] == -1 and b"line 1" in lib.swg_alnstats_last_error()      # the BED before the context
        p, n, _m = slots()
        assert lib.swg_paf_lift_closure(None, None, st.ctypes.data, b"", 0, 0, 3, 2, 10, p, n) == -1
        assert lib.swg_paf_lift_closure(None, paf.handle, st.ctypes.data, b"", 0, 0, 3, 2, 10, None, n) == -1
        assert lib.swg_paf_lift_closure(None, paf.handle, st.ctypes.data, None, 5, 0, 3, 2, 10, p, n) == -1
    with PafFile(text=REBASED) as paf:       # rebased columns: refused before the BED or a context is looked at
        with pytest.raises(SwgError) as e:
            LiftClosure.from_paf(paf, np.ones(1, dtype=np.uint8), "a\t5\t1\n", 2)
        assert e.value.code == -6 and "2^32" in str(e.value)


def test_command_line_usage_errors(lib, tmp_path):
    from sweepga_amd import build
    bed, bad, paf = tmp_path / "r.bed", tmp_path / "bad.bed", tmp_path / "in.paf"
    bed.write_text(HAND_BED)
    bad.write_text("gA#1#x\t1\t2\ngA#1#x\t9\t2\n")
    paf.write_text(hand_paf()[0])
    run = lambda *a: subprocess.run([build.CLI, str(paf), *a], capture_output=True, text=True)      # noqa: E731
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--lift-hops N", "--lift-closure FILE", "--lift-closure-summary FILE", "--lift-min-length N", "default 100", "rounded outward"):
        assert flag in r.stdout, flag
    for flag in ("--lift-closure", "--lift-closure-summary"):
        r = run(flag + "=")
        assert r.returncode == 2 and "empty value for " + flag in r.stderr, (flag, r.stderr)
    for flag in ("--lift-hops", "--lift-closure", "--lift-closure-summary", "--lift-min-length"):
        r = run(flag)
        assert r.returncode == 2 and flag in r.stderr
    for extra in (["--lift-closure", "x.tsv"], ["--lift-closure-summary", "x.tsv"], ["--lift-min-length", "5"]):     # ... without --lift-hops
        for more in ([], ["--lift-regions", str(bed), "--lift", str(tmp_path / "l.tsv")]):
            r = run(*extra, *more)
            assert r.returncode == 2 and "need --lift-hops" in r.stderr, (extra, r.stderr)
    r = run("--lift-hops", "2", "--lift-closure", "x.tsv")
    assert r.returncode == 2 and "--lift-hops needs --lift-regions" in r.stderr
    r = run("--lift-hops", "2", "--lift-regions", str(bed))
    assert r.returncode == 2 and "--lift-hops needs --lift-closure or --lift-closure-summary" in r.stderr
    r = run("--lift-hops", "2", "--lift-regions", str(bed), "--lift", str(tmp_path / "l.tsv"))      # (the one-hop output is not a closure output)
    assert r.returncode == 2 and "--lift-hops needs --lift-closure or --lift-closure-summary" in r.stderr
    for v in ("0", "65536", "-1", "two", "", "1.5", "99999999999999999999"):
        r = run("--lift-regions", str(bed), "--lift-closure", "x.tsv", "--lift-hops=" + v)
        assert r.returncode == 2 and "invalid value for --lift-hops" in r.stderr, (v, r.stderr)
    for v in ("-1", "x", "", "4294967296"):
        r = run("--lift-regions", str(bed), "--lift-closure", "x.tsv", "--lift-hops", "2", "--lift-min-length=" + v)
        assert r.returncode == 2 and "invalid value for --lift-min-length" in r.stderr, (v, r.stderr)
    r = run("--lift-regions", str(tmp_path / "missing.bed"), "--lift-hops", "2", "--lift-closure", "x.tsv")
    assert r.returncode == 2 and "cannot open" in r.stderr
    r = run("--lift-regions", str(bad), "--lift-hops", "2", "--lift-closure", str(tmp_path / "x.tsv"))
    assert r.returncode == 2 and "BED line 2" in r.stderr and "start > end" in r.stderr and not (tmp_path / "x.tsv").exists()
    assert r.stdout == "" and not (tmp_path / "l.tsv").exists()


def test_command_line_refuses_64_bit_columns_before_it_filters(lib, tmp_path):
    from sweepga_amd import build
    inp, out, rep, bed = tmp_path / "in.paf", tmp_path / "out.paf", tmp_path / "closure.out", tmp_path / "r.bed"
    inp.write_text(REBASED)
    bed.write_text("a#1#x\t0\t10\n")
    for flag in ("--lift-closure", "--lift-closure-summary"):
        for extra in ([], ["--no-filter"]):
            r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--lift-regions", str(bed), "--lift-hops", "3", flag, str(rep), *extra],
                               capture_output=True, text=True)
            assert r.returncode == 3 and "2^32" in r.stderr, r.stderr
            assert r.stdout == "" and not out.exists() and not rep.exists()
