"""The base-exact lift without a GPU: the brute-force model of tests/lift_exact_model.py against rows worked out by hand, and the
host side of the feature -- header, ctypes mirrors, exported symbols, the no-device paths of swg_paf_lift_exact, the usage errors of
--lift-exact, and the tag finder and row formatter under the host sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import lift_exact_model as em
from tests import lift_model as lm
from tests.test_lift_cpu import HAND_BED, MALFORMED, REBASED, hand_paf, slots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B = 0, 1
G = "5=2I6=4D5X2="       # x: 5 = | 2 I | 6 = | (4 D) | 5 X | 2 =   -> 20;   y: 5 = | 6 = | 4 D | 5 X | 2 =   -> 22
H = "3I4=2I3D2=1I"       # begins and ends with I, an I directly followed by a D: x 12, y 9


def hand_case():
    """Twelve records, query on A and target on B: (qs, qe, ts, te, strand, CIGAR or None = outside the set)
       0  100  120 1000 1022 +  G     columns (x, y): = (0-4, 0-4), I x 5-6, = (7-12, 5-10), D y 11-14, X (13-17, 15-19), = (18-19, 20-21)
       1  200  220 2000 2022 -  G     the same walk; query coordinate 219 - x
       2  300  310 3000 3010 +  10M   M only: matches 0
       3  400  412 4000 4009 +  H     I x 0-2, = (3-6, 0-3), I x 7-8, D y 4-6, = (9-10, 7-8), I x 11
       4  500  512 5000 5009 -  H     query coordinate 511 - x
       5  600  610 6000 6010 +  5=x5=          state 1 (a foreign byte)
       6  620  630 6020 6030 +  4294967296D10= state 2
       7  640  650 6040 6049 +  9=             state 4 (x = 9, Lq = 10; y = 9 = Lt)
       8  660  669 6060 6070 +  9=             state 8
       9  680  690 6080 6090 +  (empty)        state 16
      10  700  710 6100 6110 +  outside the set
      11 1100 1104 1100 1107 +  2D4=1D  begins and ends with D: columns (0-3, 2-5)
    Regions and the exact rows (dst_start, dst_end, aligned, matches):
       0  A 102 104   record 0: x 2-3, inside the first = run                       -> 1002 1004  2 2
       1  A 103 106   x 3-5: ends inside the I; columns x 3, 4                      -> 1003 1005  2 2
       2  A 105 107   wholly inside the I, B = x 0-4: p = 1004 + 1                  -> 1005 1005  0 0
       3  B 1009 1013 target axis, y 9-12: ends inside the D; columns y 9, 10 = x 11, 12 -> 111 113  2 2
       4  B 1012 1014 wholly inside the D, B = y < 12: the last is y 10 = x 12: p = 112 + 1 -> 113 113  0 0
       5  A 110 116   x 10-15: = x 10-12 (y 8-10), X x 13-15 (y 15-17)               -> 1008 1018  6 3
       6  A 202 204   record 1, '-': x = 219 - 203 .. 219 - 202 = 16, 17: X, y 18, 19  -> 2018 2020  2 0
       7  A 213 215   '-': x 5, 6: the I.  B = coordinates < 213 = x > 6: the first is x 7 = y 5: p = min dst = 2005 -> 2005 2005 0 0
       8  A 400 403   record 3: the leading I, B empty: p = d0                       -> 4000 4000  0 0
       9  A 500 501   record 4, '-': x 11, the trailing I; no coordinate < 500: B empty: p = d1 -> 5009 5009 0 0
      10  A 407 409   record 3: x 7, 8, the I in front of the D; B ends at x 6 = y 3: p = 4004 -> 4004 4004 0 0
      11  A 509 512   record 4, '-': x 0-2, the leading I; B = x > 2: the first is x 3 = y 0: p = 5000 -> 5000 5000 0 0
      12  A 600 1000  records 5-10 whole: interpolated rows, [ts, te), aligned = matches = 0
      13  B 1100 1107 record 11 on the target axis, whole: y 2-5 = x 0-3              -> 1100 1104  4 4
      14  B 1100 1102 the leading D, B empty, '+': p = d0 = the query's start        -> 1100 1100  0 0
      15  A 302 305   record 2                                                        -> 3002 3005  3 0
      16  A 404 412   record 3: x 4-11: = x 4-6 (y 1-3), = x 9-10 (y 7-8)             -> 4001 4009  5 5
    -> (cols, strand, regions, cigars {record: text}, rows, states)"""
    recs = [(100, 120, 1000, 1022, 0, G), (200, 220, 2000, 2022, 1, G), (300, 310, 3000, 3010, 0, "10M"), (400, 412, 4000, 4009, 0, H),
            (500, 512, 5000, 5009, 1, H), (600, 610, 6000, 6010, 0, "5=x5="), (620, 630, 6020, 6030, 0, "4294967296D10="),
            (640, 650, 6040, 6049, 0, "9="), (660, 669, 6060, 6070, 0, "9="), (680, 690, 6080, 6090, 0, ""), (700, 710, 6100, 6110, 0, None),
            (1100, 1104, 1100, 1107, 0, "2D4=1D")]
    n = len(recs)
    cols = {"q_id": np.full(n, A, dtype=np.uint32), "t_id": np.full(n, B, dtype=np.uint32)}
    for i, k in enumerate(("q_start", "q_end", "t_start", "t_end")):
        cols[k] = np.array([r[i] for r in recs], dtype=np.uint32)
    strand = np.array([r[4] for r in recs], dtype=np.uint8)
    cigars = {i: r[5] for i, r in enumerate(recs) if r[5] is not None}
    regions = [(A, 102, 104), (A, 103, 106), (A, 105, 107), (B, 1009, 1013), (B, 1012, 1014), (A, 110, 116), (A, 202, 204), (A, 213, 215),
               (A, 400, 403), (A, 500, 501), (A, 407, 409), (A, 509, 512), (A, 600, 1000), (B, 1100, 1107), (B, 1100, 1102), (A, 302, 305),
               (A, 404, 412)]
    E = em.EXACT
    #        region record ca cb dst_seq dst_start dst_end flags aligned matches
    rows = [(0, 0, 102, 104, B, 1002, 1004, E, 2, 2), (1, 0, 103, 106, B, 1003, 1005, E, 2, 2), (2, 0, 105, 107, B, 1005, 1005, E, 0, 0),
            (3, 0, 1009, 1013, A, 111, 113, E | 2, 2, 2), (4, 0, 1012, 1014, A, 113, 113, E | 2, 0, 0), (5, 0, 110, 116, B, 1008, 1018, E, 6, 3),
            (6, 1, 202, 204, B, 2018, 2020, E | 1, 2, 0), (7, 1, 213, 215, B, 2005, 2005, E | 1, 0, 0), (8, 3, 400, 403, B, 4000, 4000, E, 0, 0),
            (9, 4, 500, 501, B, 5009, 5009, E | 1, 0, 0), (10, 3, 407, 409, B, 4004, 4004, E, 0, 0), (11, 4, 509, 512, B, 5000, 5000, E | 1, 0, 0),
            (12, 5, 600, 610, B, 6000, 6010, 0, 0, 0), (12, 6, 620, 630, B, 6020, 6030, 0, 0, 0), (12, 7, 640, 650, B, 6040, 6049, 0, 0, 0),
            (12, 8, 660, 669, B, 6060, 6070, 0, 0, 0), (12, 9, 680, 690, B, 6080, 6090, 0, 0, 0), (12, 10, 700, 710, B, 6100, 6110, 0, 0, 0),
            (13, 11, 1100, 1107, A, 1100, 1104, E | 2, 4, 4), (14, 11, 1100, 1102, A, 1100, 1100, E | 2, 0, 0), (15, 2, 302, 305, B, 3002, 3005, E, 3, 0),
            (16, 3, 404, 412, B, 4001, 4009, E, 5, 5)]
    states = {0: 0, 1: 0, 2: 0, 3: 0, 4: 0, 5: 1, 6: 2, 7: 4, 8: 8, 9: 16, 11: 0}
    return cols, strand, regions, cigars, rows, states


def test_model_against_rows_worked_out_by_hand():
    cols, strand, regions, cigars, rows, states = hand_case()
    got, summary, got_states = em.lift_exact(cols, strand, None, regions, cigars, 0, 3)
    assert got == rows
    assert got_states == states
    plain, plain_summary = lm.lift(cols, strand, None, regions, 0, 3)
    assert np.array_equal(summary, plain_summary)
    assert [r[:5] for r in got] == [r[:5] for r in plain]                          # hits, clips and order are the lift's
    assert [g[:8] for g in got if not g[7] & em.EXACT] == [p for g, p in zip(got, plain) if not g[7] & em.EXACT]
    for axes in (1, 2):
        assert em.lift_exact(cols, strand, None, regions, cigars, 0, axes)[0] == [r for r in rows if (r[7] >> 1 & 1) == axes - 1]
    kept = np.arange(len(strand)) % 2 == 0
    assert em.lift_exact(cols, strand, kept, regions, cigars, 1, 3)[0] == [r for r in rows if kept[r[1]]]
    assert em.lift_exact(cols, strand, None, regions, {}, 0, 3)[0] == [p + (0, 0) for p in plain]      # no set: every row interpolated
    assert em.hit_records(got) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]


def test_the_parser_of_the_model():
    assert em.parse("0M4294967295D3=") == (0, [(0, "M"), (2**32 - 1, "D"), (3, "=")])
    assert em.parse("4294967296D3=") == (em.VALUE, [(3, "=")])
    assert em.parse("12345678901M3=") == (em.SYNTAX, [(3, "=")])                     # 11 digits: syntax, whatever the value
    assert em.parse("M3=") == (em.SYNTAX, [(3, "=")])
    assert em.parse("3=5") == (em.SYNTAX, [(3, "=")])
    assert em.parse("3m2=") == (em.SYNTAX, [(2, "=")])
    assert em.parse("3=\t2=")[0] == em.SYNTAX
    assert em.entry_state("", 0, 0) == em.EMPTY and em.entry_state("0M", 0, 0) == 0
    assert em.entry_state("3=2I", 5, 3) == 0 and em.entry_state("3=2I", 5, 4) == em.T_SUM and em.entry_state("3=2I", 4, 4) == em.Q_SUM | em.T_SUM
    assert em.entry_state("3=x", 3, 3) == em.SYNTAX                                   # the sums are not looked at behind an error
    assert em.entry_state(str(2**32 - 1) + "D" + str(2**32 - 1) + "D", 0, 2**33 - 2) == 0      # 64-bit sums


def test_single_m_is_the_interpolated_lift():
    rng = np.random.default_rng(11)
    n = 40
    L = rng.integers(1, 60, n)
    cols = {"q_id": np.zeros(n, dtype=np.uint32), "t_id": np.ones(n, dtype=np.uint32), "q_start": rng.integers(0, 300, n).astype(np.uint32),
            "t_start": rng.integers(0, 300, n).astype(np.uint32)}
    cols["q_end"] = (cols["q_start"] + L).astype(np.uint32)
    cols["t_end"] = (cols["t_start"] + L).astype(np.uint32)
    strand = rng.integers(0, 2, n).astype(np.uint8)
    regions = [(int(s), int(a), int(a + w)) for s, a, w in zip(rng.integers(0, 2, 60), rng.integers(0, 350, 60), rng.integers(0, 40, 60))]
    cigars = {i: "%dM" % L[i] for i in range(n)}
    rows, _, states = em.lift_exact(cols, strand, None, regions, cigars, 0, 3)
    plain, _ = lm.lift(cols, strand, None, regions, 0, 3)
    assert len(rows) > 50 and set(states.values()) == {0}
    assert [r[:7] + (r[7] & 3,) for r in rows] == plain
    assert all(r[7] & em.EXACT and r[8] == r[3] - r[2] and r[9] == 0 for r in rows)


@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib, lift
    structs = (("swg_cigar_set", _lib.SwgCigarSet), ("swg_lift_exact_row", _lib.SwgLiftExactRow), ("swg_lift_exact_request", _lib.SwgLiftExactRequest),
               ("swg_lift_row", _lib.SwgLiftRow), ("swg_lift_request", _lib.SwgLiftRequest))
    prints = ['printf("%%zu\\n", sizeof(%s));' % name for name, _ in structs]
    prints += ['printf("%%zu\\n", offsetof(%s, %s));' % (name, f) for name, cls in structs for f, _ in cls._fields_]
    prints += ['printf("%u %u %u %u %u %u %u %u\\n", SWG_LIFT_MINUS, SWG_LIFT_ON_TARGET, SWG_LIFT_EXACT, SWG_CIGAR_SYNTAX, SWG_CIGAR_VALUE, '
               'SWG_CIGAR_QUERY_SUM, SWG_CIGAR_TARGET_SUM, SWG_CIGAR_EMPTY);']
    prints.append('printf("%zu %d\\n", sizeof(swg_records), SWG_ABI_VERSION);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(cls) for _, cls in structs] + [getattr(cls, f).offset for _, cls in structs for f, _ in cls._fields_]
    want += [1, 2, 4, 1, 2, 4, 8, 16, 128, 1]
    assert got == want
    assert got[:5] == [32, 40, 88, 32, 56]
    for _, cls in structs:      # no implicit padding
        assert sum(C.sizeof(t) for _, t in cls._fields_) == C.sizeof(cls)
    assert lift.EXACT_ROW_DTYPE.itemsize == 40 and lift.EXACT_ROW_DTYPE.names[:8] == lift.ROW_DTYPE.names
    assert [lift.EXACT_ROW_DTYPE.fields[f][1] for f, _ in _lib.SwgLiftExactRow._fields_] == [getattr(_lib.SwgLiftExactRow, f).offset
                                                                                           for f, _ in _lib.SwgLiftExactRow._fields_]
    assert (lift.EXACT, lift.CIGAR_EMPTY) == (em.EXACT, em.EMPTY)


def test_symbols_are_exported_and_declared(lib):
    import sweepga_amd
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_lift_exact_records", "swg_lift_exact_records_device", "swg_lift_hit_records", "swg_lift_hit_records_device", "swg_paf_lift_exact"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    assert lib.swg_abi_version() == 1
    for name in ("LiftExactResult", "lift_exact_records", "lift_exact_records_device", "lift_hit_records", "lift_hit_records_device"):
        assert hasattr(sweepga_amd, name)


def paf_lift_exact(lib, paf, status, bed, set_=0, axes=3, ctx=None, rows=True, summary=True):
    """-> (rc, rows text, summary text)"""
    p, n, _m = slots(rows, summary)
    bed = bed.encode()
    rc = lib.swg_paf_lift_exact(ctx, paf.handle, status.ctypes.data if status is not None else None, bed, len(bed), set_, axes, p, n)
    text = [None, None]
    for k in range(2):
        if p[k]:
            text[k] = C.string_at(p[k], n[k]).decode()
            lib.swg_free(C.c_void_p(p[k]))
        else:
            assert n[k] == 0
    return rc, text[0], text[1]


def test_paf_lift_exact_without_a_device(lib):
    """An empty BED, a record-free PAF and a malformed BED need no device; the refusals come before a context is looked at."""
    from sweepga_amd import Lift, PafFile, SwgError
    for text in ("", "# nothing\nfew\tfields\n"):
        with PafFile(text=text) as paf:
            for st in (None, np.zeros(1, dtype=np.uint8)):
                assert paf_lift_exact(lib, paf, st, HAND_BED) == (0, "", lm.SUMMARY_HEADER)
                assert paf_lift_exact(lib, paf, st, "") == (0, "", lm.SUMMARY_HEADER)
            assert paf_lift_exact(lib, paf, None, HAND_BED, rows=False) == (0, None, lm.SUMMARY_HEADER)
            assert paf_lift_exact(lib, paf, None, HAND_BED, summary=False) == (0, "", None)
            got = Lift.from_paf(paf, None, HAND_BED, set="all", exact=True)
            assert (got.text, got.summary_text, got.exact_counts) == ("", lm.SUMMARY_HEADER, (0, 0, 0, 0))
            assert em.paf_texts(text, None, HAND_BED, 0, 3) == ("", lm.SUMMARY_HEADER, (0, 0, 0, 0))
            assert len(got.rows) == 0 and got.rows.dtype.names[-3:] == ("aligned", "matches", "mode")
            for bed, line in MALFORMED:
                rc, r, s = paf_lift_exact(lib, paf, None, bed)
                assert rc == -1 and r is None and s is None, bed
                err = lib.swg_alnstats_last_error()
                assert ("BED line %d:" % line).encode() in err and b"swg_paf_lift_exact:" in err, (bed, err)
                with pytest.raises(SwgError):
                    Lift.from_paf(paf, None, bed, set="all", exact=True)
    text, kept = hand_paf()
    st = kept.astype(np.uint8)
    with PafFile(text=text) as paf:
        assert paf_lift_exact(lib, paf, st, HAND_BED)[0] == -1 and b"swg_paf_lift_exact: NULL context" in lib.swg_alnstats_last_error()
        assert paf_lift_exact(lib, paf, st, "")[1:] == ("", lm.SUMMARY_HEADER)                   # no region: no device
        assert paf_lift_exact(lib, paf, None, HAND_BED, set_=1)[0] == -1 and b"status" in lib.swg_alnstats_last_error()
        for set_, axes in ((2, 3), (0, 0), (0, 4), (1, 7)):
            assert paf_lift_exact(lib, paf, st, HAND_BED, set_=set_, axes=axes)[0] == -1
        assert paf_lift_exact(lib, paf, st, HAND_BED, rows=False, summary=False)[0] == -1
        p, n, _m = slots()
        assert lib.swg_paf_lift_exact(None, None, st.ctypes.data, b"", 0, 0, 3, p, n) == -1
        assert lib.swg_paf_lift_exact(None, paf.handle, st.ctypes.data, None, 5, 0, 3, p, n) == -1
    with PafFile(text=REBASED) as paf:
        with pytest.raises(SwgError) as e:
            Lift.from_paf(paf, np.ones(1, dtype=np.uint8), "a\t5\t1\n", exact=True)
        assert e.value.code == -6 and "2^32" in str(e.value)


def test_record_seams_refuse_without_a_device(lib):
    """A NULL context: there is no CPU path, and nothing the caller owns is touched."""
    from sweepga_amd import _lib
    from sweepga_amd.lift import EXACT_ROW_DTYPE, REGION_DTYPE, cigar_set
    cols, strand, regions, cigars, _, _ = hand_case()
    rec = _lib.SwgRecords()
    rec.n = len(strand)
    for k, a in cols.items():
        setattr(rec, k, a.ctypes.data)
    rec.strand = strand.ctypes.data
    rec.n_seq = 2
    regs = np.array([(s, a, b, 0) for s, a, b in regions], dtype=REGION_DTYPE)
    record, offset, text = cigar_set(sorted(cigars), [cigars[i] for i in sorted(cigars)])
    cs = _lib.SwgCigarSet()
    cs.record, cs.offset, cs.text, cs.k = record.ctypes.data, offset.ctypes.data, text.ctypes.data, len(record)
    poison = np.frombuffer(bytearray(b"\xab" * 40 * 4), dtype=EXACT_ROW_DTYPE)
    for fn in (lib.swg_lift_exact_records, lib.swg_lift_exact_records_device):
        req = _lib.SwgLiftExactRequest()
        req.set, req.axes, req.n, req.capacity, req.rows, req.ops = 0, 3, 12345, 4, poison.ctypes.data, 77
        assert fn(None, C.byref(rec), None, regs.ctypes.data, len(regs), C.byref(cs), C.byref(req)) == -1
        assert poison.tobytes() == b"\xab" * 160 and req.n == 12345 and req.ops == 77
    out = np.full(4, 0xabababab, dtype=np.uint32)
    k = C.c_uint64(99)
    for fn in (lib.swg_lift_hit_records, lib.swg_lift_hit_records_device):
        assert fn(None, C.byref(rec), None, regs.ctypes.data, len(regs), 0, 3, out.ctypes.data, 4, C.byref(k)) == -1
        assert k.value == 99 and (out == 0xabababab).all()


def test_command_line_usage_errors(lib, tmp_path):
    from sweepga_amd import build
    bed, paf = tmp_path / "r.bed", tmp_path / "in.paf"
    bed.write_text(HAND_BED)
    paf.write_text(hand_paf()[0])
    out = tmp_path / "out.paf"
    run = lambda *a: subprocess.run([build.CLI, str(paf), "--output-file", str(out), *a], capture_output=True, text=True)      # noqa: E731
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--lift-exact" in r.stdout and "aligned matches mode" in r.stdout
    for extra in ([], ["--lift-regions", str(bed), "--lift-summary", str(tmp_path / "s.tsv")], ["--lift", str(tmp_path / "x.tsv")],
                  ["--lift-regions", str(bed), "--lift-hops", "2", "--lift-closure", str(tmp_path / "c.tsv")]):
        r = run("--lift-exact", *extra)
        assert r.returncode == 2, (extra, r.stderr)
        assert "--lift-exact needs --lift-regions and --lift" in r.stderr or "need --lift-regions" in r.stderr, (extra, r.stderr)
        assert r.stdout == "" and not out.exists() and not (tmp_path / "s.tsv").exists() and not (tmp_path / "x.tsv").exists()
    r = run("--lift-exact", "--lift-regions", str(tmp_path / "missing.bed"), "--lift", str(tmp_path / "x.tsv"))
    assert r.returncode == 2 and "cannot open" in r.stderr and not out.exists()


# ---- the tag finder and the row formatter --------------------------------------------------------------------------------------------
FIELDS12 = "q\t100\t0\t50\t+\tt\t100\t0\t50\t50\t50\t60"
TAG_LINES = [
    (FIELDS12 + "\tcg:Z:50=", "50="),                                          # the tag first (and last)
    (FIELDS12 + "\tcg:Z:50=\ttp:A:P\tdv:f:0.01", "50="),                       # first, others behind
    (FIELDS12 + "\ttp:A:P\tcg:Z:20=1X29=", "20=1X29="),                        # last
    (FIELDS12 + "\tcg:Z:50M\ttp:A:P\tcg:Z:49=1X\tnm:i:1", "49=1X"),            # twice: the last one counts
    (FIELDS12 + "\ttp:A:P\tcg:Z:", ""),                                        # cg:Z: as the line's final bytes: an empty value
    (FIELDS12 + "\tcg:Z:\ttp:A:P", ""),
    (FIELDS12 + "\ttp:A:P", None),                                             # no tag
    (FIELDS12, None),
    (FIELDS12 + "\txx:Z:cg:Z:5M\tyy:Z:a cg:Z:7M", None),                       # the prefix inside other tags' values
    (FIELDS12 + "\tcg:Z:50=\txx:Z:cg:Z:5M", "50="),
    (FIELDS12 + "\txcg:Z:5M\tcg:Z", None),
    ("cg:Z:1=\t100\t0\t50\t+\tcg:Z:2=\t100\t0\t50\t50\t50\tcg:Z:3=", None),    # in the first twelve fields: no tag
    (FIELDS12 + "\tcg:Z:50=\r", "50="),                                        # a carriage return is no part of the value
    (FIELDS12 + "\tcg:Z:3=\t", "3="),
    ("", None), ("\t", None), ("cg:Z:", None),
]


def test_tag_finder_and_formatter_under_the_host_sanitizers(tmp_path):
    """tests/native/cigar_text_check.cpp: a stand-alone program over csrc/host/cigar_text.cpp, built with the address and
    undefined-behaviour sanitizers; its answers must be the model's byte for byte."""
    exe = str(tmp_path / "cigar_text_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "cigar_text_check.cpp"),
                           os.path.join(ROOT, "sweepga_amd", "csrc", "host", "cigar_text.cpp")])
    names = ["a#1#x", "", "c#2#z"]      # the program's own table
    top = 2**32 - 1
    rows = [(0, 7, 10, 20, 2, 110, 120, 4, 10, 9, "gene", "a#1#x"), (1, 0, 0, 1, 0, 5, 5, 1, 0, 0, "a#1#x:0-1", "a#1#x"),
            (top, top, top, top, 1, top, top, 7, top, top, "", ""), (2, 3, 4, 5, 2, 6, 7, 2, 0, 0, "l", "s")]
    feed, want = [], []
    for line, value in TAG_LINES:
        assert em.last_cigar_tag(line) == value, line
        feed += ["T", line]
        want.append("0\n" if value is None else "1\t" + value + "\n")
    for r in rows:
        feed += ["R", " ".join(str(v) for v in r[:10]), r[10], r[11]]
        want.append("\t".join([names[r[4]], str(r[5]), str(r[6]), r[10], r[11], str(r[2]), str(r[3]), "-" if r[7] & 1 else "+",
                               "t" if r[7] & 2 else "q", str(r[1]), str(r[8]), str(r[9]), "exact" if r[7] & 4 else "interp"]) + "\n")
    r = subprocess.run([exe], input=("\n".join(feed) + "\n").encode(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.decode() == "".join(want)
    assert "\t4294967295\t4294967295\texact\n" in r.stdout.decode()
