"""The gaps model (tests/gaps_model.py) against answers worked out by hand, then under the oracle's status and chain on the
hand-derived scaffold fixtures of tests/kat_scaffold.py and on tests/golden/syeast.paf.gz, and the host side of the feature:
structure layout, symbols, the command line's usage errors, the calls that need no device.  No GPU."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import blocks_model as bm
from tests import gaps_model as gm
from tests import kat_scaffold as K
from tests import orc
from tests.test_blocks_cpu import kat_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, R = 1, 2
E, I, D, V = gm.EVEN, gm.INS, gm.DEL, gm.INV


def columns(records):
    """records: (q_id, t_id, q_start, q_end, t_start, t_end, strand) per record."""
    a = np.asarray(records, dtype=np.int64).reshape(-1, 7)
    return {k: a[:, j].astype(np.uint8 if k == "strand" else np.uint32) for j, k in enumerate(gm.COLUMNS)}


def hand_case():
    """-> (columns, status, chain, seq_genome, every link and inversion in row order as (FIELDS..., dq, dt, size)).
    Sequences 0..5, genomes: 0, 1 -> 0; 2, 3 -> 1; 4, 5 -> 2.  Chains 3, 4, 6, 8 and 9."""
    rec = [
        # chain 3, '+' on (0, 2): r0 -> r2 an insertion of 80, r2 -> r4 a deletion of 30; r1 rescued and r3 chain-less, both ignored
        (0, 2, 100, 200, 1000, 1100, 0),    # r0
        (0, 2, 210, 220, 1110, 1120, 0),    # r1 RESCUED: between r0 and r2 in q_start, takes no part
        (0, 2, 300, 400, 1120, 1220, 0),    # r2: dq = 300 - 200 = 100, dt = 1120 - 1100 = 20, size +80
        (0, 2, 410, 420, 1230, 1240, 0),    # r3 SCAFFOLD without a chain: takes no part
        (0, 2, 450, 500, 1300, 1350, 0),    # r4: dq = 450 - 400 = 50, dt = 1300 - 1220 = 80, size -30
        # chain 4, '-' on (1, 3): dt = t_start[a] - t_end[b].  In INPUT order the later record comes first.
        (1, 3, 2000, 2100, 5000, 5100, 1),  # r5 second in q_start
        (1, 3, 1000, 1500, 5400, 5900, 1),  # r6 first: dq = 2000 - 1500 = 500, dt = 5400 - 5100 = 300, size +200
        # chain 6, '+' on (4, 0): overlaps.  r7 -> r8 overlaps on the query (flag 1), r8 -> r9 on the target (flag 2),
        # r9 -> r10 on both (flags 3) with size 0
        (4, 0, 0, 1000, 0, 1000, 0),        # r7
        (4, 0, 900, 2000, 1010, 2100, 0),   # r8: dq = -100, dt = 10, size -110
        (4, 0, 2050, 3000, 2000, 3000, 0),  # r9: dq = 50, dt = -100, size +150
        (4, 0, 2990, 4000, 2990, 4000, 0),  # r10: dq = -10, dt = -10, size 0
        # chain 8, '+' on (2, 5): a captured inversion between two core records -- the link skips it, its row sorts between
        (2, 5, 100, 200, 100, 200, 0),      # r11 core
        (2, 5, 220, 290, 150, 220, 1),      # r12 inverted, 70 bases of query
        (2, 5, 300, 400, 240, 340, 0),      # r13 core: a = r11, dq = 100, dt = 40, size +60
        (2, 5, 250, 260, 500, 510, 1),      # r14 inverted, 10 bases: q_start between r12 and r13
        # chain 9, '-' on (5, 4): ties in q_start, broken by index: order r15, r16, r17
        (5, 4, 700, 800, 900, 1000, 1),     # r15
        (5, 4, 700, 750, 700, 800, 1),      # r16: a = r15, dq = 700 - 800 = -100, dt = 900 - 800 = 100, size -200
        (5, 4, 700, 720, 100, 200, 1),      # r17: a = r16, dq = 700 - 750 = -50, dt = 700 - 200 = 500, size -550
    ]
    status = np.array([S, R, S, S, S, S, S, S, S, S, S, S, S, S, S, S, S, S], dtype=np.uint8)
    chain = np.array([3, 3, 3, 0, 3, 4, 4, 6, 6, 6, 6, 8, 8, 8, 8, 9, 9, 9], dtype=np.uint32)
    seq_genome = np.array([0, 0, 1, 1, 2, 2], dtype=np.uint32)
    want = [
        # chain left right q_lo q_hi t_lo t_hi kind flags | dq dt size
        (3, 0, 2, 200, 300, 1100, 1120, I, 0, 100, 20, 80),
        (3, 2, 4, 400, 450, 1220, 1300, D, 0, 50, 80, -30),
        (4, 6, 5, 1500, 2000, 5100, 5400, I, 0, 500, 300, 200),
        (6, 7, 8, 900, 1000, 1000, 1010, D, 1, -100, 10, -110),
        (6, 8, 9, 2000, 2050, 2000, 2100, I, 2, 50, -100, 150),
        (6, 9, 10, 2990, 3000, 2990, 3000, E, 3, -10, -10, 0),
        (8, 12, 12, 220, 290, 150, 220, V, 0, 0, 0, 70),
        (8, 14, 14, 250, 260, 500, 510, V, 0, 0, 0, 10),
        (8, 11, 13, 200, 300, 200, 240, I, 0, 100, 40, 60),
        (9, 15, 16, 700, 800, 800, 900, D, 1, -100, 100, -200),
        (9, 16, 17, 700, 750, 200, 700, D, 1, -50, 500, -550),
    ]
    return columns(rec), status, chain, seq_genome, want


def full(rows):
    return [tuple(int(e[f]) for f in gm.FIELDS + ("dq", "dt", "size")) for e in rows]


def test_model_against_hand_derived_answers():
    cols, status, chain, genome, want = hand_case()
    assert full(gm.gaps(cols, status, chain, 0)) == want                                       # min_size 0: every link, EVEN included
    assert full(gm.gaps(cols, status, chain, 50)) == [w for w in want if abs(w[-1]) >= 50]     # drops -30, 0 and the 10-base inversion
    assert [w[-1] for w in full(gm.gaps(cols, status, chain, 50))] == [80, 200, -110, 150, 70, 60, -200, -550]
    assert gm.gaps(cols, status, chain, 551) == [] and len(gm.gaps(cols, status, chain, 550)) == 1      # above every size
    assert gm.gaps(cols, status, chain, 2**32 - 1) == []
    # EVEN only with min_size 0
    assert [w for w in full(gm.gaps(cols, status, chain, 1)) if w[7] == E] == []
    # the rescued and the chain-less record change nothing: without them the rows are the same
    keep = np.array([i for i in range(len(status)) if i not in (1, 3)])
    renumber = {int(old): new for new, old in enumerate(keep)}
    got = full(gm.gaps({k: v[keep] for k, v in cols.items()}, status[keep], chain[keep], 0))
    assert got == [w[:1] + (renumber[w[1]], renumber[w[2]]) + w[3:] for w in want]


def test_model_summary_and_spectrum_by_hand():
    cols, status, chain, genome, _ = hand_case()
    pairs, spectrum = gm.summary(cols, status, chain, genome, 50)
    # genome pairs: chain 3 (0,1); chain 4 (0,1); chain 6 (2,0); chain 8 (1,2); chain 9 (2,2)
    assert pairs == [
        (0, 1, 3, 2, 280, 0, 0, 0, 0),       # links r0-r2 (+80), r2-r4 (-30: below 50, a link all the same), r6-r5 (+200)
        (1, 2, 1, 1, 60, 0, 0, 1, 70),       # the 10-base inversion is below 50
        (2, 0, 3, 1, 150, 1, 110, 0, 0),     # the EVEN link counts as a link only
        (2, 2, 2, 0, 0, 2, 750, 0, 0),
    ]
    ins, dele = spectrum
    assert {b: c for b, c in enumerate(ins) if c} == {6: 1, 7: 1, 8: 2}      # 60 has 6 bits, 80 has 7, 200 and 150 have 8
    assert {b: c for b, c in enumerate(dele) if c} == {7: 1, 8: 1, 10: 1}    # 110, 200, 550
    pairs0, spectrum0 = gm.summary(cols, status, chain, genome, 0)
    assert pairs0[0] == (0, 1, 3, 2, 280, 1, 30, 0, 0) and pairs0[1] == (1, 2, 1, 1, 60, 0, 0, 2, 80)
    assert sum(spectrum0[0]) == 4 and sum(spectrum0[1]) == 4 and spectrum0[0][0] == spectrum0[1][0] == 0     # EVEN is not counted
    none, spectrum_none = gm.summary(cols, status, chain, genome, 2**32 - 1)
    assert [p[:3] for p in none] == [(0, 1, 3), (1, 2, 1), (2, 0, 3), (2, 2, 2)] and all(sum(p[3:]) == 0 for p in none)
    assert gm.bit_length_bin(1) == 1 and gm.bit_length_bin(2**31 - 1) == 31 and gm.bit_length_bin(2**31) == 32 and gm.bit_length_bin(2**33 - 2) == 32


def test_model_order_and_the_index_tie_break():
    cols, status, chain, genome, want = hand_case()
    # under a permutation that keeps the tied records r15, r16, r17 in their order the rows are the same, indices mapped
    perm = np.array([9, 3, 13, 0, 15, 7, 12, 1, 16, 5, 10, 2, 17, 6, 14, 4, 11, 8])
    where = {int(old): new for new, old in enumerate(perm)}
    assert where[15] < where[16] < where[17]
    got = full(gm.gaps({k: v[perm] for k, v in cols.items()}, status[perm], chain[perm], 0))
    assert got == [w[:1] + (where[w[1]], where[w[2]]) + w[3:] for w in want]
    # swapping two tied records swaps their roles: the index breaks the tie
    swap = np.arange(len(status))
    swap[[15, 16]] = [16, 15]
    got = full(gm.gaps({k: v[swap] for k, v in cols.items()}, status[swap], chain[swap], 0))
    assert got[-2][:3] == (9, 15, 16) and got[-2][-3:] == (700 - 750, 700 - 1000, -50 + 300)


def test_model_refuses_a_chain_over_two_pairs():
    cols, status, chain, genome, _ = hand_case()
    cols["t_id"][2] = 3
    with pytest.raises(gm.GapError):
        gm.gaps(cols, status, chain, 0)


def test_texts_written_out():
    cols, status, chain, genome, _ = hand_case()
    names = ["a#1#c1", "a#1#c2", "b#1#c1", "b#1#c2", "c#1#c1", "c#1#c2"]
    text = gm.rows_text(gm.gaps(cols, status, chain, 100), cols, names).decode().split("\n")
    assert text[0] == "#query\tq_start\tq_end\ttarget\tt_start\tt_end\tkind\tsize\tchain\tdq\tdt\tleft\tright"
    assert text[1] == "a#1#c2\t1500\t2000\tb#1#c2\t5100\t5400\tINS\t200\t4\t500\t300\t6\t5"
    assert text[2] == "c#1#c1\t900\t1000\ta#1#c1\t1000\t1010\tDEL\t-110\t6\t-100\t10\t7\t8"
    text = gm.rows_text(gm.gaps(cols, status, chain, 0), cols, names).decode().split("\n")
    assert "c#1#c1\t2990\t3000\ta#1#c1\t2990\t3000\tEVEN\t0\t6\t-10\t-10\t9\t10" in text
    assert "b#1#c1\t220\t290\tc#1#c2\t150\t220\tINV\t70\t8\t0\t0\t12\t12" in text
    pairs, spectrum = gm.summary(cols, status, chain, genome, 50)
    text = gm.summary_text(pairs, spectrum, ["a#1#", "b#1#", "c#1#"]).decode().split("\n")
    assert text[0] == "#query_genome\ttarget_genome\tlinks\tins\tins_bases\tdel\tdel_bases\tinv\tinv_bases"
    assert text[1] == "a#1#\tb#1#\t3\t2\t280\t0\t0\t0\t0" and text[2] == "b#1#\tc#1#\t1\t1\t60\t0\t0\t1\t70"
    assert text[5:] == ["#spectrum\tINS\t32\t63\t1", "#spectrum\tINS\t64\t127\t1", "#spectrum\tINS\t128\t255\t2", "#spectrum\tDEL\t64\t127\t1",
                        "#spectrum\tDEL\t128\t255\t1", "#spectrum\tDEL\t512\t1023\t1", ""]


# ---- the model under the oracle's status and chain -------------------------------------------------------------------------------
def check_against_blocks(cols, status, chain, jump, what):
    """With min_size 0: per chain n_core - 1 link rows and n_inverted INV rows (tests/blocks_model.py), and every link bridges
    -floor(J / 5) <= dq, dt <= J (the reading of src/paf_filter.rs:799-835: a link is made only inside that window)."""
    rows = gm.gaps(cols, status, chain, 0)
    blocks = bm.blocks(cols, status, chain)
    n_links, n_inv = {}, {}
    for e in rows:
        d = n_inv if e["kind"] == V else n_links
        d[e["chain"]] = d.get(e["chain"], 0) + 1
    assert {b["chain"]: b["n_core"] - 1 for b in blocks if b["n_core"] > 1} == n_links, what
    assert {b["chain"]: b["n_inverted"] for b in blocks if b["n_inverted"]} == n_inv, what
    for e in rows:
        if e["kind"] != V:
            assert -(jump // 5) <= e["dq"] <= jump and -(jump // 5) <= e["dt"] <= jump, (what, e)
    keys = [(e["chain"], int(cols["q_start"][e["right"]]), e["right"]) for e in rows]
    assert keys == sorted(keys) and len(set(keys)) == len(keys), what
    return rows, blocks


@pytest.mark.parametrize("case", K.CASES, ids=[c["name"] for c in K.CASES])
def test_model_under_the_oracle_on_the_hand_derived_fixtures(case):
    case, cols, status, chain = kat_case(case["name"])
    check_against_blocks(cols, status, chain, case["cfg"].get("scaffold_gap", orc.Config().scaffold_gap), case["name"])


def test_fixtures_read_off_the_hand_derivations():
    # '-' chains {A, B, C} and {D, E} of kat_scaffold case 1: q gaps of 100 throughout; target gaps 100, then an overlap of 150,
    # and 1000 between D and E
    _, cols, status, chain = kat_case("minus_strand_gaps")
    rows = gm.gaps(cols, status, chain, 0)
    assert [(e["chain"], e["left"], e["right"], e["dq"], e["dt"], e["size"], e["flags"]) for e in rows] == [
        (1, 1, 3, 100, 100, 0, 0), (1, 3, 0, 100, -150, 250, 2), (2, 5, 4, 100, 1000, -900, 0)]
    assert [e["kind"] for e in rows] == [E, I, D]
    # inversion capture: one '+' core record and four captured '-' ones: no link, four INV rows of 100 bases in q_start order
    _, cols, status, chain = kat_case("inversion_capture_window_and_sqrt2")
    rows = gm.gaps(cols, status, chain, 0)
    assert [e["kind"] for e in rows] == [V] * 4 and [e["size"] for e in rows] == [100] * 4
    assert [e["q_lo"] for e in rows] == [8900, 12000, 16000, 21000] and gm.gaps(cols, status, chain, 101) == []
    # rescue: rescued records make no row
    _, cols, status, chain = kat_case("rescue_distance_boundaries")
    assert int((status == R).sum()) == 3 and gm.gaps(cols, status, chain, 0) == []


@pytest.fixture(scope="module")
def syeast():
    text = gzip.open(os.path.join(ROOT, "tests", "golden", "syeast.paf.gz"), "rb").read().decode()
    rec = orc.parse_paf_text(text)
    ids = {}
    cols = {"q_id": [ids.setdefault(x, len(ids)) for x in rec.qname], "t_id": [ids.setdefault(x, len(ids)) for x in rec.tname],
            "q_start": rec.qs, "q_end": rec.qe, "t_start": rec.ts, "t_end": rec.te, "matches": rec.matches, "block_len": rec.block_length,
            "strand": (rec.strand == ord("-")).astype(np.uint8)}
    return rec, {k: np.asarray(v) for k, v in cols.items()}


ORACLE_FLAGS = {"default": orc.Config(),
                "one_to_one_rescue": orc.Config(mapping_filter_mode=orc.ONE_TO_ONE, mapping_max_per_query=1, mapping_max_per_target=1,
                                                scaffold_filter_mode=orc.ONE_TO_ONE, scaffold_max_per_query=1, scaffold_max_per_target=1,
                                                scaffold_max_deviation=20_000)}


@pytest.mark.parametrize("flags", list(ORACLE_FLAGS))
def test_model_under_the_oracle_on_syeast(syeast, flags):
    rec, cols = syeast
    cfg = ORACLE_FLAGS[flags]
    status, chain = orc.apply_filters(cfg, rec)
    status, chain = status[:len(rec)], chain[:len(rec)]
    rows, blocks = check_against_blocks(cols, status, chain, cfg.scaffold_gap, flags)
    assert sum(e["kind"] != V for e in rows) > 10_000 and sum(e["kind"] == V for e in rows) > 100     # (not vacuous: inversions are captured)
    if flags == "one_to_one_rescue":
        assert int((status == R).sum()) >= 1 and sum(b["n_rescued"] for b in blocks) >= 1
    # the default size cut keeps a part of them, and only those
    cut = gm.gaps(cols, status, chain, 50)
    assert 0 < len(cut) < len(rows) and cut == [e for e in rows if abs(e["size"]) >= 50]


# ---- the host side of the library ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbols_are_exported_and_declared(lib):
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_gaps_records", "swg_gaps_records_device", "swg_paf_gaps"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    assert lib.swg_abi_version() == 1
    import sweepga_amd
    from sweepga_amd import gaps
    assert sweepga_amd.Gaps is gaps.Gaps and sweepga_amd.gaps_records is gaps.gaps_records
    assert sweepga_amd.gaps_records_device is gaps.gaps_records_device
    for name, value in (("SWG_GAP_EVEN", gaps.EVEN), ("SWG_GAP_INS", gaps.INS), ("SWG_GAP_DEL", gaps.DEL), ("SWG_GAP_INV", gaps.INV),
                        ("SWG_GAPS_ROWS", gaps.ROWS), ("SWG_GAPS_SUMMARY", gaps.SUMMARY)):
        assert "#define %s %du\n" % (name, value) in hdr
    assert (gaps.EVEN, gaps.INS, gaps.DEL, gaps.INV, gaps.BINS) == (gm.EVEN, gm.INS, gm.DEL, gm.INV, gm.BINS) and "#define SWG_GAPS_BINS 33\n" in hdr


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib
    from sweepga_amd.gaps import PAIR_DTYPE, ROW_DTYPE
    structs = (("swg_gap_row", _lib.SwgGapRow), ("swg_gap_pair", _lib.SwgGapPair), ("swg_gaps_request", _lib.SwgGapsRequest))
    prints, want = [], []
    for name, cls in structs:
        prints.append('printf("%%zu\\n", sizeof(%s));' % name)
        want.append(C.sizeof(cls))
        for f, _ in cls._fields_:
            prints.append('printf("%%zu\\n", offsetof(%s, %s));' % (name, f))
            want.append(getattr(cls, f).offset)
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == want
    assert (C.sizeof(_lib.SwgGapRow), C.sizeof(_lib.SwgGapPair), C.sizeof(_lib.SwgGapsRequest)) == (32, 64, 72)
    for cls, dtype in ((_lib.SwgGapRow, ROW_DTYPE), (_lib.SwgGapPair, PAIR_DTYPE)):
        assert dtype.itemsize == C.sizeof(cls)
        for f, t in cls._fields_:
            assert dtype.fields[f][1] == getattr(cls, f).offset and dtype.fields[f][0].itemsize == C.sizeof(t), f
    # no implicit padding: the fields fill the structure
    for _, cls in structs:
        assert sum(C.sizeof(t) for _, t in cls._fields_) == C.sizeof(cls)


def test_command_line_lists_the_flags_and_its_usage_errors(lib):
    from sweepga_amd import build
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--gaps FILE" in r.stdout and "--gaps-summary FILE" in r.stdout and "--gaps-min-size N" in r.stdout
    for flag in ("--gaps", "--gaps-summary", "--gaps-min-size"):
        r = subprocess.run([build.CLI, "in.paf", flag], capture_output=True, text=True)          # no value
        assert r.returncode == 2 and flag in r.stderr, (flag, r.stderr)
    for flag in ("--gaps", "--gaps-summary"):
        r = subprocess.run([build.CLI, "in.paf", flag + "="], capture_output=True, text=True)    # an empty one
        assert r.returncode == 2 and flag in r.stderr, (flag, r.stderr)
    for bad in ("x", "5q", "5g", ""):     # 5g = 5 * 10^9 does not fit 32 bits
        r = subprocess.run([build.CLI, "in.paf", "--gaps", "g.tsv", "--gaps-min-size=" + bad], capture_output=True, text=True)
        assert r.returncode == 2 and "--gaps-min-size" in r.stderr, (bad, r.stderr)
    r = subprocess.run([build.CLI, "in.paf", "--gaps-min-size", "1k"], capture_output=True, text=True)   # the option without a report
    assert r.returncode == 2 and "--gaps-min-size needs --gaps" in r.stderr


LINE = "a#1#x\t100\t0\t50\t+\tb#1#y\t200\t10\t60\t50\t50\t60\n"
HEADERS = (gm.ROWS_HEADER.encode(), gm.SUMMARY_HEADER.encode())


def test_no_records_or_no_chain_needs_no_device(lib):
    from sweepga_amd import Gaps, PafFile
    for text in ("", "# nothing\nfew\tfields\n"):
        with PafFile(text=text) as paf:
            assert paf.n == 0
            g = Gaps.from_paf(None, paf, np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint32))
            assert (g.rows, g.summary) == HEADERS and g.table is None
            g = Gaps.from_paf(None, paf, np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint32), summary=False)
            assert g.rows == HEADERS[0] and g.summary is None
    # records, none of which takes part: kept ones without a chain (what --scaffold-jump 0 leaves), a rescued one with a chain, a
    # chain number on a dropped record
    with PafFile(text=LINE * 4) as paf:
        g = Gaps.from_paf(None, paf, np.array([1, 3, 2, 0], dtype=np.uint8), np.array([0, 0, 4, 4], dtype=np.uint32))
        assert (g.rows, g.summary) == HEADERS
        g = Gaps.from_paf(None, paf, np.array([1, 3, 2, 0], dtype=np.uint8), np.array([0, 0, 4, 4], dtype=np.uint32), rows=False)
        assert g.rows is None and g.summary == HEADERS[1]
        p, n = C.c_void_p(), C.c_uint64()
        assert lib.swg_paf_gaps(None, paf.handle, None, None, 50, None, None, None, None) == -1      # neither text
        assert lib.swg_paf_gaps(None, paf.handle, None, None, 50, C.byref(p), C.byref(n), None, None) == -1 and not p.value   # no status


def test_a_null_context_is_refused_where_a_device_is_needed(lib):
    from sweepga_amd import PafFile, _lib
    cols, status, chain, genome, _ = hand_case()
    rec = _lib.SwgRecords()
    rec.n = len(status)
    for k, a in cols.items():
        setattr(rec, k, a.ctypes.data)
    rec.n_seq = 6
    req = _lib.SwgGapsRequest()
    req.want = 3
    for fn in (lib.swg_gaps_records, lib.swg_gaps_records_device):   # (refused before any pointer is looked at)
        assert fn(None, C.byref(rec), status.ctypes.data, chain.ctypes.data, genome.ctypes.data, 3, C.byref(req)) == -1
    with PafFile(text=LINE) as paf:
        p, n = C.c_void_p(), C.c_uint64()
        st, ch = np.array([1], dtype=np.uint8), np.array([1], dtype=np.uint32)
        assert lib.swg_paf_gaps(None, paf.handle, st.ctypes.data, ch.ctypes.data, 50, C.byref(p), C.byref(n), None, None) == -1 and not p.value
        assert b"NULL context" in lib.swg_alnstats_last_error()


def test_64_bit_columns_are_refused_without_a_device(lib, tmp_path):
    from sweepga_amd import build, PafFile
    ln = "\t".join(["a#1#x", str(2**33), str(2**32), str(2**32 + 50), "+", "b#1#y", "900", "10", "60", "50", "50", "60"]) + "\n"
    with PafFile(text=ln) as paf:
        assert paf.is_rebased
        p, n = C.c_void_p(), C.c_uint64()
        st, ch = np.array([1], dtype=np.uint8), np.array([1], dtype=np.uint32)
        assert lib.swg_paf_gaps(None, paf.handle, st.ctypes.data, ch.ctypes.data, 50, C.byref(p), C.byref(n), None, None) == -6
        assert b"2^32" in lib.swg_alnstats_last_error()
    inp, out = tmp_path / "in.paf", tmp_path / "out.paf"
    inp.write_text(ln)
    for flag in ("--gaps", "--gaps-summary"):
        for extra in ([], ["--no-filter"]):
            rep = tmp_path / "g.tsv"
            r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), flag, str(rep), *extra], capture_output=True, text=True)
            assert r.returncode == 3 and "--gaps" in r.stderr and "2^32" in r.stderr, r.stderr
            assert r.stdout == "" and not out.exists() and not rep.exists()


def test_command_line_writes_the_header_lines_without_a_device(lib, tmp_path):
    from sweepga_amd import build
    inp, empty, rows, summ, out = (tmp_path / x for x in ("in.paf", "empty.paf", "g.tsv", "s.tsv", "out.paf"))
    inp.write_text(LINE * 2)
    empty.write_text("")
    r = subprocess.run([build.CLI, str(inp), "--no-filter", "--gaps", str(rows), "--gaps-summary", str(summ)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == LINE * 2 and (rows.read_bytes(), summ.read_bytes()) == HEADERS, r.stderr
    for extra in ([], ["--scaffold-jump", "0"]):     # a PAF without records opens no device either
        rows.write_bytes(b"stale")
        r = subprocess.run([build.CLI, str(empty), "--output-file", str(out), "--gaps", str(rows), "--gaps-min-size", "1k", "--quiet", *extra],
                           capture_output=True, text=True)
        assert r.returncode == 0 and rows.read_bytes() == HEADERS[0], r.stderr
    r = subprocess.run([build.CLI, str(inp), "--no-filter", "--gaps-summary", "-"], capture_output=True)       # - = standard error
    assert r.returncode == 0 and r.stdout == (LINE * 2).encode() and r.stderr == HEADERS[1]
