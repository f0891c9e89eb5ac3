"""The block table's model (tests/blocks_model.py) against answers worked out by hand and against the hand-derived scaffold
fixtures of tests/kat_scaffold.py under the oracle's status and chain, and the host side of the feature: symbols, structure
layout, --help, the calls that need no device.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import blocks_model as bm
from tests import kat_scaffold as K
from tests import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, R = bm.SCAFFOLD, bm.RESCUED


def columns(records):
    """records: (q_id, t_id, q_start, q_end, t_start, t_end, matches, block_len, strand) per record."""
    a = np.asarray(records, dtype=np.int64).reshape(-1, 9)
    return {k: a[:, j].astype(np.uint8 if k == "strand" else np.uint32) for j, k in enumerate(bm.COLUMNS)}


def hand_case():
    """-> (columns, status, chain, expected rows in bm.FIELDS order).  Sequences 0..3; chains 2, 5 and 9 (gaps: 1, 3, 4, 6..8)."""
    rec = [
        # chain 5, '+': core r0, r2; captured inversion r3 ('-', SCAFFOLD); rescued r5 outside the core span; r1 is dropped
        (0, 1, 100, 200, 1000, 1100, 90, 100, 0),    # r0 core
        (0, 1, 0, 5000, 0, 5000, 1, 1, 0),           # r1 status 0: takes no part although it names chain 5
        (0, 1, 150, 300, 1150, 1300, 140, 150, 0),   # r2 core, overlaps r0 on the query by 50, apart on the target by 50
        (0, 1, 120, 130, 1250, 1260, 9, 10, 1),      # r3 inverted: inside the core's cover on both axes
        (0, 1, 0, 5000, 0, 5000, 1, 1, 1),           # r4 chain 0: takes no part
        (0, 1, 900, 950, 2000, 2050, 40, 50, 0),     # r5 rescued, beyond q_end = 300 and t_end = 1300
        # chain 2, '-': r6, r8 core; touching on the query, a zero-length record r7 (rescued) that adds nothing
        (2, 3, 10, 20, 50, 60, 10, 10, 1),           # r6
        (2, 3, 500, 500, 700, 700, 0, 0, 1),         # r7 zero length on both axes, rescued
        (2, 3, 20, 30, 40, 50, 9, 10, 1),            # r8 touches r6 on both axes
        # chain 9, '+': r9 contains r10 on the query; on the target they are apart
        (3, 0, 0, 1000, 0, 1000, 900, 1000, 0),      # r9
        (3, 0, 100, 200, 3000, 3100, 90, 100, 0),    # r10 contained (query)
    ]
    status = np.array([S, 0, S, S, S, R, S, R, S, S, S], dtype=np.uint8)
    chain = np.array([5, 5, 5, 5, 0, 5, 2, 2, 2, 9, 9], dtype=np.uint32)
    want = [
        # chain q t strand qs qe ts te nc ni nr matches block q_bases t_bases q_cover t_cover first
        (2, 2, 3, 1, 10, 30, 40, 60, 2, 0, 1, 19, 20, 20, 20, 20, 20, 6),
        (5, 0, 1, 0, 100, 300, 1000, 1300, 2, 1, 1, 279, 310, 310, 310, 250, 300, 0),
        (9, 3, 0, 0, 0, 1000, 0, 3100, 2, 0, 0, 990, 1100, 1100, 1100, 1000, 1100, 9),
    ]
    return columns(rec), status, chain, want


def test_model_against_hand_derived_answers():
    cols, status, chain, want = hand_case()
    assert bm.rows(bm.blocks(cols, status, chain)) == want
    # the same under a permutation: only first_record moves, through the permutation
    perm = np.array([7, 3, 10, 0, 9, 4, 1, 8, 2, 6, 5])
    got = bm.rows(bm.blocks({k: v[perm] for k, v in cols.items()}, status[perm], chain[perm]))
    where = {int(old): new for new, old in enumerate(perm)}
    assert got == [w[:-1] + (min(where[r] for r in core),) for w, core in zip(want, ([6, 8], [0, 2], [9, 10]))]


def test_union_length_by_hand():
    assert bm.union_length([], []) == 0
    assert bm.union_length([5], [5]) == 0
    assert bm.union_length([0, 10], [10, 20]) == 20            # touching
    assert bm.union_length([0, 11], [10, 20]) == 19            # a gap of one
    assert bm.union_length([0, 3, 5], [100, 4, 5]) == 100      # contained, zero length
    assert bm.union_length([50, 0], [60, 55]) == 60            # order does not matter


def test_model_refuses_the_two_input_errors():
    cols, status, chain, _ = hand_case()
    two = {k: v.copy() for k, v in cols.items()}
    two["t_id"][2] = 2
    with pytest.raises(bm.BlockError):
        bm.blocks(two, status, chain)
    masked = status.copy()
    masked[[6, 8]] = R
    with pytest.raises(bm.BlockError):
        bm.blocks(cols, masked, chain)


def kat_case(name):
    case = next(c for c in K.CASES if c["name"] == name)
    rec = orc.parse_paf_text(K.paf_text(case))
    cfg = orc.Config(**{k: ({"OneToOne": orc.ONE_TO_ONE}[v] if isinstance(v, str) else v) for k, v in case["cfg"].items()})
    status, chain = orc.apply_filters(cfg, rec)
    ids = {}
    cols = {"q_id": [ids.setdefault(x, len(ids)) for x in rec.qname], "t_id": [ids.setdefault(x, len(ids)) for x in rec.tname],
            "q_start": rec.qs, "q_end": rec.qe, "t_start": rec.ts, "t_end": rec.te, "matches": rec.matches, "block_len": rec.block_length,
            "strand": (rec.strand == ord("-")).astype(np.uint8)}
    return case, cols, status[:len(rec)], chain[:len(rec)]


def test_fixtures_inversion_capture_and_rescue_read_off_the_hand_derivations():
    # inversion capture: P is the '+' core, M1 M3 M4 M6 are captured; the block's span is P's, whatever the captured ones reach
    case, cols, status, chain = kat_case("inversion_capture_window_and_sqrt2")
    (b,) = bm.blocks(cols, status, chain)
    assert (b["chain"], b["strand"], b["n_core"], b["n_inverted"], b["n_rescued"]) == (1, 0, 1, 4, 0) and b["n_inverted"] >= 1
    assert (b["q_start"], b["q_end"], b["t_start"], b["t_end"], b["first_record"]) == (10000, 20000, 30000, 40000, 1)
    assert b["matches"] == 9500 + 4 * 95 and b["block_len"] == 10000 + 4 * 100 and b["q_bases"] == b["t_bases"] == 10400
    # M1, M3 lie inside P on both axes; M4 [8900,9000) and M6 [21000,21100) outside on both
    assert b["q_cover"] == 10000 + 200 and b["t_cover"] == 10000 + 200
    # rescue at D: X1 the core; R1, R3, R5 rescued, all inside X1's query and target range
    case, cols, status, chain = kat_case("rescue_distance_boundaries")
    (b,) = bm.blocks(cols, status, chain)
    assert (b["n_core"], b["n_inverted"], b["n_rescued"]) == (1, 0, 3) and b["n_rescued"] >= 1
    assert (b["q_start"], b["q_end"], b["t_start"], b["t_end"], b["first_record"]) == (0, 3000, 0, 3000, 2)
    assert b["q_cover"] == 3000 and b["t_cover"] == 3000 and b["q_bases"] == 3000 + 100 + 100 + 101 and b["matches"] == 2970 + 95 + 95 + 96
    # a rescued record beyond the core span: Z q[3100,3300) t[5000,5200) against X1 [0,3000)
    case, cols, status, chain = kat_case("filtered_scaffold_members_not_rescued")
    (b,) = bm.blocks(cols, status, chain)
    assert (b["n_core"], b["n_rescued"], b["q_end"], b["t_end"], b["q_cover"], b["t_cover"]) == (1, 1, 3000, 3000, 3200, 3200)
    # '-' chains
    case, cols, status, chain = kat_case("minus_strand_gaps")
    b1, b2 = bm.blocks(cols, status, chain)
    assert (b1["strand"], b1["n_core"], b1["q_start"], b1["q_end"], b1["t_start"], b1["t_end"], b1["first_record"]) == (1, 3, 0, 3200, 7000, 10000, 0)
    assert (b2["strand"], b2["n_core"], b2["q_start"], b2["q_end"], b2["t_start"], b2["t_end"], b2["first_record"]) == (1, 2, 3300, 5400, 4500, 7300, 4)
    assert b1["t_cover"] == 1000 + 1000 + 1050 - 150 and b1["n_inverted"] == 0


@pytest.mark.parametrize("case", K.CASES, ids=[c["name"] for c in K.CASES])
def test_parser_of_the_output_paf_rebuilds_the_table(case):
    """The table from the columns under the oracle's status and chain == the table rebuilt from the expected output text alone
    (ids and first_record aside: the output has its own), and the rendering of both is the same text."""
    _, cols, status, chain = kat_case(case["name"])
    from_columns = bm.blocks(cols, status, chain)
    from_text, out_lines = bm.blocks_of_output_paf(K.expected_output(case))
    drop = ("q_id", "t_id", "first_record")
    assert [{k: v for k, v in b.items() if k not in drop} for b in from_columns] == [{k: v for k, v in b.items() if k not in drop} for b in from_text]
    in_lines = K.paf_text(case).splitlines()
    assert bm.render(from_columns, in_lines) == bm.render(from_text, out_lines) == bm.render_from_output_paf(K.expected_output(case))
    assert len(from_columns) == len({c for _, c in case["expect"] if c})


def test_format_of_a_line_written_out():
    b = dict(zip(bm.FIELDS, (5, 0, 1, 0, 100, 300, 1000, 1300, 2, 1, 1, 279, 310, 310, 310, 250, 300, 0)))
    assert bm.format_line(b, "g1#1#chrA", "1000000", "g2#1#chrB", "0900") == (
        "g1#1#chrA\t1000000\t100\t300\t+\tg2#1#chrB\t0900\t1000\t1300\t279\t310\t255\tch:Z:chain_5\tnc:i:2\tni:i:1\tnr:i:1\tqc:i:250\ttc:i:300\tid:f:0.900000\n")
    b.update(strand=1, matches=0, block_len=0)
    assert bm.format_line(b, "a", "1", "b", "2").endswith("\tid:f:0.000000\n") and "\t-\tb\t" in bm.format_line(b, "a", "1", "b", "2")


# ---- the host side of the library ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbols_are_exported_and_declared(lib):
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_blocks_records", "swg_blocks_records_device", "swg_paf_blocks"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    assert lib.swg_abi_version() == 1 and "#define SWG_ABI_VERSION 1\n" in hdr
    import sweepga_amd
    assert sweepga_amd.Blocks is not None and sweepga_amd.blocks_records is not None and sweepga_amd.blocks_records_device is not None


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib
    from sweepga_amd.blocks import BLOCK_DTYPE
    block_fields = [f for f, _ in _lib.SwgBlock._fields_]
    table_fields = [f for f, _ in _lib.SwgBlockTable._fields_]
    prints = ['printf("%zu\\n", sizeof(swg_block));', 'printf("%zu\\n", sizeof(swg_block_table));']
    prints += ['printf("%%zu\\n", offsetof(swg_block, %s));' % f for f in block_fields]
    prints += ['printf("%%zu\\n", offsetof(swg_block_table, %s));' % f for f in table_fields]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [104, 24] + [getattr(_lib.SwgBlock, f).offset for f in block_fields] + [getattr(_lib.SwgBlockTable, f).offset for f in table_fields]
    assert got == want and C.sizeof(_lib.SwgBlock) == BLOCK_DTYPE.itemsize == 104
    assert [BLOCK_DTYPE.fields[f][1] for f in block_fields] == got[2:2 + len(block_fields)]


def test_command_line_lists_the_flag_and_wants_a_value(lib):
    from sweepga_amd import build
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--blocks FILE" in r.stdout
    r = subprocess.run([build.CLI, "in.paf", "--blocks"], capture_output=True, text=True)
    assert r.returncode == 2 and "--blocks" in r.stderr


LINE = "a#1#x\t100\t0\t50\t+\tb#1#y\t200\t10\t60\t50\t50\t60\n"


def test_no_records_or_no_chain_needs_no_device(lib):
    from sweepga_amd import Blocks, PafFile
    for text in ("", "# nothing\nfew\tfields\n"):
        with PafFile(text=text) as paf:
            assert paf.n == 0
            p, n = C.c_void_p(), C.c_uint64(7)
            assert lib.swg_paf_blocks(None, paf.handle, None, None, C.byref(p), C.byref(n)) == 0 and n.value == 0 and p.value
            lib.swg_free(p)
            b = Blocks.from_paf(None, paf, np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint32))
            assert b.text == b"" and len(b.table) == 0
    with PafFile(text=LINE * 3) as paf:   # kept records, none of them in a chain -- and a chain number on a dropped record
        b = Blocks.from_paf(None, paf, np.array([1, 3, 0], dtype=np.uint8), np.array([0, 0, 4], dtype=np.uint32))
        assert b.text == b"" and len(b.table) == 0


def test_a_null_context_is_refused_where_a_device_is_needed(lib):
    from sweepga_amd import PafFile, _lib
    cols, status, chain, _ = hand_case()
    rec = _lib.SwgRecords()
    rec.n = len(status)
    for k, a in cols.items():
        setattr(rec, k, a.ctypes.data)
    rec.n_seq = 4
    table = _lib.SwgBlockTable()
    for fn in (lib.swg_blocks_records, lib.swg_blocks_records_device):   # (refused before any pointer is looked at)
        assert fn(None, C.byref(rec), status.ctypes.data, chain.ctypes.data, C.byref(table)) == -1
    with PafFile(text=LINE) as paf:
        p, n = C.c_void_p(), C.c_uint64()
        st, ch = np.array([1], dtype=np.uint8), np.array([1], dtype=np.uint32)
        assert lib.swg_paf_blocks(None, paf.handle, st.ctypes.data, ch.ctypes.data, C.byref(p), C.byref(n)) == -1 and not p.value
        assert b"NULL context" in lib.swg_alnstats_last_error()


def test_64_bit_columns_are_refused_without_a_device(lib, tmp_path):
    from sweepga_amd import build, PafFile
    ln = "\t".join(["a#1#x", str(2**33), str(2**32), str(2**32 + 50), "+", "b#1#y", "900", "10", "60", "50", "50", "60"]) + "\n"
    with PafFile(text=ln) as paf:
        assert paf.is_rebased
        p, n = C.c_void_p(), C.c_uint64()
        st, ch = np.array([1], dtype=np.uint8), np.array([1], dtype=np.uint32)
        assert lib.swg_paf_blocks(None, paf.handle, st.ctypes.data, ch.ctypes.data, C.byref(p), C.byref(n)) == -6
        assert b"2^32" in lib.swg_alnstats_last_error()
    inp, out, blk = tmp_path / "in.paf", tmp_path / "out.paf", tmp_path / "b.paf"
    inp.write_text(ln)
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--blocks", str(blk)], capture_output=True, text=True)
    assert r.returncode == 3 and "--blocks" in r.stderr and "2^32" in r.stderr, r.stderr
    assert r.stdout == "" and not out.exists() and not blk.exists()


def test_command_line_no_filter_writes_an_empty_file_without_a_device(lib, tmp_path):
    from sweepga_amd import build
    inp, blk = tmp_path / "in.paf", tmp_path / "b.paf"
    inp.write_text(LINE * 2)
    r = subprocess.run([build.CLI, str(inp), "--no-filter", "--blocks", str(blk)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == LINE * 2 and blk.read_bytes() == b"", r.stderr
