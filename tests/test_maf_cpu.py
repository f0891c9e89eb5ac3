"""The alignment blocks without a GPU: the model of tests/maf_model.py against blocks worked out by hand on both strands, every op
letter, comp_raw, breakers at every place, the unusable reasons, the model's properties on 1,000 random entries per seed and
split_gap, the MAF text by hand, and the host side of the feature -- header, ctypes mirrors, exported symbols, the record seams'
refusal without a context, the rules of csrc/swg_maf_walk.h run on a CPU under the host sanitizers against the model, the PAF seam's
no-device paths and refusals, the usage errors of --maf, and the block formatter under the host sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import maf_model as mm
from tests import variants_model as vm
from tests.test_eqx_cpu import widen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = b"ACGTACGTAC"


def eb(text, minus, q_start, q_end, t_start, T_, Q, g=0):
    """-> ([(op_first, op_end, t_start, t_bases, q_start, q_bases, aligned, target row, query row)], the non-zero sums)"""
    blocks, sums = mm.entry_blocks(text, minus, q_start, q_end, t_start, T_, Q, g)
    rows = [(b["op_first"], b["op_end"], b["t_start"], b["t_bases"], b["q_start"], b["q_bases"], b["aligned"], b["rows"][:b["columns"]].decode(),
             b["rows"][b["columns"]:].decode()) for b in blocks]
    return rows, {k: v for k, v in sums.items() if v}


# ---- the model against blocks worked out by hand ------------------------------------------------------------------------------------------
def test_blocks_by_hand_on_both_strands():
    assert eb("10M", False, 0, 10, 0, T, b"ACCTACGTAG") == ([(0, 1, 0, 10, 0, 10, 10, "ACGTACGTAC", "ACCTACGTAG")], {})
    # the query holds the walk's reverse complement: CTACGTAGGT walked from its last base gives ACCTACGTAG
    assert eb("10M", True, 0, 10, 0, T, b"CTACGTAGGT") == ([(0, 1, 0, 10, 0, 10, 10, "ACGTACGTAC", "ACCTACGTAG")], {})
    # offsets on both sides, an insertion and a deletion: ACG--TACGT against ACGttTA-GT
    assert eb("3=2I2=1D2=", False, 1, 10, 0, T, b"gACGttTAGTa") == ([(0, 5, 0, 8, 1, 9, 7, "ACG--TACGT", "ACGttTA-GT")], {})
    # the same from the other strand: the query interval [2, 11) of ttACTAaaCGTc
    assert eb("3=2I2=1D2=", True, 2, 11, 0, T, b"ttACTAaaCGTc") == ([(0, 5, 0, 8, 2, 9, 7, "ACG--TACGT", "ACGttTA-GT")], {})
    assert eb("2=", False, 1, 3, 4, T, b"cACc") == ([(0, 1, 4, 2, 1, 2, 2, "AC", "AC")], {})


def test_one_case_per_op_letter():
    assert eb("2M2=2X", False, 0, 6, 0, T, b"ACGTTT")[0] == [(0, 3, 0, 6, 0, 6, 6, "ACGTAC", "ACGTTT")]      # M = X: both bytes, equal or not
    assert eb("1=2I1=", False, 0, 4, 0, T, b"AggC")[0] == [(0, 3, 0, 2, 0, 4, 2, "A--C", "AggC")]             # I: '-' above the query's bases
    assert eb("1=2D1=", False, 0, 2, 0, T, b"AT")[0] == [(0, 3, 0, 4, 0, 2, 2, "ACGT", "A--T")]               # D: '-' below the target's
    assert eb("1=2N1=", False, 0, 2, 0, T, b"AT")[0] == [(0, 3, 0, 4, 0, 2, 2, "ACGT", "A--T")]               # N: as D
    assert eb("3S1H2=0P5H", False, 0, 2, 0, T, b"AC")[0] == [(0, 5, 0, 2, 0, 2, 2, "AC", "AC")]                # S H P: in the run, no columns
    assert eb("0I2=0D0N0M0X0=", False, 0, 2, 0, T, b"AC")[0] == [(0, 7, 0, 2, 0, 2, 2, "AC", "AC")]            # zero-length ops
    assert eb("002=01I0003D01X", False, 0, 4, 0, T, b"ACtT")[0] == [(0, 4, 0, 6, 0, 4, 3, "AC-GTAC", "ACt---T")]      # leading zeros


def test_comp_raw_on_all_256_bytes_against_the_header(tmp_path):
    src = tmp_path / "table.c"
    src.write_text('#include <stdio.h>\n#include "sweepga_gpu.h"\nstatic const unsigned char t[] = SWG_MAF_COMP_RAW;\n'
                   'int main(void){printf("%zu\\n", sizeof(t));for(int i=0;i<256;++i)printf("%d\\n",t[i]);return 0;}\n')
    exe = tmp_path / "table"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == 256 and got[1:] == [mm.comp_raw(b) for b in range(256)]
    pairs = dict(zip("ACGTRYKMBVDHU", "TGCAYRMKVBHDA"))
    for b in range(256):
        ch = chr(b)
        want = pairs.get(ch) or (pairs[ch.upper()].lower() if ch.upper() in pairs and ch.islower() else ch)
        assert mm.comp_raw(b) == ord(want), b
    assert all(mm.comp_raw(mm.comp_raw(b)) == b for b in range(256) if chr(b) not in "Uu")


def test_lower_case_and_iupac_are_kept():
    t, q = b"acGRYn*SWk", b"ACgryN*swK"
    assert eb("10M", False, 0, 10, 0, t, q)[0] == [(0, 1, 0, 10, 0, 10, 10, "acGRYn*SWk", "ACgryN*swK")]
    # on '-' every byte goes through comp_raw and the order turns round: mWS*NryCGU read backwards and complemented
    assert eb("10M", True, 0, 10, 0, t, b"mWS*NryCGU")[0] == [(0, 1, 0, 10, 0, 10, 10, "acGRYn*SWk", "ACGryN*SWk")]
    assert eb("3=", True, 0, 3, 0, b"BDH", b"dhv")[0] == [(0, 1, 0, 3, 0, 3, 3, "BDH", "bdh")]


def test_breakers_by_hand():
    q = b"ACttGTACGTAC"      # ACGTACGTAC with tt inserted behind AC
    one = [(0, 3, 0, 10, 0, 12, 10, "AC--GTACGTAC", "ACttGTACGTAC")]
    assert eb("2=2I8=", False, 0, 12, 0, T, q, 0) == (one, {})
    assert eb("2=2I8=", False, 0, 12, 0, T, q, 3) == (one, {})                                                   # l = g - 1: no breaker
    two = [(0, 1, 0, 2, 0, 2, 2, "AC", "AC"), (2, 3, 2, 8, 4, 8, 8, "GTACGTAC", "GTACGTAC")]
    assert eb("2=2I8=", False, 0, 12, 0, T, q, 2) == (two, {"breakers": 1, "skipped_q": 2})                      # l = g
    assert eb("2=2I8=", False, 0, 12, 0, T, q, 1) == (two, {"breakers": 1, "skipped_q": 2})
    # on '-' the second block lies in FRONT of the first on the forward strand
    rc = bytes(reversed(q.translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))))
    assert eb("2=2I8=", True, 0, 12, 0, T, rc, 2)[0] == [(0, 1, 0, 2, 10, 2, 2, "AC", "AC"), (2, 3, 2, 8, 0, 8, 8, "GTACGTAC", "GTACGTAC")]
    # a breaker as first and as last op, D and N alike; S and zero-length ops stay with their run
    assert eb("3D2=1S0I2N", False, 0, 2, 0, T, b"TA", 2) == ([(1, 4, 3, 2, 0, 2, 2, "TA", "TA")], {"breakers": 2, "skipped_t": 5})
    # two adjacent breakers: no candidate between them
    assert eb("2=3I3D2=", False, 0, 7, 0, T, b"ACgggTA", 3) == ([(0, 1, 0, 2, 0, 2, 2, "AC", "AC"), (3, 4, 5, 2, 5, 2, 2, "CG", "TA")],
                                                                {"breakers": 2, "skipped_t": 3, "skipped_q": 3})
    # a candidate of I ops only, and one of a zero-length op only, are gap_only; their bases are in no block
    assert eb("2=3D1I3D2=", False, 0, 5, 0, T, b"ACgGT", 3) == ([(0, 1, 0, 2, 0, 2, 2, "AC", "AC"), (4, 5, 8, 2, 3, 2, 2, "AC", "GT")],
                                                                {"gap_only": 1, "breakers": 2, "skipped_t": 6, "lost_q": 1})
    assert eb("3D0M3D", False, 0, 0, 0, T, b"A", 3) == ([], {"gap_only": 1, "breakers": 2, "skipped_t": 6})
    # an entry all of whose candidates are gap-only
    assert eb("1I3D2I", False, 0, 3, 0, T, b"ggg", 3) == ([], {"gap_only": 2, "breakers": 1, "skipped_t": 3, "lost_q": 3})
    assert eb("5I", False, 0, 5, 0, T, b"ggggg", 5) == ([], {"breakers": 1, "skipped_q": 5})                     # breakers only: no candidate
    assert eb("5I", False, 0, 5, 0, T, b"ggggg", 0) == ([], {"gap_only": 1, "lost_q": 5})


def small_table():
    """Seven records over targets 0, 1, 2 (absent) and queries 3, 4; record 5 ends behind its target, record 6 is outside the set."""
    seqs = [T, b"GGGGG", b"", b"ttCCa", b"ACGTTT"]
    cols = {"q_id": [3, 4, 3, 4, 3, 3, 3], "t_id": [0, 1, 2, 0, 1, 0, 0], "q_start": [2, 0, 0, 0, 2, 2, 2], "q_end": [4, 2, 2, 6, 4, 4, 4],
            "t_start": [0, 0, 0, 4, 0, 8, 1], "t_end": [2, 2, 2, 10, 2, 11, 3]}
    cig = {0: "2X", 1: "2M", 2: "2X", 3: "3M2I2D1M", 4: "2=", 5: "2X1D", 6: "2M"}
    return {k: np.array(v) for k, v in cols.items()}, np.array([0, 0, 0, 0, 1, 0, 0], dtype=np.uint8), cig, seqs


def test_every_unusable_reason():
    cols, strand, cig, seqs = small_table()
    got = mm.maf_records(cols, strand, cig, seqs)
    assert (got["usable"], got["no_sequence"], got["out_of_sequence"], got["cigar_bad"], got["empty"]) == (5, 1, 1, 0, 0)
    assert got["text"] == b"AC" b"CC" + b"GG" b"AC" + b"ACG--TAC" b"ACGTT--T" + b"GG" b"GG" + b"CG" b"CC"
    assert [b[:2] for b in got["blocks"]] == [(0, 0), (1, 1), (3, 3), (4, 4), (6, 6)] and [b[12] for b in got["blocks"]] == [0, 4, 8, 24, 28]
    assert got["blocks"][2] == (3, 3, 0, 4, 4, 6, 0, 6, 4, 8, 0, 0, 8, 0) and got["blocks"][3][10] == mm.MINUS
    assert (got["n_blocks"], got["columns"], got["aligned"], got["text_bytes"], got["ops"]) == (5, 16, 12, 32, 11)
    split = mm.maf_records(cols, strand, cig, seqs, g=2)
    assert (split["n_blocks"], split["breakers"], split["skipped_t"], split["skipped_q"], split["gap_only"]) == (6, 2, 2, 2, 0)
    assert split["blocks"][2:4] == [(3, 3, 0, 1, 4, 3, 0, 3, 3, 3, 0, 0, 8, 0), (3, 3, 3, 4, 9, 1, 5, 1, 1, 1, 0, 5, 14, 0)]
    kept = mm.maf_records(cols, strand, cig, seqs, kept=np.array([1, 0, 1, 0, 0, 1, 0], dtype=bool), set_=1)
    assert (kept["usable"], kept["no_sequence"], kept["out_of_sequence"], kept["text"]) == (1, 1, 1, b"ACCC")
    for bad, name in (("2x", "cigar_bad"), ("4294967296X", "cigar_bad"), ("3X", "cigar_bad"), ("2X1D", "cigar_bad"), ("2", "cigar_bad"), ("", "empty")):
        for set_ in (0, 1):      # the state is looked at first: a bad or empty entry counts whether its record is in the set or not
            one = mm.maf_records(cols, strand, {0: bad}, seqs, kept=np.zeros(7, dtype=bool), set_=set_)
            assert (one["usable"], one["text"], one[name], one["blocks"]) == (0, b"", 1, []), bad


# ---- the properties on random entries ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, iupac", [(1, 0.0), (2, 0.0), (3, 0.03)])
def test_properties_on_random_entries(seed, iupac):
    """1,000 entries per seed and split_gap, both strands, fused M ops, lower case, zero-length ops, clips and leading zeros: the
    model asserts its properties on everything it produces; here the counts are held against one another across the split gaps."""
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(50):
        cols, strand, _, cig, seqs = vm.random_case(rng, 20, iupac=iupac)
        cases.append((cols, strand, {i: widen(rng, t) for i, t in cig.items()}, seqs))
    seen = {}
    for g in (0, 1, 3, 50):
        tot = dict.fromkeys(mm.FIELDS, 0)
        for cols, strand, cig, seqs in cases:
            got = mm.maf_records(cols, strand, cig, seqs, g=g)
            assert got["usable"] == 20 and got["cigar_bad"] == 0
            for k in mm.FIELDS:
                tot[k] += got[k]
            for b in got["blocks"]:
                assert b[9] == b[5] + b[7] - b[8] and b[3] > b[2]
        seen[g] = tot
    assert seen[0]["breakers"] == seen[50]["breakers"] == 0 and seen[0]["n_blocks"] == seen[50]["n_blocks"] <= 1000
    assert seen[1]["breakers"] > seen[3]["breakers"] > 500 and seen[1]["n_blocks"] > seen[3]["n_blocks"] > 1000 and seen[3]["gap_only"] > 0
    assert seen[1]["columns"] == seen[1]["aligned"] == seen[0]["aligned"]      # g = 1: every gap is a breaker
    assert all(seen[g]["aligned"] == seen[0]["aligned"] for g in seen)         # an aligned column is in a block whatever the split


# ---- the host side ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib, maf
    structs = (("swg_maf_request", _lib.SwgMafRequest), ("swg_maf_options", _lib.SwgMafOptions), ("swg_maf_counts", _lib.SwgMafCounts))
    prints = ['printf("%%zu\\n", sizeof(%s));' % name for name in ("swg_maf_block", "swg_maf_request", "swg_maf_options", "swg_maf_counts")]
    prints += ['printf("%%zu\\n", offsetof(%s, %s));' % (name, f) for name, cls in structs for f, _ in cls._fields_]
    prints += ['printf("%%zu\\n", offsetof(swg_maf_block, %s));' % f for f in maf.MAF_BLOCK_DTYPE.names]
    prints += ['printf("%u %u %d\\n", SWG_MAF_MINUS, SWG_MAF_TEXT_TILE, SWG_ABI_VERSION);']
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [64, 152, 24, 128] + [getattr(cls, f).offset for _, cls in structs for f, _ in cls._fields_]
    want += [maf.MAF_BLOCK_DTYPE.fields[f][1] for f in maf.MAF_BLOCK_DTYPE.names]
    assert got == want + [mm.MINUS, 4096, 1]
    for _, cls in structs:      # no implicit padding
        assert sum(C.sizeof(t) for _, t in cls._fields_) == C.sizeof(cls) == {"SwgMafRequest": 152, "SwgMafOptions": 24, "SwgMafCounts": 128}[cls.__name__]
    assert maf.MAF_BLOCK_DTYPE.itemsize == 64 and maf.MAF_BLOCK_DTYPE.names == mm.BLOCK_FIELDS and maf.FIELDS == mm.FIELDS and _lib.MAF_COUNTS == mm.COUNTS
    assert maf.MINUS == mm.MINUS


def test_symbols_are_exported_and_declared(lib):
    import sweepga_amd
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_maf_records", "swg_maf_records_device", "swg_paf_maf_write", "swg_paf_maf_text"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    assert lib.swg_abi_version() == 1
    for name in ("MAF_BLOCK_DTYPE", "Maf", "MafResult", "maf_records", "maf_records_device"):
        assert hasattr(sweepga_amd, name)
    assert "swg_maf.hip" in sweepga_amd.build.SOURCES and os.path.join("host", "maf_text.cpp") in sweepga_amd.build.SOURCES


def test_record_seams_refuse_without_a_device(lib):
    """A NULL context: there is no CPU path, and nothing the caller owns is touched."""
    from sweepga_amd import _lib
    from sweepga_amd.lift import cigar_set
    from sweepga_amd.variants import sequence_set
    cols, strand, cig, seqs = small_table()
    keep = {k: np.ascontiguousarray(v, dtype=np.uint32) for k, v in cols.items()}
    rec = _lib.SwgRecords()
    rec.n = 7
    for k, a in keep.items():
        setattr(rec, k, a.ctypes.data)
    rec.strand, rec.n_seq = strand.ctypes.data, 5
    record, offset, text = cigar_set(sorted(cig), [cig[i] for i in sorted(cig)])
    cs = _lib.SwgCigarSet()
    cs.record, cs.offset, cs.text, cs.k = record.ctypes.data, offset.ctypes.data, text.ctypes.data, 7
    s_off, s_bases = sequence_set(seqs)
    ss = _lib.SwgSeqSet()
    ss.offset, ss.bases, ss.n_seq = s_off.ctypes.data, s_bases.ctypes.data, 5
    poison = np.full(64 * 8, 0xab, dtype=np.uint8)
    for fn in (lib.swg_maf_records, lib.swg_maf_records_device):
        req = _lib.SwgMafRequest()
        req.block_capacity, req.blocks, req.text_capacity, req.text, req.usable, req.text_bytes = 7, poison.ctypes.data, 64, poison.ctypes.data + 448, 77, 12345
        assert fn(None, C.byref(rec), None, C.byref(cs), C.byref(ss), C.byref(req)) == -1
        assert (poison == 0xab).all() and req.usable == 77 and req.text_bytes == 12345


def walk_lines(rng, n, g):
    """n random entries -> (the input lines of maf_walk_check, what the model says of each)"""
    lines, want = [], []
    for k in range(n):
        cols, strand, _, cig, seqs = vm.random_case(rng, 1, n_targets=1, n_queries=1, iupac=0.0, flank=3)
        if k % 3 == 0:      # IUPAC codes and foreign bytes, but none that a line of text cannot carry and no '-'
            seqs = [vm.plant(rng, s, 0.0, 0.0) for s in seqs]
            seqs = [bytes(b"RYKMBDHVNSWU*"[int(rng.integers(13))] if rng.random() < 0.05 else c for c in s) for s in seqs]
        rec = tuple(int(cols[c][0]) for c in ("q_start", "q_end", "t_start", "t_end"))
        text = widen(rng, cig[0])
        lines.append("%d %d %d %d %d %s %s %s" % (strand[0], rec[0], rec[1], rec[2], g, seqs[0].decode(), seqs[1].decode(), text))
        blocks, s = mm.entry_blocks(text, bool(strand[0]), rec[0], rec[1], rec[2], seqs[0], seqs[1], g)
        for b in blocks:
            n_ = b["columns"]
            want.append("B %d %d %d %d %d %d %d %d %d %d %s %s" % (b["op_first"], b["op_end"], b["t_start"], b["t_bases"], b["q_start"], b["q_bases"], b["aligned"], n_,
                                                                 mm.MINUS if strand[0] else 0, b["walk_x"], b["rows"][:n_].decode(), b["rows"][n_:].decode()))
        want.append("E %d %d %d %d" % (s["gap_only"], s["breakers"], s["skipped_t"], s["skipped_q"]))
    return lines, want


def test_the_rules_of_the_walk_header_on_a_cpu(tmp_path):
    """tests/native/maf_walk_check.cpp: csrc/swg_maf_walk.h as a host compiler takes it, under the sanitizers, against the model: the
    blocks, both rows and the sums of 200 random entries per split gap, and comp_raw of every byte."""
    exe = str(tmp_path / "maf_walk_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "maf_walk_check.cpp")])
    rng = np.random.default_rng(4)
    lines, want = ["comp"], [" ".join(str(mm.comp_raw(b)) for b in range(256))]
    for g in (0, 1, 3, 50):
        ln, w = walk_lines(rng, 200, g)
        lines += ln
        want += w
    hand = [("0 0 5 0 3 %s ACgGT 2=3D1I3D2=" % T.decode(), ["B 0 1 0 2 0 2 2 2 0 0 AC AC", "B 4 5 8 2 3 2 2 2 0 3 AC GT", "E 1 2 6 0"]),
            ("0 0 2 0 2 %s TA 3D2=1S0I2N" % T.decode(), ["B 1 4 3 2 0 2 2 2 0 0 TA TA", "E 0 2 5 0"]),
            ("1 0 3 0 0 BDH dhv 3=", ["B 0 1 0 3 0 3 3 3 1 0 BDH bdh", "E 0 0 0 0"])]
    for ln, w in hand:
        lines.append(ln)
        want += w
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = r.stdout.strip().split("\n")
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (k, a, b)
    assert sum(w.startswith("B") for w in want) > 1200 and sum(w.startswith("E") and not w.startswith("E 0") for w in want) > 10      # blocks, and gap-only candidates


# ---- the PAF seam without a device ---------------------------------------------------------------------------------------------------------
def test_the_maf_text_by_hand():
    t, q = b"ACGTACGTAC", b"ttGTAGCTAGGT"      # the query's [2, 12) on '-' reads ACCTAGCTAC: ACGTA-CGTAC against ACCTAGCT-AC
    line = "q#1#a\t12\t2\t12\t-\tt#1#b\t10\t0\t10\t5\t9\t60\tNM:i:9\tcg:Z:5M1I2M1D2M\tde:f:0.1"
    paf = line + "\n" + line.replace("cg:Z:5M1I2M1D2M", "xx:Z:none") + "\n"
    fasta = [("t#1#b", t), ("q#1#a", q), ("t#1#b", b"TTTTTTTTTT")]
    text, counts = mm.paf_text(paf, None, fasta, 0)
    # the '-' row starts at 12 - 2 - 10 = 0 on the reverse strand
    assert text == "##maf version=1\na score=9\ns t#1#b 0 10 + 10 ACGTA-CGTAC\ns q#1#a 0 10 - 12 ACCTAGCT-AC\n\n"
    assert counts == dict(dict.fromkeys(mm.COUNTS[:-1], 0), records=2, usable=1, untagged=1, blocks=1, columns=11, aligned=9, file_bytes=len(text))
    text, counts = mm.paf_text(paf, None, fasta, 0, 1)
    # the three blocks lie at [7, 12), [4, 6) and [2, 4) of the forward strand: from the reverse strand's start 0, 6 and 8
    assert text == ("##maf version=1\na score=5\ns t#1#b 0 5 + 10 ACGTA\ns q#1#a 0 5 - 12 ACCTA\n\n"
                    "a score=2\ns t#1#b 5 2 + 10 CG\ns q#1#a 6 2 - 12 CT\n\n" "a score=2\ns t#1#b 8 2 + 10 AC\ns q#1#a 8 2 - 12 AC\n\n")
    assert (counts["blocks"], counts["breakers"], counts["skipped_t"], counts["skipped_q"], counts["columns"]) == (3, 2, 1, 1, 9)
    assert mm.paf_text(paf, None, [("t#1#b", t + b"A"), ("q#1#a", q)], 0)[1] == dict(dict.fromkeys(mm.COUNTS[:-1], 0), records=2, untagged=1, no_sequence=1,
                                                                                    length_mismatch=1, file_bytes=16)
    assert mm.paf_text(paf, np.array([0, 0]), [], 1) == (mm.HEADER, dict(dict.fromkeys(mm.COUNTS[:-1], 0), file_bytes=16))
    assert mm.batch_costs("a\t9\t0\t9\t+\tb\t20\t0\t10\t0\t0\t0\tcg:Z:10M\n", None, 0) == [3 + 9 + 10]


def paf_maf(lib, paf, status, fasta, ctx=None, want=True, **kw):
    """swg_paf_maf_text -> (rc, text or None, counts)"""
    from sweepga_amd import _lib
    opts = _lib.SwgMafOptions()
    for k, v in (kw or {}).items():
        setattr(opts, k, v)
    counts = _lib.SwgMafCounts()
    p, n = C.c_void_p(), C.c_uint64()
    rc = lib.swg_paf_maf_text(ctx, paf.handle, status.ctypes.data if status is not None else None, fasta, C.byref(opts) if kw is not None else None,
                              C.byref(counts), C.byref(p) if want else None, C.byref(n) if want else None)
    if rc != 0:
        assert not p.value
        return rc, None, None
    text = C.string_at(p.value, n.value).decode() if p.value else None
    lib.swg_free(p)
    return rc, text, {k: int(getattr(counts, k)) for k in mm.COUNTS}


def test_paf_seam_without_a_device(lib, tmp_path):
    """A PAF without records of the set gives the header line alone and needs no device; the refusals come before a context is looked
    at and before a file is opened."""
    from sweepga_amd import Maf, PafFile, SwgError
    from sweepga_amd.variants import _FastaHandle
    from tests.test_lift_cpu import REBASED
    from tests.test_ucsc_chain_cpu import mixed_paf
    fa = tmp_path / "s.fa"
    fa.write_text(">g1#1#q\nACGT\n>g2#1#t\nAC\nGT\n")
    zero = dict(dict.fromkeys(mm.COUNTS, 0), file_bytes=16)
    with _FastaHandle(lib, [str(fa)]) as fasta:
        for text in ("", "# nothing\nfew\tfields\n"):
            with PafFile(text=text) as paf:
                for st in (None, np.zeros(1, dtype=np.uint8)):
                    assert paf_maf(lib, paf, st, fasta, set=0) == (0, mm.HEADER, zero)
                    assert paf_maf(lib, paf, st, fasta, set=0, split_gap=7, batch_bytes=5) == (0, mm.HEADER, zero)
                got = Maf.from_paf(paf, None, fasta=[str(fa)], set="all")
                assert (got.text, got.counts) == (mm.HEADER, zero)
                out = tmp_path / "empty.maf"
                assert Maf.write_paf(paf, None, out, fasta=[str(fa)], set="all", split_gap=3) == zero and out.read_text() == mm.HEADER
        text, kept = mixed_paf()
        with PafFile(text=text) as paf:
            none, st = np.zeros(paf.n, dtype=np.uint8), kept.astype(np.uint8)
            assert paf_maf(lib, paf, none, fasta, set=1) == (0, mm.HEADER, zero)      # a set that is never in status: no device
            assert paf_maf(lib, paf, st, fasta, set=1)[0] == -1 and b"swg_paf_maf_text: NULL context" in lib.swg_alnstats_last_error()
            for kw, word in ((dict(set=2), b"set"), (dict(set=1, reserved=1), b"reserved")):
                assert paf_maf(lib, paf, st, fasta, **kw)[0] == -1 and word in lib.swg_alnstats_last_error(), kw
            assert paf_maf(lib, paf, None, fasta, set=1)[0] == -1 and b"status" in lib.swg_alnstats_last_error()
            assert paf_maf(lib, paf, st, None, set=1)[0] == -1 and b"NULL sequences" in lib.swg_alnstats_last_error()
            assert paf_maf(lib, paf, st, fasta, **{})[0] == -1      # (set = 0 over records: a NULL context)
            assert paf_maf(lib, paf, st, fasta, want=False, set=1)[0] == -1 and b"NULL argument" in lib.swg_alnstats_last_error()
            out = tmp_path / "no.maf"
            assert lib.swg_paf_maf_write(None, paf.handle, st.ctypes.data, fasta, None, str(out).encode(), None) == -1 and not out.exists()
            assert b"NULL options" in lib.swg_alnstats_last_error()
            with pytest.raises(SwgError):
                Maf.write_paf(paf, st, out, fasta=[str(fa)], set=2)
            assert not out.exists()
            with pytest.raises(SwgError):
                Maf.from_paf(paf, st, fasta=[str(tmp_path / "missing.fa")])
        with PafFile(text=REBASED) as paf:
            with pytest.raises(SwgError) as e:
                Maf.from_paf(paf, np.ones(1, dtype=np.uint8), fasta=[str(fa)])
            assert e.value.code == -6 and "2^32" in str(e.value)


def test_command_line_usage_errors(lib, tmp_path):
    from sweepga_amd import build
    from tests.test_ucsc_chain_cpu import mixed_paf
    paf, fa = tmp_path / "in.paf", tmp_path / "s.fa"
    paf.write_text(mixed_paf()[0])
    fa.write_text(">g1#1#q\nACGT\n")
    out, maf = tmp_path / "out.paf", tmp_path / "e.maf"
    run = lambda *a: subprocess.run([build.CLI, str(paf), "--output-file", str(out), *a], capture_output=True, text=True)      # noqa: E731
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(w in r.stdout for w in ("--maf FILE", "--maf-fasta FASTA", "--maf-set kept|all", "--maf-split-gap N", "--maf-batch BYTES"))
    assert re.search(r"score is the block's aligned columns", r.stdout)
    need, fasta = "need --maf", ["--maf-fasta", str(fa)]
    cases = [(["--maf", str(maf)], "--maf needs --maf-fasta"),
             (fasta, need), (["--maf-set", "all"], need), (["--maf-split-gap", "50"], need), (["--maf-batch", "4k"], need),
             (["--maf", str(maf), *fasta, "--maf-set", "lost"], "--maf-set: kept or all"),
             (["--maf", str(maf), *fasta, "--maf-split-gap", "many"], "--maf-split-gap"),
             (["--maf", str(maf), *fasta, "--maf-split-gap", "5g"], "--maf-split-gap"),
             (["--maf", str(maf), *fasta, "--maf-batch", "0"], "--maf-batch"),
             (["--maf", str(maf), *fasta, "--maf-batch", "many"], "--maf-batch"),
             (["--maf", str(maf), "--maf-fasta", str(tmp_path / "missing.fa")], "--maf-fasta"),
             (["--maf", str(maf), "--maf-fasta", "-"], "--maf-fasta needs a file"),
             (["--maf", str(maf), "--maf-fasta", ""], "--maf-fasta needs a file"),
             (["--maf", "-", *fasta], "not a standard error report"),
             (["--maf", "", *fasta], "empty value for --maf")]
    for extra, word in cases:
        r = run(*extra)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)
        assert r.stdout == "" and not out.exists() and not maf.exists(), extra


def test_block_formatter_under_the_host_sanitizers(tmp_path):
    """tests/native/maf_text_check.cpp: a stand-alone program over csrc/host/maf_text.cpp, built with the address and
    undefined-behaviour sanitizers; every block must be the model's byte for byte."""
    exe = str(tmp_path / "maf_text_check")
    host = os.path.join(ROOT, "sweepga_amd", "csrc", "host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "maf_text_check.cpp"), os.path.join(host, "maf_text.cpp"),
                           os.path.join(host, "ucsc_text.cpp"), os.path.join(host, "cigar_text.cpp"), "-lpthread"])
    top = 2**32 - 1
    head = "q\t%d\t%d\t%d\t%s\tt\t%d\t%d\t%d\t7\t9\t60\tcg:Z:9M"
    # (line, t_start, t_bases, q_start, q_bases, aligned, columns, flags, rows)
    cases = [(head % (top, top - 9, top, "-", top, top - 9, top), top - 9, 9, top - 9, 9, 9, 9, 1, "ACGTACGTA" "ACGTACGTA"),      # 10-digit fields; '-' from the end: 0
             (head % (100, 10, 19, "-", 50, 0, 9), 0, 9, 10, 9, 9, 9, 1, "ACGTACGTA" "ACGTACGTA"),                                 # 100 - 10 - 9 = 81
             (head % (100, 10, 19, "+", 50, 0, 9), 0, 9, 10, 9, 9, 9, 0, "ACGTACGTA" "ACGTACGTA"),
             (head % (100, 10, 13, "+", 50, 4, 9), 4, 5, 10, 3, 1, 7, 0, "AC--GTA" "-Cgg---"),                                     # gaps in both rows
             (head % (7, 0, 1, "-", 1, 0, 1) + "\r", 0, 1, 0, 1, 1, 1, 1, "N" "n")]                                                # one column; a '\r' at the line's end
    stdin = "".join("%s\n%d %d %d %d %d %d %d\n%s\n" % (c[0], *c[1:8], c[8] or ".") for c in cases)
    r = subprocess.run([exe, "long"], input=stdin.encode("latin-1"), capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]

    def want_of(line, t_start, t_bases, q_start, q_bases, aligned, columns, flags, rows):
        f = line.rstrip("\r").split("\t")
        return mm.block_text(f[5], int(f[6]), f[0], int(f[1]), dict(t_start=t_start, t_bases=t_bases, q_start=q_start, q_bases=q_bases, aligned=aligned,
                                                                    columns=columns, flags=flags), rows)
    want = "".join(want_of(*c) for c in cases)
    q, t = "q" * 100_000, "t" * 100_000
    want += want_of(q + "\t4294967295\t5\t70005\t-\t" + t + "\t4294967295\t4294900000\t4294967295\t1\t2\t60\tcg:Z:1M", 4294900000, 67295, 5, 70000, 67295, 70000, 1,
                    "A" * 70000 + "c" * 70000)
    assert r.stdout.decode("latin-1") == want
    assert want.startswith("a score=9\ns t %d 9 + %d ACGTACGTA\ns q 0 9 - %d ACGTACGTA\n\na score=9\ns t 0 9 + 50 ACGTACGTA\ns q 81 9 - 100 ACGTACGTA\n\n" % (top - 9, top, top))
