"""The resolved CIGARs without a GPU: the model of tests/eqx_model.py against lines worked out by hand on both strands, its
invariants on 3,000 random entries (state and advances of the output, idempotence, the columns, the variant calls' sums, the
difference list's counts), and the host side of the feature -- header, ctypes mirrors, exported symbols, the record seams' refusal
without a context, the rules of csrc/swg_eqx_walk.h run on a CPU under the host sanitizers against the model, the PAF seam's
no-device paths and refusals, the usage errors of --eqx, and the line formatter under the host sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import diffs_model as dm
from tests import eqx_model as xm
from tests import lift_exact_model as em
from tests import variants_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = b"ACGTACGTAC"


def ee(text, minus, q_start, q_end, t_start, T_, Q):
    """-> (output text, out_ops, the non-zero sums)"""
    new, n_out, sums = xm.entry_eqx(text, minus, q_start, q_end, t_start, T_, Q)
    return new, n_out, {k: v for k, v in sums.items() if v}


# ---- the model against lines worked out by hand -----------------------------------------------------------------------------------------
def test_m_ops_by_hand_on_both_strands():
    assert ee("10M", False, 0, 10, 0, T, T) == ("10=", 1, {"matches": 10, "m_columns": 10})
    assert ee("10M", True, 0, 10, 0, T, b"GTACGTACGT") == ("10=", 1, {"matches": 10, "m_columns": 10})      # the reverse complement
    # a mismatch on the first, a middle and the last column
    assert ee("10M", False, 0, 10, 0, T, b"CCGTAGGTAG") == ("1X4=1X3=1X", 5, {"matches": 7, "mismatches": 3, "m_columns": 10})
    # ... and from the other strand: the query holds the walk's reverse complement
    assert ee("10M", True, 2, 12, 0, T, b"ttCTACCTACGGa") == ("1X4=1X3=1X", 5, {"matches": 7, "mismatches": 3, "m_columns": 10})
    assert ee("4M", False, 1, 5, 3, T, b"gTACCg") == ("3=1X", 2, {"matches": 3, "mismatches": 1, "m_columns": 4})      # offsets on both sides


def test_runs_merge_split_and_vanish_by_hand():
    assert ee("3M0=2X4M", False, 0, 9, 0, T, T[:9]) == ("9=", 1, {"matches": 9, "x_wrong": 2, "m_columns": 7})      # a run merges across ops
    assert ee("5M0I5M", False, 0, 10, 0, T, T) == ("5=0I5=", 3, {"matches": 10, "m_columns": 10})      # a zero-length foreign op splits the run and is copied
    assert ee("2I0M3D", False, 0, 2, 0, T, b"GG") == ("2I3D", 2, {"inserted": 2, "deleted": 3})      # 0M alone between I and D vanishes
    assert ee("0M", False, 0, 0, 0, T, T) == ("", 0, {})
    assert ee("007I03=", False, 0, 10, 0, T, b"GGGGGGGACG") == ("007I3=", 2, {"matches": 3, "inserted": 7})      # 007I is kept, 03= is written anew
    assert ee("2=1X2=", False, 0, 5, 0, T, b"ACCTA") == ("2=1X2=", 3, {"matches": 4, "mismatches": 1})      # nothing to change


def test_wrong_letters_n_and_case_by_hand():
    assert ee("3=", False, 0, 3, 0, T, b"ACC") == ("2=1X", 2, {"matches": 2, "mismatches": 1, "eq_wrong": 1})      # an = over a differing base
    assert ee("1=2X", False, 0, 3, 0, T, b"ACC") == ("2=1X", 2, {"matches": 2, "mismatches": 1, "x_wrong": 1})      # an X over equal bases
    # N and IUPAC on either side give X, count in n_columns and are never equal, not even to themselves
    assert ee("5M", False, 0, 5, 0, b"ANGRA", b"ACNRA") == ("1=3X1=", 3, {"matches": 2, "mismatches": 3, "n_columns": 3, "m_columns": 5})
    assert ee("2=", True, 0, 2, 0, b"N-", b"*N") == ("2X", 1, {"mismatches": 2, "n_columns": 2, "eq_wrong": 2})
    assert ee("4M", False, 0, 4, 0, b"acGT", b"ACgt") == ("4=", 1, {"matches": 4, "m_columns": 4})      # lower case is equal
    assert ee("4M", True, 0, 4, 0, b"acGT", b"acGT") == ("4=", 1, {"matches": 4, "m_columns": 4})      # ACGT is its own reverse complement


def test_foreign_ops_are_verbatim_by_hand():
    got = ee("2S1H3M2N0P2M1S00D", False, 0, 5, 0, T, b"ACGCG")
    assert got == ("2S1H3=2N0P2=1S00D", 8, {"matches": 5, "m_columns": 5})      # N advances the target and is no deleted base
    assert ee("1D2N1D1M", False, 0, 1, 0, T, b"A") == ("1D2N1D1=", 4, {"matches": 1, "m_columns": 1, "deleted": 2})


def test_digit_counts_by_hand():
    big = b"A" * 100_000
    for k in range(1, 6):
        for L in (10**k - 1, 10**k):
            new, n_out, sums = xm.entry_eqx("%dM" % L, False, 0, L, 0, big, big)
            assert (new, n_out, sums["matches"]) == ("%d=" % L, 1, L) and len(new) == len(str(L)) + 1
    q = b"A" * 99_999 + b"C"
    assert xm.entry_eqx("100000M", True, 0, 100_000, 0, b"T" * 100_000, q)[0] == "1X99999="


def small_table():
    """Seven records over targets 0, 1, 2 (absent) and queries 3, 4; record 5 ends behind its target, record 6 is outside the set."""
    seqs = [T, b"GGGGG", b"", b"ttCCa", b"ACGTTT"]
    cols = {"q_id": [3, 4, 3, 4, 3, 3, 3], "t_id": [0, 1, 2, 0, 1, 0, 0], "q_start": [2, 0, 0, 0, 2, 2, 2], "q_end": [4, 2, 2, 6, 4, 4, 4],
            "t_start": [0, 0, 0, 4, 0, 8, 1], "t_end": [2, 2, 2, 10, 2, 11, 3]}
    cig = {0: "2X", 1: "2M", 2: "2X", 3: "6M", 4: "2=", 5: "2X1D", 6: "2M"}
    return {k: np.array(v) for k, v in cols.items()}, np.zeros(7, dtype=np.uint8), cig, seqs


def test_every_unusable_reason():
    cols, strand, cig, seqs = small_table()
    got = xm.eqx_records(cols, strand, cig, seqs)
    assert (got["usable"], got["no_sequence"], got["out_of_sequence"], got["cigar_bad"], got["empty"]) == (5, 1, 1, 0, 0)
    # record 0: AC against CC; 1: GG against AC; 3: ACGTAC against ACGTTT; 4: GG under = against CC; 6: CG against CC
    assert got["text"] == "1X1=" + "2X" + "4=2X" + "2X" + "1=1X" and got["changed"] == 5 and got["out_ops"] == 8 and got["text_bytes"] == 16
    assert [e[0] for e in got["entries"]] == list(range(7)) and got["entries"][2] == (2,) + (0,) * 13 and got["entries"][5] == (5,) + (0,) * 13
    assert got["entries"][3] == (3, 3, 4, 2, 4, 2, 0, 0, 0, 6, 0, 0, 6, 6) and got["entries"][4][7] == 2 and got["entries"][0][8] == 1
    assert (got["columns"], got["matches"], got["mismatches"], got["eq_wrong"], got["x_wrong"], got["m_columns"]) == (14, 6, 8, 2, 1, 10)
    kept = xm.eqx_records(cols, strand, cig, seqs, kept=np.array([1, 0, 1, 0, 0, 1, 0], dtype=bool), set_=1)
    assert (kept["usable"], kept["no_sequence"], kept["out_of_sequence"], kept["text"]) == (1, 1, 1, "1X1=")
    for bad, name in (("2x", "cigar_bad"), ("4294967296X", "cigar_bad"), ("3X", "cigar_bad"), ("2X1D", "cigar_bad"), ("2", "cigar_bad"), ("", "empty")):
        for set_ in (0, 1):      # the state is looked at first: a bad or empty entry counts whether its record is in the set or not
            one = xm.eqx_records(cols, strand, {0: bad}, seqs, kept=np.zeros(7, dtype=bool), set_=set_)
            assert (one["usable"], one["text"], one[name], one["entries"]) == (0, "", 1, [(0,) + (0,) * 13]), bad


# ---- invariants on random entries ------------------------------------------------------------------------------------------------------------
def widen(rng, text):
    """zero-length ops, leading zeros and clips sprinkled into a text of state 0 (the advances stay)"""
    out = []
    for digits, ch in xm.raw_ops(text):
        r = rng.random()
        if r < 0.08:
            out.append("0" + "MIDNSHP=X"[int(rng.integers(9))])
        elif r < 0.12:
            out.append("%dS" % int(rng.integers(0, 4)))
        out.append(("0" * int(rng.integers(0, 3)) if rng.random() < 0.1 else "") + digits + ch)
    return "".join(out)


@pytest.mark.parametrize("seed, iupac", [(1, 0.0), (2, 0.0), (3, 0.03)])
def test_invariants_on_random_entries(seed, iupac):
    """1,000 entries per case, both strands, fused M ops, lower case, X ops over equal bases, zero-length ops and leading zeros.  The
    variant calls compare the columns under X and M only, so their sums are held against the entries' in two ways: on the input as it
    stands with the columns under = taken off (matches - (= columns - eq_wrong) = same + m_equal, mismatches - eq_wrong = snvs +
    n_columns), and, as stated for an input whose columns all lie under X and M, on the same input with every = written as M:
    matches = same + m_equal and mismatches = snvs + n_columns, per genome pair."""
    rng = np.random.default_rng(seed)
    n_changed = n_strand = 0
    for _ in range(50):
        cols, strand, genome, cig, seqs = vm.random_case(rng, 20, iupac=iupac)
        cig = {i: widen(rng, t) for i, t in cig.items()}
        got = xm.eqx_records(cols, strand, cig, seqs)
        assert got["usable"] == 20 and got["cigar_bad"] == 0
        n_changed += got["changed"]
        n_strand += int(np.sum(strand))
        out = {}
        pair_sums, eq_columns = {}, {}
        for row in got["entries"]:
            e = dict(zip(xm.ENTRY_FIELDS, row))
            i = e["record"]
            rec = tuple(int(cols[c][i]) for c in ("q_start", "q_end", "t_start", "t_end"))
            new = got["text"][e["text_first"]:e["text_first"] + e["text_len"]]
            out[i] = new
            assert em.entry_state(new, rec[1] - rec[0], rec[3] - rec[2]) == 0 if new else rec[0] == rec[1] and rec[2] == rec[3]
            assert "M" not in new and e["out_ops"] == len(xm.raw_ops(new)) and bool(e["flags"] & xm.CHANGED) == (new != cig[i])
            letters = [ch for _, ch in xm.raw_ops(new)]
            assert all(not (a in "=X" and a == b) for a, b in zip(letters, letters[1:]))      # inside a run no two neighbours alike
            assert not any(int(d) == 0 for d, ch in xm.raw_ops(new) if ch in "=X")
            d_in = dm.entry_diffs(cig[i], bool(strand[i]), *rec, check=False)[1]
            assert e["matches"] + e["mismatches"] == d_in["aligned"] and e["block"] == d_in["aligned"] + d_in["ins_bases"] + d_in["del_bases"]
            if new:
                d_out = dm.entry_diffs(new, bool(strand[i]), *rec, check=False)[1]
                assert d_out["m_columns"] == 0 and all(d_out[k] == d_in[k] for k in ("aligned", "ins_bases", "del_bases", "n_ins", "n_del", "skip_bases"))
                assert (d_out["eq"], d_out["snp_bases"]) == (e["matches"], e["mismatches"])
            key = (int(genome[cols["q_id"][i]]), int(genome[cols["t_id"][i]]))
            acc = pair_sums.setdefault(key, dict.fromkeys(("matches", "mismatches", "eq_wrong"), 0))
            for k in acc:
                acc[k] += e[k]
            eq_columns[key] = eq_columns.get(key, 0) + d_in["eq"]
        # idempotence: the output fed back gives itself, with nothing wrong and nothing under M
        again = xm.eqx_records(cols, strand, out, seqs)
        assert again["text"] == got["text"] and (again["eq_wrong"], again["x_wrong"], again["m_columns"], again["changed"]) == (0, 0, 0, 0)
        assert [e[2:] for e in again["entries"]] == [e[2:7] + (0, 0, 0) + e[10:] for e in got["entries"]]
        var = vm.variant_records(cols, strand, genome, 2, cig, seqs, check=False)
        as_m = vm.variant_records(cols, strand, genome, 2, {i: t.replace("=", "M") for i, t in cig.items()}, seqs, check=False)
        assert sorted(pair_sums) == [p[:2] for p in var["pairs"]] == [p[:2] for p in as_m["pairs"]]
        for p, pm in zip(var["pairs"], as_m["pairs"]):
            v, m, acc = dict(zip(vm.SUMS, p[2:])), dict(zip(vm.SUMS, pm[2:])), pair_sums[p[:2]]
            assert acc["matches"] - (eq_columns[p[:2]] - acc["eq_wrong"]) == v["same"] + v["m_equal"] and acc["mismatches"] - acc["eq_wrong"] == v["snvs"] + v["n_columns"]
            assert acc["matches"] == m["same"] + m["m_equal"] and acc["mismatches"] == m["snvs"] + m["n_columns"]
    assert n_changed > 500 and 300 < n_strand < 700


# ---- the host side ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib, eqx
    structs = (("swg_eqx_request", _lib.SwgEqxRequest), ("swg_eqx_options", _lib.SwgEqxOptions), ("swg_eqx_counts", _lib.SwgEqxCounts))
    prints = ['printf("%%zu\\n", sizeof(%s));' % name for name in ("swg_eqx_entry", "swg_eqx_request", "swg_eqx_options", "swg_eqx_counts")]
    prints += ['printf("%%zu\\n", offsetof(%s, %s));' % (name, f) for name, cls in structs for f, _ in cls._fields_]
    prints += ['printf("%%zu\\n", offsetof(swg_eqx_entry, %s));' % f for f in eqx.EQX_ENTRY_DTYPE.names]
    prints += ['printf("%u %u %u %u %u %u %d\\n", SWG_EQX_USABLE, SWG_EQX_CHANGED, SWG_EQX_KEEP, SWG_EQX_DROP, SWG_EQX_COLUMN_TILE, SWG_EQX_TEXT_TILE, SWG_ABI_VERSION);']
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [64, 168, 24, 128] + [getattr(cls, f).offset for _, cls in structs for f, _ in cls._fields_]
    want += [eqx.EQX_ENTRY_DTYPE.fields[f][1] for f in eqx.EQX_ENTRY_DTYPE.names]
    assert got == want + [xm.USABLE, xm.CHANGED, 0, 1, 4096, 4096, 1]
    for _, cls in structs:      # no implicit padding
        assert sum(C.sizeof(t) for _, t in cls._fields_) == C.sizeof(cls) == {"SwgEqxRequest": 168, "SwgEqxOptions": 24, "SwgEqxCounts": 128}[cls.__name__]
    assert eqx.EQX_ENTRY_DTYPE.itemsize == 64 and eqx.EQX_ENTRY_DTYPE.names == xm.ENTRY_FIELDS and eqx.FIELDS == xm.FIELDS and _lib.EQX_COUNTS == xm.COUNTS
    assert (eqx.USABLE, eqx.CHANGED, eqx.UNRESOLVED) == (xm.USABLE, xm.CHANGED, {"keep": 0, "drop": 1})


def test_symbols_are_exported_and_declared(lib):
    import sweepga_amd
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_eqx_records", "swg_eqx_records_device", "swg_paf_eqx_write", "swg_paf_eqx_text"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    assert lib.swg_abi_version() == 1
    for name in ("EQX_ENTRY_DTYPE", "Eqx", "EqxResult", "eqx_records", "eqx_records_device"):
        assert hasattr(sweepga_amd, name)
    assert "swg_eqx.hip" in sweepga_amd.build.SOURCES and os.path.join("host", "eqx_text.cpp") in sweepga_amd.build.SOURCES


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
    for fn in (lib.swg_eqx_records, lib.swg_eqx_records_device):
        req = _lib.SwgEqxRequest()
        req.entry_capacity, req.entries, req.text_capacity, req.text, req.usable, req.text_bytes = 7, poison.ctypes.data, 64, poison.ctypes.data + 448, 77, 12345
        assert fn(None, C.byref(rec), None, C.byref(cs), C.byref(ss), C.byref(req)) == -1
        assert (poison == 0xab).all() and req.usable == 77 and req.text_bytes == 12345


def walk_lines(rng, n):
    """n random entries -> (the input lines of eqx_walk_check, what the model says of each)"""
    lines, want = [], []
    for k in range(n):
        cols, strand, _, cig, seqs = vm.random_case(rng, 1, n_targets=1, n_queries=1, iupac=0.05 if k % 3 == 0 else 0.0, flank=3)
        rec = tuple(int(cols[c][0]) for c in ("q_start", "q_end", "t_start", "t_end"))
        text = widen(rng, cig[0])
        lines.append("%d %d %d %d %s %s %s" % (strand[0], rec[0], rec[1], rec[2], seqs[0].decode(), seqs[1].decode(), text))
        new, n_out, s = xm.entry_eqx(text, bool(strand[0]), rec[0], rec[1], rec[2], seqs[0], seqs[1])
        want.append("%s %d %s" % (new or "-", n_out, " ".join(str(s[f]) for f in xm.SUMS)))
    return lines, want


def test_the_rules_of_the_walk_header_on_a_cpu(tmp_path):
    """tests/native/eqx_walk_check.cpp: csrc/swg_eqx_walk.h as a host compiler takes it, under the sanitizers, against the model: the
    output text, its ops and the six sums of 400 random entries, and the digits of every length around a power of ten."""
    exe = str(tmp_path / "eqx_walk_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "eqx_walk_check.cpp")])
    lines, want = walk_lines(np.random.default_rng(4), 400)
    lengths = sorted({v for k in range(1, 10) for v in (10**k - 1, 10**k, 10**k + 1)} | {1, 2, 4294967295, 4000000000, 1234567890})
    lines += ["digits %d" % v for v in lengths]
    want += ["%d %d=" % (len(str(v)), v) for v in lengths]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = r.stdout.strip().split("\n")
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (k, lines[k], a, b)
    assert sum("X" in w for w in want[:400]) > 200 and sum(w.startswith("-") for w in want[:400]) < 20


# ---- the PAF seam without a device ---------------------------------------------------------------------------------------------------------
def test_the_model_text_by_hand():
    t, q = b"ACGTACGTAC", b"ACCTAGCGAC"          # ACGTA-CGTAC against ACCTAGCG-AC
    line = "q#1#a\t10\t0\t10\t+\tt#1#b\t10\t0\t10\t5\t9\t60\tNM:i:9\tcg:Z:5M1I2M1D2M\tde:f:0.1"
    paf = line + "\n" + line.replace("cg:Z:5M1I2M1D2M", "xx:Z:none") + "\n"
    text, counts = xm.paf_text(paf, None, [("t#1#b", t), ("q#1#a", q), ("t#1#b", b"TTTTTTTTTT")], 0)
    assert text == "q#1#a\t10\t0\t10\t+\tt#1#b\t10\t0\t10\t8\t11\t60\tNM:i:9\tcg:Z:2=1X2=1I2=1D2=\tde:f:0.1\n" + paf.split("\n")[1] + "\n"
    assert counts == dict(dict.fromkeys(xm.COUNTS[:-1], 0), records=2, usable=1, untagged=1, changed=1, lines=2, columns=9, matches=8, mismatches=1, m_columns=9)
    assert xm.paf_text(paf, None, [("t#1#b", t), ("q#1#a", q)], 0, "drop")[0] == text.split("\n")[0] + "\n"
    assert xm.paf_text(paf, None, [("t#1#b", t + b"A"), ("q#1#a", q)], 0)[1] == dict(dict.fromkeys(xm.COUNTS[:-1], 0), records=2, untagged=1, no_sequence=1,
                                                                                    length_mismatch=1, lines=2)
    assert xm.paf_text(paf, np.array([0, 0]), [], 1) == ("", dict.fromkeys(xm.COUNTS[:-1], 0))
    assert xm.batch_costs("a\t9\t0\t9\t+\tb\t20\t0\t10\t0\t0\t0\tcg:Z:10M\n", None, 0) == [3 + 9]


def paf_eqx(lib, paf, status, fasta, ctx=None, want=True, **kw):
    """swg_paf_eqx_text -> (rc, text or None, counts)"""
    from sweepga_amd import _lib
    opts = _lib.SwgEqxOptions()
    for k, v in (kw or {}).items():
        setattr(opts, k, v)
    counts = _lib.SwgEqxCounts()
    p, n = C.c_void_p(), C.c_uint64()
    rc = lib.swg_paf_eqx_text(ctx, paf.handle, status.ctypes.data if status is not None else None, fasta, C.byref(opts) if kw is not None else None,
                              C.byref(counts), C.byref(p) if want else None, C.byref(n) if want else None)
    if rc != 0:
        assert not p.value
        return rc, None, None
    text = C.string_at(p.value, n.value).decode() if p.value else None
    lib.swg_free(p)
    return rc, text, {k: int(getattr(counts, k)) for k in xm.COUNTS}


def test_paf_seam_without_a_device(lib, tmp_path):
    """A PAF without records of the set gives an empty text and needs no device; the refusals come before a context is looked at and
    before a file is opened."""
    from sweepga_amd import Eqx, PafFile, SwgError
    from sweepga_amd.variants import _FastaHandle
    from tests.test_lift_cpu import REBASED
    from tests.test_ucsc_chain_cpu import mixed_paf
    fa = tmp_path / "s.fa"
    fa.write_text(">g1#1#q\nACGT\n>g2#1#t\nAC\nGT\n")
    zero = dict.fromkeys(xm.COUNTS, 0)
    with _FastaHandle(lib, [str(fa)]) as fasta:
        for text in ("", "# nothing\nfew\tfields\n"):
            with PafFile(text=text) as paf:
                for st in (None, np.zeros(1, dtype=np.uint8)):
                    assert paf_eqx(lib, paf, st, fasta, set=0) == (0, "", zero)
                    assert paf_eqx(lib, paf, st, fasta, set=0, unresolved=1, batch_bytes=5) == (0, "", zero)
                got = Eqx.from_paf(paf, None, fasta=[str(fa)], set="all")
                assert (got.text, got.counts) == ("", zero)
                out = tmp_path / "empty.paf"
                assert Eqx.write_paf(paf, None, out, fasta=[str(fa)], set="all", unresolved="drop") == zero and out.read_bytes() == b""
        text, kept = mixed_paf()
        with PafFile(text=text) as paf:
            none, st = np.zeros(paf.n, dtype=np.uint8), kept.astype(np.uint8)
            assert paf_eqx(lib, paf, none, fasta, set=1) == (0, "", zero)      # a set that is never in status: no device
            assert paf_eqx(lib, paf, st, fasta, set=1)[0] == -1 and b"swg_paf_eqx_text: NULL context" in lib.swg_alnstats_last_error()
            for kw, word in ((dict(set=2), b"set"), (dict(set=1, reserved=1), b"reserved"), (dict(set=1, unresolved=2), b"unresolved")):
                assert paf_eqx(lib, paf, st, fasta, **kw)[0] == -1 and word in lib.swg_alnstats_last_error(), kw
            assert paf_eqx(lib, paf, None, fasta, set=1)[0] == -1 and b"status" in lib.swg_alnstats_last_error()
            assert paf_eqx(lib, paf, st, None, set=1)[0] == -1 and b"NULL sequences" in lib.swg_alnstats_last_error()
            assert paf_eqx(lib, paf, st, fasta, **{})[0] == -1      # (set = 0 over records: a NULL context)
            assert paf_eqx(lib, paf, st, fasta, want=False, set=1)[0] == -1 and b"NULL argument" in lib.swg_alnstats_last_error()
            out = tmp_path / "no.paf"
            assert lib.swg_paf_eqx_write(None, paf.handle, st.ctypes.data, fasta, None, str(out).encode(), None) == -1 and not out.exists()
            assert b"NULL options" in lib.swg_alnstats_last_error()
            with pytest.raises(SwgError):
                Eqx.write_paf(paf, st, out, fasta=[str(fa)], set=2)
            with pytest.raises(SwgError):
                Eqx.write_paf(paf, st, out, fasta=[str(fa)], unresolved=7)
            assert not out.exists()
            with pytest.raises(SwgError):
                Eqx.from_paf(paf, st, fasta=[str(tmp_path / "missing.fa")])
        with PafFile(text=REBASED) as paf:
            with pytest.raises(SwgError) as e:
                Eqx.from_paf(paf, np.ones(1, dtype=np.uint8), fasta=[str(fa)])
            assert e.value.code == -6 and "2^32" in str(e.value)


def test_command_line_usage_errors(lib, tmp_path):
    from sweepga_amd import build
    from tests.test_ucsc_chain_cpu import mixed_paf
    paf, fa = tmp_path / "in.paf", tmp_path / "s.fa"
    paf.write_text(mixed_paf()[0])
    fa.write_text(">g1#1#q\nACGT\n")
    out, eqx = tmp_path / "out.paf", tmp_path / "e.paf"
    run = lambda *a: subprocess.run([build.CLI, str(paf), "--output-file", str(out), *a], capture_output=True, text=True)      # noqa: E731
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(w in r.stdout for w in ("--eqx FILE", "--eqx-fasta FASTA", "--eqx-set kept|all", "--eqx-unresolved keep|drop",
                                                              "--eqx-batch BYTES"))
    need, fasta = "need --eqx", ["--eqx-fasta", str(fa)]
    cases = [(["--eqx", str(eqx)], "--eqx needs --eqx-fasta"),
             (fasta, need), (["--eqx-set", "all"], need), (["--eqx-unresolved", "drop"], need), (["--eqx-batch", "4k"], need),
             (["--eqx", str(eqx), *fasta, "--eqx-set", "lost"], "--eqx-set: kept or all"),
             (["--eqx", str(eqx), *fasta, "--eqx-unresolved", "maybe"], "--eqx-unresolved: keep or drop"),
             (["--eqx", str(eqx), *fasta, "--eqx-batch", "0"], "--eqx-batch"),
             (["--eqx", str(eqx), *fasta, "--eqx-batch", "many"], "--eqx-batch"),
             (["--eqx", str(eqx), "--eqx-fasta", str(tmp_path / "missing.fa")], "--eqx-fasta"),
             (["--eqx", str(eqx), "--eqx-fasta", "-"], "--eqx-fasta needs a file"),
             (["--eqx", str(eqx), "--eqx-fasta", ""], "--eqx-fasta needs a file"),
             (["--eqx", "-", *fasta], "not a standard error report"),
             (["--eqx", "", *fasta], "empty value for --eqx")]
    for extra, word in cases:
        r = run(*extra)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)
        assert r.stdout == "" and not out.exists() and not eqx.exists(), extra


def test_line_formatter_under_the_host_sanitizers(tmp_path):
    """tests/native/eqx_text_check.cpp: a stand-alone program over csrc/host/eqx_text.cpp, built with the address and
    undefined-behaviour sanitizers; every rewritten line must be the model's byte for byte."""
    exe = str(tmp_path / "eqx_text_check")
    host = os.path.join(ROOT, "sweepga_amd", "csrc", "host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "eqx_text_check.cpp"), os.path.join(host, "eqx_text.cpp"),
                           os.path.join(host, "ucsc_text.cpp"), os.path.join(host, "cigar_text.cpp"), "-lpthread"])
    top = 2**32 - 1
    head = "q\t%d\t%d\t%d\t-\tt\t%d\t%d\t%d" % (top, top - 9, top, top, top - 9, top)
    cases = [(head + "\t7\t9\t60\tcg:Z:9M", top, 3 * top, "4294967295="),                                   # 10-digit columns, the tag alone
             (head + "\t7\t9\t60\tcg:Z:9M\tNM:i:2\tde:f:0.01", 0, 0, "9X"),                                  # first among the tags
             (head + "\t1234567\t7654321\t0\tNM:i:2\tcg:Z:3=3X3=\tde:f:0.01", 6, 9, "3=3X3="),               # in the middle; shorter columns
             (head + "\t7\t9\t60\tNM:i:2\tde:f:0.01\tcg:Z:9M", 9, 9, "9="),                                  # last
             (head + "\t7\t9\t60\tcg:Z:4M\tNM:i:2\tcg:Z:9M\txcg:Z:1M", 8, 10, "4=1X4="),                     # two tags: the last counts, the first stays
             (head + "\t7\t9\t60\tzz:Z:cg:Z:5M\tcg:Z:2I", 0, 2, "2I"),                                       # the bytes inside another value are no tag
             (head + "\t\t\t60\tcg:Z:0M", 0, 0, ""),                                                        # empty columns, an empty text
             (head + "\t7\t9", 1, 1, "1=")]                                                                 # no tags at all
    stdin = "".join("%s\n%d %d\n%s\n" % (ln, m, b, new or "-") for ln, m, b, new in cases)
    r = subprocess.run([exe, "long"], input=stdin.encode("latin-1"), capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]
    got = r.stdout.decode("latin-1").split("\n")
    want = [xm.rewrite_line(ln, m, b, new) for ln, m, b, new in cases[:-1]] + ["NO-TAG"]
    q, t = "q" * 100_000, "t" * 100_000
    want.append(xm.rewrite_line(q + "\t9\t0\t9\t-\t" + t + "\t9\t0\t9\t1\t2\t60\tNM:i:3\tcg:Z:9M\tzz:Z:" + q, top, 3 * top, "=" * 70_000 + "1X"))
    assert got == want + [""]
    assert want[4] == head + "\t8\t10\t60\tcg:Z:4M\tNM:i:2\tcg:Z:4=1X4=\txcg:Z:1M"
