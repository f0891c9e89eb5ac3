"""The variant calls without a GPU: the model of tests/variants_model.py against variants worked out by hand on both strands, its
three invariants on 3,000 random entries (the sums, the difference list's counts, the consensus property), and the host side of the
feature -- header, ctypes mirrors, exported symbols, the record seams' refusal without a context, the rules of
csrc/swg_variants_walk.h run on a CPU under the host sanitizers against the model, the texts of the PAF seam by hand, its no-device
paths and refusals, the usage errors of --vcf, and the formatters and the batch merge under the host sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import variants_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNP, INS, DEL, MINUS = vm.SNP, vm.INS, vm.DEL, vm.MINUS
T = b"ACGTACGTAC"


def ev(text, minus, q_start, q_end, t_start, t_end, T_, Q, **kw):
    """-> (variants without the record, the non-zero sums)"""
    got, sums = vm.entry_variants(text, minus, q_start, q_end, t_start, t_end, T_, Q, **kw)
    return [v[1:] for v in got], {k: v for k, v in sums.items() if v}


# ---- the model against lines worked out by hand -----------------------------------------------------------------------------------------
def test_both_strands_by_hand():
    # target bases 2 .. 9: GT = | A x | (an inserted G) | CG = | TA deleted | C =; the walk reads GT T G CG C
    sums = {"compared": 1, "snvs": 1, "A>T": 1, "n_ins": 1, "ins_bases": 1, "n_del": 1, "del_bases": 2}
    plus = ev("2=1X1I2=2D1=", False, 3, 10, 2, 10, T, b"aaaGTTGCGCtt")
    assert plus == ([(SNP, 4, "A", "T", 5), (INS, 4, "A", "AG", 6), (DEL, 6, "GTA", "G", 9)], sums)
    # the same alignment from the other strand: the query holds the walk's reverse complement, its coordinates descend
    minus = ev("2=1X1I2=2D1=", True, 3, 10, 2, 10, T, b"aaaGCGCAACtt")
    assert minus == ([(SNP | MINUS, 4, "A", "T", 7), (INS | MINUS, 4, "A", "AG", 6), (DEL | MINUS, 6, "GTA", "G", 4)], sums)


def test_first_and_last_op_and_the_first_base_by_hand():
    assert ev("1X2=1X", False, 1, 5, 0, 4, T, b"tCCGGa")[0] == [(SNP, 0, "A", "C", 1), (SNP, 3, "T", "G", 4)]
    assert ev("1X2=1X", True, 1, 5, 0, 4, T, b"tCCGGa")[0] == [(SNP | MINUS, 0, "A", "C", 4), (SNP | MINUS, 3, "T", "G", 1)]      # CCGG is its own reverse complement
    assert ev("1I2=1I", False, 0, 4, 1, 3, T, b"TCGA")[0] == [(INS, 0, "A", "AT", 0), (INS, 2, "G", "GA", 3)]
    assert ev("1D2=1D", False, 2, 4, 1, 5, T, b"ccGT")[0] == [(DEL, 0, "AC", "A", 2), (DEL, 3, "TA", "T", 4)]
    # at a contig's first base the anchor is the base BEHIND the indel
    assert ev("2I3=", False, 0, 5, 0, 3, T, b"TTACG") == ([(INS, 0, "A", "TTA", 0)], {"n_ins": 1, "ins_bases": 2})
    assert ev("2I3=", True, 0, 5, 0, 3, T, b"CGTAA") == ([(INS | MINUS, 0, "A", "TTA", 3)], {"n_ins": 1, "ins_bases": 2})
    assert ev("2D3=", False, 4, 7, 0, 5, T, b"ccccGTA") == ([(DEL, 0, "ACG", "G", 4)], {"n_del": 1, "del_bases": 2})
    assert ev("2D3=", True, 4, 7, 0, 5, T, b"ccccTAC") == ([(DEL | MINUS, 0, "ACG", "G", 7)], {"n_del": 1, "del_bases": 2})
    # a deletion of the whole target has no anchor
    assert ev("3D", False, 2, 2, 0, 3, b"ACG", b"tttt") == ([], {"n_del": 1, "del_bases": 3, "unanchored": 1})
    assert ev("3D", False, 2, 2, 0, 3, b"ACGT", b"tttt") == ([(DEL, 0, "ACGT", "T", 2)], {"n_del": 1, "del_bases": 3})
    assert ev("1D", True, 0, 0, 0, 1, b"g", b"a") == ([], {"n_del": 1, "del_bases": 1, "unanchored": 1})
    # I directly before D: both anchored on base 3
    assert ev("2=1I1D2=", False, 0, 5, 2, 7, T, b"GTCCG")[0] == [(INS, 3, "T", "TC", 2), (DEL, 3, "TA", "T", 3)]


def test_columns_by_hand():
    assert ev("2X", False, 0, 2, 0, 2, T, b"CA") == ([(SNP, 0, "A", "C", 0), (SNP, 1, "C", "A", 1)], {"compared": 2, "snvs": 2, "A>C": 1, "C>A": 1})      # no MNP
    assert ev("4M", False, 0, 4, 0, 4, T, b"acgt") == ([], {"compared": 4, "m_equal": 4})
    assert ev("4M", True, 0, 4, 0, 4, T, b"ACCT") == ([(SNP | MINUS, 1, "C", "G", 2)], {"compared": 4, "snvs": 1, "C>G": 1, "m_equal": 3})
    assert ev("4M", False, 0, 4, 0, 4, b"AnGT", b"CCRT") == ([(SNP, 0, "A", "C", 0)], {"compared": 4, "snvs": 1, "A>C": 1, "n_columns": 2, "m_equal": 1})
    assert ev("2X", False, 0, 2, 0, 2, b"A-", b"*G") == ([], {"compared": 2, "n_columns": 2})
    assert ev("1X1=1X", False, 0, 3, 0, 3, T, b"AcG") == ([], {"compared": 2, "same": 2})      # X ops over equal bases
    assert ev("1N1X1S1H1P0X0I0D", False, 0, 1, 0, 2, T, b"G") == ([(SNP, 1, "C", "G", 0)], {"compared": 1, "snvs": 1, "C>G": 1})
    # N may stand in an indel allele
    assert ev("1=2I1=", False, 0, 4, 0, 2, b"nC", b"NRYC")[0] == [(INS, 0, "N", "NNN", 1)]
    assert ev("1=2D", False, 0, 1, 0, 3, b"AyG", b"A")[0] == [(DEL, 0, "ANG", "A", 1)]


def test_max_indel_by_hand():
    for max_indel, variants, n_long in ((0, 2, 0), (2, 0, 2), (3, 2, 0), (4, 2, 0)):
        got, sums = ev("1=3I1=3D1=", False, 0, 6, 0, 6, T, b"ATTTCC", max_indel=max_indel)
        assert len(got) == variants and sums.get("long_indels", 0) == n_long and (sums["n_ins"], sums["ins_bases"], sums["n_del"], sums["del_bases"]) == (1, 3, 1, 3)
    assert ev("3D", False, 0, 0, 0, 3, b"ACG", b"t", max_indel=1)[1] == {"n_del": 1, "del_bases": 3, "unanchored": 1}      # unanchored whatever the limit is


def small_table():
    """Six records over targets 0 (genome 0), 1 (genome 1), 2 (absent) and queries 3 (genome 0), 4 (genome 2)."""
    seqs = [T, b"GGGGG", b"", b"ttCCa", b"ACGTTT"]
    cols = {"q_id": [3, 4, 3, 4, 3, 3], "t_id": [0, 1, 2, 0, 1, 0], "q_start": [2, 0, 0, 0, 2, 2], "q_end": [4, 2, 2, 6, 4, 4],
            "t_start": [0, 0, 0, 4, 0, 8], "t_end": [2, 2, 2, 10, 2, 11]}
    cig = {0: "2X", 1: "2M", 2: "2X", 3: "6M", 4: "2X", 5: "2X1D"}
    return {k: np.array(v) for k, v in cols.items()}, np.zeros(6, dtype=np.uint8), [0, 1, 1, 0, 2], cig, seqs


def test_filters_absent_sequences_bounds_and_states():
    cols, strand, genome, cig, seqs = small_table()
    got = vm.variant_records(cols, strand, genome, 3, cig, seqs)
    assert (got["usable"], got["no_sequence"], got["out_of_sequence"], got["cigar_bad"]) == (4, 1, 1, 0)      # record 2: no target; record 5: t_end = len + 1
    assert [p[:3] for p in got["pairs"]] == [(0, 0, 1), (0, 1, 1), (2, 0, 1), (2, 1, 1)] and got["columns"] == 12
    # record 0: AC against CC; 1: GG against AC; 3: ACGTAC against ACGTTT; 4: GG against CC
    assert [v[0] for v in got["variants"]] == [0, 1, 1, 3, 3, 4, 4] and got["pool"] == b"ACGAGCATCTGCGC" and got["variants"][-1] == (4, SNP, 1, 1, 1, 3, 12)
    by = {kw: vm.variant_records(cols, strand, genome, 3, cig, seqs, **dict([kw])) for kw in (("t_genome", 0), ("t_genome", 1), ("q_genome", 0), ("q_genome", 2),
                                                                                             ("q_genome", 1), ("t_genome", vm.ANY))}
    assert [by[k]["usable"] for k in by] == [2, 2, 2, 2, 0, 4] and by[("t_genome", 1)]["no_sequence"] == 1 and by[("t_genome", 0)]["no_sequence"] == 0
    assert by[("q_genome", 2)]["out_of_sequence"] == 0 and by[("q_genome", 0)]["out_of_sequence"] == 1
    kept = vm.variant_records(cols, strand, genome, 3, cig, seqs, kept=np.array([1, 0, 1, 0, 0, 1], dtype=bool), set_=1)
    assert (kept["usable"], kept["no_sequence"], kept["out_of_sequence"], kept["n_variants"]) == (1, 1, 1, 1)
    for bad in ("2x", "4294967296X", "3X", "2X1D", "", "2"):      # every bad state gives nothing
        one = vm.variant_records(cols, strand, genome, 3, {0: bad}, seqs)
        assert (one["usable"], one["n_variants"], one["n_pairs"], one["pool"]) == (0, 0, 0, b"") and one["cigar_bad"] == (bad != "")


@pytest.mark.parametrize("seed, iupac", [(1, 0.0), (2, 0.0), (3, 0.03)])
def test_the_three_invariants_on_random_entries(seed, iupac):
    """1,000 entries per case, both strands, fused M ops, lower case, X ops over equal bases; the consensus property must have run on
    most of them."""
    rng = np.random.default_rng(seed)
    ran = [0]
    inner = vm.consensus

    def counted(*a):
        out = inner(*a)
        ran[0] += out is not None
        return out
    vm.consensus = counted
    try:
        for _ in range(50):
            cols, strand, genome, cig, seqs = vm.random_case(rng, 20, iupac=iupac)
            got = vm.variant_records(cols, strand, genome, 2, cig, seqs)      # (check=True: every entry is held against the invariants)
            assert got["usable"] == 20 and got["cigar_bad"] == 0
    finally:
        vm.consensus = inner
    assert ran[0] > (900 if iupac == 0 else 300) and 0 < int(np.sum(strand)) < 20


# ---- the host side ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib, variants
    structs = (("swg_seq_set", _lib.SwgSeqSet), ("swg_variant_request", _lib.SwgVariantRequest))
    prints = ['printf("%%zu\\n", sizeof(%s));' % name for name in ("swg_seq_set", "swg_variant_request", "swg_variant", "swg_variant_pair")]
    prints += ['printf("%%zu\\n", offsetof(%s, %s));' % (name, f) for name, cls in structs for f, _ in cls._fields_]
    prints += ['printf("%%zu\\n", offsetof(swg_variant, %s));' % f for f in variants.VARIANT_DTYPE.names]
    prints += ['printf("%%zu\\n", offsetof(swg_variant_pair, %s));' % f for f in ("q_genome", "t_genome", "entries", "compared", "snvs", "sub", "same", "m_equal",
                                                                                 "n_columns", "n_ins", "ins_bases", "n_del", "del_bases", "long_indels", "unanchored")]
    prints += ['printf("%u %u %u %u %u %d\\n", SWG_VARIANTS_ANY == SWG_WINDOWS_ANY, SWG_VARIANT_SNP, SWG_VARIANT_INS, SWG_VARIANT_DEL, SWG_VARIANT_MINUS, SWG_ABI_VERSION);']
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P = variants.PAIR_DTYPE
    want = [24, 144, 32, 200] + [getattr(cls, f).offset for _, cls in structs for f, _ in cls._fields_]
    want += [variants.VARIANT_DTYPE.fields[f][1] for f in variants.VARIANT_DTYPE.names]
    want += [P.fields[f][1] for f in ("q_genome", "t_genome", "entries", "compared", "snvs", "A>C", "same", "m_equal", "n_columns", "n_ins", "ins_bases", "n_del",
                                      "del_bases", "long_indels", "unanchored")]
    assert got == want + [1, SNP, INS, DEL, MINUS, 1]
    for _, cls in structs:      # no implicit padding
        assert sum(C.sizeof(t) for _, t in cls._fields_) == C.sizeof(cls) == {"SwgSeqSet": 24, "SwgVariantRequest": 144}[cls.__name__]
    assert variants.VARIANT_DTYPE.itemsize == 32 and P.itemsize == 200 and _lib.VARIANT_SUMS == vm.SUMS and variants.FIELDS == vm.FIELDS
    assert [P.fields[s][1] for s in vm.SUBS] == list(range(32, 128, 8)) and vm.SUBS[:4] == ("A>C", "A>G", "A>T", "C>A") and vm.SUBS[-1] == "T>G"
    assert (variants.SNP, variants.INS, variants.DEL, variants.MINUS, variants.ANY) == (SNP, INS, DEL, MINUS, vm.ANY)


def test_symbols_are_exported_and_declared(lib):
    import sweepga_amd
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_variant_records", "swg_variant_records_device"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    assert lib.swg_abi_version() == 1
    for name in ("VARIANT_DTYPE", "VariantsResult", "variant_records", "variant_records_device"):
        assert hasattr(sweepga_amd, name)
    assert "swg_variants.hip" in sweepga_amd.build.SOURCES


def test_record_seams_refuse_without_a_device(lib):
    """A NULL context: there is no CPU path, and nothing the caller owns is touched."""
    from sweepga_amd import _lib
    from sweepga_amd.lift import cigar_set
    from sweepga_amd.variants import sequence_set
    cols, strand, genome, cig, seqs = small_table()
    keep = {k: np.ascontiguousarray(v, dtype=np.uint32) for k, v in cols.items()}
    rec = _lib.SwgRecords()
    rec.n = 6
    for k, a in keep.items():
        setattr(rec, k, a.ctypes.data)
    rec.strand, rec.n_seq = strand.ctypes.data, 5
    g = np.array(genome, dtype=np.uint32)
    record, offset, text = cigar_set(sorted(cig), [cig[i] for i in sorted(cig)])
    cs = _lib.SwgCigarSet()
    cs.record, cs.offset, cs.text, cs.k = record.ctypes.data, offset.ctypes.data, text.ctypes.data, 6
    s_off, s_bases = sequence_set(seqs)
    assert s_off.tolist() == [0, 10, 15, 15, 20, 26] and s_bases.tobytes() == b"".join(seqs)
    ss = _lib.SwgSeqSet()
    ss.offset, ss.bases, ss.n_seq = s_off.ctypes.data, s_bases.ctypes.data, 5
    poison = np.full(32 * 4, 0xab, dtype=np.uint8)
    for fn in (lib.swg_variant_records, lib.swg_variant_records_device):
        req = _lib.SwgVariantRequest()
        req.t_genome = req.q_genome = vm.ANY
        req.variant_capacity, req.variants, req.pool_capacity, req.pool, req.n_variants, req.usable = 4, poison.ctypes.data, 64, poison.ctypes.data + 64, 12345, 77
        assert fn(None, C.byref(rec), g.ctypes.data, 3, None, C.byref(cs), C.byref(ss), C.byref(req)) == -1
        assert (poison == 0xab).all() and req.n_variants == 12345 and req.usable == 77


def walk_lines(rng, n):
    """n random entries -> (the input lines of variants_walk_check, what the model says of each)"""
    lines, want = [], []
    for k in range(n):
        cols, strand, _, cig, seqs = vm.random_case(rng, 1, n_targets=1, n_queries=1, iupac=0.05 if k % 3 == 0 else 0.0, flank=3)
        rec = tuple(int(cols[c][0]) for c in ("q_start", "q_end", "t_start", "t_end"))
        text = cig[0] if k % 5 else cig[0] + "%dD" % (len(seqs[0]) - rec[3])      # some deletions reach the target's last base ...
        t_end = rec[3] if k % 5 else len(seqs[0])
        if k % 10 == 0:                                                          # ... and some entries delete a whole target
            text, rec, t_end = "%dD" % len(seqs[0]), (rec[0], rec[0], 0, 0), len(seqs[0])
        max_indel = (0, 2, 3)[k % 3]
        ops = vm.em.parse(text)[1]
        lines.append("%d %d %d %d %d %d %s %s %d %s" % (strand[0], rec[0], rec[1], rec[2], max_indel, k % 4, seqs[0].decode(), seqs[1].decode(), len(ops),
                                                       " ".join("%d %s" % op for op in ops)))
        got, sums = vm.entry_variants(text, bool(strand[0]), rec[0], rec[1], rec[2], t_end, seqs[0], seqs[1], max_indel=max_indel, check=max_indel == 0)
        out = ["%d %d %d %d %d %s %s" % (kf, pos, len(ref), len(alt), q_pos, ref, alt) for _, kf, pos, ref, alt, q_pos in got]
        out.append("= " + " ".join(str(sums[s]) for s in vm.SUBS + ("same", "m_equal", "n_columns", "long_indels", "unanchored")))
        want.append(out)
    return lines, want


def test_the_rules_of_the_walk_header_on_a_cpu(tmp_path):
    """tests/native/variants_walk_check.cpp: csrc/swg_variants_walk.h as a host compiler takes it, under the sanitizers, against the
    model: every variant's words and allele bytes, the 15 column counters and the fate of every indel of 400 random entries."""
    exe = str(tmp_path / "variants_walk_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "variants_walk_check.cpp")])
    lines, want = walk_lines(np.random.default_rng(4), 400)
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got = [block.strip().split("\n") for block in r.stdout.split("--\n") if block.strip()]
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, (k, lines[k], a, b)
    assert sum(len(b) for b in want) > 1500 and sum(b[-1].endswith(" 1") for b in want) >= 40      # (unanchored entries among them)


# ---- the PAF seam without a device ---------------------------------------------------------------------------------------------------------
def test_qname_escaping_and_the_model_texts_by_hand():
    assert vm.escape("a;b=c,d%e f\tg\x01h#1|x") == "a%3Bb%3Dc%2Cd%25e%20f%09g%01h#1|x"
    assert vm.vcf_line("chr1", "q 1", 9, "A", "AT", 4, True, 7) == "chr1\t10\t.\tA\tAT\t.\t.\tQNAME=q%201;QSTART=4;QSTRAND=-;REC=7\n"
    assert vm.vcf_line("chr1", "q", 0, "AC", "A", 0, False, 0, True).endswith(";QSTRAND=+;REC=0\tGT\t1\n")
    head = vm.vcf_header([("t1", 10)], "g1#1#")
    assert head.startswith("##fileformat=VCFv4.2\n##source=sweepga-gpu\n##contig=<ID=t1,length=10>\n##INFO=<ID=QNAME,") and "Date" not in head
    assert head.endswith('##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tg1#1#\n')
    # a hand-made PAF: the query differs from the target by one base, one insertion and one deletion; the VCF is sorted by position
    t, q = b"ACGTACGTAC", b"ACCTAGCGAC"          # ACGTA-CGTAC against ACCTAGCG-AC: 2=1X2=1I2=1D2=
    paf = "q#1#a\t10\t0\t10\t+\tt#1#b\t10\t0\t10\t8\t11\t60\tcg:Z:2=1X2=1I2=1D2=\n"
    vcf, summary, counts = vm.paf_texts(paf, None, [("t#1#b", t), ("q#1#a", q), ("t#1#b", b"TTTTTTTTTT")], 0, query="q#1")
    assert vcf.split("\n")[-4:] == ["t#1#b\t3\t.\tG\tC\t.\t.\tQNAME=q#1#a;QSTART=2;QSTRAND=+;REC=0\tGT\t1",
                                    "t#1#b\t5\t.\tA\tAG\t.\t.\tQNAME=q#1#a;QSTART=5;QSTRAND=+;REC=0\tGT\t1",
                                    "t#1#b\t7\t.\tGT\tG\t.\t.\tQNAME=q#1#a;QSTART=8;QSTRAND=+;REC=0\tGT\t1", ""]
    assert summary == vm.SUMMARY_HEADER + "q#1#\tt#1#\t1\t1\t1" + "\t0" * 7 + "\t1" + "\t0" * 4 + "\t0\t0\t0\t1\t1\t1\t1\t0\t0\t0\t1\n"      # G>C: a transversion
    assert counts["variants"] == 3 and counts["usable"] == 1 and vm.paf_texts(paf, None, [("t#1#b", t)], 0)[2]["no_sequence"] == 1
    assert vm.paf_texts(paf, None, [("t#1#b", t + b"A"), ("q#1#a", q)], 0)[2] == dict(counts, usable=0, variants=0, snvs=0, n_ins=0, n_del=0, no_sequence=1,
                                                                                   length_mismatch=1)


def paf_vcf(lib, paf, status, fasta, ctx=None, want=(True, True), **kw):
    """swg_paf_vcf_text -> (rc, VCF or None, summary or None, counts)"""
    from sweepga_amd import _lib
    opts = _lib.SwgVcfOptions()
    for k, v in kw.items():
        setattr(opts, k, v)
    counts = _lib.SwgVcfCounts()
    p, n = (C.c_void_p(), C.c_void_p()), (C.c_uint64(), C.c_uint64())
    rc = lib.swg_paf_vcf_text(ctx, paf.handle, status.ctypes.data if status is not None else None, fasta, C.byref(opts) if kw is not None else None,
                              C.byref(counts), C.byref(p[0]) if want[0] else None, C.byref(n[0]) if want[0] else None, C.byref(p[1]) if want[1] else None,
                              C.byref(n[1]) if want[1] else None)
    if rc != 0:
        assert not p[0].value and not p[1].value
        return rc, None, None, None
    texts = []
    for q, m in zip(p, n):
        texts.append(C.string_at(q.value, m.value).decode() if q.value else None)
        lib.swg_free(q)
    return rc, texts[0], texts[1], {k: int(getattr(counts, k)) for k in vm.VCF_COUNTS}


def test_paf_seam_without_a_device(lib, tmp_path):
    """A PAF without records of the set gives empty outputs and needs no device; the refusals come before a context is looked at and
    before a file is opened."""
    from sweepga_amd import PafFile, SwgError, Variants
    from sweepga_amd.variants import _FastaHandle
    from tests.test_lift_cpu import REBASED
    from tests.test_ucsc_chain_cpu import mixed_paf
    fa = tmp_path / "s.fa"
    fa.write_text(">g1#1#q\nACGT\n>g2#1#t\nAC\nGT\n")
    zero = dict.fromkeys(vm.VCF_COUNTS, 0)
    with _FastaHandle(lib, [str(fa)]) as fasta:
        for text in ("", "# nothing\nfew\tfields\n"):
            with PafFile(text=text) as paf:
                for st in (None, np.zeros(1, dtype=np.uint8)):
                    assert paf_vcf(lib, paf, st, fasta, set=0) == (0, "", "", zero)
                    assert paf_vcf(lib, paf, st, fasta, set=0, ref_genome=b"no such genome", batch_bytes=5, want=(True, False)) == (0, "", None, zero)
                got = Variants.from_paf(paf, None, fasta=[str(fa)], set="all")
                assert (got.text, got.summary_text, got.counts, got.variants, got.pairs) == ("", "", zero, [], [])
        text, kept = mixed_paf()
        with PafFile(text=text) as paf:
            none, st = np.zeros(paf.n, dtype=np.uint8), kept.astype(np.uint8)
            assert paf_vcf(lib, paf, none, fasta, set=1) == (0, "", "", zero)      # a set that is never in status: no device
            assert paf_vcf(lib, paf, st, fasta, set=1)[0] == -1 and b"swg_paf_vcf_text: NULL context" in lib.swg_alnstats_last_error()
            for kw, word in ((dict(set=2), b"set"), (dict(set=1, reserved=1), b"reserved"), (dict(set=1, ref_genome=b"g9#1"), b"unknown genome 'g9#1'"),
                             (dict(set=1, query_genome=b"g1"), b"unknown genome 'g1'")):
                assert paf_vcf(lib, paf, st, fasta, **kw)[0] == -1 and word in lib.swg_alnstats_last_error(), kw
            assert paf_vcf(lib, paf, None, fasta, set=1)[0] == -1 and b"status" in lib.swg_alnstats_last_error()
            assert paf_vcf(lib, paf, st, None, set=1)[0] == -1 and b"NULL sequences" in lib.swg_alnstats_last_error()
            assert paf_vcf(lib, paf, st, fasta, set=1, want=(False, False))[0] == -1 and b"neither text" in lib.swg_alnstats_last_error()
            out = tmp_path / "no.vcf"
            opts = None
            assert lib.swg_paf_vcf_write(None, paf.handle, st.ctypes.data, fasta, opts, str(out).encode(), None, None) == -1 and not out.exists()
            with pytest.raises(SwgError):
                Variants.write_paf(paf, st, out, fasta=[str(fa)], set=2)
            with pytest.raises(SwgError):
                Variants.from_paf(paf, st, fasta=[str(fa)], ref="nobody")
            assert not out.exists()
            with pytest.raises(SwgError):
                Variants.from_paf(paf, st, fasta=[str(tmp_path / "missing.fa")])
        with PafFile(text=REBASED) as paf:
            with pytest.raises(SwgError) as e:
                Variants.from_paf(paf, np.ones(1, dtype=np.uint8), fasta=[str(fa)])
            assert e.value.code == -6 and "2^32" in str(e.value)


def test_command_line_usage_errors(lib, tmp_path):
    from sweepga_amd import build
    from tests.test_ucsc_chain_cpu import mixed_paf
    paf, fa = tmp_path / "in.paf", tmp_path / "s.fa"
    paf.write_text(mixed_paf()[0])
    fa.write_text(">g1#1#q\nACGT\n")
    out, vcf, summ = tmp_path / "out.paf", tmp_path / "v.vcf", tmp_path / "s.tsv"
    run = lambda *a: subprocess.run([build.CLI, str(paf), "--output-file", str(out), *a], capture_output=True, text=True)      # noqa: E731
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(w in r.stdout for w in ("--vcf FILE", "--vcf-summary FILE", "--vcf-fasta FASTA", "--vcf-ref GENOME", "--vcf-query GENOME",
                                                              "--vcf-set kept|all", "--vcf-max-indel N", "--vcf-batch BYTES", "default 10000"))
    need, fasta = "need --vcf or --vcf-summary", ["--vcf-fasta", str(fa)]
    cases = [(["--vcf", str(vcf)], "need --vcf-fasta"), (["--vcf-summary", str(summ)], "need --vcf-fasta"),
             (fasta, need), (["--vcf-ref", "g1#1"], need), (["--vcf-query", "g1#1"], need), (["--vcf-set", "all"], need), (["--vcf-max-indel", "5"], need),
             (["--vcf-batch", "4k"], need),
             (["--vcf", str(vcf), *fasta, "--vcf-set", "lost"], "--vcf-set: kept or all"),
             (["--vcf", str(vcf), *fasta, "--vcf-max-indel", "few"], "--vcf-max-indel"),
             (["--vcf", str(vcf), *fasta, "--vcf-max-indel", "4294967296"], "--vcf-max-indel"),
             (["--vcf", str(vcf), *fasta, "--vcf-batch", "0"], "--vcf-batch"),
             (["--vcf-summary", str(summ), *fasta, "--vcf-batch", "many"], "--vcf-batch"),
             (["--vcf", str(vcf), "--vcf-fasta", str(tmp_path / "missing.fa")], "--vcf-fasta"),
             (["--vcf", str(vcf), "--vcf-fasta", "-"], "--vcf-fasta needs a file"),
             (["--vcf", str(vcf), *fasta, "--vcf-ref", ""], "empty value for --vcf-ref"),
             (["--vcf", str(vcf), *fasta, "--vcf-ref", "g9#1", "--diffs", str(summ)], "--vcf-ref: unknown genome 'g9#1'"),
             (["--vcf-summary", str(summ), *fasta, "--vcf-ref", "g2#1", "--vcf-query", "g1"], "--vcf-query: unknown genome 'g1'"),
             (["--vcf", "-", *fasta], "not a standard error report"), (["--vcf-summary", "-", *fasta], "not a standard error report"),
             (["--vcf", "", *fasta], "empty value for --vcf"), (["--vcf-summary", "", *fasta], "empty value for --vcf-summary")]
    for extra, word in cases:
        r = run(*extra)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)
        assert r.stdout == "" and not out.exists() and not vcf.exists() and not summ.exists(), extra


def test_text_helpers_under_the_host_sanitizers(tmp_path):
    """tests/native/variants_text_check.cpp: a stand-alone program over csrc/host/variants_text.cpp, built with the address and
    undefined-behaviour sanitizers; its answers must be the model's byte for byte."""
    exe = str(tmp_path / "variants_text_check")
    host = os.path.join(ROOT, "sweepga_amd", "csrc", "host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "variants_text_check.cpp"), os.path.join(host, "variants_text.cpp"),
                           os.path.join(host, "ucsc_text.cpp"), os.path.join(host, "cigar_text.cpp"), "-lpthread"])
    r = subprocess.run([exe], capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]
    got = r.stdout.decode("latin-1").split("--\n")
    top = 2**32 - 1
    assert got[0] == vm.vcf_header([("chr1", top), ("g2#1#t", 9000)]) and got[1] == vm.vcf_header([], "g1#1#")
    big = "CC" + "A" * 99_999 + "T"      # 100,002 allele bytes
    lines = [vm.vcf_line("chr1", "q", top - 1, "A", "C", top, False, top), vm.vcf_line("", "", top - 1, "G", "T", top, True, top, True),
             vm.vcf_line("n" * 5000, "n" * 5000, 0, big[:1], big[1:], 0, False, 0), vm.vcf_line("t", "a;b=c,d%e f\tg\x01h", 0, big[:-1], big[-1:], 0, True, 0, True)]
    assert got[2] == "".join(lines)

    def pair(q, t, seeds):
        v = [sum(s * (f + 1) + (top if f == 7 else 0) for s in seeds) for f in range(24)]
        v[2] = sum(v[3:15])
        return (q, t) + tuple(v)
    merged = [pair(0, 0, [11]), pair(0, 1, [3]), pair(1, 0, [5, 13]), pair(2, 2, [7, 17])]
    assert got[3] == got[4] == vm.summary_text(["g0#1#", "g1#1#", "g2"], merged) and got[5] == ""
