"""Breadth without a GPU: the model of tests/breadth_model.py against answers derived by hand, its two formulations against each
other, the report renderer against a report written out here, and the host side of the feature -- header, ctypes mirrors,
exported symbols, the NULL-context refusals, a record-free PAF, the command line's flag."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import breadth_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hand_case():
    """Sequences a1, a2 (genome A = 0), b1, b2 (genome B = 1), c1 (genome C = 2).  -> (columns, seq_genome, status, expected ALL,
    expected KEPT); expected rows are (q_genome, t_genome, q_bases, t_bases, q_union, t_union, first_record)."""
    a1, a2, b1, c1, b2 = 0, 1, 2, 3, 4
    seq_genome = np.array([0, 0, 1, 2, 1], dtype=np.uint32)
    rows = [
        # (q, t, qs, qe, ts, te, status)
        (a1, b1, 0, 100, 1000, 1100, 1),    # 0
        (a1, b1, 10, 50, 1000, 1040, 0),    # 1  nested on both sides; dropped
        (a1, b1, 0, 100, 2000, 2100, 2),    # 2  identical on the query, apart on the target
        (a1, b1, 100, 150, 1100, 1150, 1),  # 3  touches record 0 on both sides
        (a1, b1, 120, 120, 5000, 5000, 1),  # 4  zero length
        (a1, c1, 50, 300, 0, 250, 3),       # 5  a1 against another genome: never merged with a1 against B
        (a2, b1, 0, 30, 1090, 1120, 0),     # 6  a second sequence of A; on b1 it straddles records 0 and 3; dropped
        (a1, a2, 0, 1000, 0, 1000, 1),      # 7  intra-genome: ignored
        (a1, a1, 0, 1000, 0, 1000, 1),      # 8  self: ignored
        (b1, a1, 0, 10, 0, 10, 1),          # 9  the pair the other way round is another pair
        (a1, b2, 500, 600, 0, 100, 1),      # 10 pair (A, B) again, a second target sequence
        (c1, a1, 0, 10_000, 0, 10_000, 0),  # 11 one long interval ... dropped, so KEPT sees what it hid
    ]
    rows += [(c1, a1, 100 * k + 100, 100 * k + 150, 20_000 + 10 * k, 20_000 + 10 * k + 5, 1) for k in range(50)]  # 12..61 inside it
    rows.append((c1, a1, 9_990, 10_010, 9_995, 10_005, 1))  # 62 pokes out of it on both sides
    arr = np.array(rows, dtype=np.int64)
    cols = {k: arr[:, i].astype(np.uint32) for i, k in enumerate(("q_id", "t_id", "q_start", "q_end", "t_start", "t_end"))}
    status = arr[:, 6].astype(np.uint8)
    # (A, B): records 0 1 2 3 4 6 10.  query: a1 [0,150) + [500,600) = 250, a2 [0,30) = 30.  target: b1 [1000,1150) + [2000,2100) = 250,
    # b2 [0,100) = 100.  (C, A): query [0,10010); target [0,10005) + 50 pieces of 5.
    want_all = [(0, 1, 420, 420, 280, 350, 0), (0, 2, 250, 250, 250, 250, 5), (1, 0, 10, 10, 10, 10, 9),
                (2, 0, 10_000 + 2_500 + 20, 10_000 + 250 + 10, 10_010, 10_005 + 250, 11)]
    # without 1, 6, 11.  (A, B): query a1 alone, 250; target b1 [1000,1150) + [2000,2100), b2 [0,100).  (C, A): the 50 short ones and
    # record 62 are all apart: union = bases
    want_kept = [(0, 1, 350, 350, 250, 350, 0), (0, 2, 250, 250, 250, 250, 5), (1, 0, 10, 10, 10, 10, 9), (2, 0, 2_520, 260, 2_520, 260, 12)]
    return cols, seq_genome, status, want_all, want_kept


def as_rows(pairs):
    return [tuple(int(p[f]) for f in bm.PAIR_FIELDS) for p in pairs]


@pytest.mark.parametrize("vectorised", [False, True])
def test_model_against_hand_derived_answers(vectorised):
    cols, seq_genome, status, want_all, want_kept = hand_case()
    assert as_rows(bm.breadth(*cols.values(), seq_genome, vectorised=vectorised)) == want_all
    assert as_rows(bm.breadth(*cols.values(), seq_genome, status != 0, vectorised=vectorised)) == want_kept
    # no order dependence: the same values per pair from a shuffled copy
    perm = np.random.default_rng(1).permutation(len(status))
    shuffled = {k: v[perm] for k, v in cols.items()}
    assert bm.by_key(bm.breadth(*shuffled.values(), seq_genome, vectorised=vectorised)) == bm.by_key(bm.breadth(*cols.values(), seq_genome))


def test_union_length_by_hand():
    assert bm.union_length([]) == 0
    assert bm.union_length([(5, 5)]) == 0
    assert bm.union_length([(0, 10), (10, 20)]) == 20            # touching
    assert bm.union_length([(0, 10), (2, 3), (0, 10)]) == 10     # nested, identical
    assert bm.union_length([(0, 10), (11, 20)]) == 19
    assert bm.union_length([(7, 9), (0, 100)] + [(k, k + 2) for k in range(0, 98, 3)]) == 100   # one long over many short
    assert bm.union_length([(k, k + 2) for k in range(0, 1000)]) == 1001                         # a chain of pairwise overlaps


def test_the_two_formulations_agree_on_random_records():
    rng = np.random.default_rng(7)
    for n, n_seq, per_genome in ((1, 2, 1), (500, 6, 2), (3_000, 40, 4), (3_000, 9, 1)):
        q = rng.integers(0, n_seq, n)
        t = rng.integers(0, n_seq, n)
        seq_genome = (np.arange(n_seq) // per_genome).astype(np.uint32)
        qs, ts = rng.integers(0, 5_000, n), rng.integers(0, 5_000, n)
        qe, te = qs + rng.integers(0, 400, n), ts + rng.integers(0, 400, n)
        sel = rng.random(n) < 0.5
        for s in (None, sel):
            a = bm.breadth(q, t, qs, qe, ts, te, seq_genome, s, vectorised=False)
            b = bm.breadth(q, t, qs, qe, ts, te, seq_genome, s, vectorised=True)
            assert bm.same_pairs(a, b) and (a["q_union"] <= a["q_bases"]).all() and (a["t_union"] <= a["t_bases"]).all()


def test_renderer_against_a_report_written_out():
    cols, seq_genome, status, _, _ = hand_case()
    all_ = bm.breadth(*cols.values(), seq_genome)
    kept = bm.breadth(*cols.values(), seq_genome, status != 0)
    names = ["A#1#", "B#1#", "C#1#"]
    sizes_all, sizes_kept = [1_000, 700, 20_000], [1_000, 0, 20_000]
    text = bm.render([("all", all_, sizes_all), ("kept", kept, sizes_kept)], names, True).decode()
    want = ("set\tquery_genome\ttarget_genome\tq_bases\tq_union\tq_size\tq_breadth_pct\tq_depth\tt_bases\tt_union\tt_size\tt_breadth_pct\tt_depth\n"
            "all\tA#1#\tB#1#\t420\t280\t1000\t28.0000\t1.5000\t420\t350\t700\t50.0000\t1.2000\n"
            "all\tA#1#\tC#1#\t250\t250\t1000\t25.0000\t1.0000\t250\t250\t20000\t1.2500\t1.0000\n"
            "all\tB#1#\tA#1#\t10\t10\t700\t1.4286\t1.0000\t10\t10\t1000\t1.0000\t1.0000\n"
            "all\tC#1#\tA#1#\t12520\t10010\t20000\t50.0500\t1.2507\t10260\t10255\t1000\t1025.5000\t1.0005\n"
            "all\t*\t*\t13200\t10550\t22700\t46.4758\t1.2512\t10940\t10865\t22700\t47.8634\t1.0069\n"
            "kept\tA#1#\tB#1#\t350\t250\t1000\t25.0000\t1.4000\t350\t350\t0\t-\t1.0000\n"
            "kept\tA#1#\tC#1#\t250\t250\t1000\t25.0000\t1.0000\t250\t250\t20000\t1.2500\t1.0000\n"
            "kept\tB#1#\tA#1#\t10\t10\t0\t-\t1.0000\t10\t10\t1000\t1.0000\t1.0000\n"
            "kept\tC#1#\tA#1#\t2520\t2520\t20000\t12.6000\t1.0000\t260\t260\t1000\t26.0000\t1.0000\n"
            "kept\t*\t*\t3130\t3030\t22000\t13.7727\t1.0330\t870\t870\t22000\t3.9545\t1.0000\n")
    assert text == want
    short = bm.render([("all", all_, sizes_all), ("kept", kept, sizes_kept)], names, False).decode().split("\n")
    assert short == [want.split("\n")[0], want.split("\n")[5], want.split("\n")[10], ""]
    empty = bm.render([("all", all_[:0], sizes_all)], names, True).decode()
    assert empty == want.split("\n")[0] + "\nall\t*\t*\t0\t0\t0\t-\t-\t0\t0\t0\t-\t-\n"


# ---- the host side of the library ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib
    from sweepga_amd.alnstats import SwgAlnstatsSummary
    from sweepga_amd.aln import SwgAlnInput
    from sweepga_amd.breadth import BREADTH_PAIR_DTYPE
    pair_fields = [f for f, _ in _lib.SwgBreadthPair._fields_]
    count_fields = [f for f, _ in _lib.SwgBreadthCounts._fields_]
    src = tmp_path / "layout.c"
    prints = ['printf("%zu\\n", sizeof(swg_breadth_pair));', 'printf("%zu\\n", sizeof(swg_breadth_counts));']
    prints += ['printf("%%zu\\n", offsetof(swg_breadth_pair, %s));' % f for f in pair_fields]
    prints += ['printf("%%zu\\n", offsetof(swg_breadth_counts, %s));' % f for f in count_fields]
    prints += ['printf("%%zu\\n", sizeof(%s));' % s for s in ("swg_config", "swg_records", "swg_stats", "swg_ani_input", "swg_aln_input",
                                                              "swg_alnstats_pair_counts", "swg_alnstats_counts", "swg_alnstats_summary")]
    prints.append('printf("%d\\n", SWG_ABI_VERSION);')
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(_lib.SwgBreadthPair), C.sizeof(_lib.SwgBreadthCounts)]
    want += [getattr(_lib.SwgBreadthPair, f).offset for f in pair_fields] + [getattr(_lib.SwgBreadthCounts, f).offset for f in count_fields]
    # the structures that existed before keep their sizes (the numbers are those of the ABI before this feature)
    want += [128, 128, 72, 56, 72, 32, 88, 88, 1]
    assert got == want
    assert [C.sizeof(x) for x in (_lib.SwgConfig, _lib.SwgRecords, _lib.SwgStats, _lib.SwgAniInput, SwgAlnInput, _lib.SwgAlnstatsPairCounts,
                                  _lib.SwgAlnstatsCounts, SwgAlnstatsSummary)] == want[-9:-1]
    assert got[0] == 48 and got[1] == 24 and BREADTH_PAIR_DTYPE.itemsize == 48
    assert [BREADTH_PAIR_DTYPE.fields[f][1] for f in pair_fields] == got[2:2 + len(pair_fields)]


def test_symbols_are_exported_and_declared(lib):
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_breadth_records", "swg_breadth_records_device", "swg_paf_breadth"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    assert lib.swg_abi_version() == 1 and "#define SWG_ABI_VERSION 1\n" in hdr


def test_a_null_context_is_refused_on_all_three_seams(lib):
    from sweepga_amd import PafFile, _lib
    cols, seq_genome, status, _, _ = hand_case()
    rec = _lib.SwgRecords()
    rec.n = len(status)
    for k, a in cols.items():
        setattr(rec, k, a.ctypes.data)
    rec.n_seq = len(seq_genome)
    counts = _lib.SwgBreadthCounts()
    for fn in (lib.swg_breadth_records, lib.swg_breadth_records_device):   # (refused before any pointer is looked at)
        assert fn(None, C.byref(rec), seq_genome.ctypes.data, 3, status.ctypes.data, C.byref(counts), None) == -1
    with PafFile(text="a#1#x\t100\t0\t50\t+\tb#1#y\t200\t10\t60\t50\t50\t60\n") as paf:
        p, n = C.c_void_p(), C.c_uint64()
        assert lib.swg_paf_breadth(None, paf.handle, None, 1, C.byref(p), C.byref(n)) == -1 and not p.value
        assert b"NULL context" in lib.swg_alnstats_last_error()


def test_a_paf_without_records_is_reported_without_a_device(lib):
    from sweepga_amd import Breadth, PafFile
    header = "\t".join(bm.HEADER) + "\n"
    zero = "\t*\t*\t0\t0\t0\t-\t-\t0\t0\t0\t-\t-\n"
    for text in ("", "# nothing\nfew\tfields\n"):
        with PafFile(text=text) as paf:
            assert paf.n == 0
            b = Breadth.from_paf(None, paf)
            assert b.text.decode() == header + "all" + zero and len(b.all) == 0 and b.kept is None
            b = Breadth.from_paf(None, paf, np.zeros(0, dtype=np.uint8), detailed=False)
            assert b.text.decode() == header + "all" + zero + "kept" + zero and len(b.kept) == 0


def test_command_line_lists_the_flag_and_wants_a_value(lib):
    from sweepga_amd import build
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--breadth REPORT" in r.stdout
    r = subprocess.run([build.CLI, "in.paf", "--breadth"], capture_output=True, text=True)
    assert r.returncode == 2 and "--breadth" in r.stderr


def test_command_line_refuses_64_bit_columns_before_it_filters(lib, tmp_path):
    """A value >= 2^32 rebases the columns; --breadth says so right after the parse -- exit 3, the reason on standard error --
    and no output PAF and no report are begun.  Needs no device: the refusal comes ahead of the first use of one."""
    from sweepga_amd import build
    ln = "\t".join(["a#1#x", str(2**33), str(2**32), str(2**32 + 50), "+", "b#1#y", "900", "10", "60", "50", "50", "60"]) + "\n"
    inp, out, rep = tmp_path / "in.paf", tmp_path / "out.paf", tmp_path / "rep.tsv"
    inp.write_text(ln)
    for extra in ([], ["--no-filter"]):
        r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--breadth", str(rep), *extra], capture_output=True, text=True)
        assert r.returncode == 3 and "--breadth" in r.stderr and "2^32" in r.stderr, r.stderr
        assert r.stdout == "" and not out.exists() and not rep.exists()
