"""Intervals without a GPU: the model of tests/intervals_model.py against answers derived by hand, its two formulations against
each other, and the host side of the feature -- header, ctypes mirrors, exported symbols, the refusals that need no device, a
record-free PAF, the command line's flags."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import intervals_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")


def hand_case():
    """Sequences a1 = 0, a2 = 1 (genome A = 0), b1 = 2, b2 = 4 (genome B = 1), c1 = 3 (genome C = 2).
    -> (columns, seq_genome, status, expected {(set, axis): [(seq, other_genome, start, end)]})."""
    a1, a2, b1, c1, b2 = 0, 1, 2, 3, 4
    seq_genome = np.array([0, 0, 1, 2, 1], dtype=np.uint32)
    rows = [
        # (q, t, qs, qe, ts, te, status); on b1 the target side mirrors the query side 10000 further up
        (a1, b1, 0, 100, 10_000, 10_100, 1),      # 0  a K that starts at its A's start
        (a1, b1, 100, 150, 10_100, 10_150, 0),    # 1  touches record 0: ALL [0,150); dropped, so [100,150) is lost (trailing, up to A.end)
        (a1, b1, 20, 50, 10_020, 10_050, 2),      # 2  nested in record 0
        (a1, b1, 300, 300, 10_300, 10_300, 1),    # 3  zero length exactly where, after a gap, the next interval starts (ALL)
        (a1, b1, 300, 400, 10_300, 10_400, 0),    # 4  an A with no K: lost whole
        (a1, b1, 420, 450, 10_420, 10_450, 0),    # 5  a second A with no K between the K of record 0 and that of record 8
        (a1, b1, 500, 600, 10_500, 10_600, 0),    # 6  an A whose K (record 8) ends at A.end: only a leading piece is lost
        (a1, b1, 550, 550, 10_550, 10_550, 3),    # 7  zero length at the start of the KEPT interval [550,600), inside an ALL interval
        (a1, b1, 550, 600, 10_550, 10_600, 1),    # 8
        (a2, c1, 77, 77, 5, 5, 1),                # 9  a zero-length record alone in its unit (query axis): no row
        (a1, a2, 0, 1_000, 0, 1_000, 1),          # 10 intra-genome: ignored
        (a1, c1, 50, 200, 0, 150, 1),             # 11 a1 against another genome: never merged with a1 against B
        (a1, b2, 1_000, 2_000, 0, 1_000, 0),      # 12 one A ...
        (a1, b2, 1_200, 1_300, 200, 300, 1),      # 13 ... with two K inside: leading piece, gap between them, trailing piece
        (a1, b2, 1_500, 1_600, 500, 600, 1),      # 14
        (b1, a1, 0, 10, 0, 10, 1),                # 15 the pair the other way round
    ]
    arr = np.array(rows, dtype=np.int64)
    cols = {k: arr[:, i].astype(np.uint32) for i, k in enumerate(COLS)}
    status = arr[:, 6].astype(np.uint8)
    A, B, C_ = 0, 1, 2
    want = {
        ("all", "q"): [(a1, B, 0, 150), (a1, B, 300, 400), (a1, B, 420, 450), (a1, B, 500, 600), (a1, B, 1_000, 2_000), (a1, C_, 50, 200), (b1, A, 0, 10)],
        ("kept", "q"): [(a1, B, 0, 100), (a1, B, 550, 600), (a1, B, 1_200, 1_300), (a1, B, 1_500, 1_600), (a1, C_, 50, 200), (b1, A, 0, 10)],
        ("lost", "q"): [(a1, B, 100, 150), (a1, B, 300, 400), (a1, B, 420, 450), (a1, B, 500, 550), (a1, B, 1_000, 1_200), (a1, B, 1_300, 1_500),
                        (a1, B, 1_600, 2_000)],
        ("all", "t"): [(a1, B, 0, 10), (b1, A, 10_000, 10_150), (b1, A, 10_300, 10_400), (b1, A, 10_420, 10_450), (b1, A, 10_500, 10_600),
                       (c1, A, 0, 150), (b2, A, 0, 1_000)],
        ("kept", "t"): [(a1, B, 0, 10), (b1, A, 10_000, 10_100), (b1, A, 10_550, 10_600), (c1, A, 0, 150), (b2, A, 200, 300), (b2, A, 500, 600)],
        ("lost", "t"): [(b1, A, 10_100, 10_150), (b1, A, 10_300, 10_400), (b1, A, 10_420, 10_450), (b1, A, 10_500, 10_550), (b2, A, 0, 200),
                        (b2, A, 300, 500), (b2, A, 600, 1_000)],
    }
    return cols, seq_genome, status, want


def random_case(rng, n, n_seq, per_genome, span=5_000, longest=400):
    q, t = rng.integers(0, n_seq, n), rng.integers(0, n_seq, n)
    seq_genome = (np.arange(n_seq) // per_genome).astype(np.uint32)
    qs, ts = rng.integers(0, span, n), rng.integers(0, span, n)
    qe = qs + rng.integers(0, longest, n) * (rng.random(n) < 0.9)     # a tenth of the records: zero length
    te = ts + rng.integers(0, longest, n) * (rng.random(n) < 0.9)
    cols = {k: v.astype(np.uint32) for k, v in zip(COLS, (q, t, qs, qe, ts, te))}
    return cols, seq_genome, rng.random(n) < 0.4


@pytest.mark.parametrize("vectorised", [False, True])
def test_model_against_hand_derived_answers(vectorised):
    cols, seq_genome, status, want = hand_case()
    got = im.intervals(*cols.values(), seq_genome, status != 0, vectorised=vectorised)
    assert {k: im.as_tuples(v) for k, v in got.items()} == want
    # no order dependence
    perm = np.random.default_rng(1).permutation(len(status))
    again = im.intervals(*[v[perm] for v in cols.values()], seq_genome, status[perm] != 0, vectorised=vectorised)
    assert {k: im.as_tuples(v) for k, v in again.items()} == want
    # no record kept: nothing covered, everything lost
    none = im.intervals(*cols.values(), seq_genome, None, vectorised=vectorised)
    for axis in im.AXES:
        assert im.as_tuples(none["all", axis]) == want["all", axis] == im.as_tuples(none["lost", axis]) and len(none["kept", axis]) == 0


def test_pieces_by_hand():
    assert im.merged([]) == [] and im.merged([(5, 5)]) == []
    assert im.merged([(0, 10), (10, 20)]) == [(0, 20)]                     # touching
    assert im.merged([(0, 10), (2, 3), (0, 10)]) == [(0, 10)]              # nested, identical
    assert im.merged([(11, 20), (0, 10)]) == [(0, 10), (11, 20)]
    assert im.merged([(0, 10), (12, 12), (12, 20)]) == [(0, 10), (12, 20)]   # zero length at the start of the next piece
    assert im.lost_by_depth([(0, 100)], []) == [(0, 100)]
    assert im.lost_by_depth([(0, 100)], [(0, 100)]) == []
    assert im.lost_by_depth([(0, 100), (100, 200)], [(50, 150)]) == [(0, 50), (150, 200)]
    assert im.lost_by_depth([(0, 10), (20, 30)], [(20, 30)]) == [(0, 10)]
    assert im.lost_by_depth([(0, 10), (10, 20)], [(10, 20)]) == [(0, 10)]


def test_the_two_formulations_agree_on_random_records():
    rng = np.random.default_rng(7)
    for n, n_seq, per_genome in ((1, 2, 1), (500, 6, 2), (3_000, 40, 4), (3_000, 9, 1)):
        cols, seq_genome, kept = random_case(rng, n, n_seq, per_genome)
        for k in (None, kept):
            a = im.intervals(*cols.values(), seq_genome, k, vectorised=False)
            b = im.intervals(*cols.values(), seq_genome, k, vectorised=True)
            assert sorted(a) == sorted(b) == sorted((s, x) for s in im.SETS for x in im.AXES)
            for key in a:
                assert im.same_rows(a[key], b[key]), key
            for axis in im.AXES:   # ALL = KEPT + LOST in bases; a list's intervals of one unit neither touch nor overlap
                total = {s: int((a[s, axis]["end"].astype(np.int64) - a[s, axis]["start"]).sum()) for s in im.SETS}
                assert total["all"] == total["kept"] + total["lost"]
                for s in im.SETS:
                    r = a[s, axis]
                    same = (r["seq"][1:] == r["seq"][:-1]) & (r["other_genome"][1:] == r["other_genome"][:-1])
                    assert (r["end"] > r["start"]).all() and (r["start"][1:][same] > r["end"][:-1][same]).all()


def test_renderer_against_text_written_out():
    cols, seq_genome, status, _ = hand_case()
    lists = im.intervals(*cols.values(), seq_genome, status != 0)
    names, genomes = ["A#1#a1", "A#1#a2", "B#1#b1", "C#1#c1", "B#1#b2"], ["A#1#", "B#1#", "C#1#"]
    assert im.render(lists, "kept", names, genomes).decode() == (
        "A#1#a1\t0\t100\tB#1#\tq\nA#1#a1\t550\t600\tB#1#\tq\nA#1#a1\t1200\t1300\tB#1#\tq\nA#1#a1\t1500\t1600\tB#1#\tq\nA#1#a1\t50\t200\tC#1#\tq\n"
        "B#1#b1\t0\t10\tA#1#\tq\nA#1#a1\t0\t10\tB#1#\tt\nB#1#b1\t10000\t10100\tA#1#\tt\nB#1#b1\t10550\t10600\tA#1#\tt\nC#1#c1\t0\t150\tA#1#\tt\n"
        "B#1#b2\t200\t300\tA#1#\tt\nB#1#b2\t500\t600\tA#1#\tt\n")


# ---- the host side of the library ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib
    from sweepga_amd.intervals import INTERVAL_DTYPE
    structs = (("swg_interval", _lib.SwgInterval), ("swg_interval_list", _lib.SwgIntervalList), ("swg_interval_request", _lib.SwgIntervalRequest))
    prints = ['printf("%%zu\\n", sizeof(%s));' % name for name, _ in structs]
    prints += ['printf("%%zu\\n", offsetof(%s, %s));' % (name, f) for name, cls in structs for f, _ in cls._fields_]
    prints += ['printf("%zu\\n", offsetof(swg_interval_request, list[2][1]));', 'printf("%d %d %d\\n", SWG_IV_ALL, SWG_IV_KEPT, SWG_IV_LOST);']
    prints += ['printf("%%zu\\n", sizeof(%s));' % s for s in ("swg_records", "swg_breadth_pair", "swg_breadth_counts")]
    prints.append('printf("%d\\n", SWG_ABI_VERSION);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(cls) for _, cls in structs] + [getattr(cls, f).offset for _, cls in structs for f, _ in cls._fields_]
    want += [_lib.SwgIntervalRequest.list.offset + 5 * C.sizeof(_lib.SwgIntervalList), 0, 1, 2]
    want += [128, 48, 24, 1]      # the structures that existed before keep their sizes
    assert got == want
    assert got[:3] == [16, 32, 200] and INTERVAL_DTYPE.itemsize == 16
    assert [INTERVAL_DTYPE.fields[f][1] for f, _ in _lib.SwgInterval._fields_] == got[3:7] == [0, 4, 8, 12]


def test_symbols_are_exported_and_declared(lib):
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_intervals_records", "swg_intervals_records_device", "swg_paf_intervals", "swg_paf_interval_texts"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    assert lib.swg_abi_version() == 1


def test_refusals_that_need_no_device(lib):
    from sweepga_amd import PafFile, _lib
    cols, seq_genome, status, _ = hand_case()
    rec = _lib.SwgRecords()
    rec.n = len(status)
    for k, a in cols.items():
        setattr(rec, k, a.ctypes.data)
    rec.n_seq = len(seq_genome)
    for fn in (lib.swg_intervals_records, lib.swg_intervals_records_device):
        for want, reserved, st in ((0x3f, 0, status), (0x3f, 1, status), (0, 0, status), (1 << 6, 0, status), (0x4, 0, None), (0x10, 0, None)):
            req = _lib.SwgIntervalRequest()
            req.want, req.reserved = want, reserved
            for s in range(3):
                for a in range(2):
                    req.list[s][a].n = 12345
            # (a NULL context is refused before any pointer is looked at; the other faults are refusals with any context)
            assert fn(None, C.byref(rec), seq_genome.ctypes.data, 3, st.ctypes.data if st is not None else None, C.byref(req)) == -1
            assert all(int(req.list[s][a].n) == 12345 for s in range(3) for a in range(2))
    with PafFile(text="a#1#x\t100\t0\t50\t+\tb#1#y\t200\t10\t60\t50\t50\t60\n") as paf:
        one = np.ones(1, dtype=np.uint8)
        p, n = C.c_void_p(), C.c_uint64()
        assert lib.swg_paf_intervals(None, paf.handle, one.ctypes.data, 2, C.byref(p), C.byref(n)) == -1 and not p.value
        assert b"NULL context" in lib.swg_alnstats_last_error()
        for bad in (-1, 3, 7):
            assert lib.swg_paf_intervals(None, paf.handle, one.ctypes.data, bad, C.byref(p), C.byref(n)) == -1 and not p.value
            assert b"a set outside" in lib.swg_alnstats_last_error()
        for needs_status in (1, 2):
            assert lib.swg_paf_intervals(None, paf.handle, None, needs_status, C.byref(p), C.byref(n)) == -1 and not p.value
            assert b"status" in lib.swg_alnstats_last_error()
        texts, lens = (C.c_void_p * 3)(), (C.c_uint64 * 3)()
        for bad in (0, 8):
            assert lib.swg_paf_interval_texts(None, paf.handle, one.ctypes.data, bad, texts, lens) == -1
        assert lib.swg_paf_intervals(None, paf.handle, one.ctypes.data, 0, None, C.byref(n)) == -1


def test_a_paf_without_records_gives_empty_text_without_a_device(lib):
    from sweepga_amd import Intervals, PafFile
    for text in ("", "# nothing\nfew\tfields\n"):
        with PafFile(text=text) as paf:
            assert paf.n == 0
            p, n = C.c_void_p(), C.c_uint64(99)
            for s, st in ((0, None), (1, np.zeros(1, dtype=np.uint8)), (2, np.zeros(1, dtype=np.uint8))):
                assert lib.swg_paf_intervals(None, paf.handle, st.ctypes.data if st is not None else None, s, C.byref(p), C.byref(n)) == 0
                assert p.value and n.value == 0
                lib.swg_free(p)
            assert Intervals.from_paf(None, paf).text == {"all": b""}
            assert Intervals.from_paf(None, paf, np.zeros(0, dtype=np.uint8)).text == {"all": b"", "kept": b"", "lost": b""}


def test_command_line_lists_the_flags_and_wants_values(lib):
    from sweepga_amd import build
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--lost FILE" in r.stdout and "--covered FILE" in r.stdout
    for flag in ("--lost", "--covered"):
        r = subprocess.run([build.CLI, "in.paf", flag + "="], capture_output=True, text=True)
        assert r.returncode == 2 and "empty value for " + flag in r.stderr
        r = subprocess.run([build.CLI, "in.paf", flag], capture_output=True, text=True)
        assert r.returncode == 2 and flag in r.stderr


def test_command_line_refuses_64_bit_columns_before_it_filters(lib, tmp_path):
    """A value >= 2^32 rebases the columns; --lost / --covered say so right after the parse -- exit 3 -- and nothing is begun."""
    from sweepga_amd import build
    ln = "\t".join(["a#1#x", str(2**33), str(2**32), str(2**32 + 50), "+", "b#1#y", "900", "10", "60", "50", "50", "60"]) + "\n"
    inp, out, rep = tmp_path / "in.paf", tmp_path / "out.paf", tmp_path / "lost.bed"
    inp.write_text(ln)
    for flag in ("--lost", "--covered"):
        for extra in ([], ["--no-filter"]):
            r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), flag, str(rep), *extra], capture_output=True, text=True)
            assert r.returncode == 3 and flag in r.stderr and "2^32" in r.stderr, r.stderr
            assert r.stdout == "" and not out.exists() and not rep.exists()
