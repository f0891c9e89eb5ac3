"""The u64 -> u32 rebasing rule at its edges, host side: tests/wide_model.py (the rule in plain integers) against hand-worked
answers, then sweepga_amd/csrc/host/rebase.h -- alone, through tests/native/rebase_check, also under ASan + UBSan and with more
than one thread -- and the PAF and .1aln front ends against the model, on the named cases of tests/wide_cases.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import wide_cases as wc
from tests import wide_model as wm

W = 2**32
SWG_ERR_INVALID, SWG_ERR_RANGE = -1, -5   # include/sweepga_gpu.h
FIELD = {name: f for f, name in enumerate(wm.FIELDS)}


# ---- the model on cases worked out by hand -----------------------------------------------------------------------------------------
def test_model_by_hand():
    # two sequences, one record: each constant is the smaller of start and end
    r = wm.rebase([0], [1], [[10], [30], [7 * W + 5], [7 * W + 2], [3], [4]], 2, [0, 1], 2)
    assert r == ("ok", "seq", [10], [7 * W + 2], [[0], [20], [3], [0], [3], [4]])
    # sequence 0 appears as query (at 100) and as target (at 40): one constant, 40
    r = wm.rebase([0, 1], [1, 0], [[100, 5], [200, 9], [50, 40], [60, 90], [1, 1], [2, 2]], 2, [0, 0], 1)
    assert r == ("ok", "seq", [40, 5], [5, 40], [[60, 0], [160, 4], [45, 0], [55, 50], [1, 1], [2, 2]])
    # the boundary: 2^32 - 1 above the constant fits, 2^32 does not; the lowest field of the lowest record is named
    assert wm.rebase([0], [1], [[5], [5 + W - 1], [0], [1], [0], [0]], 2, [0, 0], 1)[4][1] == [0xFFFFFFFF]
    assert wm.rebase([0], [1], [[5], [5 + W], [0], [1], [0], [0]], 2, [0, 0], 1) == ("range", 0, 1)
    assert wm.rebase([0, 0], [1, 1], [[5, 5 + W], [6, 5 + W], [0, 0], [1, W + 1], [0, 0], [0, 0]], 2, [0, 0], 1) == ("range", 1, 0)
    assert wm.rebase([0, 0], [1, 1], [[5, 5], [6, 6], [0, 0], [W, W + 1], [0, 0], [0, 0]], 2, [0, 0], 1) == ("range", 0, 3)
    # matches and block length are not rebased
    assert wm.rebase([0], [1], [[W], [W + 1], [W], [W + 1], [W - 1], [W - 1]], 2, [0, 1], 2)[4][4:] == [[W - 1], [W - 1]]
    assert wm.rebase([0], [1], [[0], [1], [0], [1], [W], [W]], 2, [0, 1], 2) == ("range", 0, 4)
    assert wm.rebase([0], [1], [[0], [1], [0], [1], [7], [W]], 2, [0, 1], 2) == ("range", 0, 5)
    # a bad id wins over everything, wherever it sits
    assert wm.rebase([0, 2], [1, 1], [[0, 0], [W, 1], [0, 0], [1, 1], [W, 0], [0, 0]], 2, [0, 1], 2) == ("invalid", 1)
    assert wm.rebase([0, 0], [1, 2], [[0, 0], [W, 1], [0, 0], [1, 1], [W, 0], [0, 0]], 2, [0, 1], 2) == ("invalid", 1)
    # sequence 0 against genome 1 (sequence 1) near 0 and against genome 2 (sequence 2) near 2^33: one constant per genome
    cols = [[10, 2 * W + 7], [20, 2 * W + 9], [1, 2], [3, 4], [0, 0], [0, 0]]
    assert wm.rebase([0, 0], [1, 2], cols, 3, [0, 1, 2], 3) == ("ok", "axis", [10, 2 * W + 7], [1, 2], [[0, 0], [10, 2], [0, 0], [2, 2], [0, 0], [0, 0]])
    # ... both targets of ONE genome: nothing to split
    assert wm.rebase([0, 0], [1, 2], cols, 3, [0, 1, 1], 2) == ("range", 1, 0)
    # ... tables that do not fit: the per-sequence answer stands (4097 * 4096 cells)
    assert wm.rebase([0, 0], [1, 2], cols, 4097, [0, 1, 2] + [0] * 4094, 4096) == ("range", 1, 0)
    assert wm.rebase([0, 0], [1, 2], cols, 4096, [0, 1, 2] + [0] * 4093, 4096)[:2] == ("ok", "axis")
    # ... a genome entry out of range is met on that path only
    assert wm.rebase([0, 0], [1, 2], cols, 3, [0, 1, 3], 3) == ("invalid", 1)
    assert wm.rebase([0], [1], [[10], [20], [1], [3], [0], [0]], 3, [0, 1, 3], 3)[:2] == ("ok", "seq")
    # ... and the axis attempt checks all six fields again
    cols = [[10, 2 * W + 7], [20, 2 * W + 9], [1, 2], [3, 4], [0, W], [0, 0]]
    assert wm.rebase([0, 0], [1, 2], cols, 3, [0, 1, 2], 3) == ("range", 1, 4)
    # the target axis is keyed by the QUERY's genome: sequence 2 as target of genome 0 (near 5) and of genome 1 (near 2^34)
    cols = [[0, 0], [1, 1], [5, 4 * W], [6, 4 * W + 1], [0, 0], [0, 0]]
    assert wm.rebase([0, 1], [2, 2], cols, 3, [0, 1, 2], 3)[:4] == ("ok", "axis", [0, 0], [5, 4 * W])
    assert wm.rebase([], [], [[], [], [], [], [], []], 1, [0], 1) == ("ok", "seq", [], [], [[], [], [], [], [], []])


def test_cases_cover_what_they_claim():
    cases = wc.all_cases()
    by = {c.name: c for c in cases}
    assert wc.EW >= 128 and {c.n for c in wc.group("boundary")} >= {0, 1, 63, 64, 65, wc.EW - 1, wc.EW, wc.EW + 1, 3 * wc.EW + 7}
    for f in range(4):   # every coordinate field, refused at index 0, 63, 64 and n - 1
        for p in (0, 63, 64, 3 * wc.EW + 6):
            assert by[f"refuse_f{f}_n{3 * wc.EW + 7}_p{p}"].result == ("range", p, f)
    assert by["two_genomes_one_too_wide"].step2 == (40, 0) and by["two_genomes_one_too_wide"].result == ("range", 80, 0)
    names = [c.name for c in wc.group("precedence")]
    assert names.index("bad_id_behind_unfixable_wide_axis1") < names.index("bad_id_behind_fixable_wide_axis0")
    for c in cases:     # an id out of range is n_seq itself, never more
        assert max(c.q_id + c.t_id + [0]) <= c.n_seq


# ---- rebase.h alone ------------------------------------------------------------------------------------------------------------------
def _write_case(d, c):
    np.array(c.q_id, dtype=np.uint32).tofile(d / f"{c.name}.q_id")
    np.array(c.t_id, dtype=np.uint32).tofile(d / f"{c.name}.t_id")
    np.array(c.genome, dtype=np.uint32).tofile(d / f"{c.name}.genome")
    for f in range(6):
        np.array(c.cols[f], dtype=np.uint64).tofile(d / f"{c.name}.c{f}")
    return f"{c.name} n={c.n} n_seq={c.n_seq} n_genome={c.n_genome}\n"


def _run_check(binary, d, cases, threads):
    (d / "cases.txt").write_text("".join(_write_case(d, c) for c in cases))
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}
    r = subprocess.run([binary, str(d / "cases.txt"), str(d), str(threads)], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert [ln[1] for ln in lines] == [c.name for c in cases]
    return {ln[1]: dict(kv.split("=") for kv in ln[2:]) for ln in lines}


def _check_against_model(d, c, got):
    want = c.result
    assert got["answer"] == want[0], (c.name, got, want[:3])
    if want[0] == "invalid":
        assert int(got["record"]) == want[1], (c.name, got)
    elif want[0] == "range":
        assert (int(got["record"]), int(got["field"])) == want[1:], (c.name, got, want)
    else:
        assert got["kind"] == want[1], (c.name, got)
        for f in range(6):
            out = np.fromfile(d / f"{c.name}.o{f}", dtype=np.uint32)
            assert [int(x) for x in out] == want[4][f], (c.name, f)
        if want[1] == "seq":
            lo = np.fromfile(d / f"{c.name}.lo", dtype=np.uint64)
            assert [int(x) for x in lo] == wm.seq_constants(c.q_id, c.t_id, c.n_seq, want), c.name
        else:
            assert [int(x) for x in np.fromfile(d / f"{c.name}.off_q", dtype=np.uint64)] == want[2], c.name
            assert [int(x) for x in np.fromfile(d / f"{c.name}.off_t", dtype=np.uint64)] == want[3], c.name


@pytest.fixture(scope="module")
def rebase_check():
    from sweepga_amd import build
    return build.build_rebase_check()


@pytest.fixture(scope="module")
def rebase_check_sanitized(tmp_path_factory):
    from sweepga_amd import build
    out = tmp_path_factory.mktemp("san") / "rebase_check_san"
    return build.build_rebase_check(out=str(out), extra=["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                         "-fno-omit-frame-pointer"])


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_rebase_h_on_every_case(which, rebase_check, rebase_check_sanitized, tmp_path):
    cases = wc.all_cases()
    got = _run_check(rebase_check if which == "plain" else rebase_check_sanitized, tmp_path, cases, 1)
    for c in cases:
        _check_against_model(tmp_path, c, got[c.name])


BIG_N = 3 * 65536 + 5   # rebase.h gives a thread 65536 records at least: up to four threads here


def _big_cases():
    """An id out of range, and separately the first value that does not fit, in the last thread's range and on a thread border (with
    later ones in other threads' ranges: the per-thread findings are merged, and the lowest record must come out)."""
    n = BIG_N
    border2, border4 = n // 2, [n * t // 4 for t in range(1, 4)]
    assert border2 == border4[1]
    base = [("A#1#a", "B#1#b", 5 * W + 10 * k, 5 * W + 10 * k + 9, 3 * W + 7 * k, 3 * W + 7 * k + 5, 8, 9) for k in range(n)]
    out = []

    def bad_ids(name, first, later):
        c = wc.Case(name, "big", base, ("invalid", first), bad_id=(first, 0))
        for i in later:
            c.t_id[i] = c.n_seq
        c.result = wm.rebase(c.q_id, c.t_id, c.cols, c.n_seq, c.genome, c.n_genome)
        assert c.result == ("invalid", first)
        return c

    def wide(name, first, later):
        recs = list(base)
        for i in [first] + later:
            recs[i] = ("A#1#a", "B#1#b", 5 * W, 5 * W + 9, 3 * W + W + 1, 3 * W + W + 5, 8, 9)
        return wc.Case(name, "big", recs, ("range", first, 2))

    out.append(bad_ids("big_bad_id_last_range", n - 3, [n - 1]))
    out.append(bad_ids("big_bad_id_on_border", border2, [border2 + 1, border4[2], n - 1]))
    out.append(bad_ids("big_bad_id_before_border", border4[0] - 1, [border4[0], border2, border4[2] + 5]))
    out.append(wide("big_wide_last_range", n - 2, [n - 1]))
    out.append(wide("big_wide_on_border", border2, [border2 + 1, border4[2], n - 1]))
    out.append(wide("big_wide_before_border", border4[0] - 1, [border4[0], border2, border4[2] + 5]))
    return out


def test_rebase_h_names_the_lowest_record_at_every_thread_count(rebase_check, rebase_check_sanitized, tmp_path):
    cases = _big_cases()
    for threads, binary in ((1, rebase_check), (2, rebase_check), (8, rebase_check), (8, rebase_check_sanitized)):
        got = _run_check(binary, tmp_path, cases, threads)
        for c in cases:
            g = got[c.name]
            assert g["answer"] == c.result[0] and int(g["record"]) == c.result[1], (threads, c.name, g)
            if c.result[0] == "range":
                assert int(g["field"]) == c.result[2], (threads, c.name, g)
    # an accepted set of that size: the merged per-thread minima are the sequence's constants
    ok = wc.Case("big_ok", "big", [("A#1#a", "B#1#b", 5 * W + (BIG_N - k), 5 * W + (BIG_N - k) + 9, 3 * W + 7 * k, 3 * W + 7 * k + 5, 8, 9)
                                   for k in range(BIG_N)], ("ok", "seq"))
    got = _run_check(rebase_check, tmp_path, [ok], 8)
    _check_against_model(tmp_path, ok, got["big_ok"])


# ---- the front ends ------------------------------------------------------------------------------------------------------------------
TEXT_CASES = [c for c in wc.all_cases() if c.text]


def _paf_text(c):
    return "".join(f"{c.qname[i]}\t1000000\t{c.cols[0][i]}\t{c.cols[1][i]}\t+\t{c.tname[i]}\t1000000\t{c.cols[2][i]}\t{c.cols[3][i]}\t"
                   f"{c.cols[4][i]}\t{c.cols[5][i]}\t60\n" for i in range(c.n))


def _check_front_end(c, want, names, q_id, t_id, col, seq_offsets, record_offsets, u64cols):
    """An opened handle against the model's ok answer."""
    n = c.n
    assert names == c.names and list(q_id) == c.q_id and list(t_id) == c.t_id, c.name
    for f, k in enumerate(("q_start", "q_end", "t_start", "t_end", "matches", "block_len")):
        assert [int(x) for x in col(k)] == want[4][f], (c.name, k)
    if want[1] == "seq":
        assert record_offsets(0) is None and record_offsets(1) is None, c.name
        if seq_offsets is None:   # nothing reached 2^32: the columns are the input's own values
            assert all(max(colv, default=0) < W for colv in u64cols), c.name
            off_q, off_t = [0] * n, [0] * n
        else:
            assert [int(x) for x in seq_offsets] == wm.seq_constants(c.q_id, c.t_id, c.n_seq, want), c.name
            off_q, off_t = want[2], want[3]
    else:
        assert seq_offsets is None, c.name
        off_q, off_t = [int(x) for x in record_offsets(0)], [int(x) for x in record_offsets(1)]
        assert off_q == want[2] and off_t == want[3], c.name
    # the columns plus the offsets give the u64 input back
    for f, k in enumerate(("q_start", "q_end", "t_start", "t_end")):
        off = off_q if f < 2 else off_t
        assert [int(v) + off[i] for i, v in enumerate(col(k))] == list(u64cols[f]), (c.name, k)


def _segment_base(c, i, f):
    """The sequence that field f of record i lies on, and the first mapped base of its stretch against the genome of record i's other
    side -- what a refusal by the per-genome attempt prints (every refusing text case fits the tables, so that attempt was made)."""
    assert c.n_seq * c.n_genome <= wm.MAX_CELLS
    mine, other = (c.q_id, c.t_id) if f < 2 else (c.t_id, c.q_id)
    a = 0 if f < 2 else 2
    seg = [min(c.cols[a][j], c.cols[a + 1][j]) for j in range(c.n) if mine[j] == mine[i] and c.genome[other[j]] == c.genome[other[i]]]
    return mine[i], min(seg)


def test_paf_front_end_against_the_model():
    from sweepga_amd import PafFile, SwgError
    seen = set()
    for c in TEXT_CASES:
        want = c.result
        assert not c.n or max(max(col) for col in c.cols) >= W, c.name   # (a narrow file is not rebased at all: no case may be one)
        seen.add(want[:2] if want[0] == "ok" else want[0])
        if want[0] == "ok":
            with PafFile(text=_paf_text(c), threads=1) as pf:
                assert pf.n == c.n
                _check_front_end(c, want, pf.names if c.n else [], pf.column("q_id"), pf.column("t_id"), pf.column, pf.seq_offsets,
                                 pf.record_offsets, c.cols)
                for f, k in enumerate(("q_start", "q_end", "t_start", "t_end")):
                    assert [int(x) for x in pf.absolute(k)] == c.cols[f], (c.name, k)
            continue
        assert want[0] == "range"
        with pytest.raises(SwgError) as e:
            PafFile(text=_paf_text(c), threads=1)
        msg = str(e.value)
        assert e.value.code == SWG_ERR_RANGE, (c.name, msg)
        m = re.search(r"(\w+) >= 2\^32 on line (\d+) is not supported", msg) or re.search(r"\((\w+) on line (\d+), first mapped base (\d+)\)", msg)
        assert m, (c.name, msg)
        assert (int(m.group(2)) - 1, FIELD[m.group(1)]) == want[1:], (c.name, msg, want)
        if want[2] < 4:
            # the first mapped base of the stretch the message is about: the per-genome segment's when that attempt was made
            assert ("against one genome" in msg), msg
            sid, base = _segment_base(c, want[1], want[2])
            assert int(m.group(3)) == base, (c.name, msg)
            assert c.names[sid] in msg
    assert seen == {("ok", "seq"), ("ok", "axis"), "range"}


def _aln_record_offsets(a, axis):
    a.lib.swg_aln_record_offsets.restype = C.POINTER(C.c_uint64)
    a.lib.swg_aln_record_offsets.argtypes = [C.c_void_p, C.c_int]
    ptr = a.lib.swg_aln_record_offsets(a.handle, axis)
    return np.ctypeslib.as_array(ptr, shape=(a.n,)).copy() if ptr and a.n else None


def test_aln_front_end_against_the_model():
    """The .1aln derivation makes its own block length (query span + target span, wrapping): the model runs on what it derives."""
    from sweepga_amd import AlnRecords, SwgError
    seen = set()
    for c in TEXT_CASES:
        block = [((c.cols[1][i] - c.cols[0][i]) + (c.cols[3][i] - c.cols[2][i])) % 2**64 for i in range(c.n)]
        cols = c.cols[:5] + [block]
        want = wm.rebase(c.q_id, c.t_id, cols, c.n_seq, c.genome, c.n_genome)
        seen.add(want[:2] if want[0] == "ok" else want[0])
        args = (c.qname, c.tname, *[np.array(col, dtype=np.uint64) for col in c.cols[:5]], "+" * c.n)
        if want[0] == "ok":
            with AlnRecords(*args) as a:
                _check_front_end(c, want, a.names, a.column("q_id"), a.column("t_id"), a.column, a.seq_offsets,
                                 lambda axis: _aln_record_offsets(a, axis), cols)
            continue
        assert want[0] == "range"
        with pytest.raises(SwgError) as e:
            AlnRecords(*args)
        msg = str(e.value)
        assert e.value.code == SWG_ERR_RANGE, (c.name, msg)
        m = re.search(r"alignment (\d+): (\w+) >= 2\^32", msg) or re.search(r"alignment (\d+): .* spans 2\^32 bases or more \((\w+), first mapped base (\d+)", msg)
        assert m, (c.name, msg)
        assert (int(m.group(1)), FIELD[m.group(2)]) == want[1:], (c.name, msg, want)
        if want[2] < 4:
            sid, base = _segment_base(c, want[1], want[2])
            assert int(m.group(3)) == base and "against that genome" in msg and f"sequence {c.names[sid]} " in msg, (c.name, msg)
    assert seen == {("ok", "seq"), ("ok", "axis"), "range"}
