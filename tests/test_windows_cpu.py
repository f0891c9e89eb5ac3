"""The windows model (tests/windows_model.py) against a brute-force count per base and against answers worked out by hand, and the
host side of the feature: structure layout, symbols, the refusals and the header-only texts that need no device, the formatter of
csrc/host/windows_text.cpp against the model's, the command line's usage errors.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import windows_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end", "matches")


def columns(records):
    """records: (q_id, t_id, q_start, q_end, t_start, t_end, matches) per record."""
    a = np.asarray(records, dtype=np.int64).reshape(-1, 7)
    return {k: a[:, j].astype(np.uint32) for j, k in enumerate(COLUMNS)}


def on_query(s, o, a, b, m=None):
    """One record that lies on s over [a, b) with the other side o (whose coordinates do not matter on axis 0)."""
    return (s, o, a, b, 0, max(b - a, 0), b - a if m is None else m)


# ---- the model against a count per base ----------------------------------------------------------------------------------------------
def brute(cols, seq_len, genome, status, axis, W, other_genome):
    """Per listed sequence and set: n, depth, covered, matches per window from per-base arrays -- the overlap of a record with a window
    is the number of its bases whose position // W is the window."""
    s, o, a, b = wm.by_role(cols, axis)
    out = {}
    for r in range(len(s)):
        if genome[s[r]] == genome[o[r]] or a[r] >= b[r] or (other_genome is not None and genome[o[r]] != other_genome):
            continue
        K = -(-int(seq_len[s[r]]) // W)
        t = out.setdefault(int(s[r]), {"n": np.zeros((2, K), dtype=object), "depth": np.zeros((2, K), dtype=object),
                                        "matches": np.zeros((2, K), dtype=object), "base": np.zeros((2, int(seq_len[s[r]])), dtype=bool),
                                        "records": [0, 0]})
        ov = np.bincount(np.arange(a[r], b[r]) // W, minlength=K)
        for which in range(2):
            if which == 1 and (status is None or status[r] == 0):
                continue
            for k in np.flatnonzero(ov):
                t["n"][which, k] += 1
                t["depth"][which, k] += int(ov[k])
                t["matches"][which, k] += int(ov[k]) * int(cols["matches"][r]) // int(b[r] - a[r])
            t["base"][which, a[r]:b[r]] = True
            t["records"][which] += 1
    return out


@pytest.mark.parametrize("W", [1, 7, 64, 2_000, 5_000])
@pytest.mark.parametrize("axis", [0, 1])
def test_model_against_a_count_per_base(W, axis):
    rng = np.random.default_rng(100 * W + axis)
    n_seq, n = 9, 260
    seq_len = rng.integers(1, 2_001, n_seq)
    seq_len[:2] = (2_000, 1_999)
    genome = np.arange(n_seq) // 3
    q, t = rng.integers(0, n_seq, n), rng.integers(0, n_seq, n)
    start = lambda ids: (rng.random(n) * seq_len[ids]).astype(np.int64)      # noqa: E731
    qs, ts = start(q), start(t)
    qe = np.minimum(qs + rng.integers(0, 700, n) * (rng.random(n) < 0.9), seq_len[q])
    te = np.minimum(ts + rng.integers(0, 700, n) * (rng.random(n) < 0.9), seq_len[t])
    cols = columns(np.stack([q, t, qs, qe, ts, te, rng.integers(0, 900, n)], axis=1))
    status = rng.choice(np.array([0, 1, 2, 3], dtype=np.uint8), n)
    for other in (None, 1):
        rows, seqs = wm.windows(cols, seq_len, genome, status, axis, W, other)
        want = brute(cols, seq_len, genome, status, axis, W, other)
        assert seqs["seq"].tolist() == sorted(want) and len(want) >= 5
        s, _, a, b = wm.by_role(cols, axis)
        taking = wm.taking(cols, seq_len, genome, status, axis, other)
        for e in seqs:
            part, t = rows[rows["seq"] == e["seq"]], want[int(e["seq"])]
            K, length = -(-int(seq_len[e["seq"]]) // W), int(seq_len[e["seq"]])
            assert part["index"].tolist() == list(range(K)) and int(e["windows"]) == K
            assert part["start"].tolist() == [k * W for k in range(K)] and part["end"].tolist() == [min((k + 1) * W, length) for k in range(K)]
            for which in range(2):
                assert part["n"][:, which].tolist() == t["n"][which].tolist() and part["depth"][:, which].tolist() == t["depth"][which].tolist()
                assert part["matches"][:, which].tolist() == t["matches"][which].tolist()
                covered = [int(t["base"][which, k * W:(k + 1) * W].sum()) for k in range(K)]
                assert part["covered"][:, which].tolist() == covered
                # the identities
                mine = [r for r in taking[which] if s[r] == e["seq"]]
                assert int(part["depth"][:, which].sum()) == sum(int(b[r] - a[r]) for r in mine) == int(e["depth"][which])
                assert int(part["covered"][:, which].sum()) == int(t["base"][which].sum()) == int(e["covered"][which])
                assert int(e["records"][which]) == len(mine) == t["records"][which] and int(e["empty"][which]) == covered.count(0)
                assert int(e["matches"][which]) == int(part["matches"][:, which].sum())
            assert (part["covered"] <= (part["end"] - part["start"])[:, None]).all() and (part["covered"] <= part["depth"]).all()
            assert (part["n"][:, 1] <= part["n"][:, 0]).all() and (part["covered"][:, 1] <= part["covered"][:, 0]).all()
        # without a status there is no kept set: every [1] entry is 0, empty[1] included
        rows0, seqs0 = wm.windows(cols, seq_len, genome, None, axis, W, other)
        for k in ("n", "covered", "depth", "matches"):
            assert not rows0[k][:, 1].any() and (rows0[k][:, 0] == rows[k][:, 0]).all()
        assert not any(seqs0[k][:, 1].any() for k in ("empty", "covered", "depth", "matches", "records"))


# ---- hand-derived answers ------------------------------------------------------------------------------------------------------------
def one(record, length=1_000, W=100, **kw):
    rows, seqs = wm.windows(columns([record]), [length, 5_000], [0, 1], window=W, **kw)
    return {int(r["index"]): (int(r["n"][0]), int(r["depth"][0]), int(r["covered"][0]), int(r["matches"][0])) for r in rows if r["n"][0]}, rows, seqs


def test_window_borders_by_hand():
    assert one(on_query(0, 1, 110, 190))[0] == {1: (1, 80, 80, 80)}                              # inside one window
    assert one(on_query(0, 1, 150, 200))[0] == {1: (1, 50, 50, 50)}                              # ends exactly on a border: one window
    assert one(on_query(0, 1, 150, 201, 102))[0] == {1: (1, 50, 50, 100), 2: (1, 1, 1, 2)}     # ... one base more: two; floor(50 * 102 / 51), floor(102 / 51)
    assert one(on_query(0, 1, 200, 260))[0] == {2: (1, 60, 60, 60)}                              # starts on a border
    assert one(on_query(0, 1, 200, 400, 100))[0] == {2: (1, 100, 100, 50), 3: (1, 100, 100, 50)}  # exactly two windows, no interior
    # three and more: 70 + 100 + 100 + 30 bases, m = 100 of 300: floor(70 / 3) = 23, 33, 33, 10 -- the floors lose one match
    assert one(on_query(0, 1, 130, 430, 100))[0] == {1: (1, 70, 70, 23), 2: (1, 100, 100, 33), 3: (1, 100, 100, 33), 4: (1, 30, 30, 10)}
    got, rows, seqs = one(on_query(0, 1, 0, 1_050, 2_100), length=1_050)                         # the whole sequence; m > b - a; a last window of 50
    assert got == {**{k: (1, 100, 100, 200) for k in range(10)}, 10: (1, 50, 50, 100)} and len(rows) == 11
    assert (int(rows[10]["start"]), int(rows[10]["end"])) == (1_000, 1_050)
    assert int(seqs[0]["windows"]) == 11 and [int(seqs[0][k][0]) for k in ("empty", "covered", "depth", "matches", "records")] == [0, 1_050, 1_050, 2_100, 1]


def test_who_takes_part_and_the_union_by_hand():
    cols = columns([on_query(0, 3, 0, 900),          # r0 inside genome 0: never
                    on_query(0, 1, 50, 250),         # r1 dropped; r2 kept and nested in it
                    on_query(0, 1, 100, 150),
                    on_query(0, 2, 250, 300),        # r3 abuts r1: one merged interval [50, 300), of another genome
                    on_query(0, 1, 700, 700),        # zero length: adds nothing
                    on_query(2, 0, 10, 20)])         # another sequence, listed after 0
    seq_len, genome, status = [1_000, 500, 400, 900], [0, 1, 2, 0], np.array([1, 0, 3, 2, 1, 1], dtype=np.uint8)
    rows, seqs = wm.windows(cols, seq_len, genome, status, window=100)
    assert seqs["seq"].tolist() == [0, 2] and len(rows) == 10 + 4
    assert [(int(r["n"][0]), int(r["covered"][0]), int(r["depth"][0])) for r in rows[:4]] == [(1, 50, 50), (2, 100, 150), (2, 100, 100), (0, 0, 0)]
    assert [(int(r["n"][1]), int(r["covered"][1]), int(r["depth"][1])) for r in rows[:4]] == [(0, 0, 0), (1, 50, 50), (1, 50, 50), (0, 0, 0)]
    assert seqs[0]["records"].tolist() == [3, 2] and seqs[0]["empty"].tolist() == [7, 8] and seqs[0]["covered"].tolist() == [250, 100]
    rows, seqs = wm.windows(cols, seq_len, genome, status, window=100, other_genome=2)
    assert seqs["seq"].tolist() == [0] and seqs[0]["covered"].tolist() == [50, 50]
    rows, seqs = wm.windows(cols, seq_len, genome, status, window=100, other_genome=3)           # a genome without records: nothing is listed
    assert len(rows) == 0 and len(seqs) == 0
    rows, seqs = wm.windows(cols, seq_len, genome, status, axis=1, window=100, weight=np.full(6, 7))
    assert seqs["seq"].tolist() == [0, 1, 2] and seqs["matches"][:, 0].tolist() == [7, 3 + 3 + 7, 7]    # [0, 200) over two windows: floor(100 * 7 / 200) each
    with pytest.raises(ValueError, match="record 1 "):
        wm.windows(cols, [249, 500, 400, 900], genome, status, window=100)
    assert wm.rows_text(rows[:1], ["a", "b", "c", "d"]) == (wm.ROWS_HEADER + "a\t0\t100\t1\t10\t10\t7\t1\t10\t10\t7\n").encode()
    assert wm.summary_text(seqs[:1], ["a", "b", "c", "d"], seq_len) == (wm.SUMMARY_HEADER + "a\t1000\t10\t9\t9\t10\t10\t10\t10\t7\t7\t1\t1\n").encode()


def test_the_report_does_not_depend_on_record_order():
    rng = np.random.default_rng(4)
    n, n_seq = 600, 12
    q, t = rng.integers(0, n_seq, n), rng.integers(0, n_seq, n)
    qs, ln = rng.integers(0, 5_000, n), rng.integers(0, 900, n)
    cols = columns(np.stack([q, t, qs, qs + ln, qs, qs + ln, rng.integers(0, 2**32, n)], axis=1))
    seq_len, genome, status = np.full(n_seq, 6_000), np.arange(n_seq) // 3, (rng.random(n) < 0.6).astype(np.uint8)
    perm = rng.permutation(n)
    for axis in (0, 1):
        a = wm.windows(cols, seq_len, genome, status, axis, 64)
        b = wm.windows({k: v[perm] for k, v in cols.items()}, seq_len, genome, status[perm], axis, 64)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and len(a[1]) == n_seq


# ---- the host side of the library ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbols_are_exported_and_declared(lib):
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_windows_records", "swg_windows_records_device", "swg_paf_windows"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    import sweepga_amd
    from sweepga_amd import windows
    assert sweepga_amd.Windows is windows.Windows and sweepga_amd.windows_records is windows.windows_records
    assert sweepga_amd.windows_records_device is windows.windows_records_device
    for name, value in (("SWG_WINDOWS_ROWS", windows.ROWS), ("SWG_WINDOWS_SUMMARY", windows.SUMMARY)):
        assert "#define %s %du\n" % (name, value) in hdr
    assert "#define SWG_WINDOWS_ANY 0xffffffffu\n" in hdr and windows.ANY == 0xffffffff
    assert windows.ROW_DTYPE == wm.ROW_DTYPE and windows.SEQ_DTYPE == wm.SEQ_DTYPE
    src = open(os.path.join(ROOT, "sweepga_amd", "build.py")).read()
    assert '"swg_windows.hip"' in src and '"windows_text.cpp"' in src


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib
    structs = (("swg_window_row", _lib.SwgWindowRow), ("swg_window_seq", _lib.SwgWindowSeq), ("swg_windows_request", _lib.SwgWindowsRequest))
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
    assert (C.sizeof(_lib.SwgWindowRow), C.sizeof(_lib.SwgWindowSeq), C.sizeof(_lib.SwgWindowsRequest)) == (64, 80, 80)
    for cls, dtype in ((_lib.SwgWindowRow, wm.ROW_DTYPE), (_lib.SwgWindowSeq, wm.SEQ_DTYPE)):
        assert dtype.itemsize == C.sizeof(cls)
        for f, t in cls._fields_:
            assert dtype.fields[f][1] == getattr(cls, f).offset and dtype.fields[f][0].itemsize == C.sizeof(t), f
    for _, cls in structs:      # no implicit padding: the fields fill the structure
        assert sum(C.sizeof(t) for _, t in cls._fields_) == C.sizeof(cls)


LINE = "a#1#x\t100\t0\t50\t+\tb#1#y\t200\t10\t60\t50\t50\t60\n"
HEADERS = (wm.ROWS_HEADER.encode(), wm.SUMMARY_HEADER.encode())


def test_no_records_needs_no_device(lib, tmp_path):
    from sweepga_amd import PafFile, Windows, build
    for text in ("", "# nothing\nfew\tfields\n"):
        with PafFile(text=text) as paf:
            assert paf.n == 0
            for axis in ("query", "target"):
                g = Windows.from_paf(None, paf, np.zeros(0, dtype=np.uint8), axis=axis, window=7, other_genome="a#1#")
                assert (g.rows, g.summary) == HEADERS
            g = Windows.from_paf(None, paf, None, summary=False)
            assert g.rows == HEADERS[0] and g.summary is None
            g = Windows.from_paf(None, paf, None, rows=False)
            assert g.rows is None and g.summary == HEADERS[1]
    empty, rows, summ, out = (tmp_path / x for x in ("empty.paf", "w.tsv", "s.tsv", "out.paf"))
    empty.write_text("")
    for extra in ([], ["--no-filter"]):     # a PAF without records opens no device either
        rows.write_bytes(b"stale")
        r = subprocess.run([build.CLI, str(empty), "--output-file", str(out), "--windows", str(rows), "--windows-summary", str(summ), "--window-size", "1k",
                            "--windows-axis", "target", "--windows-genome", "x", "--quiet", *extra], capture_output=True, text=True)
        assert r.returncode == 0 and (rows.read_bytes(), summ.read_bytes()) == HEADERS, r.stderr
    r = subprocess.run([build.CLI, str(empty), "--no-filter", "--windows-summary", "-"], capture_output=True)       # - = standard error
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == HEADERS[1]


def test_refusals_that_need_no_device(lib):
    from sweepga_amd import PafFile, _lib
    cols = columns([on_query(0, 1, 100, 400)])
    rec = _lib.SwgRecords()
    rec.n = 1
    for k, a in cols.items():
        setattr(rec, k, a.ctypes.data)
    rec.n_seq = 2
    seq_len, genome, status = np.array([1000, 5000], dtype=np.uint32), np.array([0, 1], dtype=np.uint32), np.ones(1, dtype=np.uint8)
    req = _lib.SwgWindowsRequest()
    req.want, req.window, req.other_genome, req.n_rows, req.n_seqs = 3, 100, 0xffffffff, 12345, 12345
    for fn in (lib.swg_windows_records, lib.swg_windows_records_device):   # a NULL context: refused before any pointer is looked at
        assert fn(None, C.byref(rec), seq_len.ctypes.data, genome.ctypes.data, 2, status.ctypes.data, C.byref(req)) == -1
        assert int(req.n_rows) == int(req.n_seqs) == 12345
    marker = C.create_string_buffer(1)

    def texts(ctx, paf, status, axis, window, genome=None, want=(True, True)):
        p, n = (C.c_void_p * 2)(), (C.c_uint64 * 2)()
        for k in range(2):
            p[k] = C.addressof(marker) if want[k] else None
        rc = lib.swg_paf_windows(ctx, paf.handle, status, axis, window, genome, p, n)
        assert rc != 0 and not p[0] and not p[1] and n[0] == n[1] == 0
        return rc, lib.swg_alnstats_last_error()
    with PafFile(text=LINE) as paf:
        st = np.array([1], dtype=np.uint8)
        assert texts(None, paf, st.ctypes.data, 0, 100) == (-1, b"swg_paf_windows: NULL context")
        assert texts(None, paf, None, 0, 100, b"a#1") == (-1, b"swg_paf_windows: NULL context")      # a known name, with or without its '#'
        assert texts(None, paf, None, 0, 100, b"b#1#") == (-1, b"swg_paf_windows: NULL context")
        assert texts(None, paf, st.ctypes.data, 0, 100, want=(False, False)) == (-1, b"swg_paf_windows: neither text is asked for")
        assert texts(None, paf, st.ctypes.data, 2, 100) == (-1, b"swg_paf_windows: axis is 0 (query) or 1 (target)")
        assert texts(None, paf, st.ctypes.data, 0, 0) == (-1, b"swg_paf_windows: the window size is at least 1")
        assert texts(None, paf, st.ctypes.data, 0, 100, b"c#9#") == (-1, b"swg_paf_windows: unknown genome 'c#9#'")
        assert texts(None, paf, st.ctypes.data, 0, 100, b"a#") == (-1, b"swg_paf_windows: unknown genome 'a#'")
        assert lib.swg_paf_windows(None, paf.handle, None, 0, 100, None, None, None) == -1
        assert lib.swg_alnstats_last_error() == b"swg_paf_windows: NULL argument"


def test_64_bit_columns_are_refused_without_a_device(lib, tmp_path):
    from sweepga_amd import build, PafFile
    ln = "\t".join(["a#1#x", str(2**33), str(2**32), str(2**32 + 50), "+", "b#1#y", "900", "10", "60", "50", "50", "60"]) + "\n"
    marker = C.create_string_buffer(1)
    with PafFile(text=ln) as paf:
        assert paf.is_rebased
        p, n = (C.c_void_p * 2)(C.addressof(marker), C.addressof(marker)), (C.c_uint64 * 2)()
        assert lib.swg_paf_windows(None, paf.handle, None, 0, 100, None, p, n) == -6 and not p[0] and not p[1]
        assert b"2^32" in lib.swg_alnstats_last_error()
    inp, out = tmp_path / "in.paf", tmp_path / "out.paf"
    inp.write_text(ln)
    for flag in ("--windows", "--windows-summary"):
        for extra in ([], ["--no-filter"]):
            rep = tmp_path / "w.tsv"
            r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), flag, str(rep), *extra], capture_output=True, text=True)
            assert r.returncode == 3 and "--windows" in r.stderr and "2^32" in r.stderr, r.stderr
            assert r.stdout == "" and not out.exists() and not rep.exists()


FLAGS = ("--windows", "--windows-summary", "--window-size", "--windows-axis", "--windows-genome")


def test_command_line_lists_the_flags_and_its_usage_errors(lib):
    from sweepga_amd import build
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for shown in ("--windows FILE", "--windows-summary FILE", "--window-size N", "--windows-axis query|target", "--windows-genome NAME"):
        assert shown in r.stdout, shown
    for flag in FLAGS:
        r = subprocess.run([build.CLI, "in.paf", flag], capture_output=True, text=True)          # no value
        assert r.returncode == 2 and flag in r.stderr, (flag, r.stderr)
    for flag in ("--windows", "--windows-summary", "--windows-genome"):
        r = subprocess.run([build.CLI, "in.paf", "--windows-summary", "s.tsv", flag + "="], capture_output=True, text=True)    # an empty one
        assert r.returncode == 2 and flag in r.stderr, (flag, r.stderr)
    for flag, bads in (("--window-size", ("x", "5q", "", "0", "4294967296", "5g", "1e30", "-1")), ("--windows-axis", ("both", "", "0"))):
        for bad in bads:     # 0 is no window; 2^32 and 5g do not fit 32 bits
            r = subprocess.run([build.CLI, "in.paf", "--windows", "w.tsv", flag + "=" + bad], capture_output=True, text=True)
            assert r.returncode == 2 and flag in r.stderr, (flag, bad, r.stderr)
    for flag, value in (("--window-size", "1k"), ("--windows-axis", "target"), ("--windows-genome", "a#1")):   # an option without a report
        r = subprocess.run([build.CLI, "in.paf", flag, value], capture_output=True, text=True)
        assert r.returncode == 2 and "need --windows or --windows-summary" in r.stderr, (flag, r.stderr)


# ---- the formatter -------------------------------------------------------------------------------------------------------------------
def test_the_formatter_against_the_model_under_the_host_sanitizers(tmp_path):
    """tests/native/windows_text_check.cpp: a stand-alone program over csrc/host/windows_text.cpp, built with the address and
    undefined-behaviour sanitizers, formats what the model computed and rows at the ends of every field's range; its two texts must
    be the model's byte for byte."""
    exe = str(tmp_path / "windows_text_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "windows_text_check.cpp"),
                           os.path.join(ROOT, "sweepga_amd", "csrc", "host", "windows_text.cpp")])
    names, seq_len = ["a#1#x", "b#1#y", "", "c#2#z"], [1000, 2**32 - 1, 0, 77]      # the program's own table
    cols = columns([on_query(0, 1, 130, 430, 100), on_query(0, 3, 50, 250), on_query(3, 0, 0, 77, 2**32 - 1), on_query(1, 0, 2**32 - 2, 2**32 - 1)])
    rows, seqs = wm.windows(cols, seq_len, [0, 1, 1, 2], np.array([1, 0, 2, 1], dtype=np.uint8), window=2**31)
    top_row = np.zeros(1, dtype=wm.ROW_DTYPE)
    top_seq = np.zeros(1, dtype=wm.SEQ_DTYPE)
    for arr in (top_row, top_seq):      # every field at the end of its range, on the sequence with the empty name
        for k in arr.dtype.names:
            arr[k] = 2 if k == "seq" else np.iinfo(arr.dtype[k].base).max
    cases = (([], []), (rows, seqs), (np.concatenate([rows, top_row]), np.concatenate([seqs, top_seq])))
    assert len(rows) == 1 + 2 + 1 and len(seqs) == 3
    for rws, sqs in cases:
        feed = []
        for r in rws:
            feed.append("R " + " ".join(str(int(x)) for x in (r["seq"], r["index"], r["start"], r["end"], *r["n"], *r["covered"], *r["depth"], *r["matches"])))
        for e in sqs:
            feed.append("S " + " ".join(str(int(x)) for x in (e["seq"], e["windows"], *e["empty"], *e["covered"], *e["depth"], *e["matches"], *e["records"])))
        r = subprocess.run([exe], input="\n".join(feed).encode(), capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout == wm.rows_text(rws, names) + b"--\n" + wm.summary_text(sqs, names, seq_len)
    assert b"\t18446744073709551615\n" in r.stdout and b"\n\t4294967295\t4294967295\t" in r.stdout
