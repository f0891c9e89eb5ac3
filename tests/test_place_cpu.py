"""The placement model (tests/place_model.py) against answers worked out by hand, then under the oracle's status on
tests/golden/syeast.paf.gz against the link sums of tests/components_model.py, and the host side of the feature: structure layout,
symbols, the command line's usage errors, the calls that need no device.  No GPU."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import components_model as cm
from tests import orc
from tests import place_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end", "strand")


def columns(records):
    """records: (q_id, t_id, q_start, q_end, t_start, t_end, strand) per record."""
    a = np.asarray(records, dtype=np.int64).reshape(-1, 7)
    return {k: a[:, j].astype(np.uint8 if k == "strand" else np.uint32) for j, k in enumerate(COLUMNS)}


def pick(row, *fields):
    return tuple(row[f] for f in fields)


# sequence 0 of genome 0 (1,000 bases) against sequence 1 of genome 1: '+' 300 + 200 bases, '-' 100
MAJORITY = [(0, 1, 100, 400, 1100, 1400, 0),   # off = 1100 - 100 = 1000, w = 300
            (0, 1, 500, 700, 1520, 1720, 0),   # off = 1520 - 500 = 1020, w = 200
            (0, 1, 700, 800, 2000, 2100, 1)]   # off = 2100 + 700 = 2800, w = 100


# ---- hand-derived answers --------------------------------------------------------------------------------------------------------
def test_a_plus_majority_and_a_minus_minority_on_both_axes():
    cols, seq_len, genome = columns(MAJORITY), [1000, 5000], [0, 1]
    (row,) = pm.place(cols, seq_len, genome)
    # fwd 500 >= rev 100: '+'; deciding r0, r1: W = 500, half = 250; by anchor 1000 (300 >= 250): offset 1000
    assert pick(row, "seq", "partner", "genome", "partner_genome", "orient", "fwd", "rev", "bases", "n_records") == (0, 1, 0, 1, 0, 500, 100, 600, 3)
    assert pick(row, "offset", "start", "q_lo", "q_hi", "t_lo", "t_hi") == (1000, 1000, 100, 700, 1100, 1720)
    assert pick(row, "total_bases", "runner_bases", "rank") == (600, 0, 0)
    # the target axis: sequence 1 placed on 0 with the target lengths; anchors -1000 (300), -1020 (200), '-': 800 + 2000 = 2800
    (row,) = pm.place(cols, seq_len, genome, axis=1)
    assert pick(row, "seq", "partner", "genome", "partner_genome", "orient", "fwd", "rev") == (1, 0, 1, 0, 0, 500, 100)
    # by anchor: -1020 (prefix 200 < 250), -1000 (500 >= 250)
    assert pick(row, "offset", "start", "q_lo", "q_hi", "t_lo", "t_hi") == (-1000, -1000, 1100, 1720, 100, 700)
    assert pm.summary([row], seq_len) == [dict(genome=1, partner_genome=0, rows=1, reversed=0, length=5000, bases=600, total_bases=600)]


def test_equal_strands_give_plus_and_a_minus_start_can_be_negative():
    tie = columns([(0, 1, 0, 100, 50, 150, 0), (0, 1, 200, 300, 400, 500, 1)])
    (row,) = pm.place(tie, [1000, 5000], [0, 1])
    assert pick(row, "orient", "fwd", "rev", "offset", "start", "q_lo", "q_hi") == (0, 100, 100, 50, 50, 0, 100)
    # '-': off = t_end + q_start = 150 + 100 = 250; start = 250 - 1000
    minus = columns([(0, 1, 100, 200, 50, 150, 1)])
    (row,) = pm.place(minus, [1000, 5000], [0, 1])
    assert pick(row, "orient", "offset", "start", "t_lo", "t_hi") == (1, 250, -750, 50, 150)
    assert pm.rows_text([row], ["a#1#x", "b#1#y"], [1000, 5000]).decode().split("\n")[1] == \
        "a#1#x\t1000\tb#1#y\t5000\t-\t-750\t250\t0\t100\t0\t100\t100\t0\t1\t100\t200\t50\t150"
    # a winner of weight 0 with '-' records only: fwd >= rev holds, but there is no '+' record to decide: '-'
    (row,) = pm.place(columns([(0, 1, 7, 7, 30, 30, 1)]), [1000, 5000], [0, 1])
    assert pick(row, "orient", "bases", "offset", "start") == (1, 0, 37, 37 - 1000)


def test_two_partners_tied_in_bases():
    cols = columns([(0, 2, 0, 100, 10, 110, 0), (0, 1, 0, 100, 500, 600, 0), (0, 3, 0, 40, 0, 40, 0)])
    (row,) = pm.place(cols, [1000] * 4, [0, 1, 1, 1])
    assert pick(row, "partner", "bases", "runner_bases", "total_bases", "offset") == (1, 100, 100, 240, 500)
    # the partners of another genome compete apart
    rows = pm.place(cols, [1000] * 4, [0, 1, 2, 1])
    assert [pick(r, "partner", "partner_genome", "bases", "runner_bases", "total_bases") for r in rows] == [(1, 1, 100, 40, 140), (2, 2, 100, 0, 100)]


def median_case(anchors_and_weights):
    """'+' records of sequence 0 on 1 with the given (anchor, weight): q = [0, w), t = [anchor, anchor + w)."""
    return columns([(0, 1, 0, w, off, off + w, 0) for off, w in anchors_and_weights])


def test_weighted_median():
    place = lambda items: pm.place(median_case(items), [100, 1000], [0, 1])[0]["offset"]   # noqa: E731
    # one heavy record outweighs two light ones on either side: W = 14, half = 7; prefixes 1, 2, 12
    assert place([(40, 1), (10, 1), (30, 10), (50, 1), (20, 1)]) == 30
    assert place([(10, 1), (20, 1), (30, 1)]) == 20          # W = 3 odd: half = 2
    assert place([(10, 2), (20, 2)]) == 10                   # W = 4 even: half = 2, reached by the first: the lower median
    assert place([(10, 2), (20, 3)]) == 20                   # W = 5: half = 3
    assert place([(70, 0), (30, 0)]) == 30                   # W = 0: the first in (anchor, index) order
    assert place([(70, 0), (30, 0), (50, 1)]) == 50          # zero weights beside a weight: half = 1 is reached by the weight only
    assert place([(20, 5), (20, 5), (10, 9)]) == 20          # equal anchors: the value does not depend on their order


def test_intra_genome_and_dropped_records_take_no_part_and_both_sets():
    cols = columns([(0, 3, 0, 900, 0, 900, 0),      # r0 inside genome 0: never
                    (0, 1, 0, 100, 200, 300, 0),    # r1 kept
                    (0, 2, 0, 500, 700, 1200, 1)])  # r2 dropped: the better partner of the ALL set
    seq_len, genome, status = [1000] * 4, [0, 1, 1, 0], np.array([1, 3, 0], dtype=np.uint8)
    assert pm.taking(cols, genome, status, 0, False) == [1, 2] and pm.taking(cols, genome, status, 0, True) == [1]
    (row,) = pm.place(cols, seq_len, genome, status, kept=False)
    assert pick(row, "partner", "orient", "bases", "runner_bases", "total_bases", "offset", "start") == (2, 1, 500, 100, 600, 1200, 200)
    (row,) = pm.place(cols, seq_len, genome, status, kept=True)
    assert pick(row, "partner", "orient", "bases", "runner_bases", "total_bases", "offset") == (1, 0, 100, 0, 100, 200)
    assert sorted(pm.candidates(cols, genome)) == [(0, 1), (0, 2)] and sorted(pm.candidates(cols, genome, axis=1)) == [(1, 0), (2, 0)]


def test_min_bases_at_and_one_above_the_winner():
    cols, seq_len, genome = columns(MAJORITY), [1000, 5000], [0, 1]
    assert len(pm.place(cols, seq_len, genome, min_bases=600)) == 1 and pm.place(cols, seq_len, genome, min_bases=601) == []


def test_rank_along_one_partner_with_equal_starts():
    cols = columns([(0, 3, 0, 100, 500, 600, 0), (1, 3, 0, 100, 100, 200, 0), (2, 3, 50, 150, 150, 250, 0), (2, 4, 0, 10, 0, 10, 0)])
    rows = pm.place(cols, [1000] * 5, [0, 0, 0, 1, 2])
    # partner 3: starts 500 (s 0), 100 (s 1), 150 - 50 = 100 (s 2): order (100, 1), (100, 2), (500, 0); then genome 2's partner 4
    assert [pick(r, "seq", "partner", "start", "rank") for r in rows] == [(1, 3, 100, 0), (2, 3, 100, 1), (0, 3, 500, 2), (2, 4, 0, 0)]
    assert [pick(p, "genome", "partner_genome", "rows", "length") for p in pm.summary(rows, [1000] * 5)] == [(0, 1, 3, 3000), (0, 2, 1, 1000)]
    text = pm.summary_text(pm.summary(rows, [1000] * 5), ["a#1#", "b#1#", "c#1#"]).decode().split("\n")
    assert text[0] + "\n" == pm.SUMMARY_HEADER and text[1:] == ["a#1#\tb#1#\t3\t0\t3000\t300\t300", "a#1#\tc#1#\t1\t0\t1000\t10\t10", ""]


def test_the_report_does_not_depend_on_record_order():
    rng = np.random.default_rng(4)
    n, n_seq = 600, 12
    q, t = rng.integers(0, n_seq, n), rng.integers(0, n_seq, n)
    qs, ts, ln = rng.integers(0, 5_000, n), rng.integers(0, 5_000, n), rng.integers(0, 30, n) * (rng.random(n) < 0.9)
    cols = columns(np.stack([q, t, qs, qs + ln, ts, ts + ln, rng.random(n) < 0.4], axis=1))
    seq_len, genome, status = rng.integers(100, 9_000, n_seq), np.arange(n_seq) // 3, (rng.random(n) < 0.6).astype(np.uint8)
    perm = rng.permutation(n)
    for axis in (0, 1):
        for kept in (False, True):
            a = pm.place(cols, seq_len, genome, status, axis, kept, 20)
            assert a == pm.place({k: v[perm] for k, v in cols.items()}, seq_len, genome, status[perm], axis, kept, 20) and len(a) > 10


# ---- the model under the oracle's status on the yeast fixture ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def syeast():
    text = gzip.open(os.path.join(ROOT, "tests", "golden", "syeast.paf.gz"), "rb").read().decode()
    rec = orc.parse_paf_text(text)
    ids = {}
    for q, t in zip(rec.qname, rec.tname):
        ids.setdefault(q, len(ids))
        ids.setdefault(t, len(ids))
    names = list(ids)
    cols = {"q_id": [ids[x] for x in rec.qname], "t_id": [ids[x] for x in rec.tname], "q_start": rec.qs, "q_end": rec.qe, "t_start": rec.ts,
            "t_end": rec.te, "strand": (rec.strand == ord("-")).astype(np.uint8)}
    prefixes = {}
    genome = [prefixes.setdefault(x[:x.rindex("#") + 1], len(prefixes)) for x in names]
    return rec, {k: np.asarray(v) for k, v in cols.items()}, names, cm.last_lengths(text, names), genome


def test_model_under_the_oracle_on_syeast(syeast):
    rec, cols, names, seq_len, genome = syeast
    status, _ = orc.apply_filters(orc.Config(), rec)
    status = status[:len(rec)]
    links = {(a, b): (n, ab, bb) for a, b, n, _, ab, bb, _ in cm.components(cols, status, seq_len)["links"] if genome[a] != genome[b]}
    cand = [pm.candidates(cols, genome, status, axis, kept=True) for axis in (0, 1)]
    # per (s, p) the candidate sums of axis 0 plus those of axis 1 are the link's sums on the side of s
    seen = {}
    for table in cand:
        for (s, p), c in table.items():
            e = seen.setdefault((s, p), [0, 0])
            e[0] += c["n_records"]
            e[1] += c["bases"]
    want = {}
    for (a, b), (n, ab, bb) in links.items():
        want[(a, b)], want[(b, a)] = [n, ab], [n, bb]
    assert seen == want and len(links) > 100
    for axis in (0, 1):
        rows = pm.place(cols, seq_len, genome, status, axis, kept=True)
        # total_bases per genome pair = the sum of its candidates
        per_pair = {}
        for (s, p), c in cand[axis].items():
            key = (genome[s], genome[p])
            per_pair[key] = per_pair.get(key, 0) + c["bases"]
        pairs = pm.summary(rows, seq_len)
        assert {(e["genome"], e["partner_genome"]): e["total_bases"] for e in pairs} == per_pair
        assert len(rows) == len({(s, genome[p]) for s, p in cand[axis]})
        assert all(r["fwd"] + r["rev"] == r["bases"] <= r["total_bases"] and r["runner_bases"] <= r["bases"] for r in rows)
        assert (len(rows), sum(r["orient"] for r in rows), len(pairs)) == OBSERVED[axis], (len(rows), sum(r["orient"] for r in rows), len(pairs))
        assert 0 < len(pm.place(cols, seq_len, genome, status, axis, kept=True, min_bases=100_000)) < len(rows)


OBSERVED = {0: (952, 4, 56), 1: (952, 4, 56)}   # (rows, reversed, genome pairs) of the yeast fixture under the default flags, per axis


# ---- the host side of the library ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbols_are_exported_and_declared(lib):
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_place_records", "swg_place_records_device", "swg_paf_place"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    assert lib.swg_abi_version() == 1
    import sweepga_amd
    from sweepga_amd import place
    assert sweepga_amd.Place is place.Place and sweepga_amd.place_records is place.place_records
    assert sweepga_amd.place_records_device is place.place_records_device
    for name, value in (("SWG_PLACE_ROWS", place.ROWS), ("SWG_PLACE_SUMMARY", place.SUMMARY)):
        assert "#define %s %du\n" % (name, value) in hdr
    assert place.ROW_DTYPE.names[:len(pm.FIELDS)] == pm.FIELDS and place.PAIR_DTYPE.names == pm.PAIR_FIELDS
    src = open(os.path.join(ROOT, "sweepga_amd", "build.py")).read()
    assert '"swg_place.hip"' in src and '"place_text.cpp"' in src


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib
    from sweepga_amd.place import PAIR_DTYPE, ROW_DTYPE
    structs = (("swg_placement", _lib.SwgPlacement), ("swg_place_pair", _lib.SwgPlacePair), ("swg_place_request", _lib.SwgPlaceRequest))
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
    assert (C.sizeof(_lib.SwgPlacement), C.sizeof(_lib.SwgPlacePair), C.sizeof(_lib.SwgPlaceRequest)) == (104, 48, 72)
    for cls, dtype in ((_lib.SwgPlacement, ROW_DTYPE), (_lib.SwgPlacePair, PAIR_DTYPE)):
        assert dtype.itemsize == C.sizeof(cls)
        for f, t in cls._fields_:
            assert dtype.fields[f][1] == getattr(cls, f).offset and dtype.fields[f][0].itemsize == C.sizeof(t), f
    # no implicit padding: the fields fill the structure
    for _, cls in structs:
        assert sum(C.sizeof(t) for _, t in cls._fields_) == C.sizeof(cls)


FLAGS = ("--place", "--place-summary", "--place-axis", "--place-set", "--place-min-bases")


def test_command_line_lists_the_flags_and_its_usage_errors(lib):
    from sweepga_amd import build
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for shown in ("--place FILE", "--place-summary FILE", "--place-axis query|target", "--place-set kept|all", "--place-min-bases N"):
        assert shown in r.stdout, shown
    for flag in FLAGS:
        r = subprocess.run([build.CLI, "in.paf", flag], capture_output=True, text=True)          # no value
        assert r.returncode == 2 and flag in r.stderr, (flag, r.stderr)
    for flag in ("--place", "--place-summary"):
        r = subprocess.run([build.CLI, "in.paf", flag + "="], capture_output=True, text=True)    # an empty one
        assert r.returncode == 2 and flag in r.stderr, (flag, r.stderr)
    for flag, bads in (("--place-axis", ("both", "", "0")), ("--place-set", ("lost", "", "1")), ("--place-min-bases", ("x", "5q", "", "1e30"))):
        for bad in bads:     # 1e30 does not fit 64 bits
            r = subprocess.run([build.CLI, "in.paf", "--place", "p.tsv", flag + "=" + bad], capture_output=True, text=True)
            assert r.returncode == 2 and flag in r.stderr, (flag, bad, r.stderr)
    for flag, value in (("--place-axis", "target"), ("--place-set", "all"), ("--place-min-bases", "1k")):   # an option without a report
        r = subprocess.run([build.CLI, "in.paf", flag, value], capture_output=True, text=True)
        assert r.returncode == 2 and "need --place or --place-summary" in r.stderr, (flag, r.stderr)


LINE = "a#1#x\t100\t0\t50\t+\tb#1#y\t200\t10\t60\t50\t50\t60\n"
HEADERS = (pm.ROWS_HEADER.encode(), pm.SUMMARY_HEADER.encode())


def test_no_records_needs_no_device(lib, tmp_path):
    from sweepga_amd import Place, PafFile, build
    for text in ("", "# nothing\nfew\tfields\n"):
        with PafFile(text=text) as paf:
            assert paf.n == 0
            for axis in ("query", "target"):
                for set_ in ("all", "kept"):
                    g = Place.from_paf(None, paf, np.zeros(0, dtype=np.uint8), axis=axis, set=set_, min_bases=5)
                    assert (g.rows, g.summary) == HEADERS and len(g.table) == 0
            g = Place.from_paf(None, paf, None, set="all", summary=False)
            assert g.rows == HEADERS[0] and g.summary is None
            g = Place.from_paf(None, paf, None, set="all", rows=False)
            assert g.rows is None and g.summary == HEADERS[1] and g.table is None
    empty, rows, summ, out = (tmp_path / x for x in ("empty.paf", "p.tsv", "s.tsv", "out.paf"))
    empty.write_text("")
    for extra in ([], ["--no-filter"]):     # a PAF without records opens no device either
        rows.write_bytes(b"stale")
        r = subprocess.run([build.CLI, str(empty), "--output-file", str(out), "--place", str(rows), "--place-summary", str(summ), "--place-min-bases", "1k",
                            "--place-axis", "target", "--place-set", "all", "--quiet", *extra], capture_output=True, text=True)
        assert r.returncode == 0 and (rows.read_bytes(), summ.read_bytes()) == HEADERS, r.stderr
    r = subprocess.run([build.CLI, str(empty), "--no-filter", "--place-summary", "-"], capture_output=True)       # - = standard error
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == HEADERS[1]


def test_refusals_that_need_no_device(lib):
    from sweepga_amd import PafFile, _lib
    cols = columns(MAJORITY)
    rec = _lib.SwgRecords()
    rec.n = 3
    for k, a in cols.items():
        setattr(rec, k, a.ctypes.data)
    rec.n_seq = 2
    seq_len, genome, status = np.array([1000, 5000], dtype=np.uint32), np.array([0, 1], dtype=np.uint32), np.ones(3, dtype=np.uint8)
    req = _lib.SwgPlaceRequest()
    req.want, req.n_rows, req.n_pairs = 3, 12345, 12345
    for fn in (lib.swg_place_records, lib.swg_place_records_device):   # a NULL context: refused before any pointer is looked at
        assert fn(None, C.byref(rec), seq_len.ctypes.data, genome.ctypes.data, 2, status.ctypes.data, C.byref(req)) == -1
        assert int(req.n_rows) == int(req.n_pairs) == 12345
    marker = C.create_string_buffer(1)

    def texts(ctx, paf, status, axis, set_, want=(True, True)):
        p, n = (C.c_void_p * 2)(), (C.c_uint64 * 2)()
        for k in range(2):
            p[k] = C.addressof(marker) if want[k] else None
        rc = lib.swg_paf_place(ctx, paf.handle, status, axis, set_, 0, p, n)
        assert rc != 0 and not p[0] and not p[1] and n[0] == n[1] == 0
        return rc, lib.swg_alnstats_last_error()
    with PafFile(text=LINE) as paf:
        st = np.array([1], dtype=np.uint8)
        assert texts(None, paf, st.ctypes.data, 0, 1) == (-1, b"swg_paf_place: NULL context")
        assert texts(None, paf, st.ctypes.data, 0, 1, (False, False))[0] == -1        # neither text
        assert texts(None, paf, st.ctypes.data, 2, 1)[0] == -1 and texts(None, paf, st.ctypes.data, 0, 2)[0] == -1
        rc, msg = texts(None, paf, None, 0, 1)                                       # the kept set without a status
        assert rc == -1 and b"status" in msg
        assert lib.swg_paf_place(None, paf.handle, None, 0, 0, 0, None, None) == -1


def test_64_bit_columns_are_refused_without_a_device(lib, tmp_path):
    from sweepga_amd import build, PafFile
    ln = "\t".join(["a#1#x", str(2**33), str(2**32), str(2**32 + 50), "+", "b#1#y", "900", "10", "60", "50", "50", "60"]) + "\n"
    marker = C.create_string_buffer(1)
    with PafFile(text=ln) as paf:
        assert paf.is_rebased
        p, n = (C.c_void_p * 2)(C.addressof(marker), C.addressof(marker)), (C.c_uint64 * 2)()
        st = np.array([1], dtype=np.uint8)
        assert lib.swg_paf_place(None, paf.handle, st.ctypes.data, 0, 1, 0, p, n) == -6 and not p[0] and not p[1]
        assert b"2^32" in lib.swg_alnstats_last_error()
    inp, out = tmp_path / "in.paf", tmp_path / "out.paf"
    inp.write_text(ln)
    for flag in ("--place", "--place-summary"):
        for extra in ([], ["--no-filter"]):
            rep = tmp_path / "p.tsv"
            r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), flag, str(rep), *extra], capture_output=True, text=True)
            assert r.returncode == 3 and "--place" in r.stderr and "2^32" in r.stderr, r.stderr
            assert r.stdout == "" and not out.exists() and not rep.exists()


def test_the_formatter_under_the_host_sanitizers(tmp_path):
    """tests/native/place_text_check.cpp: a stand-alone program over csrc/host/place_text.cpp with rows at the ends of every
    field's range, built with the address and undefined-behaviour sanitizers."""
    import json
    exe = str(tmp_path / "place_text_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "place_text_check.cpp"),
                           os.path.join(ROOT, "sweepga_amd", "csrc", "host", "place_text.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"ok": True, "failures": 0}
