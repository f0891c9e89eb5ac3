"""The lift slices without a GPU: the brute-force model of tests/lift_paf_model.py against lines worked out by hand and against the
three consequences of the definitions on random CIGARs, and the host side of the feature -- header, ctypes mirrors, exported symbols,
the no-device paths and refusals of swg_paf_lift_paf_write / _text, the usage errors of --lift-paf, and the rules header, the line
writer and the batch planner under the host sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import lift_exact_model as lem
from tests import lift_model as lm
from tests import lift_paf_model as pm
from tests.test_lift_cpu import REBASED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_model_against_lines_worked_out_by_hand():
    assert pm.paf_text(pm.HAND_PAF, None, pm.HAND_BED, 0, 3) == (pm.HAND_TEXT, pm.HAND_COUNTS)
    # one axis only: the query-side regions have no hit on the target axis
    text, counts = pm.paf_text(pm.HAND_PAF, None, pm.HAND_BED, 0, 2)
    assert text == "".join(ln + "\n" for ln in pm.HAND_TEXT.split("\n") if "rn:Z:geneT" in ln or "rn:Z:r2" in ln) and counts["rows"] == 2
    # min_aligned at aligned - 1, aligned, aligned + 1 of the five-column slice
    for m, n, short in ((4, 2, 1), (5, 2, 1), (6, 1, 2)):
        t, c = pm.paf_text(pm.HAND_PAF, None, pm.HAND_BED, 0, 3, m)
        assert (c["slices"], c["too_short"], c["empty"]) == (n, short, 1) and ("rn:Z:r2" in t) == (m <= 5)
    S = pm.slice_row
    # inside one op; a head number with fewer digits; the clip's edge on an I, a D and an N: trimmed, block without the trimmed gap
    assert S("100=", 1, 0, 1010, 1017, 0, 100, 1000, 1100)["cigar"] == "7="
    assert S("3000000000=", 1, 0, 5, 2000000005, 0, 3000000000, 0, 3000000000) == {
        "q_start": 5, "q_end": 2000000005, "t_start": 5, "t_end": 2000000005, "aligned": 2000000000, "matches": 2000000000, "block": 2000000000,
        "cigar": "2000000000=", "has_eq": True}
    got = S("5=3I5=", 0, 0, 105, 109, 100, 113, 200, 210)                 # query 105 .. 108: the I; 100 + 8 = the first column behind it
    assert (got["cigar"], got["q_start"], got["q_end"], got["t_start"], got["t_end"], got["block"]) == ("1=", 108, 109, 205, 206, 1)
    got = S("5=3D2N5=", 1, 0, 203, 209, 100, 110, 200, 215)               # target 203, 204 are columns, 205 .. 208 deleted
    assert (got["cigar"], got["t_start"], got["t_end"], got["q_start"], got["q_end"], got["block"], got["aligned"]) == ("2=", 203, 205, 103, 105, 2, 2)
    assert S("5=3I5=", 0, 0, 105, 108, 100, 113, 200, 210) is None and S("5=3D5=", 1, 0, 205, 208, 100, 110, 200, 213) is None
    # zero-length ops and S, H, P between the two ends are copied as they stand, at the ends they are left out
    got = S("2S3=0I1H02X0D4=5S", 0, 0, 101, 108, 100, 109, 200, 209)
    assert (got["cigar"], got["aligned"], got["matches"], got["has_eq"]) == ("2=0I1H02X0D3=", 7, 5, True)
    assert S("4M", 0, 0, 0, 4, 0, 4, 0, 4)["has_eq"] is False and S("0=4M", 0, 0, 0, 4, 0, 4, 0, 4)["has_eq"] is False


def test_random_cigars_meet_the_three_consequences():
    """slice_row against every column listed; check_slice (state 0, the re-lift) on every slice; adjacent regions that partition the
    source side sum to the record's totals and neither overlap nor reorder."""
    rng = np.random.default_rng(35)
    checked = 0
    for trial in range(300):
        text, x, y = pm.random_cigar(rng, int(rng.integers(1, 25)))
        minus, axis = int(rng.integers(2)), int(rng.integers(2))
        q_start, t_start = int(rng.integers(0, 50)), int(rng.integers(0, 50))
        rec = (q_start, q_start + x, t_start, t_start + y)
        if lem.entry_state(text, x, y) != 0:
            continue
        s0, s1 = (rec[2], rec[3]) if axis else (rec[0], rec[1])
        cuts = sorted({s0, s1, *(int(v) for v in rng.integers(s0, s1 + 1, size=4))})
        total = pm.slice_row(text, axis, minus, s0, s1, *rec)
        parts = []
        for ca, cb in zip(cuts, cuts[1:]):
            got = pm.slice_row(text, axis, minus, ca, cb, *rec)
            want = pm.slice_expanded(text, axis, minus, ca, cb, *rec)
            assert (got is None) == (want is None)
            if got is None:
                continue
            assert tuple(got[k] for k in ("q_start", "q_end", "t_start", "t_end", "aligned", "matches", "block")) == want
            pm.check_slice(got, axis, minus)
            src = (got["t_start"], got["t_end"]) if axis else (got["q_start"], got["q_end"])
            assert ca <= src[0] < src[1] <= cb
            parts.append(got)
            checked += 1
        if total is None:
            assert not parts
            continue
        assert sum(p["aligned"] for p in parts) == total["aligned"] and sum(p["matches"] for p in parts) == total["matches"]
        for a, b in zip(parts, parts[1:]):      # along the source in order; along the other side in order on '+', reversed on '-'
            assert a["t_end"] <= b["t_start"] if (axis or not minus) else a["t_start"] >= b["t_end"]
            assert a["q_end"] <= b["q_start"] if (not axis or not minus) else a["q_start"] >= b["q_end"]
    assert checked > 500


@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib, lift
    structs = (("swg_lift_slice", _lib.SwgLiftSlice), ("swg_lift_slice_request", _lib.SwgLiftSliceRequest), ("swg_lift_paf_counts", _lib.SwgLiftPafCounts))
    prints = ['printf("%%zu\\n", sizeof(%s));' % name for name, _ in structs]
    prints += ['printf("%%zu\\n", offsetof(%s, %s));' % (name, f) for name, cls in structs for f, _ in cls._fields_]
    prints += ['printf("%u %u %d\\n", SWG_SLICE_HAS_EQ, SWG_SLICE_TEXT_TILE, SWG_ABI_VERSION);']
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(cls) for _, cls in structs] + [getattr(cls, f).offset for _, cls in structs for f, _ in cls._fields_]
    want += [8, lift.slice_text_tile(), 1]
    assert got == want
    assert got[:3] == [56, 120, 64]
    for _, cls in structs:      # no implicit padding
        assert sum(C.sizeof(t) for _, t in cls._fields_) == C.sizeof(cls)
    assert lift.SLICE_DTYPE.itemsize == 56 and lift.SLICE_DTYPE.names == pm.SLICE_FIELDS == tuple(f for f, _ in _lib.SwgLiftSlice._fields_)
    assert [lift.SLICE_DTYPE.fields[f][1] for f, _ in _lib.SwgLiftSlice._fields_] == [getattr(_lib.SwgLiftSlice, f).offset for f, _ in _lib.SwgLiftSlice._fields_]
    assert lift.SLICE_HAS_EQ == pm.HAS_EQ and lift.slice_text_tile() % 1024 == 0
    assert tuple(f for f, _ in _lib.SwgLiftPafCounts._fields_) == lift.PAF_COUNTS
    assert tuple(f for f, _ in _lib.SwgLiftSliceRequest._fields_[-8:]) == lift.SLICE_COUNTS


def test_symbols_are_exported_and_declared(lib):
    import sweepga_amd
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_lift_slice_records", "swg_lift_slice_records_device", "swg_lift_slice_text_tile", "swg_paf_lift_paf_write", "swg_paf_lift_paf_text"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    for name in ("LiftPaf", "LiftSliceResult", "lift_slice_records", "lift_slice_records_device"):
        assert hasattr(sweepga_amd, name)


def paf_text(lib, paf, status, bed, set_=0, axes=3, min_aligned=1, batch=0, ctx=None):
    """swg_paf_lift_paf_text -> (rc, text or None, counts)"""
    from sweepga_amd import _lib, lift
    counts, p, n = _lib.SwgLiftPafCounts(), C.c_void_p(77), C.c_uint64(77)
    rc = lib.swg_paf_lift_paf_text(ctx, paf.handle, status.ctypes.data if status is not None else None, bed, len(bed), set_, axes, min_aligned, batch,
                                   C.byref(counts), C.byref(p), C.byref(n))
    text = None
    if p.value:
        text = C.string_at(p.value, n.value).decode()
        lib.swg_free(p)
    else:
        assert n.value == 0
    return rc, text, {k: int(getattr(counts, k)) for k in lift.PAF_COUNTS}


def test_paf_seams_without_a_device(lib, tmp_path):
    """An empty BED or a PAF without records gives an empty file and text and needs no device; the refusals and a malformed BED come
    before a context is looked at, and before the file is touched."""
    from sweepga_amd import LiftPaf, PafFile, SwgError, lift
    zero = {k: 0 for k in lift.PAF_COUNTS}
    out = tmp_path / "x.paf"
    bed = pm.HAND_BED.encode()
    for text in ("", "# nothing\nfew\tfields\n"):
        with PafFile(text=text) as paf:
            for st in (None, np.zeros(1, dtype=np.uint8)):
                assert paf_text(lib, paf, st, bed) == (0, "", zero)
                assert paf_text(lib, paf, st, bed, axes=1, min_aligned=9, batch=5) == (0, "", zero)
            out.write_text("stale")
            assert LiftPaf.write_paf(paf, None, pm.HAND_BED, out, set="all") == zero and out.read_bytes() == b""
            got = LiftPaf.from_paf(paf, None, pm.HAND_BED, set="all")
            assert (got.text, got.counts, got.rows()) == ("", zero, [])
    with PafFile(text=pm.HAND_PAF) as paf:
        st = np.ones(paf.n, dtype=np.uint8)
        for empty in (b"", b"# only a comment\n\ntrack name=x\n"):
            assert paf_text(lib, paf, st, empty, set_=1) == (0, "", zero)
        assert lib.swg_paf_lift_paf_write(None, paf.handle, None, b"", 0, 0, 3, 1, 0, str(out).encode(), None) == 0 and out.read_bytes() == b""   # counts may be NULL
        out.write_text("stale")
        rc, t, _ = paf_text(lib, paf, st, bed, set_=1)
        assert rc == -1 and t is None and b"swg_paf_lift_paf_text: NULL context" in lib.swg_alnstats_last_error()
        for set_, axes, word in ((2, 3, b"set"), (0, 0, b"axes"), (1, 4, b"axes")):
            rc, t, _ = paf_text(lib, paf, st, bed, set_=set_, axes=axes)
            assert rc == -1 and t is None and word in lib.swg_alnstats_last_error()
            assert lib.swg_paf_lift_paf_write(None, paf.handle, st.ctypes.data, bed, len(bed), set_, axes, 1, 0, str(out).encode(), None) == -1
            assert out.read_text() == "stale"
        assert paf_text(lib, paf, None, bed, set_=1)[0] == -1 and b"status" in lib.swg_alnstats_last_error()
        for bad, line in ((b"tB\t5\n", 1), (b"tB\t1\t2\n\ntB\t9\t3\n", 3), (b"tB\t1\t4294967296\n", 1)):
            rc, t, _ = paf_text(lib, paf, st, bad)
            assert rc == -1 and t is None and ("swg_paf_lift_paf_text: BED line %d:" % line).encode() in lib.swg_alnstats_last_error()
            assert lib.swg_paf_lift_paf_write(None, paf.handle, st.ctypes.data, bad, len(bad), 0, 3, 1, 0, str(out).encode(), None) == -1
            assert out.read_text() == "stale"
        assert lib.swg_paf_lift_paf_write(None, paf.handle, st.ctypes.data, b"", 0, 0, 3, 1, 0, str(tmp_path / "no" / "dir.paf").encode(), None) == -1
        assert b"cannot open" in lib.swg_alnstats_last_error()
        p, n = C.c_void_p(), C.c_uint64()
        assert lib.swg_paf_lift_paf_text(None, None, None, b"", 0, 0, 3, 1, 0, None, C.byref(p), C.byref(n)) == -1
        assert lib.swg_paf_lift_paf_text(None, paf.handle, None, b"", 0, 0, 3, 1, 0, None, None, C.byref(n)) == -1
        assert lib.swg_paf_lift_paf_text(None, paf.handle, None, None, 5, 0, 3, 1, 0, None, C.byref(p), C.byref(n)) == -1
        assert lib.swg_paf_lift_paf_write(None, paf.handle, None, b"", 0, 0, 3, 1, 0, None, None) == -1
        with pytest.raises(SwgError):
            LiftPaf.from_paf(paf, st, pm.HAND_BED, set=2)
    with PafFile(text=REBASED) as paf:
        with pytest.raises(SwgError) as e:
            LiftPaf.from_paf(paf, np.ones(1, dtype=np.uint8), "x\t1\t2\n")
        assert e.value.code == -6 and "2^32" in str(e.value)
        out.write_text("stale")
        with pytest.raises(SwgError):
            LiftPaf.write_paf(paf, np.ones(1, dtype=np.uint8), "x\t1\t2\n", out)
        assert out.read_text() == "stale"


def test_record_seams_refuse_without_a_device(lib):
    """A NULL context: there is no CPU path, and nothing the caller owns is touched."""
    from sweepga_amd import _lib
    from sweepga_amd.lift import cigar_set, regions_array
    cols, strand, _ = lm.parse_paf(pm.HAND_PAF)
    rec = _lib.SwgRecords()
    rec.n = len(strand)
    for k, a in cols.items():
        setattr(rec, k, a.ctypes.data)
    rec.strand, rec.n_seq = strand.ctypes.data, 2
    regs = regions_array([(1, 505, 520)])
    record, offset, text = cigar_set([0, 1], ["10=2I5X3D13=", "4M2D6M"])
    cs = _lib.SwgCigarSet()
    cs.record, cs.offset, cs.text, cs.k = record.ctypes.data, offset.ctypes.data, text.ctypes.data, 2
    poison = np.full(56 * 2, 0xab, dtype=np.uint8)
    for fn in (lib.swg_lift_slice_records, lib.swg_lift_slice_records_device):
        req = _lib.SwgLiftSliceRequest()
        req.set, req.axes = 0, 3
        req.slice_capacity, req.slices, req.n_slices, req.text_bytes = 2, poison.ctypes.data, 12345, 77
        assert fn(None, C.byref(rec), None, regs.ctypes.data, 1, C.byref(cs), C.byref(req)) == -1
        assert (poison == 0xab).all() and req.n_slices == 12345 and req.text_bytes == 77


def test_command_line_usage_errors(lib, tmp_path):
    from sweepga_amd import build
    paf, bed = tmp_path / "in.paf", tmp_path / "genes.bed"
    paf.write_text(pm.HAND_PAF)
    bed.write_text(pm.HAND_BED)
    out, sliced = tmp_path / "out.paf", tmp_path / "genes.paf"
    run = lambda *a: subprocess.run([build.CLI, str(paf), "--output-file", str(out), *a], capture_output=True, text=True)      # noqa: E731
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(w in r.stdout for w in ("--lift-paf FILE", "--lift-paf-min-aligned N", "--lift-batch BYTES"))
    regions = ["--lift-regions", str(bed)]
    cases = [(["--lift-paf", str(sliced)], "need --lift-regions"), (["--lift-paf-min-aligned", "5"], "need --lift-regions"),
             (["--lift-batch", "4k"], "need --lift-regions"),
             (regions + ["--lift", str(tmp_path / "rows.tsv"), "--lift-batch", "4k"], "need --lift-paf"),
             (regions + ["--lift", str(tmp_path / "rows.tsv"), "--lift-paf-min-aligned", "3"], "need --lift-paf"),
             (regions + ["--lift-paf", str(sliced), "--lift-paf-min-aligned", "0"], "--lift-paf-min-aligned"),
             (regions + ["--lift-paf", str(sliced), "--lift-paf-min-aligned", "4294967296"], "--lift-paf-min-aligned"),
             (regions + ["--lift-paf", str(sliced), "--lift-batch", "0"], "--lift-batch"),
             (regions + ["--lift-paf", str(sliced), "--lift-batch", "many"], "--lift-batch"),
             (regions + ["--lift-paf", "-"], "not a standard error report"), (regions + ["--lift-paf", ""], "empty value for --lift-paf"),
             (regions, "--lift-regions needs"),
             (["--lift-regions", str(tmp_path / "missing.bed"), "--lift-paf", str(sliced)], "cannot open")]
    bad_bed = tmp_path / "bad.bed"
    bad_bed.write_text("tB\t9\t3\n")
    cases.append((["--lift-regions", str(bad_bed), "--lift-paf", str(sliced)], "BED line 1"))
    for extra, word in cases:
        r = run(*extra)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)
        assert r.stdout == "" and not out.exists() and not sliced.exists(), extra


def test_rules_header_under_the_host_sanitizers(tmp_path):
    """tests/native/slice_walk_check.cpp: swg_slice_walk.h on a CPU, built with the address and undefined-behaviour sanitizers, against
    the model on vectors the model prints."""
    exe = str(tmp_path / "slice_walk_check")
    subprocess.check_call(SAN + ["-o", exe, os.path.join(ROOT, "tests", "native", "slice_walk_check.cpp")])
    rng = np.random.default_rng(36)
    feed, want = [], []

    def case(text, axis, minus, ca, cb, rec):
        feed.append("%s %d %d %d %d %d %d %d" % (text, axis, minus, ca, cb, rec[0], rec[1], rec[2]))
        s = pm.slice_row(text, axis, minus, ca, cb, *rec)
        want.append("-" if s is None else "%d %d %d %d %d %d %d %d %s" % (s["q_start"], s["q_end"], s["t_start"], s["t_end"], s["aligned"], s["matches"],
                                                                        s["block"], int(s["has_eq"]), s["cigar"]))
    for trial in range(400):
        text, x, y = pm.random_cigar(rng, int(rng.integers(1, 20)), max_len=int(rng.choice([3, 9, 120])))
        if lem.entry_state(text, x, y) != 0:
            continue
        minus, axis = int(rng.integers(2)), int(rng.integers(2))
        q_start, t_start = int(rng.integers(0, 50)), int(rng.integers(0, 50))
        rec = (q_start, q_start + x, t_start, t_start + y)
        s0, s1 = (rec[2], rec[3]) if axis else (rec[0], rec[1])
        if s1 == s0:
            continue
        ca = int(rng.integers(s0, s1))
        cb = int(rng.integers(ca + 1, s1 + 1))
        case(text, axis, minus, ca, cb, rec)
        case(text, axis, minus, s0, s1, rec)
    top = 2**32 - 1
    case("4294967295=", 0, 0, 1, top, (0, top, 0, top))                   # 10-digit numbers at both ends of one op
    case("4000000000=5I294967290X", 1, 1, 3999999990, 4000000003, (0, top, 0, top - 5))
    case("1000000000M", 0, 1, 999999, 1000006, (0, 1000000000, 7, 1000000007))
    assert len(feed) > 500
    r = subprocess.run([exe], input=("\n".join(feed) + "\n").encode(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.decode().split("\n")[:-1] == want


def test_text_helpers_under_the_host_sanitizers(tmp_path):
    """tests/native/slice_text_check.cpp: the line writer and the batch planner of csrc/host/slice_text.cpp, built with the address and
    undefined-behaviour sanitizers; its answers must be the model's byte for byte."""
    exe = str(tmp_path / "slice_text_check")
    host = os.path.join(ROOT, "sweepga_amd", "csrc", "host")
    subprocess.check_call(SAN + ["-o", exe, os.path.join(ROOT, "tests", "native", "slice_text_check.cpp"), os.path.join(host, "slice_text.cpp"), "-lpthread"])
    top = 2**32 - 1
    feed, want = [], []
    # the hand-worked lines, then every field at its extreme, a record line with and without a line end and with further tags
    own = pm.HAND_PAF.split("\n")
    for ln, src in zip(pm.HAND_TEXT.split("\n")[:3], (own[0], own[0], own[1])):
        f = ln.split("\t")
        flags = (1 if f[4] == "-" else 0) | (8 if "=" in src else 0)
        aligned = {"geneT": 12, "qA:110-113": 1, "r2": 5}[f[13][5:]]
        feed += ["L", " ".join([f[2], f[3], f[7], f[8], str(flags), str(aligned), f[9] if flags & 8 else "0", f[10], f[14][5:], str(len(f[12]) - 5)]),
                 f[0], f[5], f[13][5:], f[12][5:] + "9=junk", src]
        want.append(ln + "\n")
    feed += ["L", " ".join(str(v) for v in (top, top, top, top, 3, top, 7, 2**64 - 1, top, 11)), "", "t t", "a\tlabel", "4294967295X", "q\t0\t1\t2\t-\tt\t%d\t3\t4\t5\t6\t255" % top]
    want.append("\t0\t%d\t%d\t-\tt t\t%d\t%d\t%d\t%d\t%d\t255\tcg:Z:4294967295X\trn:Z:a\tlabel\tri:i:%d\n" % (top, top, top, top, top, top, 2**64 - 1, top))
    feed += ["L", "1 2 3 4 8 9 7 5 0 2", "q", "t", "l", "1=", "q\t10\t1\t2\t+\tt\t20\t3\t4\t5\t6\t17\ttp:A:P\tcg:Z:1=\r"]
    want.append("q\t10\t1\t2\t+\tt\t20\t3\t4\t7\t5\t17\tcg:Z:1=\trn:Z:l\tri:i:0\n")

    def plan(batch, costs):
        first, held = [0], 0
        bound = batch if 0 < batch < top else top
        for r, v in enumerate(costs):
            if r > first[-1] and held + v > bound:
                first.append(r)
                held = 0
            held += v
        return first + ([len(costs)] if costs else [])
    rng = np.random.default_rng(37)
    for batch, costs in ((0, []), (0, [5, 6, 7]), (1, [5, 6, 7]), (11, [5, 6, 7]), (12, [5, 6, 1, 7, 0, 0, 30, 1]), (7, [0, 0, 0]), (top + 5, [top - 1, 1, 1]),
                         (0, [top, 1]), (13, [int(v) for v in rng.integers(0, 14, size=200)])):
        feed += ["P", " ".join(str(v) for v in [batch, len(costs)] + costs)]
        got = plan(batch, costs)
        want.append(" ".join(str(v) for v in got) + "\n")
        for a, b in zip(got, got[1:]):          # the planner's contract, on the model's answer
            assert b > a and (sum(costs[a:b]) <= (batch if 0 < batch < top else top) or b == a + 1)
    r = subprocess.run([exe], input=("\n".join(feed) + "\n").encode(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.decode() == "".join(want)
