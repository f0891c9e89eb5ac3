"""The lift slices on the device (sweepga_amd/csrc/swg_slice.hip) against tests/lift_paf_model.py: in every case the host seam
against the model and the device seam against the host seam, slice for slice and byte for byte.  The shapes are the smallest at which
each part can go wrong: clips inside one op and on every edge of short CIGARs, every bad state beside intact neighbours, the borders
of the build's parse tile and rank chunks, the borders of the text kernel's tile (its size read from the library), the capacity
protocol; then the texts of swg_paf_lift_paf_text / _write / LiftPaf / --lift-paf byte for byte and fed back into the chain writer.
Every comparison is exact: integers and bytes."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import lift_exact_model as lem
from tests import lift_model as lm
from tests import lift_paf_model as pm
from tests.test_gpu_lift import Dev
from tests.test_gpu_lift_exact import filler, records_of, regions_over
from tests.test_gpu_wide import Hip

pytestmark = pytest.mark.gpu
COLS = lm.COLS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARSE_TILE = 4096      # text bytes per tile of the build's parser


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


@pytest.fixture(scope="module")
def T(sw):
    from sweepga_amd import lift
    return lift.slice_text_tile()


def same(a, b):
    return a.counts == b.counts and a.slices.tobytes() == b.slices.tobytes() and a.text == b.text and a.state.tobytes() == b.state.tobytes()


def both_seams(sw, cols, strand, n_seq, regions, cig, status=None, set_=0, axes=3, min_aligned=1, shift=0):
    """The result of the host seam, after checking that the device seam gives the same.  shift: the device text starts that many
    bytes behind a 16-byte boundary."""
    from sweepga_amd.lift import cigar_set, lift_slice_records, lift_slice_records_device, regions_array
    ctx = sw.default_context()
    recs = sorted(cig)
    got = lift_slice_records(ctx, cols, strand, n_seq, regions, recs, [cig[i] for i in recs], status=status, set=set_, axes=axes, min_aligned=min_aligned)
    regs = regions_array(regions)
    record, offset, text = cigar_set(recs, [cig[i] for i in recs])
    hip = Hip()
    try:
        dcols = {k: Dev(hip, cols[k], np.uint32) for k in COLS}
        dtext = Dev(hip, np.concatenate([np.zeros(shift, dtype=np.uint8), text]))
        dtext.ptr += shift
        dev = lift_slice_records_device(ctx, dcols, Dev(hip, strand, np.uint8), n_seq, Dev(hip, regs.view(np.uint32)), len(regs), Dev(hip, record),
                                        Dev(hip, offset), dtext, len(recs), status=Dev(hip, status, np.uint8) if status is not None else None, set=set_,
                                        axes=axes, min_aligned=min_aligned)
    finally:
        hip.free()
    assert same(dev, got)
    return got


def check(sw, cols, strand, n_seq, regions, cig, status=None, set_=0, axes=3, min_aligned=1, what="", shift=0):
    """Both seams against the model."""
    cols = {k: np.asarray(cols[k]).astype(np.uint32) for k in COLS}
    strand = np.asarray(strand).astype(np.uint8)
    got = both_seams(sw, cols, strand, n_seq, regions, cig, status, set_, axes, min_aligned, shift)
    slices, texts, counts, states = pm.lift_slices(cols, strand, None if status is None else np.asarray(status) != 0, regions, cig, set_, axes, min_aligned)
    counts["ops"] = sum(sum(ch not in "0123456789" for ch in t) for t in cig.values())
    assert got.counts == counts, (what, got.counts, counts)
    want = pm.slices_array(slices)
    if got.slices.tobytes() != want.tobytes():
        bad = [k for k in range(len(slices)) if got.slices[k].tobytes() != want[k].tobytes()]
        raise AssertionError((what, len(bad), [(tuple(got.slices[k]), slices[k]) for k in bad[:5]]))
    if got.text != "".join(texts).encode():
        bad = [k for k in range(len(slices)) if got.cigar(k) != texts[k]]
        raise AssertionError((what, len(bad), [(got.cigar(k), texts[k]) for k in bad[:5]]))
    assert got.state.tolist() == [states[i] for i in sorted(cig)], what
    return got


def test_clips_inside_one_op(sw):
    """`100=` cut to `7=` (a head number with fewer digits), a 10-digit op cut to 10 and to 9 digits, both strands, both axes."""
    for strand in (0, 1):
        cols = {"q_id": [0, 0], "t_id": [1, 2], "q_start": [50, 200], "q_end": [150, 3000000200], "t_start": [1000, 7], "t_end": [1100, 3000000007]}
        cig = {0: "100=", 1: "3000000000M"}
        regions = [(1, 1010, 1017), (0, 60, 67), (0, 149, 150), (2, 8, 2000000008), (2, 2999999000, 3000000007), (0, 201, 3000000200), (0, 1234, 1235),
                   (0, 0, 2**32 - 1)]
        got = check(sw, cols, [strand, strand], 3, regions, cig, what="one op, strand %d" % strand)
        assert [got.cigar(k) for k in range(3)] == ["7=", "7=", "1="] and got.cigar(3) == "2000000000M" and got.cigar(4) == "1007M"
        assert got.cigar(5) == "2999999999M" and got.cigar(6) == "1M" and [got.cigar(7), got.cigar(8)] == ["100=", "3000000000M"]
        assert (got.slices["flags"] & 8).tolist() == [8, 8, 8, 0, 0, 0, 0, 8, 0]


EDGE_TEXTS = ["5=3I5=", "5=3D2N5=", "2S3=0I1H02X0D4=5S", "3I4=2I3D2=1I", "0M2D0=3M0P", "7M", "1=1X1=1I1D1=", "4N", "2I", "0=3I0X"]


@pytest.mark.parametrize("axes", [1, 2])
def test_every_clip_of_short_cigars(sw, axes):
    """Every clip [a, b) over records of a few ops: edges on an I, a D and an N (the slice trims to the columns, block leaves the
    trimmed gap out), clips over inserted or deleted bases only (empty), zero-length ops and S, H, P at the ends and in between,
    M-only entries, entries without a column; both strands.  Then the partition: adjacent regions sum to the whole record's slice."""
    rng = np.random.default_rng(40 + axes)
    texts = EDGE_TEXTS * 2
    cols, strand = records_of(texts, rng, strands=[0] * len(EDGE_TEXTS) + [1] * len(EDGE_TEXTS))
    seq = axes - 1
    top = int((cols["t_end"] if seq else cols["q_end"]).max())
    regions = [(seq, a, b) for a in range(top + 1) for b in range(a + 1, min(a + 14, top + 1))]
    got = check(sw, cols, strand, 2, regions, dict(enumerate(texts)), axes=axes, what="every clip")
    assert got.counts["n_empty"] > 50 and got.counts["n_slices"] > 500
    cuts = sorted({0, top, *(int(v) for v in rng.integers(0, top, 12))})
    parts = check(sw, cols, strand, 2, [(seq, a, b) for a, b in zip(cuts, cuts[1:])] + [(seq, 0, top)], dict(enumerate(texts)), axes=axes, what="partition")
    whole = parts.slices[parts.slices["region"] == len(cuts) - 1]
    for w in whole:
        mine = parts.slices[(parts.slices["record"] == w["record"]) & (parts.slices["region"] < len(cuts) - 1)]
        assert int(mine["aligned"].sum()) == int(w["aligned"]) and int(mine["matches"].sum()) == int(w["matches"])
        order = mine["t_start"].argsort()
        assert (mine["t_end"][order][:-1] <= mine["t_start"][order][1:]).all()
    assert len(whole) == 2 * (len(EDGE_TEXTS) - 3)


def test_min_aligned_around_a_slice(sw):
    cols = {"q_id": [0], "t_id": [1], "q_start": [100], "q_end": [130], "t_start": [500], "t_end": [531]}
    cig, regions = {0: "10=2I5X3D13="}, [(1, 505, 520), (0, 110, 112)]       # 12 aligned columns; inserted bases only
    for m, n in ((0, 1), (1, 1), (11, 1), (12, 1), (13, 0), (2**32 - 1, 0)):
        got = check(sw, cols, [0], 2, regions, cig, min_aligned=m, what="min_aligned %d" % m)
        assert (got.counts["n_slices"], got.counts["n_short"], got.counts["n_empty"]) == (n, 1 - n, 1)
        assert got.text == (b"5=2I5X3D2=" if n else b"")


def test_both_strands_both_axes_and_a_record_of_one_sequence(sw):
    """A record with q_id == t_id is hit on both axes by one region; the kept set; every axes mask."""
    rng = np.random.default_rng(42)
    texts = [pm.random_cigar(rng, 12)[0] for _ in range(40)]
    texts = [t for t in texts if lem.entry_state(t, *lem.advances(lem.parse(t)[1])) == 0]
    cols, strand = records_of(texts, rng)
    n = len(texts)
    cols["t_id"][:] = 0                      # every record lies on one sequence, its two sides apart
    cols["t_start"] += 5000
    cols["t_end"] += 5000
    status = (np.arange(n) % 3 != 0).astype(np.uint8)
    regions = [(0, 0, 2**32 - 1), (0, 10, 5040)] + [(0, int(a), int(a) + int(w)) for a, w in zip(rng.integers(0, 5400, 80), rng.integers(1, 60, 80))]
    for set_, axes in ((0, 3), (1, 3), (0, 1), (1, 2)):
        got = check(sw, cols, strand, 1, regions, dict(enumerate(texts)), status=status, set_=set_, axes=axes, what="one sequence %d %d" % (set_, axes))
        if axes == 3:
            whole = got.slices[got.slices["region"] == 0]
            assert sorted(whole["flags"] & 2) == [0] * (len(whole) // 2) + [2] * (len(whole) // 2) and len(whole) == 2 * (n if set_ == 0 else int(status.sum()))


def test_bad_entries_and_records_without_an_entry_beside_intact_neighbours(sw):
    rng = np.random.default_rng(43)
    faulty = [("5=x5=", lem.SYNTAX), ("3=4294967296D", lem.VALUE), ("12345678901M", lem.SYNTAX), ("4294967296D5", lem.SYNTAX | lem.VALUE), ("", lem.EMPTY)]
    texts = []
    for f, _ in faulty:
        texts += [filler(int(rng.integers(2, 40)), rng), f]
    texts += [filler(24, rng), "9=", "9=", filler(30, rng), filler(12, rng)]
    cols, strand = records_of(texts, rng)
    k = 2 * len(faulty)
    cols["q_end"][k + 1] += 1                # the query sum, the target sum, both
    cols["t_end"][k + 2] += 1
    cig = dict(enumerate(texts))
    del cig[k + 3]                           # a record without an entry
    got = check(sw, cols, strand, 2, regions_over(cols, rng, 300, 30), cig, what="bad entries")
    assert got.state[1:k:2].tolist() == [s for _, s in faulty] and got.state[k + 1:k + 3].tolist() == [lem.Q_SUM, lem.T_SUM]
    assert got.counts["cigar_bad"] == 6 and got.counts["n_interp"] > 20 and not got.state[0:k:2].any()
    seen = set(got.slices["record"].tolist())
    assert seen <= set(range(0, k, 2)) | {k, k + 4} and len(seen) >= k // 2          # the neighbours of the bad ones are sliced
    # a set of empty entries, and no set at all (host seam): every row is counted interp
    got = check(sw, cols, strand, 2, regions_over(cols, rng, 50, 30), {i: "" for i in range(0, len(texts), 2)}, what="no usable entry")
    assert got.counts["n_interp"] == got.counts["n_rows"] > 0 and got.counts["n_slices"] == 0 and got.text == b""
    from sweepga_amd.lift import lift_slice_records
    none = lift_slice_records(sw.default_context(), cols, strand, 2, regions_over(cols, rng, 50, 30), [], [])
    assert none.counts["n_interp"] == none.counts["n_rows"] > 0 and none.counts["n_slices"] == none.counts["ops"] == 0 and none.text == b""


@pytest.mark.parametrize("shift", [0, 5])
def test_borders_of_the_build(sw, shift):
    """Entries that straddle the parser's tiles of 4,096 bytes, and op letters on every byte of a 16-byte rank chunk (the entries'
    lengths run through every residue); the device text on and off a 16-byte boundary."""
    rng = np.random.default_rng(44 + shift)
    texts = [filler(PARSE_TILE - 7, rng), filler(30, rng), filler(PARSE_TILE + 3, rng)] + [filler(17 + k, rng) for k in range(40)] + [filler(2 * PARSE_TILE, rng)]
    cols, strand = records_of(texts, rng)
    got = check(sw, cols, strand, 2, regions_over(cols, rng, 400, 600), dict(enumerate(texts)), what="build borders", shift=shift)
    assert not got.state.any() and got.counts["n_slices"] > 300 and int(got.slices["text_len"].max()) > 2 * PARSE_TILE - 200


def whole_entries(lengths, rng):
    """Entries of exactly these lengths whose first and last ops are aligned and one base long: a region over the whole record gives
    the entry's own text as the slice's"""
    return ["1=" + (filler(n - 4, rng) if n >= 6 else "") + "1X" if n >= 4 else "1=" for n in lengths]


def test_borders_of_the_text_tile(sw, T):
    """A slice longer than three tiles, a slice ending on a tile's last byte, more slices in one tile than a work-group has threads,
    and a text of one tile and of one tile plus a byte."""
    rng = np.random.default_rng(45)
    for lengths, what in (([3 * T + 101, 7, T - 108], "a slice longer than three tiles, the last ending on a border"),
                          ([T - 2] + [2] * 700 + [T - 1398, 9], "a slice ending on a tile's last byte, 700 slices in the next tile"),
                          ([T], "one tile"), ([T + 1], "one tile and a byte"), ([2] * (T // 2), "a tile of two-byte slices"), ([2] * (T // 2) + [2], "... and one more")):
        texts = whole_entries(lengths, rng)
        assert [len(t) for t in texts] == lengths
        cols, strand = records_of(texts, rng, strands=[0] * len(texts))
        got = check(sw, cols, strand, 2, [(0, 0, 2**32 - 1)], dict(enumerate(texts)), axes=1, what=what)
        assert got.text == "".join(texts).encode() and got.slices["text_first"].tolist() == np.cumsum([0] + lengths[:-1]).tolist(), what
        assert len(got.text) % T in (0, 1, 2, 9), what
    # the same tiles cut by clips: shortened heads and tails in front of and behind the verbatim ranges
    texts = whole_entries([3 * T + 50, 40, T + 7, 2 * T - 3], rng)
    cols, strand = records_of(texts, rng)
    got = check(sw, cols, strand, 2, regions_over(cols, rng, 40, 3 * T), dict(enumerate(texts)), what="clips over tiles")
    assert got.counts["text_bytes"] > 10 * T


def test_capacities_with_poisoned_arrays(sw):
    """text NULL, slices NULL, a capacity one short on each: the counts are right and nothing is written."""
    from sweepga_amd import _lib
    from sweepga_amd.lift import SLICE_DTYPE, cigar_set, regions_array
    ctx = sw.default_context()
    rng = np.random.default_rng(46)
    texts = [filler(int(n), rng) for n in rng.integers(10, 80, 30)]
    cols, strand = records_of(texts, rng)
    regions = regions_over(cols, rng, 60, 50)
    want = check(sw, cols, strand, 2, regions, dict(enumerate(texts)), what="capacities")
    n, nbytes = want.counts["n_slices"], want.counts["text_bytes"]
    assert n > 20
    rec = _lib.SwgRecords()
    rec.n, rec.n_seq, rec.strand = len(strand), 2, strand.ctypes.data
    for k in COLS:
        setattr(rec, k, cols[k].ctypes.data)
    regs = regions_array(regions)
    record, offset, text = cigar_set(range(len(texts)), texts)
    cs = _lib.SwgCigarSet()
    cs.record, cs.offset, cs.text, cs.k = record.ctypes.data, offset.ctypes.data, text.ctypes.data, len(texts)
    for slice_cap, text_cap, give_slices, give_text in ((n, nbytes, True, False), (n, nbytes, False, True), (n - 1, nbytes, True, True),
                                                        (n, nbytes - 1, True, True), (0, 0, True, True), (n + 3, nbytes + 5, True, True)):
        slices = np.full(n + 3, 0xab, dtype=np.uint8).repeat(56).view(SLICE_DTYPE)
        out = np.full(nbytes + 5, 0xab, dtype=np.uint8)
        req = _lib.SwgLiftSliceRequest()
        req.set, req.axes, req.min_aligned = 0, 3, 1
        req.slice_capacity, req.slices = slice_cap, slices.ctypes.data if give_slices else None
        req.text_capacity, req.text = text_cap, out.ctypes.data if give_text else None
        ctx.check(ctx.lib.swg_lift_slice_records(ctx.handle, C.byref(rec), None, regs.ctypes.data, len(regs), C.byref(cs), C.byref(req)))
        assert {k: int(getattr(req, k)) for k in want.counts} == want.counts
        if give_slices and slice_cap >= n:
            assert slices[:n].tobytes() == want.slices.tobytes() and (slices[n:].view(np.uint8) == 0xab).all()
        else:
            assert (slices.view(np.uint8) == 0xab).all()
        if give_text and text_cap >= nbytes:
            assert out[:nbytes].tobytes() == want.text and (out[nbytes:] == 0xab).all()
        else:
            assert (out == 0xab).all()


def test_refusals(sw):
    from sweepga_amd import SwgError
    from sweepga_amd.lift import lift_slice_records
    ctx = sw.default_context()
    cols = {k: np.array(v, dtype=np.uint32) for k, v in (("q_id", [0, 0]), ("t_id", [1, 1]), ("q_start", [0, 10]), ("q_end", [5, 15]), ("t_start", [0, 10]), ("t_end", [5, 15]))}
    strand = np.zeros(2, dtype=np.uint8)
    for kw, recs in (({"set": 2}, [0, 1]), ({"axes": 0}, [0, 1]), ({"set": "kept"}, [0, 1]), ({}, [1, 0]), ({}, [0, 2])):
        with pytest.raises(SwgError):
            lift_slice_records(ctx, cols, strand, 2, [(0, 0, 20)], recs, ["5=", "5="], **kw)
    with pytest.raises(SwgError):
        lift_slice_records(ctx, cols, strand, 2, [(7, 0, 20)], [0, 1], ["5=", "5="])
    got = lift_slice_records(ctx, cols, strand, 2, [], [0, 1], ["5=", "5x"])      # no region: the set is still parsed
    assert got.counts["n_rows"] == 0 and got.state.tolist() == [0, 1] and got.counts["cigar_bad"] == 1 and got.counts["ops"] == 2


def paf_of(cols, strand, texts, names=("q#1#a", "t#1#b", "u#1#c"), lens=(4_000_000_000, 4_000_000_001, 4_000_000_002)):
    lines = []
    for i, text in enumerate(texts):
        f = [names[cols["q_id"][i]], lens[cols["q_id"][i]], cols["q_start"][i], cols["q_end"][i], "-" if strand[i] else "+", names[cols["t_id"][i]],
             lens[cols["t_id"][i]], cols["t_start"][i], cols["t_end"][i], 1 + i % 50, 60 + i % 7, i % 61]
        lines.append("\t".join([str(v) for v in f] + (["tp:A:P", "cg:Z:" + text, "nm:i:%d" % i] if i % 5 else ["cg:Z:" + text])))
    return "\n".join(lines) + "\n"


def test_texts_of_an_open_paf_for_every_batch_size(sw, tmp_path, T):
    """swg_paf_lift_paf_text with batch_bytes of 1, of a small prime and of the default: identical bytes, the model's; the file of
    swg_paf_lift_paf_write; two calls give the same bytes.  Then the three consequences on the device's output: the text opened
    as a PAF goes through the chain writer without a bad entry, and every line re-lifted through itself gives itself."""
    rng = np.random.default_rng(47)
    texts = whole_entries([T + 30, 60, 2 * T + 1], rng) + [filler(int(n), rng) for n in rng.integers(10, 200, 60)] + ["30M", "10M5D10M"]
    cols, strand = records_of(texts, rng)
    text = paf_of(cols, strand, texts)
    bed_text = "# genes\n" + "".join("%s\t%d\t%d%s\n" % (("q#1#a", "t#1#b", "absent")[k % 3 if k % 10 else 2], a, a + w, "\tgene%d" % k if k % 4 else "")
                                     for k, (a, w) in enumerate(zip(rng.integers(0, 11_000, 90), np.where(np.arange(90) % 3 == 0, rng.integers(1, 4, 90), rng.integers(0, 900, 90)))))
    bed_text += "q#1#a\t0\t4294967295\twhole\n"
    status = (np.arange(len(texts)) % 4 != 1).astype(np.uint8)
    out = tmp_path / "genes.paf"
    with sw.PafFile(text=text) as paf:
        for set_, axes, m in ((1, 3, 1), (0, 1, 1), (0, 2, 25)):
            want, want_counts = pm.paf_text(text, status != 0, bed_text, set_, axes, m)
            assert want.count("\n") > 40 and (want_counts["empty"] > 0 if m == 1 else want_counts["too_short"] > 0)
            seen = set()
            for batch in (0, 1, 997, 50_000):
                got = sw.LiftPaf.from_paf(paf, status, bed_text, set=set_, axes=axes, min_aligned=m, batch_bytes=batch)
                assert got.text == want, (set_, axes, m, batch)
                assert {k: got.counts[k] for k in want_counts} == want_counts
                seen.add(got.counts["batches"])
            assert len(seen) >= 3                                                       # the batch sizes did cut the BED differently
            assert sw.LiftPaf.from_paf(paf, status, bed_text, set=set_, axes=axes, min_aligned=m).text == want      # determinism
            counts = sw.LiftPaf.write_paf(paf, status, bed_text, out, set=set_, axes=axes, min_aligned=m, batch_bytes=997)
            assert out.read_text() == want and {k: counts[k] for k in want_counts} == want_counts
        got = sw.LiftPaf.from_paf(paf, None, bed_text, set="all")
    rows = got.rows()
    assert any(r[9] != r[10] for r in rows) and {"rn:Z:whole", "rn:Z:gene1"} <= {r[13] for r in rows}
    m_only = [r for r in rows if r[14] in ("ri:i:%d" % (len(texts) - 2), "ri:i:%d" % (len(texts) - 1))]
    assert m_only and all("=" not in r[12] and r[9] == sum(int(d) for d, ch in pm.tokens(r[12][5:]) if ch == "M") for r in m_only)   # col10 = aligned
    with sw.PafFile(text=got.text) as sliced:
        assert sliced.n == len(rows)
        chains = sw.UcscChain.from_paf(sliced, None, set="all")
        assert chains.counts["bad"] == 0 and chains.counts["beyond"] == 0 and chains.counts["chains"] == len(rows)
    for r in rows:
        minus, cg, rec = r[4] == "-", r[12][5:], (r[2], r[3], r[7], r[8])
        assert lem.entry_state(cg, r[3] - r[2], r[8] - r[7]) == 0
        for axis in (0, 1):
            again = pm.slice_row(cg, axis, minus, *((r[7], r[8]) if axis else (r[2], r[3])), *rec)
            assert (again["q_start"], again["q_end"], again["t_start"], again["t_end"], again["cigar"]) == (*rec, cg)
            # (col10 follows the ENTRY's '=' columns: a slice of X ops only, cut from an entry with '=' elsewhere, says 0 matches)
            assert again["block"] == r[10] and (r[9] == again["matches"] if again["has_eq"] else r[9] in (0, again["aligned"]))


def test_command_line_round_trip_on_the_golden_paf(sw, tmp_path):
    """--lift-paf on tests/golden/syeast.paf.gz (its lines carry cg:Z:), the model's bytes; the file goes through --ucsc-chain with no
    bad entry; the filtered PAF is the one a run without the option writes."""
    from sweepga_amd import build
    from tests.test_gpu_intervals import kept_mask
    text = gzip.open(os.path.join(ROOT, "tests", "golden", "syeast.paf.gz"), "rb").read().decode()
    assert "cg:Z:" in text
    bed_text = ("S288C#1#chrI\t1000\t9000\tgeneA\nSGDref#1#chrI\t20000\t21500\nS288C#1#chrIV\t100000\t130000\tlong\nabsent\t5\t9\nSGDref#1#chrII\t0\t400\tedge\n"
                "S288C#1#chrII\t50000\t50001\tbase\n")
    inp, bed = tmp_path / "in.paf", tmp_path / "genes.bed"
    inp.write_text(text, newline="")
    bed.write_text(bed_text, newline="")
    plain, out, sliced, chain = (tmp_path / x for x in ("plain.paf", "out.paf", "genes.paf", "genes.chain"))
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), "--quiet"], capture_output=True)
    assert r0.returncode == 0 and plain.stat().st_size > 0, r0.stderr
    kept = kept_mask(text, plain.read_bytes().decode())
    want, counts = pm.paf_text(text, kept, bed_text, 1, 3, 20)
    assert want.count("\n") >= 4
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--lift-regions", str(bed), "--lift-paf", str(sliced), "--lift-paf-min-aligned", "20",
                        "--lift-batch", "20k"], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"" and out.read_bytes() == plain.read_bytes(), r.stderr
    assert sliced.read_text() == want
    assert ("--lift-paf: %d lines of %d rows, %d without a usable CIGAR, %d without an aligned column, %d below" %
            (counts["slices"], counts["rows"], counts["interp"], counts["empty"], counts["too_short"])).encode() in r.stderr
    r = subprocess.run([build.CLI, str(sliced), "--output-file", str(tmp_path / "again.paf"), "--no-filter", "--ucsc-chain", str(chain)], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert ("--ucsc-chain: %d chains of %d records" % (counts["slices"], counts["slices"])).encode() in r.stderr and b" 0 bad, 0 beyond" in r.stderr
    assert chain.read_text().count("chain ") == counts["slices"]
