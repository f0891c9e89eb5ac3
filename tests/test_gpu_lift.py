"""The lift on the device (sweepga_amd/csrc/swg_lift.hip) against tests/lift_model.py: in every case the host seam against the
model and the device seam against the host seam, row for row.  The shapes are the smallest at which each part can go wrong: the
tile of T = 1024 candidates and its borders, regions without candidates inside and across tiles, more region heads than a wavefront
in one tile, the binary searches' corners, the prefix-maximum prune, ties of the start, the largest values, the axes and sets, the
capacity protocol, permutations, breadth's shapes under a real 1:1 status, 10^5 random records, a memory limit, and the texts of
swg_paf_lift / Lift.from_paf / --lift byte for byte.  Every comparison is exact: integers and bytes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import lift_model as lm
from tests.test_gpu_alnstats import filter_cfgs, gen_text, records_of, run_filter
from tests.test_gpu_breadth import SHAPE_NAMES, shape_texts
from tests.test_gpu_intervals import kept_mask
from tests.test_gpu_wide import Hip
from tests.test_lift_cpu import HAND_BED, HAND_SUMMARY, hand_case, hand_paf

pytestmark = pytest.mark.gpu
COLS = lm.COLS
T = 1024
U = lm.UNKNOWN


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


class Dev:
    """A numpy array in device memory with what lift_records_device asks of a tensor."""

    def __init__(self, hip, a, dtype=None):
        self.a = np.ascontiguousarray(a, dtype=dtype)
        self.ptr = hip.up(self.a)

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.a.size

    def element_size(self):
        return self.a.itemsize

    def is_contiguous(self):
        return True


def same(a, b):
    return a.n == b.n and a.candidates == b.candidates and np.array_equal(a.summary, b.summary) and a.rows.tobytes() == b.rows.tobytes()


def both_seams(sw, cols, strand, n_seq, regions, status, set_=0, axes=3, ctx=None):
    """The result of the host seam, after checking that the device seam gives the same rows in the same order."""
    from sweepga_amd.lift import lift_records, lift_records_device, regions_array
    ctx = ctx or sw.default_context()
    got = lift_records(ctx, cols, strand, n_seq, regions, status=status, set=set_, axes=axes)
    regs = regions_array(regions)
    hip = Hip()
    try:
        dcols = {k: Dev(hip, cols[k], np.uint32) for k in COLS}
        dev = lift_records_device(ctx, dcols, Dev(hip, strand, np.uint8), n_seq, Dev(hip, regs.view(np.uint32)), len(regs),
                                  status=Dev(hip, status, np.uint8) if status is not None else None, set=set_, axes=axes)
    finally:
        hip.free()
    assert same(dev, got)
    return got


def check(sw, cols, strand, n_seq, regions, status, set_=0, axes=3, what="", ctx=None):
    """Both seams against the model."""
    cols = {k: np.asarray(cols[k]).astype(np.uint32) for k in COLS}
    strand = np.asarray(strand).astype(np.uint8)
    got = both_seams(sw, cols, strand, n_seq, regions, status, set_, axes, ctx)
    rows, summary = lm.lift(cols, strand, None if status is None else np.asarray(status) != 0, regions, set_, axes)
    assert got.n == len(rows) == len(got.rows), (what, got.n, len(rows))
    assert got.rows.tobytes() == lm.rows_array(rows).tobytes(), (what, [tuple(r) for r in got.rows[:5]], rows[:5])
    assert np.array_equal(got.summary, summary), what
    assert list(got.candidates) == lm.candidates(cols, regions, axes), what
    return got


def columns(rows):
    """rows of (q, t, qs, qe, ts, te, strand, status) -> (cols, strand, status)"""
    arr = np.array(rows, dtype=np.int64).reshape(-1, 8)
    return {k: arr[:, i].astype(np.uint32) for i, k in enumerate(COLS)}, arr[:, 6].astype(np.uint8), arr[:, 7].astype(np.uint8)


def test_hand_case(sw):
    cols, strand, kept, regions, rows, summary = hand_case()
    status = kept.astype(np.uint8) * 2
    got = check(sw, cols, strand, 3, regions, status, what="hand")
    assert [tuple(int(v) for v in r) for r in got.rows] == rows and np.array_equal(got.summary, summary)
    check(sw, cols, strand, 3, regions, None, what="hand, no status")


# ---- the tile ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [T - 1, T, T + 1, 3 * T + 5])
def test_one_region_over_c_candidates_half_of_them_hits(sw, c):
    """Record k starts at k and ends beyond a = 10^5 when k is even: all are candidates of (0, 10^5, 10^6) (the first one ends
    beyond a), every other one a hit."""
    rows = [(0, 1, k, 200_000 + k if k % 2 == 0 else 50_000 + k, 7 * k, 7 * k + 100 + k % 13, k % 3 == 0, k % 4 != 1) for k in range(c)]
    cols, strand, status = columns(rows)
    for set_ in (0, 1):
        got = check(sw, cols, strand, 2, [(0, 100_000, 1_000_000)], status, set_, 1, "c = %d" % c)
        assert got.candidates == (c, 0) and int(got.summary[0, 0, 0]) == (c + 1) // 2
        assert (np.diff(got.rows["record"].astype(np.int64)) > 0).all()


@pytest.mark.parametrize("apart", [False, True])
def test_300_regions_without_candidates_between_two_with_40(sw, apart):
    """Sequence 0 and sequence 2 hold 40 records each under their region (with `apart`: sequence 0 holds 1,000 more that the first
    region also looks at, so that the second region lies in the next tile); the 300 regions between lie on sequence 1, which has no
    record, on an unknown name, or are empty."""
    rows = [(0, 3, 10 * k, 10 * k + 500, k, k + 9, 0, k % 2) for k in range(40)] + [(2, 3, 10 * k, 10 * k + 500, k, k + 5, 1, 1) for k in range(40)]
    if apart:
        rows += [(0, 3, 100 + k % 7, 300 + k, 5, 6, 0, 0) for k in range(1_000)]
    between = [((1, 5 * k, 5 * k + 100), (U, 0, 9), (0, k, k))[k % 3] for k in range(300)]
    regions = [(0, 0, 1_000)] + between + [(2, 0, 1_000)]
    cols, strand, status = columns(rows)
    got = check(sw, cols, strand, 4, regions, status, 0, 1, "300 empty regions")
    assert got.candidates[0] == (1_080 if apart else 80) and int(got.summary[301, 0, 0]) == 40 and not got.summary[1:301].any()
    check(sw, cols, strand, 4, regions, status, 1, 3, "300 empty regions, kept, both axes")


def test_65_regions_of_one_candidate_each(sw):
    rows = [(0, 1, 100 * k, 100 * k + 50, 3 * k, 3 * k + 2, k & 1, k % 3 != 0) for k in range(65)]
    regions = [(0, 100 * k + 10, 100 * k + 20) for k in range(65)]
    got = check(sw, *columns(rows)[:2], 2, regions, columns(rows)[2], 0, 3, "65 heads")
    assert got.candidates == (65, 0) and got.n == 65 and (got.summary[:, 0, 0] == 1).all()
    # and 2,500 regions of one candidate or none, over three tiles
    rows = [(k % 5, 5, 100 * k, 100 * k + 50, 3 * k, 3 * k + 2, k & 1, k % 3 != 0) for k in range(2_500)]
    regions = [(k % 5, 100 * k + 10, 100 * k + 20) if k % 4 else (k % 5, 100 * k + 60, 100 * k + 70) for k in range(2_500)]
    check(sw, *columns(rows)[:2], 6, regions, columns(rows)[2], 1, 3, "2,500 heads")


# ---- the searches ------------------------------------------------------------------------------------------------------------------
def test_the_binary_searches_corners(sw):
    """Records on sequences 0, 2 and 4 of five; the smallest start is 100, the largest end 900."""
    rows = [(s, 0, 100 + 50 * k, 150 + 50 * k + 100 * (k == 3), 0, 10, 0, 1) for s in (0, 2, 4) for k in range(14)]
    rows += [(2, 0, 100, 900, 0, 10, 1, 0), (4, 4, 100, 100, 5, 5, 0, 1)]
    regions = [(0, 0, 5_000), (4, 0, 5_000),            # the first and the last sequence id
               (1, 0, 5_000), (3, 100, 200),            # sequences without records between two that have them
               (2, 0, 100), (2, 0, 101),                # b equal to the smallest start: nothing; one more: the first record
               (2, 900, 5_000), (2, 899, 5_000),        # a equal to the largest end: nothing
               (2, 300, 300), (0, 0, 0), (4, 2**32 - 1, 2**32 - 1),      # a = b
               (0, 0, 2**32 - 1), (U, 0, 2**32 - 1)]
    cols, strand, status = columns(rows)
    for axes in (1, 2, 3):
        got = check(sw, cols, strand, 5, regions, status, 0, axes, "corners")
    assert [int(v) for v in got.summary[:, 0, 0]] == [14, 14, 0, 0, 0, 2, 0, 1, 0, 0, 0, 14, 0]
    assert int(got.summary[0, 0, 1]) == 43 and int(got.summary[1, 0, 1]) == 0      # (the zero-length record is a hit on neither side)


@pytest.mark.parametrize("long_record", [True, False])
def test_the_prefix_maximum_prune(sw, long_record):
    """2,000 short records that end before a, and (long_record) one that spans the sequence in front of them: the prune then
    keeps every one of them a candidate for the one hit."""
    rows = [(0, 1, 10 * k, 10 * k + 5, k, k + 5, 0, 1) for k in range(2_000)] + [(0, 1, 30_000, 30_100, 0, 100, 0, 1)]
    if long_record:
        rows = [(0, 1, 0, 100_000, 0, 50_000, 1, 1)] + rows
    got = check(sw, *columns(rows)[:2], 2, [(0, 29_990, 30_050)], columns(rows)[2], 0, 1, "prune")
    assert got.candidates == ((2_002, 0) if long_record else (1, 0)) and got.n == (2 if long_record else 1)


def test_64_records_with_one_start_come_in_record_order(sw):
    rows = [(1, 0, 5, 9, 0, 1, 0, 1)] * 3 + [(0, 1, 700, 800 + k, 10 * k, 10 * k + 3, k & 1, k % 5 != 0) for k in range(64)] + [(0, 1, 699, 705, 0, 9, 0, 1)]
    got = check(sw, *columns(rows)[:2], 2, [(0, 750, 760)], columns(rows)[2], 0, 3, "ties")
    assert [int(r) for r in got.rows["record"]] == list(range(3, 67))


def test_the_largest_values_on_both_strands(sw):
    top = 2**32 - 1
    rows = [(0, 1, 0, top, 1, top, 0, 1), (0, 1, 0, top, 1, top, 1, 1), (1, 0, top - 1, top, 0, top, 0, 0), (1, 1, top - 5, top, top - 5, top, 1, 1)]
    regions = [(0, 1, top - 1), (0, 0, top), (0, top - 1, top), (1, top - 1, top), (1, 0, top), (0, 1, 2)]
    got = check(sw, *columns(rows)[:2], 2, regions, columns(rows)[2], 0, 3, "2^32 - 1")
    assert tuple(int(v) for v in got.rows[0]) == (0, 0, 1, top - 1, 1, 1, top, 0)      # f(1) = 0, c(L - 1) = D
    check(sw, *columns(rows)[:2], 2, regions, columns(rows)[2], 1, 3, "2^32 - 1, kept")


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def raw_call(ctx, cols, strand, n_seq, status, regions, set_, axes, capacity, rows, summary, fn=None):
    from sweepga_amd._lib import SwgLiftRequest
    from sweepga_amd.lift import regions_array
    rec = records_of({**cols, "strand": strand}, n_seq)
    regs = regions_array(regions)
    req = SwgLiftRequest()
    req.set, req.axes, req.n, req.capacity = set_, axes, 12345, capacity
    req.candidates[0] = req.candidates[1] = 12345
    req.rows = rows.ctypes.data if rows is not None else None
    req.summary = summary.ctypes.data if summary is not None else None
    rc = (fn or ctx.lib.swg_lift_records)(ctx.handle, C.byref(rec), status.ctypes.data if status is not None else None, regs.ctypes.data, len(regs), C.byref(req))
    return rc, req


def test_axes_sets_and_the_capacity_protocol(sw):
    from sweepga_amd.lift import ROW_DTYPE
    ctx = sw.default_context()
    cols, strand, kept, regions, rows, summary = hand_case()
    status = kept.astype(np.uint8)
    poison_row = np.frombuffer(b"\xab" * 32, dtype=ROW_DTYPE)[0]
    for set_ in (0, 1):
        for axes in (1, 2, 3):
            want = [r for r in rows if (axes >> (r[7] >> 1) & 1) and (set_ == 0 or kept[r[1]])]
            want_summary = summary.copy()
            for ax in (0, 1):
                if not (axes >> ax & 1):
                    want_summary[:, :, ax] = 0
            got = check(sw, cols, strand, 3, regions, status, set_, axes, "set %d axes %d" % (set_, axes))
            assert [tuple(int(v) for v in r) for r in got.rows] == want and np.array_equal(got.summary, want_summary)
            assert (got.candidates[0] > 0) == bool(axes & 1) and (got.candidates[1] > 0) == bool(axes & 2)
            n = len(want)
            for capacity in (0, n - 1, n, n + 3):
                buf = np.frombuffer(bytearray(b"\xab" * 32 * (n + 3)), dtype=ROW_DTYPE)
                summ = np.full((len(regions), 2, 2), 0xabababab, dtype=np.uint32)
                rc, req = raw_call(ctx, cols, strand, 3, status, regions, set_, axes, capacity, buf, summ)
                assert rc == 0 and int(req.n) == n and np.array_equal(summ, want_summary), (set_, axes, capacity)
                assert list(req.candidates) == list(got.candidates)
                written = n if capacity >= n else 0      # n > capacity: the rows are left alone
                assert buf[:written].tobytes() == lm.rows_array(want)[:written].tobytes() and (buf[written:] == poison_row).all(), (set_, axes, capacity)
    # no rows array and no summary: the counts alone; KEPT needs a status; the ALL rows do not
    rc, req = raw_call(ctx, cols, strand, 3, status, regions, 0, 3, 0, None, None)
    assert rc == 0 and int(req.n) == len(rows)
    rc, req = raw_call(ctx, cols, strand, 3, None, regions, 1, 3, 0, None, None)
    assert rc == -1 and int(req.n) == 12345
    summ = np.full((len(regions), 2, 2), 7, dtype=np.uint32)
    rc, req = raw_call(ctx, cols, strand, 3, None, regions, 0, 3, 0, None, summ)
    assert rc == 0 and np.array_equal(summ[:, 0], summary[:, 0]) and not summ[:, 1].any()
    # no regions, no records: no device work, zeroed summaries
    rc, req = raw_call(ctx, cols, strand, 3, status, [], 0, 3, 0, None, None)
    assert rc == 0 and int(req.n) == 0 and list(req.candidates) == [0, 0]
    empty = {k: np.zeros(0, dtype=np.uint32) for k in COLS}
    summ = np.full((len(regions), 2, 2), 7, dtype=np.uint32)
    rc, req = raw_call(ctx, empty, np.zeros(0, dtype=np.uint8), 3, None, regions, 0, 3, 0, None, summ)
    assert rc == 0 and int(req.n) == 0 and not summ.any()


def test_refusals_on_the_device(sw):
    ctx = sw.default_context()
    cols, strand, kept, regions, _, _ = hand_case()
    status = kept.astype(np.uint8)
    for set_, axes in ((2, 3), (0, 0), (0, 4)):
        assert raw_call(ctx, cols, strand, 3, status, regions, set_, axes, 0, None, None)[0] == -1
    bad = {c: v.copy() for c, v in cols.items()}
    bad["t_id"][6] = 3
    assert raw_call(ctx, bad, strand, 3, status, regions, 0, 1, 0, None, None)[0] == -1 and b"n_seq" in ctx.lib.swg_last_error(ctx.handle)
    from sweepga_amd.lift import regions_array
    for what, field, value in (("reserved", "reserved", 1), ("start > end", "start", 300), ("n_seq nor", "seq", 3)):
        regs = regions_array(regions)
        regs[0][field] = value
        assert raw_call(ctx, cols, strand, 3, status, regs, 0, 3, 0, None, None)[0] == -1 and what.encode() in ctx.lib.swg_last_error(ctx.handle), what
        hip = Hip()      # the device seam finds the same through its error word
        try:
            dcols = {k: hip.up(cols[k]) for k in COLS}
            rec = records_of({**dcols, "strand": hip.up(strand)}, 3, len(strand))
            from sweepga_amd._lib import SwgLiftRequest
            req = SwgLiftRequest()
            req.set, req.axes = 0, 3
            rc = ctx.lib.swg_lift_records_device(ctx.handle, C.byref(rec), hip.up(status), hip.up(regs.view(np.uint32)), len(regs), C.byref(req))
        finally:
            hip.free()
        assert rc == -1 and what.encode() in ctx.lib.swg_last_error(ctx.handle), what
    assert raw_call(ctx, cols, strand, 3, status, regions, 0, 3, 0, None, None)[0] == 0


# ---- permutations, shapes, random ----------------------------------------------------------------------------------------------
def by_region(rows):
    return {r: rows[rows["region"] == r] for r in np.unique(rows["region"])}


def check_permutations(sw, cols, strand, n_seq, regions, status, got, rng):
    # the regions permuted: the rows of each region are the same
    order = rng.permutation(len(regions))
    again = both_seams(sw, cols, strand, n_seq, [regions[k] for k in order], status, 1, 3)
    assert np.array_equal(again.summary, got.summary[order]) and again.candidates == got.candidates
    mine, theirs = by_region(got.rows), by_region(again.rows)
    for new, old in enumerate(order):
        a, b = mine.get(old), theirs.get(new)
        assert (a is None) == (b is None)
        if a is not None:
            b = b.copy()
            b["region"] = old
            assert a.tobytes() == b.tobytes()
    # the records permuted: equal after mapping `record` back and sorting ties again
    perm = rng.permutation(len(strand))
    again = both_seams(sw, {c: cols[c][perm] for c in COLS}, strand[perm], n_seq, regions, status[perm], 1, 3)
    back = again.rows.copy()
    back["record"] = perm[back["record"]]
    s0 = np.where(back["flags"] & 2, cols["t_start"][back["record"]], cols["q_start"][back["record"]])
    back = back[np.lexsort((back["record"], s0, back["flags"] >> 1, back["region"]))]
    # (the candidates may differ: among records with one start the prune looks at those behind the first that reaches beyond a)
    assert back.tobytes() == got.rows.tobytes() and np.array_equal(again.summary, got.summary)


def random_regions(rng, cols, n_seq, m):
    seq = rng.integers(0, n_seq, m)
    top = int(max(cols["q_end"].max(), cols["t_end"].max())) + 1_000
    start = rng.integers(0, top, m)
    out = [(int(s), int(a), int(a + w)) for s, a, w in zip(seq, start, rng.integers(1_000, 100_000, m))]
    for k in range(0, m, 37):
        out[k] = (out[k][0], out[k][1], out[k][1])      # some empty ones
    for k in range(5, m, 53):
        out[k] = (U, out[k][1], out[k][2])              # ... and unknown names
    return out


@pytest.fixture(scope="module")
def shapes():
    return shape_texts()


@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_breadths_shapes_under_a_real_filter_status(sw, shapes, shape):
    rng = np.random.default_rng(len(shape))
    with sw.PafFile(text=shapes[shape]) as paf:
        status, _ = run_filter(sw, paf, filter_cfgs(sw)["one_to_one"])
        cols = {c: paf.column(c).copy() for c in COLS}
        strand = paf.column("strand").copy()
        n_seq = int(paf.records.n_seq)
    assert int((status != 0).sum()) > 0
    regions = random_regions(rng, cols, n_seq, 500)
    got = check(sw, cols, strand, n_seq, regions, status, 1, 3, shape)
    assert got.summary[:, 0].sum() >= got.summary[:, 1].sum() > 0
    check_permutations(sw, cols, strand, n_seq, regions, status, got, rng)


def test_100000_random_records_and_2000_regions(sw):
    rng = np.random.default_rng(41)
    n, n_seq = 100_000, 50
    qs, ts = rng.integers(0, 5_000_000, n), rng.integers(0, 5_000_000, n)
    ln = np.where(rng.random(n) < 0.02, rng.integers(0, 2_000_000, n), rng.integers(0, 20_000, n))
    cols = {"q_id": rng.integers(0, n_seq, n), "t_id": rng.integers(0, n_seq, n), "q_start": qs, "q_end": qs + ln, "t_start": ts,
            "t_end": ts + (ln * rng.uniform(0.5, 1.5, n)).astype(np.int64)}
    cols = {k: np.asarray(v).astype(np.uint32) for k, v in cols.items()}
    strand, status = (rng.random(n) < 0.3).astype(np.uint8), (rng.random(n) < 0.5).astype(np.uint8)
    regions = random_regions(rng, cols, n_seq, 2_000)
    got = check(sw, cols, strand, n_seq, regions, status, 0, 3, "random")
    assert got.n > 10_000 and sum(got.candidates) > got.n
    check(sw, cols, strand, n_seq, regions[:300], status, 1, 2, "random, kept, target axis")


def test_a_memory_limit_too_small_is_a_clean_oom(sw):
    from sweepga_amd.lift import lift_records
    ctx = sw.Context(0)
    try:
        n = 200_000
        cols = {k: np.arange(n, dtype=np.uint32) % 1_000 + (100 if k.endswith("end") else 0) for k in COLS}
        cols["q_id"] = cols["t_id"] = np.zeros(n, dtype=np.uint32)
        strand = np.zeros(n, dtype=np.uint8)
        ctx.set_memory_limit(4 << 20)       # the index of one axis alone is 24 bytes per record: 4.8 MB
        with pytest.raises(sw.SwgError) as e:
            lift_records(ctx, cols, strand, 1, [(0, 0, 10)], axes=1)
        assert e.value.code == -4
        hand = hand_case()
        got = lift_records(ctx, hand[0], hand[1], 3, hand[3], status=hand[2].astype(np.uint8))      # the same context, a call that fits
        assert [tuple(int(v) for v in r) for r in got.rows] == hand[4]
        ctx.set_memory_limit(0)
        big = lift_records(ctx, cols, strand, 1, [(0, 0, 10)], axes=1, capacity=0)
        assert big.n == 10 * (n // 1_000) and big.rows is None
    finally:
        ctx.close()


# ---- the texts -----------------------------------------------------------------------------------------------------------------
def random_bed(rng, text, m):
    names = lm.parse_paf(text)[2]
    lines = ["# regions", "track name=genes"]
    for k in range(m):
        nm = names[int(rng.integers(0, len(names)))] if k % 11 else "absent#%d" % k
        a = int(rng.integers(0, 400_000))
        b = a + int(rng.integers(0, 50_000)) * (k % 13 != 0)
        lines.append("\t".join([nm, str(a), str(b)] + (["gene%d" % k] if k % 3 else [])))
    return "\n".join(lines) + "\n"


def test_texts_of_an_open_paf_equal_the_model_rendering(sw):
    text, kept = hand_paf()
    with sw.PafFile(text=text) as paf:
        got = sw.Lift.from_paf(paf, kept.astype(np.uint8), HAND_BED, set="all")
        assert got.summary_text == HAND_SUMMARY and (got.text, got.summary_text) == lm.paf_texts(text, kept, HAND_BED, 0, 3)
        assert len(got.rows) == 15 and list(got.summary["state"][-4:]) == ["none", "unknown", "kept", "lost"]
        got = sw.Lift.from_paf(paf, None, HAND_BED, set="all", axes="query", ctx=sw.default_context())
        assert (got.text, got.summary_text) == lm.paf_texts(text, None, HAND_BED, 0, 1)
    text = gen_text(61, 12_000, n_genomes=4, chrs_per_genome=3, span=300_000)
    bed = random_bed(np.random.default_rng(3), text, 400)
    with sw.PafFile(text=text) as paf:
        status, _ = run_filter(sw, paf, filter_cfgs(sw)["one_to_one"])
        assert 0 < int((status != 0).sum()) < len(status)
        for set_, axes in (("kept", "both"), ("all", "target"), ("kept", "query")):
            got = sw.Lift.from_paf(paf, status, bed, set=set_, axes=axes)
            want = lm.paf_texts(text, status != 0, bed, sw.lift.SETS[set_], sw.lift.AXES[axes])
            assert (got.text, got.summary_text) == want and want[0].count("\n") > 400, (set_, axes)
        assert {"kept", "none", "unknown"} <= set(sw.Lift.from_paf(paf, status, bed).summary["state"])
        only = sw.Lift.from_paf(paf, status, bed, rows=False)
        assert only.text is None and only.summary_text == lm.paf_texts(text, status != 0, bed, 1, 3)[1]
        # more rows than the first guess at their number holds
        wide = "".join("%s\t0\t400000\n" % nm for nm in lm.parse_paf(text)[2]) * 8
        got = sw.Lift.from_paf(paf, status, wide, set="all")
        assert (got.text, got.summary_text) == lm.paf_texts(text, status != 0, wide, 0, 3) and got.text.count("\n") > 2**16


def test_cli_lift(sw, tmp_path):
    from sweepga_amd import build
    text = gen_text(71, 15_000, n_genomes=4, chrs_per_genome=3, span=400_000)
    bed_text = random_bed(np.random.default_rng(9), text, 300)
    inp, bed = tmp_path / "in.paf", tmp_path / "r.bed"
    inp.write_text(text, newline="")
    bed.write_text(bed_text, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-jump", "10k", "--scaffold-mass", "2k", "--quiet"]
    plain, out, rows, summ = (tmp_path / x for x in ("plain.paf", "out.paf", "lift.tsv", "lift_summary.tsv"))
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), *flags], capture_output=True)
    assert r0.returncode == 0 and plain.stat().st_size > 0, r0.stderr
    kept = kept_mask(text, plain.read_bytes().decode())
    for extra, set_, axes, given in (([], 1, 3, ("rows", "summary")), (["--lift-set", "all", "--lift-axis=target"], 0, 2, ("rows", "summary")),
                                     (["--lift-axis", "query"], 1, 1, ("rows",)), (["--lift-set=kept"], 1, 3, ("summary",))):
        want = lm.paf_texts(text, kept, bed_text, set_, axes)
        for p in (out, rows, summ):
            p.unlink(missing_ok=True)
        files = (["--lift", str(rows)] if "rows" in given else []) + (["--lift-summary", str(summ)] if "summary" in given else [])
        r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--lift-regions", str(bed), *files, *extra, *flags], capture_output=True)
        assert r.returncode == 0 and r.stdout == b"" and out.read_bytes() == plain.read_bytes(), r.stderr     # the PAF does not change
        assert rows.exists() == ("rows" in given) and summ.exists() == ("summary" in given)
        assert "rows" not in given or rows.read_text() == want[0]
        assert "summary" not in given or summ.read_text() == want[1]
    # the summary on standard error
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--lift-regions", str(bed), "--lift-summary", "-", *flags], capture_output=True)
    assert r.returncode == 0 and r.stderr.decode() == lm.paf_texts(text, kept, bed_text, 1, 3)[1] and out.read_bytes() == plain.read_bytes()
    # --no-filter: every line to standard output, kept = all
    r = subprocess.run([build.CLI, str(inp), "--no-filter", "--lift-regions", str(bed), "--lift", str(rows), "--lift-summary", str(summ)], capture_output=True)
    every = lm.paf_texts(text, np.ones(len(kept), dtype=bool), bed_text, 1, 3)
    assert r.returncode == 0 and r.stdout == text.encode() and rows.read_text() == every[0] and summ.read_text() == every[1]


def test_smallest_shapes_on_a_fresh_context(sw):
    """The seams around the kernels at the smallest shapes -- one record; three records of one sequence pair in one chain -- on a
    context of its own: its first call sizes the arena from the input, the later ones find it sized.  Each shape twice, host seam
    against device seam byte for byte and both against the model."""
    rows = [(0, 1, 10, 110, 20, 125, 0, 1), (0, 1, 200, 300, 210, 310, 1, 1), (0, 1, 400, 450, 420, 470, 0, 1)]
    regions = [(0, 0, 500), (1, 100, 300)]
    ctx = sw.Context(0)
    try:
        for n in (1, 3, 1, 3):
            cols, strand, kept = columns(rows[:n])
            for status in (None, kept):   # (None: the optional column stays NULL on its way to the device)
                got = check(sw, cols, strand, 2, regions, status, 1 if status is not None else 0, 3, f"n = {n}", ctx=ctx)
                assert got.n >= n
    finally:
        ctx.close()
