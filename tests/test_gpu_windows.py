"""Windows on the device (sweepga_amd/csrc/swg_windows.hip) against tests/windows_model.py, host seam against device seam byte for
byte and then field by field against the model: window borders by hand, the extremes of W, carries across the scans' tile seams,
the wrapping 64-bit differences, thousands of records on one address, the union across windows, who takes part, a free
permutation of the records, the request's variants and errors, a memory limit, the smallest shapes on a fresh context, and the
status of a real swg_filter_device run with the texts of swg_paf_windows / --windows byte for byte against the model's formatter.
Every comparison is exact: integers and bytes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import windows_model as wm
from tests.test_gpu_alnstats import gen_text, records_of
from tests.test_gpu_blocks import SEED_WITH_RESCUES, flag_sets
from tests.test_gpu_gaps import genome_names
from tests.test_gpu_place import filter_on_the_device, last_lengths
from tests.test_gpu_wide import Hip
from tests.test_windows_cpu import COLUMNS, columns, on_query

pytestmark = pytest.mark.gpu
TOP = 2**32 - 1
SCAN_TILE = 4096     # SCAN_TILE of csrc/swg_sort.hip (SCAN_THREADS * SCAN_ITEMS): what one work-group of the library's scans covers


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


def axis_columns(axis):
    return ("q_id", "t_id") + (("t_start", "t_end") if axis else ("q_start", "q_end"))


def both_seams(sw, cols, seq_len, genome, status=None, axis=0, window=100, other=None, weight=None, n_genome=None, ctx=None, want=3):
    """The result of the host seam, after checking that the device seam gives the same bytes."""
    from sweepga_amd.windows import _call, windows_records
    ctx = ctx or sw.default_context()
    names = axis_columns(axis) + (("matches",) if weight is None else ())
    cols = {k: np.ascontiguousarray(cols[k], dtype=np.uint32) for k in names}
    seq_len, genome = np.ascontiguousarray(seq_len, dtype=np.uint32), np.ascontiguousarray(genome, dtype=np.uint32)
    status = None if status is None else np.ascontiguousarray(status, dtype=np.uint8)
    weight = None if weight is None else np.ascontiguousarray(weight, dtype=np.uint32)
    if n_genome is None:
        n_genome = int(genome.max()) + 1
    host = windows_records(ctx, cols, seq_len, genome, status, axis=axis, window=window, other_genome=other, weight=weight, n_genome=n_genome, want=want)
    hip = Hip()
    try:
        rec = records_of({k: hip.up(v) for k, v in cols.items()}, len(genome), len(cols["q_id"]))
        dev = _call(ctx, ctx.lib.swg_windows_records_device, rec, hip.up(seq_len), hip.up(genome), n_genome,
                    hip.up(status) if status is not None else None, axis, window, other, hip.up(weight) if weight is not None else None, want)
    finally:
        hip.free()
    for a, b in ((host.rows, dev.rows), (host.seqs, dev.seqs)):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()
    return host


def check(sw, cols, seq_len, genome, status=None, variants=((0, 100, None),), what="", weight=None, **kw):
    """variants: (axis, window, other_genome).  -> the result of the first."""
    out = None
    for axis, window, other in variants:
        got = both_seams(sw, cols, seq_len, genome, status, axis, window, other, weight, **kw)
        rows, seqs = wm.windows(cols, seq_len, genome, status, axis, window, other, weight)
        wm.same(got.rows, rows, (what, axis, window, other, "rows"))
        wm.same(got.seqs, seqs, (what, axis, window, other, "summary"))
        out = out or got
    return out


def random_table(rng, n, n_seq=40, per_genome=4, max_len=60_000, max_span=5_000):
    """n records between random sequences, both axes inside their sequences; -> cols, seq_len, genome, status (0 .. 3)."""
    genome = (np.arange(n_seq) // per_genome).astype(np.uint32)
    seq_len = rng.integers(1, max_len, n_seq)
    q, t = rng.integers(0, n_seq, n), rng.integers(0, n_seq, n)
    out = {"q_id": q, "t_id": t}
    for ids, a, b in ((q, "q_start", "q_end"), (t, "t_start", "t_end")):
        start = (rng.random(n) * seq_len[ids]).astype(np.int64)
        span = rng.integers(0, max_span, n) * (rng.random(n) < 0.97)
        out[a], out[b] = start, np.minimum(start + span, seq_len[ids])
    out["matches"] = rng.integers(0, max_span, n)
    return {k: np.asarray(v) for k, v in out.items()}, seq_len, genome, rng.choice(np.array([0, 1, 2, 3], dtype=np.uint8), n)


# ---- 1. window borders, by hand ------------------------------------------------------------------------------------------------------
BORDERS = {"inside": (110, 190), "ends_on_a_border": (150, 200), "one_base_over": (150, 201), "starts_on_a_border": (200, 260),
           "two_windows": (200, 400), "four_windows": (130, 430), "whole": (0, None)}


@pytest.mark.parametrize("layout", ["alone_1000", "alone_1050", "followed"])
def test_window_borders_by_hand(sw, layout):
    """Every layout has a record that ends in the last window of its sequence.  alone: the table ends there -- a count closed one slot
    further would fall on slot T; followed: a second listed sequence comes next in the table (sequence 1 lies between and is not
    listed), and nothing of sequence 0 may show in its first window."""
    length = 1_050 if layout == "alone_1050" else 1_000
    for name, (a, b) in BORDERS.items():
        b = length if b is None else b
        records = [on_query(0, 3, a, b, 77), on_query(0, 3, 900, length, 5)]          # the second ends in the last window, whatever the first does
        if layout == "followed":
            records.append(on_query(2, 3, 0, 40, 9))
        got = check(sw, columns(records), [length, 500, 300, 5_000], [0, 0, 0, 1], np.array([1] * len(records)), what=(layout, name))
        first = a // 100, (b - 1) // 100
        assert int(got.rows["n"][first[0], 0]) >= 1 and len(got.rows) == -(-length // 100) + (3 if layout == "followed" else 0)
        if name == "one_base_over":
            assert got.rows["n"][:4, 0].tolist() == [0, 1, 1, 0] and got.rows["depth"][:4, 0].tolist() == [0, 50, 1, 0]
        if name == "whole":
            assert (got.rows["covered"][:first[1] + 1, 0] == got.rows["end"][:first[1] + 1] - got.rows["start"][:first[1] + 1]).all()
            assert int(got.rows["end"][first[1]]) == length
        if layout == "followed":
            assert got.rows["n"][-3:, 0].tolist() == [1, 0, 0] and got.seqs["seq"].tolist() == [0, 2]


# ---- 2. the extremes of W ------------------------------------------------------------------------------------------------------------
def test_extremes_of_the_window(sw):
    rng = np.random.default_rng(2)
    cols, seq_len, genome, status = random_table(rng, 400, n_seq=6, per_genome=2, max_len=300, max_span=120)
    seq_len[0] = 299
    got = check(sw, cols, seq_len, genome, status, ((0, 1, None), (1, 1, None), (0, 299, None), (0, 300, None), (1, 100_000, None), (0, TOP, None)), what="W")
    assert (got.rows["end"] - got.rows["start"] == 1).all() and len(got.rows) == int(seq_len[got.seqs["seq"]].sum())
    # W = 2^32 - 1 with coordinates up to 2^32 - 1, and W = 2^31 on the same: two windows, the second one base short
    big = columns([on_query(0, 1, 0, TOP, TOP), on_query(0, 1, TOP - 1, TOP, 3), on_query(1, 0, 5, TOP - 5, 1)])
    got = check(sw, big, [TOP, TOP], [0, 1], np.array([1, 0, 1]), ((0, TOP, None), (0, 2**31, None), (1, 2**31 + 1, None)), what="2^32 - 1")
    assert got.rows["depth"][:, 0].tolist() == [TOP + 1, TOP - 10] and got.rows["covered"][:, 0].tolist() == [TOP, TOP - 10]
    # a sequence of length 0 that carries only zero-length records is not listed, and the record is no error
    zero = columns([on_query(0, 1, 0, 0), on_query(0, 1, 0, 0), on_query(1, 0, 3, 9)])
    got = check(sw, zero, [0, 50], [0, 1], variants=((0, 10, None), (0, 1, None)), what="length 0")
    assert got.seqs["seq"].tolist() == [1] and len(got.rows) == 5


# ---- 3. carries across the scans' tile seams -------------------------------------------------------------------------------------------
def test_one_record_over_20000_windows(sw):
    """T + 1 = 20,001 entries of the difference arrays are four scan tiles of 4,096 (SCAN_TILE of swg_sort.hip) and a fifth begun: the one +1
    of the long record is carried across every seam, in the count and in the full-window and matches differences."""
    assert 20_001 > 3 * SCAN_TILE + 1
    rng = np.random.default_rng(3)
    W, length, n = 16, 320_000, 3_000
    start = rng.integers(0, length - 200, n)
    span = rng.integers(1, 200, n)
    records = [on_query(0, 1, 0, length, 123_457)] + [on_query(0, 1, int(a), int(a + s), int(m)) for a, s, m in zip(start, span, rng.integers(0, 400, n))]
    status = rng.choice(np.array([0, 1, 2, 3], dtype=np.uint8), n + 1)
    status[0] = 1
    got = check(sw, columns(records), [length, 1_000], [0, 1], status, ((0, W, None),), what="20,000 windows")
    assert len(got.rows) == 20_000 and (got.rows["n"] >= 1).all() and (got.rows["covered"] == W).all()
    assert int(got.rows["matches"][-1, 1]) >= W * 123_457 // length


def test_300_listed_sequences_among_1000_ids(sw):
    rng = np.random.default_rng(33)
    n_seq, W = 1_000, 64
    listed = np.sort(rng.choice(n_seq - 1, 300, replace=False))            # sparse: absent sequences between the listed ones
    seq_len = rng.integers(1, 3_000, n_seq)
    seq_len[listed[::2]] = W * rng.integers(1, 40, len(listed[::2]))        # every other one a multiple of W
    genome = np.zeros(n_seq, dtype=np.uint32)
    genome[n_seq - 1] = 1                                                    # the one partner: listed on the target axis only
    s = np.r_[listed, listed[rng.integers(0, 300, 2_700)]]
    start = (rng.random(len(s)) * seq_len[s]).astype(np.int64)
    end = np.minimum(start + rng.integers(1, 900, len(s)), seq_len[s])
    end[:300] = seq_len[listed]                                              # every listed sequence has a record that closes on its last slot
    cols = columns(np.stack([s, np.full(len(s), n_seq - 1), start, end, start, end, rng.integers(0, 900, len(s))], axis=1))
    seq_len[n_seq - 1] = 3_000
    got = check(sw, cols, seq_len, genome, rng.choice(np.array([0, 1], dtype=np.uint8), len(s)), ((0, W, None), (0, 7, 1), (1, W, None)), what="300 of 1000")
    assert got.seqs["seq"].tolist() == listed.tolist() and int((seq_len[listed] % W == 0).sum()) >= 150


# ---- 4. the wrapping 64-bit differences ------------------------------------------------------------------------------------------------
def test_large_matches_in_the_differences(sw):
    W = 100
    records = [on_query(0, 1, 99, 99 + 2 * W + 2, TOP),        # just above 2 W: c = floor(W * (2^32 - 1) / 202) added at one slot, taken off two further
               on_query(0, 1, 0, 2 * W + 1, TOP),              # no interior at all
               on_query(0, 1, 350, 950, TOP), on_query(0, 1, 351, 951, TOP - 1),
               on_query(0, 1, 40, 45, 4_000_000_000),          # m > b - a
               on_query(2, 1, 0, 900, TOP)]
    got = check(sw, columns(records), [1_000, 77, 900], [0, 1, 0], np.array([1, 0, 1, 1, 0, 1]), ((0, W, None), (0, 1, None), (0, 3, None)), what="2^32 - 1 matches")
    assert int(got.rows["matches"][1, 0]) == W * TOP // 202 + W * TOP // 201 and int(got.rows["matches"][0, 0]) >= 4_000_000_000
    # window [300, 400): one base of the first record, 50 and 49 bases of the two of 600
    assert int(got.rows["n"][3, 0]) == 3 and int(got.rows["matches"][3, 0]) == TOP // 202 + 50 * TOP // 600 + 49 * (TOP - 1) // 600


# ---- 5. one address ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["inside_one_window", "fan_out"])
def test_4096_records_on_one_window(sw, shape):
    rng = np.random.default_rng(5)
    n, W = 4_096, 8
    if shape == "inside_one_window":
        a = 10_000 + rng.integers(0, 50, n)
        records = [on_query(0, 1, int(x), int(x + y), int(m)) for x, y, m in zip(a, rng.integers(1, 50, n), rng.integers(0, 1_000, n))]
        got = check(sw, columns(records), [40_000, 9], [0, 1], rng.choice(np.array([0, 3], dtype=np.uint8), n), ((0, 10_000, None),), what=shape)
        assert got.rows["n"][:, 0].tolist() == [0, n, 0, 0]
    else:       # all start in window 0 and end in 4,096 different ones
        records = [on_query(0, 1, int(rng.integers(0, 4)), W * i + int(rng.integers(5, W + 1)), int(m)) for i, m in zip(rng.permutation(n), rng.integers(0, 10**6, n))]
        got = check(sw, columns(records), [W * n, 9], [0, 1], rng.choice(np.array([0, 1], dtype=np.uint8), n), ((0, W, None),), what=shape)
        assert got.rows["n"][:, 0].tolist() == list(range(n, 0, -1)) and (got.rows["covered"][:-1, 0] == W).all()


# ---- 6. the union across windows ---------------------------------------------------------------------------------------------------------
def test_the_union_across_windows(sw):
    W = 100
    records = [on_query(0, 1, 0, W), on_query(0, 1, W, 2 * W),                    # abutting: one merged interval over two windows
               on_query(0, 1, 250, 650), on_query(0, 1, 300, 350),                # nested
               on_query(0, 1, 600, 820), on_query(0, 1, 780, 1_130),              # overlapping: [250, 1130) spans windows no single record spans
               on_query(0, 1, 1_400, 1_700), on_query(0, 1, 1_450, 1_460),        # a kept record nested in a dropped one
               on_query(0, 1, 1_900, 1_950), on_query(0, 1, 1_900, 1_950)]        # twice the same
    status = np.array([1, 2, 3, 0, 1, 0, 0, 3, 2, 2], dtype=np.uint8)              # every status value there is
    got = check(sw, columns(records), [2_000, 9], [0, 1], status, ((0, W, None), (0, 64, None), (0, 2_000, None)), what="union")
    assert got.rows["covered"][14, :].tolist() == [100, 10] and got.rows["covered"][:2, 0].tolist() == [100, 100]
    assert got.rows["covered"][19].tolist() == [50, 50] and got.rows["depth"][19].tolist() == [100, 100]
    assert got.rows["covered"][2:12, 0].tolist() == [50, 100, 100, 100, 100, 100, 100, 100, 100, 30]
    rng = np.random.default_rng(6)
    cols, seq_len, genome, status = random_table(rng, 5_000, n_seq=12, per_genome=3, max_len=20_000, max_span=3_000)   # deep piles: long merged intervals
    got = check(sw, cols, seq_len, genome, status, ((0, 100, None), (1, 1_000, None)), what="random union")
    assert (got.rows["covered"][:, 1] < got.rows["covered"][:, 0]).any() and (got.rows["covered"] <= got.rows["depth"]).all()


# ---- 7. who takes part -------------------------------------------------------------------------------------------------------------------
def test_who_takes_part(sw):
    rng = np.random.default_rng(7)
    cols, seq_len, genome, status = random_table(rng, 3_000, n_seq=20, per_genome=4)      # a fifth of the records lie inside one genome
    s, o, _, _ = wm.by_role(cols, 0)
    assert 300 < int((genome[s] == genome[o]).sum()) < 1_000
    got = check(sw, cols, seq_len, genome, status, ((0, 1_000, None), (0, 1_000, 2), (1, 1_000, 2), (1, 777, None), (0, 1_000, 5)), what="taking part", n_genome=6)
    none = both_seams(sw, cols, seq_len, genome, status, 0, 1_000, 5, n_genome=6)           # a genome without records: nothing is listed
    assert len(none.rows) == 0 and len(none.seqs) == 0 and len(got.seqs) == 20
    weight = rng.integers(0, 2**32, 3_000)
    by_weight = check(sw, cols, seq_len, genome, status, ((0, 1_000, None), (1, 333, 1)), what="weight", weight=weight)
    assert by_weight.rows["depth"].tobytes() == got.rows["depth"].tobytes() and by_weight.rows["matches"].tobytes() != got.rows["matches"].tobytes()
    bare = check(sw, cols, seq_len, genome, None, ((0, 1_000, None), (1, 1_000, 0)), what="no status")
    assert not any(bare.rows[k][:, 1].any() for k in ("n", "covered", "depth", "matches"))
    assert not any(bare.seqs[k][:, 1].any() for k in ("empty", "covered", "depth", "matches", "records"))
    assert bare.rows["depth"][:, 0].tobytes() == got.rows["depth"][:, 0].tobytes()
    cols["t_id"] = cols["q_id"] ^ 1                                                        # every record inside its genome
    nothing = both_seams(sw, cols, seq_len, genome, status, 0, 1_000)
    assert len(nothing.rows) == 0 and len(nothing.seqs) == 0


# ---- 8. order independence -----------------------------------------------------------------------------------------------------------------
def test_a_free_permutation_of_the_records(sw):
    rng = np.random.default_rng(8)
    cols, seq_len, genome, status = random_table(rng, 6_000)
    cols["matches"] = rng.integers(0, 2**32, 6_000)
    a = check(sw, cols, seq_len, genome, status, ((0, 500, None), (1, 64, None)), what="as generated")
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(6_000)
        for axis, window in ((0, 500), (1, 64)):
            b = both_seams(sw, {k: v[perm] for k, v in cols.items()}, seq_len, genome, status[perm], axis, window)
            want = a if axis == 0 else both_seams(sw, cols, seq_len, genome, status, axis, window)
            assert b.rows.tobytes() == want.rows.tobytes() and b.seqs.tobytes() == want.seqs.tobytes() and len(b.seqs) == 40


# ---- 9. the request ------------------------------------------------------------------------------------------------------------------------
def test_each_want_bit(sw):
    rng = np.random.default_rng(9)
    cols, seq_len, genome, status = random_table(rng, 3_000)
    for axis in (0, 1):
        both = both_seams(sw, cols, seq_len, genome, status, axis, 1_000)
        rows_only = both_seams(sw, cols, seq_len, genome, status, axis, 1_000, want=1)
        summary_only = both_seams(sw, cols, seq_len, genome, status, axis, 1_000, want=2)
        assert rows_only.seqs is None and rows_only.rows.tobytes() == both.rows.tobytes() and len(both.rows) > 500
        assert summary_only.rows is None and summary_only.seqs.tobytes() == both.seqs.tobytes() and len(both.seqs) == 40


def test_input_errors_and_the_capacity_protocol(sw):
    from sweepga_amd._lib import SwgWindowRow, SwgWindowSeq, SwgWindowsRequest
    from sweepga_amd.windows import windows_records
    ctx = sw.default_context()
    rng = np.random.default_rng(41)
    cols, seq_len, genome, status = random_table(rng, 500, n_seq=12, per_genome=3)
    cols = {k: np.ascontiguousarray(v, dtype=np.uint32) for k, v in cols.items()}
    seq_len, genome = seq_len.astype(np.uint32), genome.astype(np.uint32)
    want_rows, want_seqs = wm.windows(cols, seq_len, genome, status, 0, 1_000)
    assert len(want_rows) > 100 and len(want_seqs) == 12
    for field, value in (("q_id", 12), ("t_id", 12), ("q_id", TOP)):      # a sequence id >= n_seq, on a record that would take part or not
        bad = {k: v.copy() for k, v in cols.items()}
        bad[field][250] = value
        with pytest.raises(sw.SwgError) as e:
            windows_records(ctx, bad, seq_len, genome, status)
        assert e.value.code == -1 and "n_seq" in str(e.value)
    with pytest.raises(sw.SwgError) as e:
        windows_records(ctx, cols, seq_len, genome, n_genome=3)            # genome id 3 >= n_genome
    assert e.value.code == -1
    with pytest.raises(sw.SwgError) as e:
        windows_records(ctx, cols, seq_len, genome, other_genome=4)        # no such genome
    assert e.value.code == -1 and "other_genome" in str(e.value)
    # a record that takes part and ends one base beyond its sequence: named, and the outputs zeroed
    takes = wm.taking(cols, seq_len, genome, None, 0)[0]
    r_bad = takes[len(takes) // 2]
    short = seq_len.copy()
    short[cols["q_id"][r_bad]] = cols["q_end"][r_bad] - 1
    first = min(r for r in takes if cols["q_end"][r] > short[cols["q_id"][r]])
    rec = records_of(cols, 12)
    req = SwgWindowsRequest()
    req.want, req.window, req.other_genome, req.n_rows, req.n_seqs = 3, 1_000, 0xffffffff, 777, 777
    assert ctx.lib.swg_windows_records(ctx.handle, C.byref(rec), short.ctypes.data, genome.ctypes.data, 4, status.ctypes.data, C.byref(req)) == -1
    assert f"record {first} " in ctx.lib.swg_last_error(ctx.handle).decode() and (int(req.n_rows), int(req.n_seqs)) == (0, 0)
    args = (seq_len.ctypes.data, genome.ctypes.data, 4, status.ctypes.data)
    call = lambda: ctx.lib.swg_windows_records(ctx.handle, C.byref(rec), *args, C.byref(req))   # noqa: E731
    req.n_rows = req.n_seqs = 777
    for field, value in (("reserved", 1), ("want", 0), ("want", 4), ("axis", 2), ("window", 0), ("other_genome", 4)):
        before = getattr(req, field)
        setattr(req, field, value)
        assert call() == -1 and (int(req.n_rows), int(req.n_seqs)) == (777, 777), field
        setattr(req, field, before)
    rec.n = 2**31                                                           # refused before a column is looked at
    assert call() == -5
    rec.n = 500
    for column in ("q_id", "t_id", "q_start", "q_end", "matches"):
        held = getattr(rec, column)
        setattr(rec, column, None)
        assert call() == -1, column
        setattr(rec, column, held)
    rec.t_start = rec.t_end = None                                          # the other axis' coordinates are not read
    assert call() == 0
    assert ctx.lib.swg_windows_records(ctx.handle, C.byref(rec), None, genome.ctypes.data, 4, status.ctypes.data, C.byref(req)) == -1
    assert ctx.lib.swg_windows_records(ctx.handle, C.byref(rec), seq_len.ctypes.data, None, 4, status.ctypes.data, C.byref(req)) == -1
    # the capacity protocol: SWG_OK, the counts say how many there are, the arrays are left alone -- each array on its own
    n_rows, n_seqs = len(want_rows), len(want_seqs)
    rows = np.frombuffer(bytearray(b"\xab" * 64 * n_rows), dtype=wm.ROW_DTYPE)
    seqs = np.frombuffer(bytearray(b"\xcd" * 80 * n_seqs), dtype=wm.SEQ_DTYPE)
    before = rows.tobytes(), seqs.tobytes()
    req.rows, req.seqs = C.cast(rows.ctypes.data, C.POINTER(SwgWindowRow)), C.cast(seqs.ctypes.data, C.POINTER(SwgWindowSeq))
    req.capacity, req.seq_capacity = n_rows - 1, n_seqs - 1
    assert call() == 0
    assert (int(req.n_rows), int(req.n_seqs)) == (n_rows, n_seqs) and (rows.tobytes(), seqs.tobytes()) == before
    req.seq_capacity = n_seqs                                              # the summary fits, the rows do not
    assert call() == 0 and rows.tobytes() == before[0]
    wm.same(seqs, want_seqs, "summary alone")
    seqs[:] = np.frombuffer(before[1], dtype=wm.SEQ_DTYPE)
    req.capacity, req.seq_capacity = n_rows, n_seqs - 1                    # ... and the other way round
    assert call() == 0 and seqs.tobytes() == before[1]
    wm.same(rows, want_rows, "rows alone")
    req.rows, req.seqs = None, None                                        # NULL arrays: the counts alone
    assert call() == 0 and (int(req.n_rows), int(req.n_seqs)) == (n_rows, n_seqs)
    check(sw, cols, seq_len, genome, status, ((0, 1_000, None), (1, 1_000, None)), what="after the refusals")


def test_too_many_windows_are_refused_before_they_are_allocated(sw):
    """One listed sequence of 2^32 - 2 bases under W = 1 carries a single short record: 2^31 windows or more is SWG_ERR_RANGE.  The
    table would take hundreds of gigabytes; a context limited to 64 MB refuses with the RANGE code, not with OOM."""
    from sweepga_amd.windows import windows_records
    ctx = sw.Context(0)
    try:
        ctx.set_memory_limit(64 << 20)
        cols = columns([on_query(0, 1, 5, 9)])
        for length, window in ((TOP - 1, 1), (TOP, 2)):
            with pytest.raises(sw.SwgError) as e:
                windows_records(ctx, cols, [length, 100], [0, 1], window=window)
            assert e.value.code == -5 and "2^31 windows" in str(e.value)
        got = windows_records(ctx, cols, [2**31 - 1, 100], [0, 1], window=2**20)      # ... and the context works on
        assert len(got.rows) == 2_048 and got.seqs["depth"][0].tolist() == [4, 0]
    finally:
        ctx.close()


def test_a_memory_limit_too_small_is_a_clean_oom(sw):
    from sweepga_amd.windows import windows_records
    ctx = sw.Context(0)
    try:
        cols, seq_len, genome, status = random_table(np.random.default_rng(51), 200_000)
        ctx.set_memory_limit(1 << 20)       # the staged columns alone are 4 MB
        with pytest.raises(sw.SwgError) as e:
            windows_records(ctx, cols, seq_len, genome, status, window=100)
        assert e.value.code == -4
        ctx.set_memory_limit(0)             # ... and the context works on
        want = both_seams(sw, cols, seq_len, genome, status, 0, 100)
        got = both_seams(sw, cols, seq_len, genome, status, 0, 100, ctx=ctx)
        ctx.set_memory_limit(1 << 30)
        limited = both_seams(sw, cols, seq_len, genome, status, 0, 100, ctx=ctx)
        for r in (got, limited):
            assert r.rows.tobytes() == want.rows.tobytes() and r.seqs.tobytes() == want.seqs.tobytes() and len(r.rows) > 5_000
        assert ctx.memory_info()[0] <= 1 << 30
    finally:
        ctx.close()


# ---- 10. the smallest shapes -----------------------------------------------------------------------------------------------------------------
def test_smallest_shapes_on_a_fresh_context(sw):
    """The seams around the kernels at the smallest shapes -- one record; three records of one chain -- on a context of its own: its
    first call sizes the arena from the input, the later ones find it sized.  Each shape twice, host seam against device seam byte
    for byte and both against the model."""
    chain = [on_query(0, 1, 100, 400, 290), on_query(0, 1, 500, 700, 150), on_query(0, 1, 700, 800, 99)]
    ctx = sw.Context(0)
    try:
        for n in (1, 3, 1, 3):
            got = check(sw, columns(chain[:n]), [1_000, 5_000], [0, 1], np.ones(n, dtype=np.uint8), ((0, 100, None), (1, 100, None)), what=f"n = {n}", ctx=ctx)
            assert len(got.rows) == 10 and got.seqs["records"][0].tolist() == [n, n] and int(got.seqs["depth"][0, 0]) == (300, 600)[n == 3]
    finally:
        ctx.close()


# ---- 11. a real filter, the texts and the command line ---------------------------------------------------------------------------------------
def paf_text(n=6_000):
    return gen_text(SEED_WITH_RESCUES, n, n_genomes=4, chrs_per_genome=3, span=400_000)


def handle_columns(paf):
    return {k: paf.column(k).copy() for k in COLUMNS}


@pytest.mark.parametrize("flags", ["default", "one_to_one_rescue"])
def test_the_status_of_a_real_filter_on_the_device(sw, flags):
    from sweepga_amd.breadth import breadth_records
    from sweepga_amd.windows import _call
    text = paf_text()
    ctx = sw.default_context()
    with sw.PafFile(text=text) as paf:
        cols = handle_columns(paf)
        n_seq, G = int(paf.records.n_seq), int(paf.records.n_genome_last)
        genome, names, gnames = paf.seq_genome_last[:n_seq].copy(), list(paf.names), genome_names(sw, paf)
        seq_len = last_lengths(text, names)
        hip = Hip()
        try:
            rec, d_status, status = filter_on_the_device(sw, paf, flag_sets(sw)[flags], hip)
            d_len = hip.up(seq_len)
            assert 0 < int((status != 0).sum()) < paf.n
            for axis, window, other in ((0, 10_000, None), (1, 777, 2)):      # the columns where the filter read them, the status where it wrote it
                dev = _call(ctx, ctx.lib.swg_windows_records_device, rec, d_len, rec.seq_genome_last, G, d_status, axis, window, other, None, 3)
                rows, seqs = wm.windows(cols, seq_len, genome, status, axis, window, other)
                wm.same(dev.rows, rows, (flags, axis, "rows"))
                wm.same(dev.seqs, seqs, (flags, axis, "summary"))
                assert len(seqs) >= 9 and (seqs["covered"][:, 1] < seqs["covered"][:, 0]).any()
        finally:
            hip.free()
        # the texts: one call for both, the model's formatter over the same status
        for axis, window, other in ((0, 10_000, None), (1, 777, 2)):
            for name in (None,) if other is None else (gnames[other], gnames[other].rstrip("#")):
                g = sw.Windows.from_paf(ctx, paf, status, axis=("query", "target")[axis], window=window, other_genome=name)
                rows, seqs = wm.windows(cols, seq_len, genome, status, axis, window, other)
                assert g.rows == wm.rows_text(rows, names) and g.summary == wm.summary_text(seqs, names, seq_len) and g.rows.count(b"\n") > 100
        one = sw.Windows.from_paf(ctx, paf, status, summary=False)
        rows, seqs = wm.windows(cols, seq_len, genome, status)
        assert one.summary is None and one.rows == wm.rows_text(rows, names)
        one = sw.Windows.from_paf(ctx, paf, None, rows=False)
        assert one.rows is None and one.summary == wm.summary_text(wm.windows(cols, seq_len, genome)[1], names, seq_len)
        with pytest.raises(sw.SwgError) as e:
            sw.Windows.from_paf(ctx, paf, status, other_genome="nobody#0")
        assert e.value.code == -1 and "nobody#0" in str(e.value)
        # covered_all over the sequences of a genome, against one other genome, is breadth's union of that ordered pair
        all_pairs, _ = breadth_records(ctx, paf.records, genome, status, n_genome=G)
        seen = 0
        for other in range(G):
            _, seqs = wm.windows(cols, seq_len, genome, status, 0, 10_000, other)
            got = sw.Windows.from_paf(ctx, paf, status, other_genome=gnames[other], rows=False).summary
            assert got == wm.summary_text(seqs, names, seq_len)
            lines = [l.split(b"\t") for l in got.splitlines()[1:]]
            for p in all_pairs[all_pairs["t_genome"] == other]:
                mine = [int(f[5]) for f in lines if genome[names.index(f[0].decode())] == p["q_genome"]]
                assert sum(mine) == int(p["q_union"]) > 0
                seen += 1
        assert seen == G * (G - 1)


def test_cli_windows(sw, tmp_path):
    from sweepga_amd import build
    from tests.test_gpu_blocks import filter_with_stats
    text = paf_text()
    inp = tmp_path / "in.paf"
    inp.write_text(text, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-filter", "1:1", "--scaffold-dist", "20k", "--quiet"]
    plain, out, rows, summ = (tmp_path / x for x in ("plain.paf", "out.paf", "w.tsv", "s.tsv"))
    with sw.PafFile(text=text) as paf:
        status, _, _ = filter_with_stats(sw, paf, flag_sets(sw)["one_to_one_rescue"])
        cols = handle_columns(paf)
        names, genome = list(paf.names), paf.seq_genome_last[:int(paf.records.n_seq)].copy()
        seq_len, gnames = last_lengths(text, names), genome_names(sw, paf)
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), *flags], capture_output=True)
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--windows", str(rows), "--windows-summary", str(summ), "--windows-axis", "target",
                        "--window-size", "5k", "--windows-genome", gnames[1].rstrip("#"), *flags], capture_output=True)
    assert r0.returncode == r.returncode == 0, r.stderr
    assert out.read_bytes() == plain.read_bytes() and out.stat().st_size > 0 and r.stdout == r0.stdout == b""
    want = wm.windows(cols, seq_len, genome, status, 1, 5_000, 1)
    assert rows.read_bytes() == wm.rows_text(want[0], names) and summ.read_bytes() == wm.summary_text(want[1], names, seq_len) and len(want[0]) > 100
    # --windows - : the rows on standard error, the PAF alone on standard output; the defaults are query, 10k, any genome
    r2 = subprocess.run([build.CLI, str(inp), "--windows", "-", *flags], capture_output=True)
    dflt = wm.windows(cols, seq_len, genome, status)
    assert r2.returncode == 0 and r2.stdout == plain.read_bytes() and r2.stderr == wm.rows_text(dflt[0], names)
    # --no-filter: kept = all
    r3 = subprocess.run([build.CLI, str(inp), "--no-filter", "--windows-summary", str(summ), "--window-size", "64"], capture_output=True)
    every = wm.windows(cols, seq_len, genome, np.ones(len(status), dtype=np.uint8), 0, 64)
    assert r3.returncode == 0 and summ.read_bytes() == wm.summary_text(every[1], names, seq_len)
    assert (every[1]["covered"][:, 0] == every[1]["covered"][:, 1]).all()
    r4 = subprocess.run([build.CLI, str(inp), "--windows", str(rows), "--windows-genome", "nobody", *flags], capture_output=True, text=True)
    assert r4.returncode == 3 and "nobody" in r4.stderr
