"""Placement on the device (sweepga_amd/csrc/swg_place.hip) against tests/place_model.py, field by field and host seam against
device seam: random candidate tables, one candidate whose median's prefix crosses two tile seams, the losing strand between the
deciding records, ties in the anchor under a free permutation, anchors at both ends of their range, weight 0, 1,500 candidates
of one (sequence, genome), sparse ids, interleaved candidates, the request's variants and errors, a memory limit, the status of a
real swg_filter_device run, and the texts of swg_paf_place / --place byte for byte against the model's formatter.  Every
comparison is exact: integers and bytes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import place_model as pm
from tests.test_gpu_alnstats import gen_text, records_of
from tests.test_gpu_blocks import SEED_WITH_RESCUES, flag_sets
from tests.test_gpu_gaps import genome_names
from tests.test_gpu_wide import Hip
from tests.test_place_cpu import COLUMNS, MAJORITY, columns

pytestmark = pytest.mark.gpu
TOP = 2**32 - 1
FILTER_COLS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end", "identity", "matches", "block_len", "strand")


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


def prepared(cols, seq_len, genome, status):
    cols = {k: np.ascontiguousarray(cols[k], dtype=np.uint8 if k == "strand" else np.uint32) for k in COLUMNS}
    return (cols, np.ascontiguousarray(seq_len, dtype=np.uint32), np.ascontiguousarray(genome, dtype=np.uint32),
            None if status is None else np.ascontiguousarray(status, dtype=np.uint8))


def both_seams(sw, cols, seq_len, genome, status=None, axis=0, kept=False, min_bases=0, n_genome=None, ctx=None, want=3):
    """The result of the host seam, after checking that the device seam gives the same bytes."""
    from sweepga_amd.place import _call, place_records
    ctx = ctx or sw.default_context()
    cols, seq_len, genome, status = prepared(cols, seq_len, genome, status)
    if n_genome is None:
        n_genome = int(genome.max()) + 1
    set_ = "kept" if kept else "all"
    host = place_records(ctx, cols, seq_len, genome, status, axis=axis, set=set_, min_bases=min_bases, n_genome=n_genome, want=want)
    hip = Hip()
    try:
        rec = records_of({k: hip.up(v) for k, v in cols.items()}, len(genome), len(cols["q_id"]))
        dev = _call(ctx, ctx.lib.swg_place_records_device, rec, hip.up(seq_len), hip.up(genome), n_genome,
                    hip.up(status) if status is not None else None, axis, set_, min_bases, want)
    finally:
        hip.free()
    for a, b in ((host.rows, dev.rows), (host.pairs, dev.pairs)):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()
    return host


def same(got, want, what):
    """Field by field, so that a difference names its row and field."""
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, i, {k: (g[k], w[k]) for k in w if g[k] != w[k]})


def check(sw, cols, seq_len, genome, status=None, variants=((0, False, 0),), what="", **kw):
    """variants: (axis, kept, min_bases).  -> the result of the first."""
    out = None
    for axis, kept, min_bases in variants:
        got = both_seams(sw, cols, seq_len, genome, status, axis, kept, min_bases, **kw)
        rows, pairs = pm.as_model(got)
        want_rows = pm.place(cols, seq_len, genome, status, axis, kept, min_bases)
        same(rows, want_rows, (what, axis, kept, min_bases))
        same(pairs, pm.summary(want_rows, seq_len), (what, axis, kept, min_bases, "summary"))
        assert not got.rows["reserved"].any()
        out = out or got
    return out


EVERY = ((0, False, 0), (1, False, 0), (0, True, 0), (1, True, 130_000))


def random_table(rng, n, n_cands, n_seq=40, per_genome=4, span=1_000_000, max_len=5_000):
    """n records over n_cands (s, p) pairs of different genomes, candidate-major; -> cols, seq_len, genome, status."""
    genome = (np.arange(n_seq) // per_genome).astype(np.uint32)
    pairs = [(s, p) for s in range(n_seq) for p in range(n_seq) if genome[s] != genome[p]]
    pairs = np.asarray(pairs)[np.sort(rng.choice(len(pairs), n_cands, replace=False))]
    which = np.sort(np.r_[np.arange(n_cands), rng.integers(0, n_cands, n - n_cands)])   # every candidate has a record
    main = rng.random(n_cands) < 0.3
    strand = np.where(rng.random(n) < 0.8, main[which], ~main[which]).astype(np.uint8)
    qs, ts = rng.integers(0, span, n), rng.integers(0, span, n)
    ln = rng.integers(0, max_len, n)
    ln[rng.random(n) < 0.02] = 0
    cols = {"q_id": pairs[which, 0], "t_id": pairs[which, 1], "q_start": qs, "q_end": qs + ln, "t_start": ts,
            "t_end": ts + np.maximum(ln + rng.integers(-20, 20, n), 0), "strand": strand}
    status = rng.choice(np.array([0, 1, 3], dtype=np.uint8), n)
    return {k: np.asarray(v) for k, v in cols.items()}, rng.integers(1_000, 2_000_000, n_seq), genome, status


# ---- 1. the record seams against the model -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["6000_over_300", "8192_over_2000", "one_candidate", "none_taking_part"])
def test_record_seams_against_the_model(sw, shape):
    rng = np.random.default_rng(len(shape))
    if shape == "6000_over_300":
        cols, seq_len, genome, status = random_table(rng, 6_000, 300)
    elif shape == "8192_over_2000":     # about 4 records per candidate: a tile holds hundreds of runs; 100 sequences, two per genome
        cols, seq_len, genome, status = random_table(rng, 8_192, 2_000, n_seq=100, per_genome=2)
    elif shape == "one_candidate":
        cols, seq_len, genome, status = random_table(rng, 3_000, 1)
    else:
        cols, seq_len, genome, status = random_table(rng, 3_000, 300)
        genome[:] = 3                   # one genome: nothing counts
    got = check(sw, cols, seq_len, genome, status, EVERY, what=shape, n_genome=100)
    if shape == "none_taking_part":
        assert len(got.rows) == 0 and len(got.pairs) == 0
    elif shape == "one_candidate":
        assert len(got.rows) == 1 and int(got.rows["n_records"][0]) == 3_000
    else:
        assert len(got.rows) > 100 and set(got.rows["orient"].tolist()) == {0, 1} and int(got.rows["rank"].max()) >= 1
        assert (got.rows["runner_bases"] > 0).any() and len(got.pairs) > 10


def test_hand_case(sw):
    got = check(sw, columns(MAJORITY), [1000, 5000], [0, 1], np.array([1, 1, 1]), ((0, False, 0), (1, True, 0), (0, False, 600), (0, True, 601)), what="hand")
    row = got.rows[0]
    assert (int(row["offset"]), int(row["start"]), int(row["fwd"]), int(row["rev"]), int(row["orient"])) == (1000, 1000, 500, 100, 0)
    assert (int(row["q_lo"]), int(row["q_hi"]), int(row["t_lo"]), int(row["t_hi"])) == (100, 700, 1100, 1720)


# ---- 2. the weighted median across tile seams -------------------------------------------------------------------------------------
@pytest.mark.parametrize("heavy", [None, 0, 2_999, 1_024])
@pytest.mark.parametrize("strand", [0, 1])
def test_one_candidate_of_3000_deciding_records(sw, heavy, strand):
    """Distinct anchors and distinct weights: the prefix that reaches half lies wherever the weights put it; with one record heavier
    than all the others together it is that record -- the first of the sorted order, the last, or the first of the second tile."""
    rng = np.random.default_rng(7)
    n = 3_000
    w = rng.permutation(n) + 1
    if heavy is not None:
        w[heavy] = 5_000_000                    # (the others sum to 4,501,500)
    off = 20_000_000 + 7 * np.arange(n)       # ascending: record i is position i of the (anchor, index) order
    qs = rng.integers(0, 40_000, n)
    if strand == 0:
        rec = [(0, 1, qs[i], qs[i] + w[i], off[i] + qs[i], off[i] + qs[i] + w[i], 0) for i in range(n)]      # off = t_start - q_start
    else:
        rec = [(0, 1, qs[i], qs[i] + w[i], off[i] - qs[i] - w[i], off[i] - qs[i], 1) for i in range(n)]      # off = t_end + q_start
    order = rng.permutation(n)
    cols = columns([rec[i] for i in order])
    got = check(sw, cols, [20_000_000, 30_000_000], [0, 1], variants=((0, False, 0), (0, False, 4_000_000)), what=("3000 deciding", heavy, strand))
    assert len(got.rows) == 1 and int(got.rows["orient"][0]) == strand
    if heavy is not None:
        assert int(got.rows["offset"][0]) == int(off[heavy])
    else:
        prefix = np.cumsum(w)
        assert int(got.rows["offset"][0]) == int(off[np.searchsorted(prefix, (prefix[-1] + 1) // 2)])


@pytest.mark.parametrize("winner", [0, 1])
def test_the_losing_strand_between_the_deciding_records(sw, winner):
    """3,000 records of the winning strand and 2,500 of the other with anchors in between, record by record in the input."""
    rng = np.random.default_rng(11)
    rec = []
    for i in range(3_000):
        off, q = 100_000 + 10 * i, int(rng.integers(0, 50_000))
        rec.append((0, 1, q, q + 100, off + q, off + q + 100, 0) if winner == 0 else (0, 1, q, q + 100, off - q - 100, off - q, 1))
        if i < 2_500:
            off += 5
            rec.append((0, 1, q, q + 90, off - q - 90, off - q, 1) if winner == 0 else (0, 1, q, q + 90, off + q, off + q + 90, 0))
    got = check(sw, columns(rec), [1_000_000, 2_000_000], [0, 1], what=("losing strand", winner))
    row = got.rows[0]
    assert int(row["orient"]) == winner and int(row["n_records"]) == 5_500
    assert (int(row["fwd"]), int(row["rev"])) == ((300_000, 225_000) if winner == 0 else (225_000, 300_000))
    assert int(row["offset"]) == 100_000 + 10 * 1_499       # W = 300,000: half is reached by the 1,500th deciding record


def test_ties_in_the_anchor_under_a_free_permutation(sw):
    rng = np.random.default_rng(21)
    n = 2_000
    off = rng.choice(np.array([5_000, 5_001, 70_000, 900_000]), n)
    qs, w = rng.integers(0, 4_000, n), rng.integers(0, 300, n)
    cols = columns([(0, 1, qs[i], qs[i] + w[i], off[i] + qs[i], off[i] + qs[i] + w[i], 0) for i in range(n)])
    seq_len, genome = [10_000, 2_000_000], [0, 1]
    a = check(sw, cols, seq_len, genome, what="ties")
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(n)
        b = check(sw, {k: v[perm] for k, v in cols.items()}, seq_len, genome, what="ties, permuted")
        assert a.rows.tobytes() == b.rows.tobytes() and a.pairs.tobytes() == b.pairs.tobytes()


# ---- 3. edges ----------------------------------------------------------------------------------------------------------------------
def test_anchors_at_both_ends_and_weight_zero(sw):
    rec = [
        (0, 4, TOP, TOP, 0, 0, 0),             # '+': off = 0 - TOP, the smallest there is; weight 0
        (1, 4, TOP, TOP, TOP, TOP, 1),         # '-': off = TOP + TOP, the largest; weight 0, no '+' record: '-'
        (2, 4, TOP - 10, TOP, 0, 10, 0),       # '+' with a weight: off = -(TOP - 10)
        (2, 4, 0, TOP, 0, TOP, 0),             # ... and the heaviest record there is, off 0: the median
        (3, 4, 0, 0, 0, 0, 1),                 # '-' at off 0 on a sequence of TOP bases: start = -TOP
        (5, 4, 7, 7, 100, 100, 0), (5, 4, 9, 9, 50, 50, 0), (5, 4, 3, 3, 60, 60, 1),   # W = 0 on both strands: '+', anchors 93, 41: 41
    ]
    seq_len = [TOP, TOP, TOP, TOP, TOP, 1000]
    got = check(sw, columns(rec), seq_len, [0, 0, 0, 0, 1, 0], variants=((0, False, 0), (1, False, 0), (0, False, 1)), what="edges")
    by_seq = {int(r["seq"]): r for r in got.rows}
    assert [(int(by_seq[s]["offset"]), int(by_seq[s]["start"]), int(by_seq[s]["orient"])) for s in (0, 1, 2, 3, 5)] == [
        (-TOP, -TOP, 0), (2 * TOP, TOP, 1), (0, 0, 0), (0, -TOP, 1), (41, 41, 0)]
    assert got.rows["seq"].tolist() == [0, 3, 2, 5, 1]          # one partner: by (start, s)
    assert got.rows["rank"].tolist() == [0, 1, 2, 3, 4] and int(got.pairs["length"][0]) == 4 * TOP + 1000


@pytest.mark.parametrize("tie", ["first_and_last", "last_two", "all_equal"])
def test_1500_candidates_of_one_sequence_and_genome(sw, tie):
    rng = np.random.default_rng(3)
    n_p = 1_500
    bases = rng.integers(1, 5_000, n_p)
    if tie == "first_and_last":
        bases[0] = bases[-1] = 9_000
    elif tie == "last_two":
        bases[-2] = bases[-1] = 9_000
    else:
        bases[:] = 77
    # sequence 0 against partners 1 .. 1,500 of genome 1; sequence 1,501 of genome 2 on two of them, so that there is a second row
    rec = [(0, p + 1, 0, bases[p], 10 * p, 10 * p + bases[p], p % 2) for p in range(n_p)]
    rec += [(n_p + 1, 5, 0, 10, 0, 10, 0), (n_p + 1, 1_400, 0, 10, 0, 10, 0)]
    order = rng.permutation(len(rec))
    genome = np.r_[0, np.ones(n_p, dtype=int), 2]
    got = check(sw, columns([rec[i] for i in order]), np.full(n_p + 2, 10_000), genome, variants=((0, False, 0), (1, False, 0)), what=tie)
    row = got.rows[0]
    want_p = {"first_and_last": 1, "last_two": n_p - 1, "all_equal": 1}[tie]
    assert (int(row["seq"]), int(row["partner"]), int(row["runner_bases"]) == int(row["bases"])) == (0, want_p, True)
    assert int(row["total_bases"]) == int(bases.sum()) and (int(got.rows[1]["partner"]), int(got.rows[1]["runner_bases"])) == (5, 10)


def test_sequence_ids_sparse_up_to_2_20(sw):
    rng = np.random.default_rng(17)
    n_seq = (1 << 20) + 1
    used = np.array([0, 5, 1 << 19, (1 << 19) + 1, (1 << 20) - 1, 1 << 20])
    genome = np.zeros(n_seq, dtype=np.uint32)
    genome[used] = [0, 900, 0, 7, 900, 7]
    seq_len = np.full(n_seq, 123, dtype=np.uint32)
    seq_len[used] = rng.integers(1_000, 100_000, len(used))
    n = 3_000
    q, t = used[rng.integers(0, len(used), n)], used[rng.integers(0, len(used), n)]
    qs, ts, ln = rng.integers(0, 90_000, n), rng.integers(0, 90_000, n), rng.integers(0, 900, n)
    cols = columns(np.stack([q, t, qs, qs + ln, ts, ts + ln, rng.random(n) < 0.5], axis=1))
    got = check(sw, cols, seq_len, genome, variants=((0, False, 0), (1, False, 0)), what="sparse", n_genome=901)
    assert len(got.rows) == 12 and got.pairs["genome"].tolist() == [0, 0, 7, 7, 900, 900]


def test_the_candidates_interleaved_one_by_one(sw):
    rng = np.random.default_rng(3)
    cols, seq_len, genome, status = random_table(rng, 6_000, 300)
    a = check(sw, cols, seq_len, genome, status, EVERY, what="candidate-major")
    key = cols["q_id"].astype(np.int64) * 64 + cols["t_id"]
    rank_in_candidate = np.zeros(len(key), dtype=np.int64)
    for k in np.unique(key):
        idx = np.flatnonzero(key == k)
        rank_in_candidate[idx] = np.arange(len(idx))
    perm = np.lexsort((key, rank_in_candidate))     # the first record of every candidate, then the second of every one, ...
    assert (np.diff(key[perm][:300]) > 0).all()
    b = check(sw, {k: v[perm] for k, v in cols.items()}, seq_len, genome, status[perm], EVERY, what="interleaved")
    assert a.rows.tobytes() == b.rows.tobytes() and a.pairs.tobytes() == b.pairs.tobytes()


# ---- 4. the request ------------------------------------------------------------------------------------------------------------------
def test_each_want_bit(sw):
    rng = np.random.default_rng(31)
    cols, seq_len, genome, status = random_table(rng, 6_000, 300)
    for axis, kept in ((0, False), (1, True)):
        both = both_seams(sw, cols, seq_len, genome, status, axis, kept, 1_000)
        rows_only = both_seams(sw, cols, seq_len, genome, status, axis, kept, 1_000, want=1)
        summary_only = both_seams(sw, cols, seq_len, genome, status, axis, kept, 1_000, want=2)
        assert rows_only.pairs is None and rows_only.rows.tobytes() == both.rows.tobytes() and len(both.rows) > 50
        assert summary_only.rows is None and summary_only.pairs.tobytes() == both.pairs.tobytes() and len(both.pairs) > 5


def request(cols, n_seq, want=3):
    from sweepga_amd._lib import SwgPlaceRequest
    req = SwgPlaceRequest()
    req.want = want
    return records_of(cols, n_seq), req


def test_input_errors_and_the_capacity_protocol(sw):
    from sweepga_amd._lib import SwgPlacePair, SwgPlacement
    from sweepga_amd.place import PAIR_DTYPE, ROW_DTYPE, place_records
    ctx = sw.default_context()
    rng = np.random.default_rng(41)
    cols, seq_len, genome, status = random_table(rng, 500, 60, n_seq=12, per_genome=3)
    cols, seq_len, genome, status = prepared(cols, seq_len, genome, status)
    want_rows = pm.place(cols, seq_len, genome)
    want_pairs = pm.summary(want_rows, seq_len)
    assert len(want_rows) > 10 and len(want_pairs) > 3
    for field, value in (("q_id", 12), ("t_id", 12), ("q_id", TOP)):      # a sequence id >= n_seq, on a record that would take part or not
        bad = {k: v.copy() for k, v in cols.items()}
        bad[field][250] = value
        with pytest.raises(sw.SwgError) as e:
            place_records(ctx, bad, seq_len, genome)
        assert e.value.code == -1 and "n_seq" in str(e.value)
    with pytest.raises(sw.SwgError) as e:
        place_records(ctx, cols, seq_len, genome, n_genome=3)              # genome id 3 >= n_genome
    assert e.value.code == -1
    with pytest.raises(sw.SwgError) as e:
        place_records(ctx, cols, seq_len, genome, None, set="kept")        # the kept set without a status
    assert e.value.code == -1
    rec, req = request(cols, 12)
    args = (seq_len.ctypes.data, genome.ctypes.data, 4, status.ctypes.data)
    call = lambda: ctx.lib.swg_place_records(ctx.handle, C.byref(rec), *args, C.byref(req))   # noqa: E731
    for field, value in (("reserved", 1), ("want", 0), ("want", 4), ("axis", 2), ("set", 2)):
        before = getattr(req, field)
        setattr(req, field, value)
        assert call() == -1, field
        setattr(req, field, before)
    rec.n = 2**31                                                           # refused before a column is looked at
    assert call() == -5
    rec.n = 500
    rec.n_seq = 2**31 + 1                                                   # the key packing's limit
    assert call() == -5
    rec.n_seq = 12
    for column in ("strand", "q_id", "t_end"):
        held = getattr(rec, column)
        setattr(rec, column, None)
        assert call() == -1, column
        setattr(rec, column, held)
    assert ctx.lib.swg_place_records(ctx.handle, C.byref(rec), None, genome.ctypes.data, 4, status.ctypes.data, C.byref(req)) == -1
    assert ctx.lib.swg_place_records(ctx.handle, C.byref(rec), seq_len.ctypes.data, None, 4, status.ctypes.data, C.byref(req)) == -1
    # the capacity protocol: SWG_OK, the counts say how many there are, the arrays are left alone -- each array on its own
    n_rows, n_pairs = len(want_rows), len(want_pairs)
    rows = np.frombuffer(bytearray(b"\xab" * 104 * n_rows), dtype=ROW_DTYPE)
    pairs = np.frombuffer(bytearray(b"\xcd" * 48 * n_pairs), dtype=PAIR_DTYPE)
    before = rows.tobytes(), pairs.tobytes()
    req.rows, req.pairs = C.cast(rows.ctypes.data, C.POINTER(SwgPlacement)), C.cast(pairs.ctypes.data, C.POINTER(SwgPlacePair))
    req.capacity, req.pair_capacity = n_rows - 1, n_pairs - 1
    assert call() == 0
    assert (int(req.n_rows), int(req.n_pairs)) == (n_rows, n_pairs) and (rows.tobytes(), pairs.tobytes()) == before
    req.pair_capacity = n_pairs                                            # the pairs fit, the rows do not
    assert call() == 0 and rows.tobytes() == before[0]
    same([{k: int(p[k]) for k in pm.PAIR_FIELDS} for p in pairs], want_pairs, "pairs alone")
    pairs[:] = np.frombuffer(before[1], dtype=PAIR_DTYPE)
    req.capacity, req.pair_capacity = n_rows, n_pairs - 1                  # ... and the other way round
    assert call() == 0 and pairs.tobytes() == before[1]
    same([{k: int(r[k]) for k in pm.FIELDS} for r in rows], want_rows, "rows alone")
    req.rows, req.pairs = None, None                                       # NULL arrays: the counts alone
    assert call() == 0 and (int(req.n_rows), int(req.n_pairs)) == (n_rows, n_pairs)
    check(sw, cols, seq_len, genome, status, EVERY, what="after the refusals")


def test_a_memory_limit_too_small_is_a_clean_oom(sw):
    from sweepga_amd.place import place_records
    ctx = sw.Context(0)
    try:
        cols, seq_len, genome, status = random_table(np.random.default_rng(51), 200_000, 1_200)
        ctx.set_memory_limit(1 << 20)       # the staged columns alone are 5 MB
        with pytest.raises(sw.SwgError) as e:
            place_records(ctx, cols, seq_len, genome, status)
        assert e.value.code == -4
        ctx.set_memory_limit(0)             # ... and the context works on
        want = both_seams(sw, cols, seq_len, genome, status, 0, True)
        got = both_seams(sw, cols, seq_len, genome, status, 0, True, ctx=ctx)
        ctx.set_memory_limit(1 << 30)
        limited = both_seams(sw, cols, seq_len, genome, status, 0, True, ctx=ctx)
        for r in (got, limited):
            assert r.rows.tobytes() == want.rows.tobytes() and r.pairs.tobytes() == want.pairs.tobytes() and len(r.rows) > 300
        assert ctx.memory_info()[0] <= 1 << 30
    finally:
        ctx.close()


# ---- 5. a real filter ----------------------------------------------------------------------------------------------------------------
def filter_on_the_device(sw, paf, cfg, hip):
    """swg_filter_device over the handle's columns -> (SwgRecords on the device, device status, host status)."""
    from sweepga_amd._lib import SwgRecords, SwgStats
    ctx = sw.default_context()
    r = SwgRecords()
    r.n, r.n_seq = paf.n, int(paf.records.n_seq)
    for k in FILTER_COLS:
        setattr(r, k, hip.up(paf.column(k)))
    r.seq_genome_last, r.n_genome_last = hip.up(paf.seq_genome_last), int(paf.records.n_genome_last)
    r.seq_genome_two, r.n_genome_two = hip.up(paf.seq_genome_two), int(paf.records.n_genome_two)
    d_status, d_chain = hip.alloc(paf.n), hip.alloc(4 * paf.n)
    cc = cfg.to_c(False, False)
    ctx.check(ctx.lib.swg_filter_device(ctx.handle, C.byref(r), C.byref(cc), C.c_void_p(d_status), C.c_void_p(d_chain), C.byref(SwgStats())))
    return r, d_status, hip.down(d_status, np.uint8, paf.n)


def paf_text(n=6_000):
    return gen_text(SEED_WITH_RESCUES, n, n_genomes=4, chrs_per_genome=3, span=400_000)


def last_lengths(text, names):
    from tests import components_model as cm
    return np.asarray(cm.last_lengths(text, names), dtype=np.uint32)


@pytest.mark.parametrize("flags", ["default", "one_to_one_rescue"])
def test_the_status_of_a_real_filter_on_the_device(sw, flags):
    from sweepga_amd.place import _call
    text = paf_text()
    ctx = sw.default_context()
    with sw.PafFile(text=text) as paf:
        cols = {k: paf.column(k).copy() for k in COLUMNS}
        n_seq, G = int(paf.records.n_seq), int(paf.records.n_genome_last)
        genome, names = paf.seq_genome_last[:n_seq].copy(), list(paf.names)
        seq_len = last_lengths(text, names)
        hip = Hip()
        try:
            rec, d_status, status = filter_on_the_device(sw, paf, flag_sets(sw)[flags], hip)
            d_len = hip.up(seq_len)
            assert 0 < int((status != 0).sum()) < paf.n
            for axis, kept, min_bases in EVERY:      # the columns where the filter read them, the status where it wrote it
                dev = _call(ctx, ctx.lib.swg_place_records_device, rec, d_len, rec.seq_genome_last, G, d_status, axis, "kept" if kept else "all", min_bases, 3)
                rows, pairs = pm.as_model(dev)
                want = pm.place(cols, seq_len, genome, status, axis, kept, min_bases)
                same(rows, want, (flags, axis, kept, min_bases))
                same(pairs, pm.summary(want, seq_len), (flags, axis, kept, min_bases, "summary"))
                assert len(rows) >= 12 or min_bases
        finally:
            hip.free()
        # the texts: one call for both, the model's formatter over the same status
        for axis, kept, min_bases in EVERY:
            g = sw.Place.from_paf(ctx, paf, status, axis=("query", "target")[axis], set="kept" if kept else "all", min_bases=min_bases)
            want = pm.place(cols, seq_len, genome, status, axis, kept, min_bases)
            assert g.rows == pm.rows_text(want, names, seq_len) and (g.rows.count(b"\n") > 12 or min_bases)
            assert g.summary == pm.summary_text(pm.summary(want, seq_len), genome_names(sw, paf))
            table = g.table
            assert table["start"].tolist() == [r["start"] for r in want] and table["sequence"].tolist() == [names[r["seq"]] for r in want]
        one = sw.Place.from_paf(ctx, paf, status, summary=False)
        assert one.summary is None and one.rows == pm.rows_text(pm.place(cols, seq_len, genome, status, 0, True), names, seq_len)
        one = sw.Place.from_paf(ctx, paf, None, set="all", rows=False)
        assert one.rows is None and one.summary == pm.summary_text(pm.summary(pm.place(cols, seq_len, genome), seq_len), genome_names(sw, paf))


# ---- 6. the command line ----------------------------------------------------------------------------------------------------------------
def test_cli_place(sw, tmp_path):
    from sweepga_amd import build
    from tests.test_gpu_blocks import filter_with_stats
    text = paf_text()
    inp = tmp_path / "in.paf"
    inp.write_text(text, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-filter", "1:1", "--scaffold-dist", "20k", "--quiet"]
    plain, out, rows, summ = (tmp_path / x for x in ("plain.paf", "out.paf", "p.tsv", "s.tsv"))
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), *flags], capture_output=True)
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--place", str(rows), "--place-summary", str(summ), "--place-axis", "target",
                        "--place-set", "all", "--place-min-bases", "170k", *flags], capture_output=True)
    assert r0.returncode == r.returncode == 0, r.stderr
    assert out.read_bytes() == plain.read_bytes() and out.stat().st_size > 0 and r.stdout == r0.stdout == b""
    with sw.PafFile(text=text) as paf:
        status, _, _ = filter_with_stats(sw, paf, flag_sets(sw)["one_to_one_rescue"])
        cols = {k: paf.column(k).copy() for k in COLUMNS}
        names, genome = list(paf.names), paf.seq_genome_last[:int(paf.records.n_seq)].copy()
        seq_len, gnames = last_lengths(text, names), genome_names(sw, paf)
    want = pm.place(cols, seq_len, genome, status, 1, False, 170_000)
    assert rows.read_bytes() == pm.rows_text(want, names, seq_len) and summ.read_bytes() == pm.summary_text(pm.summary(want, seq_len), gnames)
    assert 3 < len(want) < len(pm.place(cols, seq_len, genome, status, 1, False, 0))
    # --place - : the rows on standard error, the PAF alone on standard output; the defaults are query, kept, 0
    r2 = subprocess.run([build.CLI, str(inp), "--place", "-", *flags], capture_output=True)
    dflt = pm.place(cols, seq_len, genome, status, 0, True, 0)
    assert r2.returncode == 0 and r2.stdout == plain.read_bytes() and r2.stderr == pm.rows_text(dflt, names, seq_len)
    # --no-filter: kept = all
    r3 = subprocess.run([build.CLI, str(inp), "--no-filter", "--place-summary", str(summ), "--place-set", "kept"], capture_output=True)
    every = pm.place(cols, seq_len, genome)
    assert r3.returncode == 0 and summ.read_bytes() == pm.summary_text(pm.summary(every, seq_len), gnames)


def test_smallest_shapes_on_a_fresh_context(sw):
    """The seams around the kernels at the smallest shapes -- one record; three records of one candidate -- on a context of its
    own: its first call sizes the arena from the input, the later ones find it sized.  Each shape twice, host seam against device
    seam byte for byte and both against the model."""
    ctx = sw.Context(0)
    try:
        for n in (1, 3, 1, 3):
            got = check(sw, columns(MAJORITY[:n]), [1000, 5000], [0, 1], variants=((0, False, 0), (1, False, 0)), what=f"n = {n}", ctx=ctx)
            assert len(got.rows) == 1 and int(got.rows["n_records"][0]) == n and len(got.pairs) == 1
    finally:
        ctx.close()
