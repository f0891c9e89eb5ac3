"""The transitive lift on the device (sweepga_amd/csrc/swg_lift_closure.hip) against tests/lift_closure_model.py: in every case the
host seam against the model and the device seam against the host seam, byte for byte.  The shapes are the smallest at which each
part can go wrong: the tile of T = 1024 candidates and the frontier's borders, regions that die between regions that live, touching
and overlapping projections, a projection that the visited set cuts three times, min_len and its border, a key of more than 64
bits, the largest coordinates, axes and sets, permutations, the capacity protocol, a memory limit, and the three texts."""
import subprocess

import numpy as np
import pytest

from tests import lift_closure_model as cm
from tests import lift_model as lm
from tests.test_gpu_alnstats import filter_cfgs, gen_text, run_filter
from tests.test_gpu_breadth import SHAPE_NAMES, shape_texts
from tests.test_gpu_intervals import kept_mask
from tests.test_gpu_lift import Dev, columns, random_bed, random_regions
from tests.test_gpu_wide import Hip
from tests.test_lift_closure_cpu import HAND_BED, HAND_ROWS, HAND_SUMMARY, HAND_SUMMARY_TEXT, HAND_TEXT, hand_case, hand_paf, paf_closure

pytestmark = pytest.mark.gpu
COLS = lm.COLS
T = 1024
U = lm.UNKNOWN


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


def same(a, b):
    return (a.n == b.n and a.hops_run == b.hops_run and a.projections == b.projections and a.candidates == b.candidates and
            a.summary.tobytes() == b.summary.tobytes() and a.rows.tobytes() == b.rows.tobytes())


def both_seams(sw, cols, strand, n_seq, regions, status, hops, min_len, set_=0, axes=3, ctx=None):
    """The result of the host seam, after checking that the device seam gives the same bytes."""
    from sweepga_amd.lift import lift_closure_records, lift_closure_records_device, regions_array
    ctx = ctx or sw.default_context()
    got = lift_closure_records(ctx, cols, strand, n_seq, regions, hops, min_len, status=status, set=set_, axes=axes)
    regs = regions_array(regions)
    hip = Hip()
    try:
        dcols = {k: Dev(hip, cols[k], np.uint32) for k in COLS}
        dev = lift_closure_records_device(ctx, dcols, Dev(hip, strand, np.uint8), n_seq, Dev(hip, regs.view(np.uint32)), len(regs), hops, min_len,
                                          status=Dev(hip, status, np.uint8) if status is not None else None, set=set_, axes=axes)
    finally:
        hip.free()
    assert same(dev, got)
    return got


def check(sw, cols, strand, n_seq, regions, status, hops, min_len=100, set_=0, axes=3, what="", ctx=None):
    """Both seams against the model."""
    cols = {k: np.asarray(cols[k]).astype(np.uint32) for k in COLS}
    strand = np.asarray(strand).astype(np.uint8)
    got = both_seams(sw, cols, strand, n_seq, regions, status, hops, min_len, set_, axes, ctx)
    rows, summary, info = cm.closure(cols, strand, None if status is None else np.asarray(status) != 0, regions, hops, min_len, set_, axes)
    assert got.n == len(rows) == len(got.rows), (what, got.n, len(rows))
    assert got.rows.tobytes() == cm.rows_array(rows).tobytes(), (what, [tuple(r) for r in got.rows[:8]], rows[:8])
    assert got.summary.tobytes() == cm.summary_array(summary).tobytes(), what
    assert (got.hops_run, got.projections, list(got.candidates)) == (info["hops_run"], info["projections"], info["candidates"]), what
    return got


def no_overlap(rows):
    for u, w in zip(rows, rows[1:]):
        assert (u["region"], u["seq"]) != (w["region"], w["seq"]) or u["end"] <= w["start"]


def test_hand_case(sw):
    cols, strand, kept, regions = hand_case()
    status = kept.astype(np.uint8) * 2
    got = check(sw, cols, strand, 3, regions, status, 3, 10, what="hand")
    assert [tuple(int(v) for v in r) for r in got.rows[:5]] == HAND_ROWS and tuple(int(v) for v in got.summary[0]) == HAND_SUMMARY
    assert got.hops_run == 3
    check(sw, cols, strand, 3, regions, None, 3, 10, what="hand, no status")
    for hops, min_len, set_, axes in ((1, 10, 0, 3), (2, 10, 0, 3), (100, 10, 0, 3), (3, 36, 0, 3), (3, 35, 0, 3), (3, 1, 0, 3), (3, 0, 0, 3), (5, 10, 1, 3),
                                      (5, 10, 0, 1), (5, 10, 0, 2), (65535, 1, 1, 2)):
        check(sw, cols, strand, 3, regions, status, hops, min_len, set_, axes, what=(hops, min_len, set_, axes))


def test_query_axis_alone_makes_the_walk_directional(sw):
    cols, strand, kept, regions = hand_case()
    got = check(sw, cols, strand, 3, regions[:1], None, 5, 10, 0, 1)
    assert [int(s) for s in got.rows["seq"]] == [0, 1, 2] and [int(h) for h in got.rows["hop"]] == [0, 1, 2]
    back = check(sw, cols, strand, 3, regions[3:], None, 5, 10, 0, 1)       # from C the query axis leads nowhere
    assert back.n == 1 and back.hops_run == 1


def small_random(seed, n=300, n_seq=6, m=20):
    rng = np.random.default_rng(seed)
    qs, ts = rng.integers(0, 20_000, n), rng.integers(0, 20_000, n)
    ln = rng.integers(0, 3_000, n)
    cols = {"q_id": rng.integers(0, n_seq, n), "t_id": rng.integers(0, n_seq, n), "q_start": qs, "q_end": qs + ln, "t_start": ts,
            "t_end": ts + (ln * rng.uniform(0.5, 1.5, n)).astype(np.int64)}
    cols = {k: np.asarray(v).astype(np.uint32) for k, v in cols.items()}
    strand, status = (rng.random(n) < 0.3).astype(np.uint8), (rng.random(n) < 0.5).astype(np.uint8)
    regions = [(int(rng.integers(0, n_seq)), int(a), int(a) + int(w)) for a, w in zip(rng.integers(0, 20_000, m), rng.integers(0, 2_000, m))]
    return cols, strand, status, regions, n_seq


@pytest.mark.parametrize("set_,axes", [(0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3)])
def test_one_hop_is_the_merged_dst_of_the_lift(sw, set_, axes):
    from sweepga_amd.lift import lift_records
    cols, strand, status, regions, n_seq = small_random(5)
    got = check(sw, cols, strand, n_seq, regions, status, 1, 100, set_, axes)
    lifted = lift_records(sw.default_context(), cols, strand, n_seq, regions, status=status, set=set_, axes=axes)
    want = {}
    for w in lifted.rows:
        if w["dst_start"] < w["dst_end"]:
            want.setdefault((int(w["region"]), int(w["dst_seq"])), []).append((int(w["dst_start"]), int(w["dst_end"])))
    have = {}
    for w in got.rows:
        if w["hop"] == 1:
            have.setdefault((int(w["region"]), int(w["seq"])), []).append((int(w["start"]), int(w["end"])))
    assert len(want) > 10
    for (r, s), ivs in want.items():
        own = [(regions[r][1], regions[r][2])] if regions[r][0] == s else []
        assert cm.minus(cm.merged(ivs), own) == have.pop((r, s), [])
    assert not have


def test_a_cycle_closes_by_itself(sw):
    rows = [(0, 1, 0, 1_000, 0, 1_000, 0, 1), (1, 2, 0, 1_000, 0, 1_000, 0, 1), (2, 0, 0, 1_000, 0, 1_000, 1, 1)]      # A -> B -> C -> A, D = L
    cols, strand, status = columns(rows)
    ten = check(sw, cols, strand, 3, [(0, 100, 200), (1, 0, 1_000)], status, 10, 1, 0, 1, "cycle, query axis")
    hundred = check(sw, cols, strand, 3, [(0, 100, 200), (1, 0, 1_000)], status, 100, 1, 0, 1)
    assert ten.hops_run < 10 and ten.hops_run == hundred.hops_run and ten.rows.tobytes() == hundred.rows.tobytes()
    assert not (ten.summary["flags"] & 1).any() and ten.n > 2
    no_overlap(ten.rows)
    both = check(sw, cols, strand, 3, [(0, 100, 200)], status, 100, 1, 0, 3, "cycle, both axes")
    assert both.hops_run < 100
    no_overlap(both.rows)


# ---- tile and frontier borders ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [T - 1, T, T + 1, 3 * T + 5])
def test_a_frontier_of_c_pieces(sw, c):
    """Record k takes all of A [0, 100) to B [3 k, 3 k + 1): hop 1 has c candidates of one region and makes c pieces 2 bases apart,
    hop 2 has c frontier pieces of one candidate each, which all lead back onto the region."""
    rows = [(0, 1, 0, 100, 3 * k, 3 * k + 1, k % 2, 1) for k in range(c)]
    cols, strand, status = columns(rows)
    got = check(sw, cols, strand, 2, [(0, 0, 100)], status, 3, 1, 0, 3, "c = %d" % c)
    assert got.n == c + 1 and got.hops_run == 2 and got.projections == 2 * c and got.candidates == (c, c)
    assert tuple(int(v) for v in got.summary[0]) == (100 + c, c + 1, 2, 1, 0)


def test_1025_overlapping_projections_merge_into_one_piece(sw):
    rows = [(0, 1, 0, 100, k, k + 500, k % 2, 1) for k in range(1_025)]
    cols, strand, status = columns(rows)
    got = check(sw, cols, strand, 2, [(0, 0, 100)], status, 1, 1, 0, 1)
    assert [tuple(int(v) for v in r) for r in got.rows] == [(0, 0, 0, 100, 0, 0), (0, 1, 0, 1_524, 1, 0)] and got.projections == 1_025


def test_touching_intervals_are_one_and_a_gap_of_one_base_separates(sw):
    rows = [(0, 1, 0, 100, 0, 10, 0, 1), (0, 1, 0, 100, 10, 20, 1, 1), (0, 2, 0, 100, 0, 10, 0, 1), (0, 2, 0, 100, 11, 20, 0, 1)]
    cols, strand, status = columns(rows)
    got = check(sw, cols, strand, 3, [(0, 0, 100)], status, 1, 1, 0, 1)
    assert [tuple(int(v) for v in r)[1:4] for r in got.rows] == [(0, 0, 100), (1, 0, 20), (2, 0, 10), (2, 11, 20)]


@pytest.mark.parametrize("apart", [False, True])
def test_300_regions_that_die_at_hop_1_between_two_that_keep_40_pieces(sw, apart):
    """Sequences 0 and 2 hold 40 records each under their region, to disjoint pieces of sequence 3 (with `apart`: sequence 0 holds
    1,000 more whose other side is empty -- candidates and hits that make no interval -- so that the last region lies in the next
    tile); the 300 regions between lie on sequence 1, which has no record, on an unknown name, or are empty."""
    rows = [(0, 3, 10 * k, 10 * k + 500, 20 * k, 20 * k + 9, 0, 1) for k in range(40)] + [(2, 3, 10 * k, 10 * k + 500, 5_000 + 20 * k, 5_005 + 20 * k, 1, 1) for k in range(40)]
    if apart:
        rows += [(0, 3, 100 + k % 7, 300 + k, 5, 5, 0, 1) for k in range(1_000)]
    between = [((1, 5 * k, 5 * k + 100), (U, 0, 9), (0, k, k))[k % 3] for k in range(300)]
    regions = [(0, 0, 1_000)] + between + [(2, 0, 1_000)]
    cols, strand, status = columns(rows)
    got = check(sw, cols, strand, 4, regions, status, 3, 1, 0, 3, "300 dying regions")
    assert int(got.summary["pieces"][0]) == 41 and int(got.summary["pieces"][301]) == 41 and got.candidates[0] == (1_080 if apart else 80)
    assert [int(p) for p in got.summary["pieces"][1:301]] == [(1, 0, 0)[k % 3] for k in range(300)]


def test_a_projection_that_the_visited_set_cuts_at_both_ends_and_in_the_middle(sw):
    """Hop 1 visits B [100, 110), [150, 160) and [200, 210); at hop 2 the first of them leads to all of B [90, 220): four new pieces."""
    rows = [(0, 1, 0, 10, 100, 110, 0, 1), (0, 1, 10, 20, 150, 160, 0, 1), (0, 1, 20, 30, 200, 210, 0, 1), (1, 1, 100, 110, 90, 220, 0, 1)]
    cols, strand, status = columns(rows)
    got = check(sw, cols, strand, 2, [(0, 0, 30)], status, 2, 1, 0, 1)
    on_b = [tuple(int(v) for v in r)[2:5] for r in got.rows if r["seq"] == 1]
    assert on_b == [(90, 100, 2), (100, 110, 1), (110, 150, 2), (150, 160, 1), (160, 200, 2), (200, 210, 1), (210, 220, 2)]
    check(sw, cols, strand, 2, [(0, 0, 30)], status, 4, 1, 0, 3)


def test_min_len_and_its_border(sw):
    """Hop 1 makes B [0, 49) and C [0, 50); with min_len = 50 only the piece on C is walked on (to E), B's is reported and left."""
    rows = [(0, 1, 0, 100, 0, 49, 0, 1), (0, 2, 0, 100, 0, 50, 0, 1), (1, 3, 0, 49, 0, 10, 0, 1), (2, 4, 0, 50, 0, 10, 1, 1)]
    cols, strand, status = columns(rows)
    got = check(sw, cols, strand, 5, [(0, 0, 100)], status, 2, 50, 0, 1)
    assert [int(s) for s in got.rows["seq"]] == [0, 1, 2, 4]
    assert [int(s) for s in check(sw, cols, strand, 5, [(0, 0, 100)], status, 2, 49, 0, 1).rows["seq"]] == [0, 1, 2, 3, 4]
    zero, one = (check(sw, cols, strand, 5, [(0, 0, 100)], status, 3, v, 0, 3) for v in (0, 1))
    assert same(zero, one) and (zero.summary["flags"] == one.summary["flags"]).all()


def test_a_key_of_more_than_64_bits(sw):
    """70,000 sequences and 70,000 regions: owner (17 bits), sequence (17 bits) and position (33 bits) do not fit one 64-bit key.  The
    records sit on the highest ids, the live regions are the highest and the lowest; positions are above 2^31."""
    n_seq = m = 70_000
    top, hi = n_seq - 1, 2**31 + 12_345
    rows = [(top, top - 1, hi, hi + 1_000, hi + 500, hi + 1_500, 0, 1), (top - 1, top - 2, hi + 600, hi + 1_400, 100, 900, 1, 1),
            (top - 2, 32_768, 0, 1_000, hi, hi + 990, 0, 1), (65_536, top, 50, 60, hi + 10, hi + 20, 0, 1), (32_767, top - 1, 7, 8, hi + 700, hi + 703, 1, 1)]
    cols, strand, status = columns(rows)
    regions = [(U, 0, 10) if k % 5 else (top, k, k) for k in range(m)]
    regions[0] = (top, hi + 100, hi + 400)
    regions[65_536] = (65_536, 0, 100)
    for k in range(m - 4, m):
        regions[k] = (top - (k % 3), hi + 100 * (k % 4), hi + 1_000)
    got = check(sw, cols, strand, n_seq, regions, status, 4, 1, 0, 3, "wide key")
    live = [0, 65_536] + list(range(m - 4, m))
    assert sorted(set(int(r) for r in got.rows["region"])) == sorted(live) and got.n > 20
    assert {top, top - 1, top - 2, 32_768, 65_536, 32_767} <= set(int(s) for s in got.rows["seq"])
    no_overlap(got.rows)


def test_coordinates_at_the_top_of_32_bits(sw):
    top = 2**32 - 1
    rows = [(0, 1, top - 100, top, top - 50, top, 0, 1), (1, 2, top - 40, top, top - 7, top, 1, 1), (2, 0, 0, top, 0, top, 0, 1)]
    cols, strand, status = columns(rows)
    got = check(sw, cols, strand, 3, [(0, top - 100, top), (0, top - 1, top), (2, 0, top)], status, 4, 1, 0, 3, "2^32 - 1")
    assert int(got.rows["end"].max()) == top and int(got.summary["bases"].max()) >= top


# ---- sets, permutations, real statuses ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shapes():
    return shape_texts()


@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_all_against_kept_under_a_real_filter_status(sw, shapes, shape):
    rng = np.random.default_rng(len(shape))
    with sw.PafFile(text=shapes[shape]) as paf:
        status, _ = run_filter(sw, paf, filter_cfgs(sw)["one_to_one"])
        cols = {c: paf.column(c).copy() for c in COLS}
        strand = paf.column("strand").copy()
        n_seq = int(paf.records.n_seq)
    assert int((status != 0).sum()) > 0
    regions = random_regions(rng, cols, n_seq, 12)
    every = check(sw, cols, strand, n_seq, regions, status, 2, 100, 0, 3, shape)
    kept = check(sw, cols, strand, n_seq, regions, status, 2, 100, 1, 3, shape)
    assert every.summary["bases"].sum() >= kept.summary["bases"].sum() and every.projections >= kept.projections > 0
    # a random permutation of the records leaves the rows' bytes unchanged
    perm = rng.permutation(len(strand))
    moved = both_seams(sw, {k: v[perm] for k, v in cols.items()}, strand[perm], n_seq, regions, status[perm], 2, 100, 1, 3)
    assert moved.rows.tobytes() == kept.rows.tobytes() and moved.summary.tobytes() == kept.summary.tobytes()
    assert (moved.hops_run, moved.projections) == (kept.hops_run, kept.projections)


@pytest.mark.parametrize("min_len", [1, 100])
def test_2000_random_records_on_16_sequences_of_4_genomes(sw, min_len):
    rng = np.random.default_rng(17)
    n, n_seq = 2_000, 16
    qs, ts = rng.integers(0, 300_000, n), rng.integers(0, 300_000, n)
    ln = np.where(rng.random(n) < 0.05, rng.integers(0, 40_000, n), rng.integers(0, 3_000, n))
    cols = {"q_id": rng.integers(0, n_seq, n), "t_id": rng.integers(0, n_seq, n), "q_start": qs, "q_end": qs + ln, "t_start": ts,
            "t_end": ts + (ln * rng.uniform(0.5, 1.5, n)).astype(np.int64)}
    cols = {k: np.asarray(v).astype(np.uint32) for k, v in cols.items()}
    strand, status = (rng.random(n) < 0.3).astype(np.uint8), (rng.random(n) < 0.5).astype(np.uint8)
    regions = random_regions(rng, cols, n_seq, 50)
    regions = [(s, a, a + (b - a) // 40) for s, a, b in regions]       # 25 - 2,500 bases
    got = check(sw, cols, strand, n_seq, regions, status, 3, min_len, 0, 3, "random")
    assert got.hops_run == 3 and got.n > 500 and got.projections > got.n
    no_overlap(got.rows)
    perm = rng.permutation(n)
    moved = both_seams(sw, {k: v[perm] for k, v in cols.items()}, strand[perm], n_seq, regions, status[perm], 3, min_len, 0, 3)
    assert moved.rows.tobytes() == got.rows.tobytes() and moved.summary.tobytes() == got.summary.tobytes()
    check(sw, cols, strand, n_seq, regions[:20], status, 3, min_len, 1, 2, "random, kept, target axis")


# ---- the protocol -------------------------------------------------------------------------------------------------------------------
def test_capacity_protocol_and_calls_without_records_or_regions(sw):
    from sweepga_amd.lift import lift_closure_records, lift_closure_records_device, regions_array
    ctx = sw.default_context()
    cols, strand, kept, regions = hand_case()
    full = lift_closure_records(ctx, cols, strand, 3, regions, 3, 10)
    assert full.n == 8
    short = lift_closure_records(ctx, cols, strand, 3, regions, 3, 10, capacity=full.n - 1)
    assert short.rows is None and short.n == full.n and short.summary.tobytes() == full.summary.tobytes() and short.projections == full.projections
    exact = lift_closure_records(ctx, cols, strand, 3, regions, 3, 10, capacity=full.n)
    assert exact.rows.tobytes() == full.rows.tobytes()
    assert lift_closure_records(ctx, cols, strand, 3, regions, 3, 10, capacity=0).rows is None
    # no regions; no records: hop 0 alone, made on the host
    assert lift_closure_records(ctx, cols, strand, 3, [], 3, 10).n == 0
    none = {k: np.zeros(0, dtype=np.uint32) for k in COLS}
    want = cm.closure(none, np.zeros(0, dtype=np.uint8), None, regions, 3, 10)
    got = lift_closure_records(ctx, none, np.zeros(0, dtype=np.uint8), 3, regions, 3, 10)
    assert got.rows.tobytes() == cm.rows_array(want[0]).tobytes() and got.summary.tobytes() == cm.summary_array(want[1]).tobytes()
    assert (got.n, got.hops_run, got.projections) == (2, 0, 0)
    hip = Hip()
    try:
        empty = Dev(hip, np.zeros(1, dtype=np.uint32))
        empty.a = empty.a[:0]
        regs = regions_array(regions)
        dev = lift_closure_records_device(ctx, {k: empty for k in COLS}, Dev(hip, np.zeros(1, dtype=np.uint8)), 3, Dev(hip, regs.view(np.uint32)), len(regs), 3, 10)
    finally:
        hip.free()
    assert same(dev, got)
    for bad in ([(3, 0, 10)], [(0, 10, 5)]):      # the regions' faults, with and without records
        for c, s in ((cols, strand), (none, np.zeros(0, dtype=np.uint8))):
            with pytest.raises(sw.SwgError) as e:
                lift_closure_records(ctx, c, s, 3, bad, 3, 10)
            assert e.value.code == -1
    for hops in (0, 65_536):
        with pytest.raises(sw.SwgError) as e:
            lift_closure_records(ctx, cols, strand, 3, regions, hops, 10)
        assert e.value.code == -1 and "max_hops" in str(e.value)


def test_a_memory_limit_too_small_is_a_clean_oom(sw):
    from sweepga_amd.lift import lift_closure_records
    ctx = sw.Context(0)
    try:
        n = 200_000
        cols = {k: np.arange(n, dtype=np.uint32) % 1_000 + (100 if k.endswith("end") else 0) for k in COLS}
        cols["q_id"] = np.zeros(n, dtype=np.uint32)
        cols["t_id"] = np.ones(n, dtype=np.uint32)
        strand = np.zeros(n, dtype=np.uint8)
        ctx.set_memory_limit(4 << 20)       # the index of one axis alone is 24 bytes per record: 4.8 MB
        with pytest.raises(sw.SwgError) as e:
            lift_closure_records(ctx, cols, strand, 2, [(0, 0, 10)], 2, 1, axes=1)
        assert e.value.code == -4
        hand = hand_case()
        got = lift_closure_records(ctx, hand[0], hand[1], 3, hand[3][:1], 3, 10)      # the same context, a call that fits
        assert [tuple(int(v) for v in r) for r in got.rows] == HAND_ROWS
        ctx.set_memory_limit(0)
        big = lift_closure_records(ctx, cols, strand, 2, [(0, 0, 10)], 2, 1, axes=1)
        assert [tuple(int(v) for v in r) for r in big.rows] == [(0, 0, 0, 10, 0, 0), (0, 1, 0, 10, 1, 0)] and big.projections == 10 * (n // 1_000)
    finally:
        ctx.close()


# ---- the texts -----------------------------------------------------------------------------------------------------------------
def test_texts_of_an_open_paf_equal_the_model_rendering(sw):
    text, kept = hand_paf()
    with sw.PafFile(text=text) as paf:
        got = sw.LiftClosure.from_paf(paf, kept.astype(np.uint8), HAND_BED, 3, 10, set="all")
        assert (got.text, got.summary_text) == (HAND_TEXT, HAND_SUMMARY_TEXT) == cm.paf_texts(text, kept, HAND_BED, 3, 10, 0, 3)
        assert len(got.rows) == 8 and list(got.summary["state"]) == ["closed", "none", "unknown", "closed"]
        lib, handle = sw._lib.load(), sw.default_context().handle
        assert paf_closure(lib, paf, kept.astype(np.uint8), HAND_BED, 3, 10, 0, 3, ctx=handle) == (0, HAND_TEXT, HAND_SUMMARY_TEXT)      # the C entry itself
        assert paf_closure(lib, paf, kept.astype(np.uint8), HAND_BED, 3, 10, 1, 3, ctx=handle, rows=False) == (0, None, cm.paf_texts(text, kept, HAND_BED, 3, 10, 1, 3)[1])
        got = sw.LiftClosure.from_paf(paf, None, HAND_BED, 2, 10, set="all", axes="query", ctx=sw.default_context())
        assert (got.text, got.summary_text) == cm.paf_texts(text, None, HAND_BED, 2, 10, 0, 1) and "cut" in set(got.summary["state"])
    text = gen_text(61, 3_000, n_genomes=4, chrs_per_genome=3, span=300_000)
    bed = random_bed(np.random.default_rng(3), text, 40)
    with sw.PafFile(text=text) as paf:
        status, _ = run_filter(sw, paf, filter_cfgs(sw)["one_to_one"])
        assert 0 < int((status != 0).sum()) < len(status)
        for set_, axes, hops, min_len in (("kept", "both", 3, 100), ("all", "target", 2, 1), ("kept", "query", 2, 1_000)):
            got = sw.LiftClosure.from_paf(paf, status, bed, hops, min_len, set=set_, axes=axes)
            want = cm.paf_texts(text, status != 0, bed, hops, min_len, sw.lift.SETS[set_], sw.lift.AXES[axes])
            assert (got.text, got.summary_text) == want and want[0].count("\n") > 40, (set_, axes)
        only = sw.LiftClosure.from_paf(paf, status, bed, 2, rows=False)
        assert only.text is None and only.summary_text == cm.paf_texts(text, status != 0, bed, 2, 100, 1, 3)[1]
    # more rows than the first guess at their number holds
    many = "".join("a#1#x\t5000\t0\t100\t+\tb#1#y\t300000\t%d\t%d\t1\t100\t60\n" % (3 * k, 3 * k + 1) for k in range(2**16 + 10))
    with sw.PafFile(text=many) as paf:
        got = sw.LiftClosure.from_paf(paf, None, "a#1#x\t10\t20\tmany\n", 1, set="all")
        assert (got.text, got.summary_text) == cm.paf_texts(many, None, "a#1#x\t10\t20\tmany\n", 1, 100, 0, 3) and got.text.count("\n") == 2**16 + 11


def test_cli_lift_hops(sw, tmp_path):
    from sweepga_amd import build
    text = gen_text(71, 3_000, n_genomes=4, chrs_per_genome=3, span=400_000)
    bed_text = random_bed(np.random.default_rng(9), text, 40)
    inp, bed = tmp_path / "in.paf", tmp_path / "r.bed"
    inp.write_text(text, newline="")
    bed.write_text(bed_text, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-jump", "10k", "--scaffold-mass", "2k", "--quiet"]
    plain, out, rows, summ, once = (tmp_path / x for x in ("plain.paf", "out.paf", "closure.tsv", "closure_summary.tsv", "lift.tsv"))
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), *flags], capture_output=True)
    assert r0.returncode == 0 and plain.stat().st_size > 0, r0.stderr
    kept = kept_mask(text, plain.read_bytes().decode())
    for extra, hops, min_len, set_, axes, given in ((["--lift-hops", "3"], 3, 100, 1, 3, ("rows", "summary")),
                                                    (["--lift-hops=2", "--lift-min-length", "1", "--lift-set", "all", "--lift-axis=target"], 2, 1, 0, 2, ("rows", "summary")),
                                                    (["--lift-hops", "2", "--lift-axis", "query"], 2, 100, 1, 1, ("rows",)),
                                                    (["--lift-hops", "4", "--lift-min-length=500"], 4, 500, 1, 3, ("summary",))):
        want = cm.paf_texts(text, kept, bed_text, hops, min_len, set_, axes)
        for p in (out, rows, summ):
            p.unlink(missing_ok=True)
        files = (["--lift-closure", str(rows)] if "rows" in given else []) + (["--lift-closure-summary", str(summ)] if "summary" in given else [])
        r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--lift-regions", str(bed), *files, *extra, *flags], capture_output=True)
        assert r.returncode == 0 and r.stdout == b"" and out.read_bytes() == plain.read_bytes(), r.stderr     # the PAF does not change
        assert rows.exists() == ("rows" in given) and summ.exists() == ("summary" in given)
        assert "rows" not in given or rows.read_text() == want[0]
        assert "summary" not in given or summ.read_text() == want[1]
    # --lift and --lift-hops in one run; the closure summary on standard error
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--lift-regions", str(bed), "--lift", str(once), "--lift-hops", "2",
                        "--lift-closure-summary", "-", *flags], capture_output=True)
    assert r.returncode == 0 and r.stderr.decode() == cm.paf_texts(text, kept, bed_text, 2, 100, 1, 3)[1] and out.read_bytes() == plain.read_bytes()
    assert once.read_text() == lm.paf_texts(text, kept, bed_text, 1, 3)[0]
    # --no-filter: every line to standard output, kept = all
    r = subprocess.run([build.CLI, str(inp), "--no-filter", "--lift-regions", str(bed), "--lift-hops", "2", "--lift-closure", str(rows),
                        "--lift-closure-summary", str(summ)], capture_output=True)
    every = cm.paf_texts(text, np.ones(len(kept), dtype=bool), bed_text, 2, 100, 1, 3)
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
                got = check(sw, cols, strand, 2, regions, status, 3, 10, 1 if status is not None else 0, 3, f"n = {n}", ctx=ctx)
                assert got.n >= 2 and got.hops_run >= 1
    finally:
        ctx.close()
