"""The mosaic on the device (sweepga_amd/csrc/swg_mosaic.hip) against tests/mosaic_model.py: the two record seams on the shapes
tests/test_gpu_breadth.py uses, the hand case of tests/test_mosaic_cpu.py, inputs built around the tile of T slots (T = 512, and 2
and 8 through SWG_MOSAIC_TILE in a child process), piles of 599 and 5000 equal boundaries, the borders of the number formats,
10^5 records under one long record, a real filter status, the capacity protocol and the want bits, the limits, a memory limit,
and the texts of swg_paf_mosaic / --mosaic / --mosaic-share byte for byte.  Every comparison is exact: integers and bytes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import mosaic_model as mm
from tests.test_gpu_alnstats import filter_cfgs, gen_text, records_of, run_filter
from tests.test_gpu_breadth import SHAPE_NAMES, shape_texts
from tests.test_gpu_intervals import kept_mask
from tests.test_gpu_wide import Hip
from tests.test_mosaic_cpu import HAND_ROWS, HAND_ROWS_T_LEN, HAND_SHARE, HAND_SHARE_T_LEN, check_hand, hand_case, hand_paf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = mm.COLS + ("matches",)
SETS = ("all", "kept")
TILE = 512


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


@pytest.fixture(scope="module")
def shapes():
    return shape_texts()


def paf_columns(paf):
    return {c: paf.column(c).copy() for c in COLS}, paf.seq_genome_last.copy()


def as_columns(**kw):
    return {k: np.asarray(v).astype(np.uint32) for k, v in kw.items()}


def same_results(a, b):
    return mm.same_rows(a.rows, b.rows) and a.bases == b.bases and ((a.share is None and b.share is None) or np.array_equal(a.share, b.share))


def both_seams(sw, cols, seq_genome, status=None, weight=None, axis=0, set_=None, want=None, ctx=None, G=None):
    """The result of the host seam, after checking that the device seam gives the same.  want: None = both bits where the share
    may be asked for (at most 4096 genomes), else the rows."""
    from sweepga_amd.mosaic import _call, mosaic_records
    ctx = ctx or sw.default_context()
    G = G or int(seq_genome.max()) + 1
    set_ = set_ or ("kept" if status is not None else "all")
    want = want or (3 if G <= 4096 else 1)
    got = mosaic_records(ctx, cols, seq_genome, status, weight, axis, set_, n_genome=G, want=want)
    hip = Hip()
    try:
        dcols = {name: hip.up(np.ascontiguousarray(cols[name], dtype=np.uint32)) for name in cols}
        rec = records_of(dcols, len(seq_genome), len(cols["q_id"]))
        d_status = hip.up(np.ascontiguousarray(status, dtype=np.uint8)) if status is not None else None
        d_weight = hip.up(np.ascontiguousarray(weight, dtype=np.uint32)) if weight is not None else None
        dev = _call(ctx, ctx.lib.swg_mosaic_records_device, rec, hip.up(np.ascontiguousarray(seq_genome, dtype=np.uint32)), G, d_status, d_weight,
                    axis, set_, want)
    finally:
        hip.free()
    assert same_results(dev, got)
    return got


def check(sw, cols, seq_genome, status=None, weight=None, axis=0, set_=None, what="", ctx=None, model=None):
    """Both seams against the model (`model`: the rows computed before): rows, bases, share, and the rows' own properties."""
    set_ = set_ or ("kept" if status is not None else "all")
    got = both_seams(sw, cols, seq_genome, status, weight, axis, set_, ctx=ctx)
    rows = model if model is not None else mm.mosaic(cols, seq_genome, np.asarray(status) != 0 if set_ == "kept" else None, weight, axis)
    assert mm.same_rows(got.rows, rows), (what, axis, set_, len(got.rows), len(rows))
    mm.check_rows(got.rows, cols, axis)
    assert got.bases == mm.bases_of(rows), (what, axis, set_)
    if got.share is not None:      # (more than 4096 genomes: the rows alone)
        assert got.bases == int(got.share.sum()), (what, axis, set_)
        assert np.array_equal(got.share, mm.share_of(rows, cols, seq_genome, axis, got.share.shape[0])) and not np.diag(got.share).any(), (what, axis, set_)
    return got


@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_record_seams_against_the_model(sw, shapes, shape):
    rng = np.random.default_rng(len(shape))
    with sw.PafFile(text=shapes[shape]) as paf:
        cols, seq_genome = paf_columns(paf)
    n = len(cols["q_id"])
    status = (rng.random(n) < 0.4).astype(np.uint8) * rng.integers(1, 4, n).astype(np.uint8)
    for axis in (0, 1):             # weight NULL = the matches column: both axes, both sets
        for set_ in SETS:
            got = check(sw, cols, seq_genome, status, None, axis, set_, shape)
            assert len(got.rows) > 0
    ranks = rng.permutation(n).astype(np.uint32)      # explicit, pairwise different weights ...
    got = check(sw, cols, seq_genome, status, ranks, 0, "kept", shape + ", ranks")
    perm = rng.permutation(n)                         # ... under which the record order does not matter
    again = both_seams(sw, {c: v[perm] for c, v in cols.items()}, seq_genome, status[perm], ranks[perm], 0, "kept")
    mapped = again.rows.copy()
    mapped["record"] = perm[again.rows["record"]]
    assert mm.same_rows(mapped, got.rows) and again.bases == got.bases
    assert (again.share is None and got.share is None) or np.array_equal(again.share, got.share)
    length = (cols["t_end"] - cols["t_start"]).astype(np.uint32)      # the length on the axis as the weight
    check(sw, cols, seq_genome, None, length, 1, "all", shape + ", length")
    # a shuffled copy with equal weights about: the lower index wins, so the rows are those of the model on the shuffled records
    shuffled = {c: v[perm] for c, v in cols.items()}
    check(sw, shuffled, seq_genome, status[perm], None, 1, "kept", shape + ", shuffled")


def test_hand_case(sw):
    cols, strand, seq_genome, status, want = hand_case()

    def get(axis, name):
        got = check(sw, cols, seq_genome, status, None, axis, name, "hand")
        assert got.bases == want["bases"][axis, name]
        return got.rows, got.share
    check_hand(get, want)
    one = both_seams(sw, cols, np.zeros(4, dtype=np.uint32), status)      # one genome: nothing counts
    assert len(one.rows) == 0 and one.bases == 0 and one.share.tolist() == [[0]]


# ---- the tile seams ------------------------------------------------------------------------------------------------------------
def unit_layer(n_slots, rng, heavy=()):
    """Records [i, i + 1) for i < n_slots - 1 on sequence 0: the boundaries are 0 .. n_slots - 1, so position = slot.  Weights 10 .. 19;
    `heavy`: [(start, end, weight)] more records in slot coordinates."""
    s = np.concatenate([np.arange(n_slots - 1), [h[0] for h in heavy]]).astype(np.int64)
    e = np.concatenate([np.arange(n_slots - 1) + 1, [h[1] for h in heavy]]).astype(np.int64)
    w = np.concatenate([rng.integers(10, 20, n_slots - 1), [h[2] for h in heavy]]).astype(np.int64)
    n = len(s)
    return as_columns(q_id=np.zeros(n), t_id=np.ones(n), q_start=s, q_end=e, t_start=3 * s, t_end=3 * e + 1, matches=w)


def tile_seam_cases(T):
    rng = np.random.default_rng(T)
    two = np.array([0, 1], dtype=np.uint32)
    cases = []
    for B in (T - 1, T, T + 1):        # B boundaries: one tile not full, full, and one slot into the second
        if B >= 2:
            cases.append(("%d boundaries" % B, unit_layer(B, rng, [(0, B - 1, 5)]), two))
    # exactly one whole tile (a == tile_lo, b == tile_hi), two whole tiles, middle to middle without a whole tile: each the
    # heaviest where it lies, and each under a lighter one that it cuts
    cases.append(("one whole tile", unit_layer(4 * T + 1, rng, [(T, 2 * T, 50), (0, 4 * T, 30)]), two))
    cases.append(("two whole tiles", unit_layer(4 * T + 1, rng, [(T, 3 * T, 50), (T // 2, 3 * T + 1, 30)]), two))
    cases.append(("middle to middle", unit_layer(3 * T + 1, rng, [(T // 2, T + T // 2, 50), (T + 1, 3 * T - 1, 30)]), two))
    # one light record over 40 T slots, heavier short ones [2 i, 2 i + 1) scattered under it, and records over 1 .. 40 whole tiles
    # so that the coarse levels 0 to 5 and the push-down are all used
    # (every position 0 .. 40 T is a boundary: position = slot; a short one is heavier than what lies over it or not)
    i = np.arange(20 * T, dtype=np.int64)
    whole = [(T * s, T * (s + c), 100 + c) for s, c in ((1, 1), (3, 2), (6, 3), (2, 4), (9, 7), (20, 8), (4, 15), (22, 16), (5, 31), (7, 32), (0, 40))]
    s = np.concatenate([[0], 2 * i, [x[0] for x in whole]])
    e = np.concatenate([[40 * T], 2 * i + 1, [x[1] for x in whole]])
    w = np.concatenate([[1], rng.integers(0, 300, 20 * T), [x[2] for x in whole]])
    n = len(s)
    cases.append(("40 tiles", as_columns(q_id=np.zeros(n), t_id=np.ones(n), q_start=s, q_end=e, t_start=s, t_end=e, matches=w), two))
    # the last boundary of sequence 0 and the first of sequence 1 in one tile, the same positions on both
    cols = as_columns(q_id=[0, 0, 1, 1], t_id=[2, 2, 2, 2], q_start=[0, 5, 0, 9], q_end=[9, 9, 9, 12], t_start=[0, 0, 0, 0], t_end=[1, 1, 1, 1],
                      matches=[7, 9, 7, 7])
    cases.append(("two sequences in one tile", cols, np.array([0, 0, 1], dtype=np.uint32)))
    return cases


def run_tile_cases(sw, T):
    ctx = sw.default_context()
    for what, cols, seq_genome in tile_seam_cases(T):
        n = len(cols["q_id"])
        status = (np.arange(n) % 5 != 1).astype(np.uint8)
        perm = np.random.default_rng(n).permutation(n)
        cols, status = {c: v[perm] for c, v in cols.items()}, status[perm]
        for set_ in SETS:
            got = check(sw, cols, seq_genome, status, None, 0, set_, "T = %d, %s" % (T, what))
            assert len(got.rows) > 0
    # the tile in force: the coarse table of the 40-tile input (40 T + 1 boundaries: 41 tiles) has six levels, five push-downs;
    # two seams, each called twice under the capacity protocol
    what, cols, seq_genome = tile_seam_cases(T)[-2]
    ctx.profile(True)
    try:
        ctx.profile_reset()
        both_seams(sw, cols, seq_genome, None, None, 0, "all", want=1, ctx=ctx)
        table = ctx.profile_table()
        assert table["mosaic_push"][0] == 4 * 5 and table["mosaic_tile"][0] == 4, (T, table)
    finally:
        ctx.profile(False)


def test_tile_seams_at_the_default_tile():
    """In a child process too: the variable is taken out of its environment, whatever this one holds."""
    code = ("import sys; sys.path.insert(0, %r); import sweepga_amd; from tests.test_gpu_mosaic import run_tile_cases; "
            "run_tile_cases(sweepga_amd, %d); print('ok')" % (ROOT, TILE))
    env = {k: v for k, v in os.environ.items() if k != "SWG_MOSAIC_TILE"}
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


@pytest.mark.parametrize("T", [2, 8])
def test_tile_seams_at_small_tiles_in_a_child_process(T):
    """SWG_MOSAIC_TILE is read once per process: a child of its own."""
    code = ("import sys; sys.path.insert(0, %r); import sweepga_amd; from tests.test_gpu_mosaic import run_tile_cases; "
            "run_tile_cases(sweepga_amd, %d); print('ok')" % (ROOT, T))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SWG_MOSAIC_TILE=str(T)), capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


# ---- piles ---------------------------------------------------------------------------------------------------------------------
def pile(starts, ends, weights):
    n = len(starts)
    return as_columns(q_id=np.arange(1, n + 1), t_id=np.zeros(n), q_start=np.zeros(n), q_end=np.full(n, 10), t_start=starts, t_end=ends,
                      matches=weights), np.concatenate([[0], 1 + np.arange(n) % 7]).astype(np.uint32)


def test_piles_of_599(sw):
    rng = np.random.default_rng(599)
    k = np.arange(599)
    status = (k % 3 != 0).astype(np.uint8)
    # one begin, staggered ends, the shorter the heavier: 599 rows, one per record
    cols, seq_genome = pile(np.zeros(599), 70_000 - 3 * k, k)
    got = check(sw, cols, seq_genome, status, None, 1, "all", "one begin")
    assert len(got.rows) == 599 and got.rows["record"].tolist() == list(range(598, -1, -1)) and got.bases == 70_000
    check(sw, cols, seq_genome, status, None, 1, "kept", "one begin")
    # staggered begins, one end, the later the heavier
    cols, seq_genome = pile(3 * k, np.full(599, 70_000), k)
    got = check(sw, cols, seq_genome, status, None, 1, "all", "one end")
    assert len(got.rows) == 599 and got.rows["record"].tolist() == list(range(599)) and got.bases == 70_000
    check(sw, cols, seq_genome, status, rng.integers(0, 5, 599), 1, "kept", "one end, few weights")
    # identical intervals of equal weight: record 0 wins -- among the kept ones, record 1
    cols, seq_genome = pile(np.full(599, 100), np.full(599, 70_000), np.full(599, 42))
    got = check(sw, cols, seq_genome, status, None, 1, "all", "identical")
    assert mm.as_tuples(got.rows) == [(0, 100, 70_000, 0)]
    assert mm.as_tuples(check(sw, cols, seq_genome, status, None, 1, "kept", "identical").rows) == [(0, 100, 70_000, 1)]


def test_a_tile_whose_entries_are_many_times_the_tile(sw):
    """5000 begins on one position and their ends on seven: one tile of the sorted entries holds 10^4 of them."""
    rng = np.random.default_rng(5)
    n = 5_000
    cols, seq_genome = pile(np.full(n, 1_000), 2_000 + 100 * rng.integers(0, 7, n), rng.integers(0, 50, n))
    got = check(sw, cols, seq_genome, (rng.random(n) < 0.5).astype(np.uint8), None, 1, "kept", "deep pile")
    assert 1 <= len(got.rows) <= 7 and got.rows["start"][0] == 1_000


def test_borders_of_the_number_formats(sw):
    top = 0xffffffff
    for n_seq in (255, 256, 257):          # 32 + bits(n_seq) key bits: 40 (five radix passes), 41, 41
        last = n_seq - 1
        cols = as_columns(q_id=[last, last, last, 0, last, last], t_id=[0, 0, 1, last, 0, 0], q_start=[0, 0, top - 10, 0, 100, 100],
                          q_end=[top, 50, top, top, 200, 200], t_start=[0] * 6, t_end=[9] * 6, matches=[0, top, 0, 0, 0, top])
        seq_genome = (np.arange(n_seq) % 3).astype(np.uint32)
        seq_genome[last] = 3
        status = np.ones(6, dtype=np.uint8)
        for axis in (0, 1):
            got = check(sw, cols, seq_genome, status, None, axis, "all", "n_seq = %d" % n_seq)
        got = check(sw, cols, seq_genome, status, None, 0, "kept", "n_seq = %d" % n_seq)
        # a start of 0, an end of 2^32 - 1; weight 2^32 - 1 beats weight 0, and among the zeroes the lower index wins
        assert mm.as_tuples(got.rows) == [(0, 0, top, 3), (last, 0, 50, 1), (last, 50, 100, 0), (last, 100, 200, 5), (last, 200, top, 0)]
        assert got.bases == 2 * top


def test_a_hundred_thousand_records_under_one_long_record(sw):
    """10^5 heavy short records under one long light one: a row per record and a row of the long one per gap, 2 * 10^5 + 1 rows."""
    n = 100_000
    rng = np.random.default_rng(91)
    i = np.arange(n, dtype=np.int64)
    s = np.concatenate([[0], 10 + 30_000 * i])
    e = np.concatenate([[30_000 * n + 500], s[1:] + rng.integers(1, 20_000, n)])
    cols = as_columns(q_id=np.zeros(n + 1), t_id=np.ones(n + 1), q_start=s, q_end=e, t_start=s // 2, t_end=e // 2,
                      matches=np.concatenate([[1], rng.integers(2, 1_000, n)]))
    perm = rng.permutation(n + 1)
    cols = {c: v[perm] for c, v in cols.items()}
    status = np.ones(n + 1, dtype=np.uint8)
    status[np.flatnonzero(perm == 0)[0]] = 0      # KEPT lacks the long one
    seq_genome = np.array([0, 1], dtype=np.uint32)
    got = check(sw, cols, seq_genome, status, None, 0, "all", "long over short")
    assert len(got.rows) == 2 * n + 1 and got.bases == 30_000 * n + 500
    got = check(sw, cols, seq_genome, status, None, 0, "kept", "short alone")
    assert len(got.rows) == n


def test_a_real_filter_status(sw):
    FM = sw.FilterMode
    cfg = sw.FilterConfig(mapping_filter_mode=FM.OneToOne, mapping_max_per_query=1, mapping_max_per_target=1)   # --num-mappings 1:1
    text = gen_text(21, 20_000, n_genomes=4, chrs_per_genome=3, span=400_000)
    with sw.PafFile(text=text) as paf:
        status, _ = run_filter(sw, paf, cfg)
        cols, seq_genome = paf_columns(paf)
    assert 0 < int((status != 0).sum()) < len(status)
    kept = [check(sw, cols, seq_genome, status, None, axis, "kept", "1:1") for axis in (0, 1)]
    every = both_seams(sw, cols, seq_genome, status, None, 0, "all")
    # the filter only takes away: less is covered, and nothing the kept records cover was uncovered before
    assert 0 < kept[0].bases < every.bases and len(kept[0].rows) > 0 and (kept[0].share <= every.share.sum()).all()


def test_the_capacity_protocol_and_the_want_bits(sw):
    from sweepga_amd._lib import SwgMosaicRequest, SwgMosaicRow
    from sweepga_amd.mosaic import ROW_DTYPE
    ctx = sw.default_context()
    cols, strand, seq_genome, status, want = hand_case()
    rec = records_of(cols, len(seq_genome))
    call = lambda req: ctx.check(ctx.lib.swg_mosaic_records(ctx.handle, C.byref(rec), seq_genome.ctypes.data, 3, status.ctypes.data, C.byref(req)))   # noqa: E731
    rows_kept = want[0, "kept"][0]
    req = SwgMosaicRequest()
    req.want, req.set = 1, 1
    poison = np.frombuffer(bytearray(b"\xab" * 16 * 4), dtype=ROW_DTYPE)
    before = poison.copy()
    req.capacity, req.rows = 4, C.cast(poison.ctypes.data, C.POINTER(SwgMosaicRow))     # too small an array
    call(req)
    assert poison.tobytes() == before.tobytes() and int(req.n) == len(rows_kept) and int(req.bases) == 1_550
    buf = np.zeros(len(rows_kept) + 1, dtype=ROW_DTYPE)
    buf[-1] = (7, 7, 7, 7)
    req.capacity, req.rows = len(rows_kept), C.cast(buf.ctypes.data, C.POINTER(SwgMosaicRow))
    call(req)
    assert mm.as_tuples(buf[:-1]) == rows_kept and mm.as_tuples(buf[-1:]) == [(7, 7, 7, 7)]
    # a clear bit leaves its part untouched, and the passes only it would need are not launched
    ctx.profile(True)
    try:
        for bits, launches in ((1, {"mosaic_keys": 1, "mosaic_tile": 1, "mosaic_rows": 1, "mosaic_bases": 1, "mosaic_share": 0}),
                               (2, {"mosaic_keys": 1, "mosaic_tile": 1, "mosaic_rows": 1, "mosaic_bases": 0, "mosaic_share": 1}),
                               (3, {"mosaic_keys": 1, "mosaic_coarse": 1, "mosaic_slots": 1, "mosaic_rows": 1, "mosaic_bases": 1, "mosaic_share": 1})):
            req = SwgMosaicRequest()
            req.want, req.set = bits, 1
            share = np.full((3, 3), 99, dtype=np.uint64)
            rows = np.zeros(16, dtype=ROW_DTYPE)
            req.n = req.bases = 12345
            req.capacity, req.rows, req.share = 16, C.cast(rows.ctypes.data, C.POINTER(SwgMosaicRow)), C.cast(share.ctypes.data, C.POINTER(C.c_uint64))
            ctx.profile_reset()
            call(req)
            table = ctx.profile_table()
            for name, count in launches.items():
                assert (table[name][0] if name in table else 0) == count, (bits, name, table)
            assert int(req.n) == (len(rows_kept) if bits & 1 else 12345) and int(req.bases) == (1_550 if bits & 1 else 12345), bits
            assert mm.as_tuples(rows[:len(rows_kept)]) == (rows_kept if bits & 1 else [(0, 0, 0, 0)] * len(rows_kept)), bits     # share alone: no row read back
            assert share.tolist() == (want[0, "kept"][1] if bits & 2 else [[99] * 3] * 3), bits
    finally:
        ctx.profile(False)


def test_limits_and_refusals(sw):
    from sweepga_amd.mosaic import mosaic_records
    ctx = sw.default_context()
    cols, strand, seq_genome, status, want = hand_case()
    for bits in (2, 3):        # 4097 genomes: no share, but the rows
        with pytest.raises(sw.SwgError) as e:
            mosaic_records(ctx, cols, seq_genome, status, n_genome=4097, want=bits)
        assert e.value.code == -5 and "4096" in str(e.value)
    got = mosaic_records(ctx, cols, seq_genome, status, n_genome=4097, want=1)
    assert mm.as_tuples(got.rows) == want[0, "kept"][0] and got.share is None
    got = mosaic_records(ctx, cols, seq_genome, status, n_genome=4096, want=2)
    assert got.share[:3, :3].tolist() == want[0, "kept"][1] and int(got.share.sum()) == 1_550 and got.rows is None
    bad = {c: v.copy() for c, v in cols.items()}
    bad["t_id"][3] = len(seq_genome)
    no_matches = {c: v for c, v in cols.items() if c != "matches"}
    for args, kw in (((bad, seq_genome, status), {}), ((cols, seq_genome, status), {"n_genome": 2}), ((cols, seq_genome, None), {"set": "kept"}),
                     ((cols, seq_genome, status), {"want": 4}), ((cols, seq_genome, status), {"want": 0}), ((no_matches, seq_genome, status), {})):
        with pytest.raises(sw.SwgError) as e:
            mosaic_records(ctx, *args, **kw)
        assert e.value.code == -1, (kw, str(e.value))
    # the refusals of the request itself, with a real context: each names its fault, launches nothing and leaves the outputs alone
    from sweepga_amd._lib import SwgMosaicRequest, SwgMosaicRow
    from sweepga_amd.mosaic import ROW_DTYPE
    rec = records_of(cols, len(seq_genome))
    no_cols = records_of({c: v for c, v in cols.items() if c != "q_end"}, len(seq_genome))
    ctx.profile(True)
    try:
        for fn in (ctx.lib.swg_mosaic_records, ctx.lib.swg_mosaic_records_device):
            for fault, text, r in (({"reserved": 1}, "reserved must be 0", rec), ({"axis": 2}, "axis is 0 (query) or 1 (target)", rec),
                                   ({"set": 2}, "set is SWG_IV_ALL or SWG_IV_KEPT", rec), ({"want": 2, "share": None}, "NULL share", rec),
                                   ({"want": 3, "share": None}, "NULL share", rec), ({"want": 0}, "want names nothing", rec),
                                   ({"want": 4}, "want names nothing", rec), ({"status": None}, "needs a status column", rec),
                                   ({}, "NULL column", no_cols), ({"seq_genome": None}, "NULL seq_genome", rec),
                                   ({"n_genome": 0}, "without sequences or genomes", rec)):
                req = SwgMosaicRequest()
                share = np.full((3, 3), 99, dtype=np.uint64)
                rows = np.frombuffer(bytearray(b"\xab" * 16 * 16), dtype=ROW_DTYPE)
                req.want, req.axis, req.set, req.reserved = fault.get("want", 3), fault.get("axis", 0), fault.get("set", 1), fault.get("reserved", 0)
                req.n = req.bases = 12345
                req.capacity, req.rows = 16, C.cast(rows.ctypes.data, C.POINTER(SwgMosaicRow))
                req.share = C.cast(share.ctypes.data, C.POINTER(C.c_uint64)) if "share" not in fault else None
                st = status.ctypes.data if "status" not in fault else None
                sg = seq_genome.ctypes.data if "seq_genome" not in fault else None
                ctx.profile_reset()
                assert fn(ctx.handle, C.byref(r), sg, fault.get("n_genome", 3), st, C.byref(req)) == -1, fault
                assert text in (ctx.lib.swg_last_error(ctx.handle) or b"").decode(), (fault, ctx.lib.swg_last_error(ctx.handle))
                assert int(req.n) == int(req.bases) == 12345 and share.tolist() == [[99] * 3] * 3 and rows.tobytes() == b"\xab" * 256, fault
                assert all(v[0] == 0 for v in ctx.profile_table().values()), (fault, ctx.profile_table())
    finally:
        ctx.profile(False)
    got = mosaic_records(ctx, no_matches, seq_genome, status, weight=cols["matches"])      # an explicit weight needs no matches column
    assert mm.as_tuples(got.rows) == want[0, "kept"][0]
    # 2^31 records are refused before any launch (no column is read: the pointers are never followed)
    rec = records_of(cols, len(seq_genome))
    rec.n = 1 << 31
    req = SwgMosaicRequest()
    req.want = 1
    assert ctx.lib.swg_mosaic_records(ctx.handle, C.byref(rec), seq_genome.ctypes.data, 3, None, C.byref(req)) == -5
    none = mosaic_records(ctx, {c: np.zeros(0, dtype=np.uint32) for c in COLS}, seq_genome, np.zeros(0, dtype=np.uint8))
    assert len(none.rows) == 0 and none.bases == 0 and not none.share.any()


def test_a_memory_limit_too_small_is_a_clean_oom(sw):
    from sweepga_amd.mosaic import mosaic_records
    ctx = sw.Context(0)
    try:
        rng = np.random.default_rng(51)
        with sw.PafFile(text=gen_text(52, 100_000, n_genomes=4, chrs_per_genome=3, span=400_000)) as paf:
            cols, seq_genome = paf_columns(paf)
        status = (rng.random(len(cols["q_id"])) < 0.5).astype(np.uint8)
        ctx.set_memory_limit(1 << 20)       # the staged columns alone are 2.9 MB
        with pytest.raises(sw.SwgError) as e:
            mosaic_records(ctx, cols, seq_genome, status)
        assert e.value.code == -4
        ctx.set_memory_limit(0)             # ... and the context works on
        model = mm.mosaic(cols, seq_genome, status != 0, None, 0)
        check(sw, cols, seq_genome, status, None, 0, "kept", "after the refusal", ctx=ctx, model=model)
        ctx.set_memory_limit(1 << 30)
        check(sw, cols, seq_genome, status, None, 0, "kept", "under a limit that holds it", ctx=ctx, model=model)
        assert ctx.memory_info()[0] <= 1 << 30
    finally:
        ctx.close()


# ---- the texts ---------------------------------------------------------------------------------------------------------------
def test_texts_of_an_open_paf_equal_the_model_rendering(sw):
    text, status = hand_paf()
    ctx = sw.default_context()
    with sw.PafFile(text=text) as paf:
        m = sw.Mosaic.from_paf(ctx, paf, status)
        assert (m.rows.decode(), m.share.decode()) == (HAND_ROWS, HAND_SHARE)
        m = sw.Mosaic.from_paf(ctx, paf, status, axis="target", set="all", by="length")
        assert (m.rows.decode(), m.share.decode()) == (HAND_ROWS_T_LEN, HAND_SHARE_T_LEN)
        m = sw.Mosaic.from_paf(ctx, paf, None, set="all")      # ALL needs no status
        assert (m.rows, m.share) == mm.paf_texts(text, None, 0, "all")
    text = gen_text(61, 12_000, n_genomes=4, chrs_per_genome=3, span=300_000)
    with sw.PafFile(text=text) as paf:
        status, _ = run_filter(sw, paf, filter_cfgs(sw)["one_to_one"])
        for axis, set_, by in (("query", "kept", "matches"), ("target", "kept", "length"), ("target", "all", "matches"), ("query", "all", "length")):
            rows, share = mm.paf_texts(text, status != 0, mm_axis(axis), set_, by)
            m = sw.Mosaic.from_paf(ctx, paf, status, axis=axis, set=set_, by=by)
            assert m.rows == rows and m.share == share and len(rows) > 0 and share.count(b"\n") >= 4, (axis, set_, by)
        rows, share = mm.paf_texts(text, status != 0)
        ctx.profile(True)      # one text alone, and only its passes
        try:
            ctx.profile_reset()
            only = sw.Mosaic.from_paf(ctx, paf, status, share=False)
            assert only.share is None and only.rows == rows and "mosaic_share" not in ctx.profile_table()
            ctx.profile_reset()
            only = sw.Mosaic.from_paf(ctx, paf, status, rows=False)
            assert only.rows is None and only.share == share and ctx.profile_table()["mosaic_share"][0] == 1
        finally:
            ctx.profile(False)
    ln = "\t".join(["a#1#x", str(2**33), str(2**32), str(2**32 + 50), "+", "b#1#y", "900", "10", "60", "50", "50", "60"]) + "\n"
    with sw.PafFile(text=ln) as paf:
        with pytest.raises(sw.SwgError) as e:
            sw.Mosaic.from_paf(ctx, paf, np.ones(1, dtype=np.uint8))
        assert e.value.code == -6 and "2^32" in str(e.value)


def mm_axis(name):
    return {"query": 0, "target": 1}[name]


def test_cli_mosaic(sw, tmp_path):
    from sweepga_amd import build
    text = gen_text(71, 15_000, n_genomes=4, chrs_per_genome=3, span=400_000)
    inp = tmp_path / "in.paf"
    inp.write_text(text, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-jump", "10k", "--scaffold-mass", "2k", "--quiet"]
    plain, out, bed, share = (tmp_path / x for x in ("plain.paf", "out.paf", "mosaic.bed", "mosaic.tsv"))
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), *flags], capture_output=True)
    assert r0.returncode == 0 and plain.stat().st_size > 0, r0.stderr
    kept = kept_mask(text, plain.read_bytes().decode())
    for given, opts in ((("bed",), []), (("share",), []), (("bed", "share"), []),
                        (("bed", "share"), ["--mosaic-axis", "target", "--mosaic-set", "all", "--mosaic-by", "length"]),
                        (("bed", "share"), ["--mosaic-axis=query", "--mosaic-set=kept", "--mosaic-by=matches"])):
        for p in (out, bed, share):
            p.unlink(missing_ok=True)
        extra = (["--mosaic", str(bed)] if "bed" in given else []) + (["--mosaic-share", str(share)] if "share" in given else [])
        r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), *extra, *opts, *flags], capture_output=True)
        assert r.returncode == 0 and r.stdout == b"" and out.read_bytes() == plain.read_bytes(), r.stderr     # the PAF does not change
        want = mm.paf_texts(text, kept, 1, "all", "length") if "target" in " ".join(opts) else mm.paf_texts(text, kept)
        assert bed.exists() == ("bed" in given) and share.exists() == ("share" in given)
        assert "bed" not in given or (bed.read_bytes() == want[0] and len(want[0]) > 0)
        assert "share" not in given or share.read_bytes() == want[1]
    # - : the text on standard error, the PAF alone on standard output
    want = mm.paf_texts(text, kept)
    r1 = subprocess.run([build.CLI, str(inp), *flags], capture_output=True)
    r2 = subprocess.run([build.CLI, str(inp), "--mosaic-share", "-", *flags], capture_output=True)
    assert r1.returncode == r2.returncode == 0 and r2.stdout == r1.stdout == plain.read_bytes() and r2.stderr == want[1]
    # --no-filter: every line to standard output, the device is opened, kept = all
    r = subprocess.run([build.CLI, str(inp), "--no-filter", "--mosaic", str(bed), "--mosaic-share", str(share)], capture_output=True)
    every = mm.paf_texts(text, np.ones(len(kept), dtype=bool))
    assert r.returncode == 0 and r.stdout == text.encode() and bed.read_bytes() == every[0] and share.read_bytes() == every[1]
    # --sparsify tree: all = the whole input, kept = what is written
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--sparsify", "tree:1", "--mosaic", str(bed), "--mosaic-share", str(share), *flags],
                       capture_output=True)
    assert r.returncode == 0 and out.stat().st_size > 0, r.stderr
    again = mm.paf_texts(text, kept_mask(text, out.read_bytes().decode()))
    assert bed.read_bytes() == again[0] and share.read_bytes() == again[1]


def test_smallest_shapes_on_a_fresh_context(sw):
    """The seams around the kernels at the smallest shapes -- one record; three records of one sequence pair in one chain -- on a
    context of its own: its first call sizes the arena from the input, the later ones find it sized.  Each shape twice, host seam
    against device seam byte for byte and both against the model."""
    a = np.array([(0, 1, 10, 110, 20, 125, 90), (0, 1, 200, 300, 210, 310, 80), (0, 1, 400, 450, 420, 470, 50)], dtype=np.uint32)
    seq_genome = np.array([0, 1], dtype=np.uint32)
    ctx = sw.Context(0)
    try:
        for n in (1, 3, 1, 3):
            cols = {c: a[:n, j].copy() for j, c in enumerate(("q_id", "t_id", "q_start", "q_end", "t_start", "t_end", "matches"))}
            for status in (None, np.ones(n, dtype=np.uint8)):   # (None: the optional columns stay NULL on their way to the device)
                for weight in (None, np.arange(n, dtype=np.uint32) + 7):
                    got = check(sw, cols, seq_genome, status, weight, 0, None, f"n = {n}", ctx=ctx)
                    assert len(got.rows) == n
    finally:
        ctx.close()
