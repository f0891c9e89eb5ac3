"""Sharing on the device (sweepga_amd/csrc/swg_sharing.hip) against tests/sharing_model.py: the two record seams on the shapes
tests/test_gpu_breadth.py uses, the hand case of tests/test_sharing_cpu.py, inputs built around the 1024-entry tile, event groups
of 600 equal keys, sequence borders, the largest coordinate, a carry over 10^5 records, 10^5 runs, the hashed segment set, a real
filter status, the capacity protocol and the want bits, the limits, a memory limit, and the texts of swg_paf_sharing / --sharing /
--sharing-bed byte for byte.  Every comparison is exact: integers and bytes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import sharing_model as sm
from tests.test_gpu_alnstats import filter_cfgs, gen_text, records_of, run_filter
from tests.test_gpu_breadth import SHAPE_NAMES, paf_columns, shape_texts
from tests.test_gpu_intervals import kept_mask
from tests.test_gpu_wide import Hip
from tests.test_sharing_cpu import COLS, HAND_SPECTRUM, HAND_TABLE, check_hand, hand_case, hand_paf

pytestmark = pytest.mark.gpu
SETS = ("all", "kept")


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


@pytest.fixture(scope="module")
def shapes():
    return shape_texts()


def same_results(a, b):
    return (sorted(a.runs) == sorted(b.runs) and all(sm.same_rows(a.runs[k], b.runs[k]) for k in a.runs) and a.bases == b.bases
            and sorted(a.spectrum) == sorted(b.spectrum) and all(np.array_equal(a.spectrum[k], b.spectrum[k]) for k in a.spectrum))


def lengths_for(cols, n_seq, slack=17):
    """A length for every sequence that holds all its records."""
    out = np.zeros(n_seq, dtype=np.int64)
    np.maximum.at(out, cols["q_id"].astype(np.int64), cols["q_end"].astype(np.int64))
    np.maximum.at(out, cols["t_id"].astype(np.int64), cols["t_end"].astype(np.int64))
    return np.minimum(out + slack, 0xffffffff).astype(np.uint32)


def both_seams(sw, cols, seq_genome, seq_len, status, want=None, ctx=None, G=None):
    """The result of the host seam, after checking that the device seam gives the same."""
    from sweepga_amd.sharing import _call, sharing_records
    ctx = ctx or sw.default_context()
    G = G or int(seq_genome.max()) + 1
    if want is None:
        want = (0xf if status is not None else 0x5) & (0xf if G <= 4096 else 0x3)
    got = sharing_records(ctx, cols, seq_genome, seq_len, status, n_genome=G, want=want)
    hip = Hip()
    try:
        dcols = {name: hip.up(np.ascontiguousarray(cols[name], dtype=np.uint32)) for name in COLS}
        rec = records_of(dcols, len(seq_genome), len(cols["q_id"]))
        d_status = hip.up(np.ascontiguousarray(status, dtype=np.uint8)) if status is not None else None
        d_len = hip.up(np.ascontiguousarray(seq_len, dtype=np.uint32)) if seq_len is not None else None
        dev = _call(ctx, ctx.lib.swg_sharing_records_device, rec, hip.up(np.ascontiguousarray(seq_genome, dtype=np.uint32)), G, d_len, d_status, want)
    finally:
        hip.free()
    assert same_results(dev, got)
    return got


def check(sw, cols, seq_genome, seq_len, status, what="", ctx=None, models=None):
    """Both seams against the model (`models`: {set: (runs, spectrum)} computed before)."""
    G = int(seq_genome.max()) + 1
    got = both_seams(sw, cols, seq_genome, seq_len, status, ctx=ctx)
    for name in SETS if status is not None else SETS[:1]:
        mask = None if name == "all" else np.asarray(status) != 0
        runs, spectrum = models[name] if models else sm.sharing(cols, seq_genome, seq_len, mask, G, spectrum=G <= 4096)
        assert sm.same_rows(got.runs[name], runs), (what, name, len(got.runs[name]), len(runs))
        assert got.bases[name] == int((runs["end"].astype(np.int64) - runs["start"]).sum()), (what, name)
        if G <= 4096:
            assert np.array_equal(got.spectrum[name], spectrum), (what, name)
            if seq_len is not None:   # a row sums to its genome's length
                assert got.spectrum[name].sum(axis=1).tolist() == [int(seq_len[seq_genome == g].astype(np.int64).sum()) for g in range(G)], (what, name)
    assert sorted(got.runs) == sorted(SETS if status is not None else SETS[:1]), what
    return got


@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_record_seams_against_the_model(sw, shapes, shape):
    rng = np.random.default_rng(len(shape))
    with sw.PafFile(text=shapes[shape]) as paf:
        cols, seq_genome = paf_columns(paf)
    n = len(cols["q_id"])
    seq_len = lengths_for(cols, len(seq_genome))
    status = (rng.random(n) < 0.4).astype(np.uint8) * rng.integers(1, 4, n).astype(np.uint8)
    got = check(sw, cols, seq_genome, seq_len, status, shape)
    only_all = both_seams(sw, cols, seq_genome, None, None)
    assert sm.same_rows(only_all.runs["all"], got.runs["all"]) and len(got.runs["all"]) > 0 and len(got.runs["kept"]) > 0
    if "all" in only_all.spectrum:      # without lengths column 0 stays 0, the other columns are the same
        assert not only_all.spectrum["all"][:, 0].any() and np.array_equal(only_all.spectrum["all"][:, 1:], got.spectrum["all"][:, 1:])
    perm = rng.permutation(n)
    assert same_results(both_seams(sw, {c: cols[c][perm] for c in COLS}, seq_genome, seq_len, status[perm]), got)


def test_hand_case(sw):
    cols, seq_genome, seq_len, status, want = hand_case()
    got = check(sw, cols, seq_genome, seq_len, status, "hand")
    check_hand(got.runs["all"], got.spectrum["all"], got.runs["kept"], got.spectrum["kept"], want)
    assert got.bases == {"all": want["bases_all"], "kept": want["bases_kept"]}
    two = both_seams(sw, cols, np.array([0, 0, 1, 1, 1], dtype=np.uint32), seq_len, status)      # two genomes: only private and core
    assert set(two.runs["all"]["depth"].tolist()) == {1} and two.spectrum["all"].shape == (2, 2)
    one = both_seams(sw, cols, np.zeros(5, dtype=np.uint32), seq_len, status)                      # one genome: everything private
    assert len(one.runs["all"]) == 0 and one.spectrum["kept"].tolist() == [[int(seq_len.sum())]]


@pytest.mark.parametrize("n", [511, 512, 513])
def test_around_the_tile_of_1024_entries(sw, n):
    """n records between sequence 0 and sequence 1: n entries per axis, 2 n sorted entries -- 1022, 1024, 1026 -- with chains of
    overlapping intervals that run across the tile's edge, zero-length records and gaps among them."""
    rng = np.random.default_rng(n)
    i = np.arange(n, dtype=np.int64)
    qs, ts = 10 * i + (i > 300) * 50, 7 * i
    qe = qs + np.where((i % 97 == 0) & (i > 0), 0, 25)      # chains [10 i, 10 i + 25), a gap after 300, some empty
    te = ts + np.where((i > n - 40) | (i < 5), 9, 3)        # apart, then one chain up to the last entry
    cols = {"q_id": np.zeros(n), "t_id": np.ones(n), "q_start": qs, "q_end": qe, "t_start": ts, "t_end": te}
    cols = {k: np.asarray(v).astype(np.uint32) for k, v in cols.items()}
    seq_genome = np.array([0, 1], dtype=np.uint32)
    status = (rng.random(n) < 0.7).astype(np.uint8)
    perm = rng.permutation(n)
    got = check(sw, {c: v[perm] for c, v in cols.items()}, seq_genome, lengths_for(cols, 2), status[perm], "tile %d" % n)
    assert sm.as_tuples(got.runs["all"])[:2] == [(0, 0, 3_025, 1), (0, 3_060, 10 * (n - 1) + 75, 1)]
    assert sm.as_tuples(got.runs["all"])[-1] == (1, 7 * (n - 39), 7 * (n - 1) + 9, 1)


def test_tile_edges_with_one_set_scanned(sw):
    """The five-tile input of tests/test_gpu_intervals.py, wanting only the ALL runs (0x1) and then only the KEPT runs (0x2): the
    other set's tile maxima are never scanned then, and a walk that read them as a carry would be using unscanned values.  The
    runs equal those of the 0xf call, in both seams."""
    from tests.test_gpu_intervals import tile_edge_case
    cols, seq_genome, status, _ = tile_edge_case()
    seq_len = lengths_for(cols, len(seq_genome))
    every = both_seams(sw, cols, seq_genome, seq_len, status, want=0xf)
    for bit, name in ((0x1, "all"), (0x2, "kept")):
        only = both_seams(sw, cols, seq_genome, seq_len, status, want=bit)
        assert sorted(only.runs) == [name] and not only.spectrum
        assert len(only.runs[name]) > 1_000 and sm.same_rows(only.runs[name], every.runs[name]), name
        assert only.bases[name] == every.bases[name], name


def piles(ends):
    """Genome g = 1 .. len(ends) covers sequence 0 (genome 0) over [0, ends[g - 1]) from the target axis."""
    k = len(ends)
    cols = {"q_id": np.arange(1, k + 1), "t_id": np.zeros(k), "q_start": np.full(k, 5), "q_end": np.full(k, 25), "t_start": np.zeros(k), "t_end": ends}
    return {c: np.asarray(v).astype(np.uint32) for c, v in cols.items()}, np.arange(k + 1, dtype=np.uint32)


def test_groups_of_600_equal_events(sw):
    """600 genomes, 599 of them over [0, 70000) of one sequence: 599 begins under one key and 599 ends under another -- groups that
    cross wavefronts, work-groups and the scan's tiles -- and one run of depth 599."""
    cols, seq_genome = piles(np.full(599, 70_000))
    seq_len = np.full(600, 80_000, dtype=np.uint32)
    status = (np.arange(599) % 3 != 0).astype(np.uint8)
    got = check(sw, cols, seq_genome, seq_len, status, "600 equal keys")
    assert sm.as_tuples(got.runs["all"])[0] == (0, 0, 70_000, 599) and sm.as_tuples(got.runs["kept"])[0] == (0, 0, 70_000, 399)
    assert len(got.runs["all"]) == 600 and got.spectrum["all"][0, 599] == 70_000 and got.spectrum["all"][0, 0] == 10_000
    # staggered ends: one genome leaves per run, and the depth steps down by one
    cols, seq_genome = piles(70_000 - 3 * np.arange(599))
    got = check(sw, cols, seq_genome, seq_len, status, "staggered")
    on0 = got.runs["all"][got.runs["all"]["seq"] == 0]
    assert on0["depth"].tolist() == list(range(599, 0, -1)) and on0["start"][1:].tolist() == on0["end"][:-1].tolist() and on0["start"][0] == 0


def test_sequence_borders_and_the_largest_coordinate(sw):
    top = 0xffffffff
    rows = [   # (q, t, qs, qe, ts, te): sequences 0, 1 of genome 0, sequences 2, 3 of genomes 1, 2
        (0, 2, 900, 1_000, 0, 100),          # sequence 0 is covered up to its last base ...
        (1, 2, 0, 50, 100, 150),             # ... and sequence 1 from base 0 on: two runs, though depth and position could pass for one
        (1, 3, 0, 50, 10, 60),               #     (depth 2 here: still no run crosses the border)
        (0, 3, 950, 1_000, top - 10, top),   # an end of 2^32 - 1
        (3, 0, top - 5, top, 990, 1_000),
    ]
    arr = np.array(rows, dtype=np.int64)
    cols = {k: arr[:, i].astype(np.uint32) for i, k in enumerate(COLS)}
    seq_genome = np.array([0, 0, 1, 2], dtype=np.uint32)
    seq_len = np.array([1_000, 50, 150, top], dtype=np.uint32)
    got = check(sw, cols, seq_genome, seq_len, np.array([1, 1, 0, 1, 1], dtype=np.uint8), "borders")
    assert sm.as_tuples(got.runs["all"]) == [(0, 900, 950, 1), (0, 950, 1_000, 2), (1, 0, 50, 2), (2, 0, 150, 1), (3, 10, 60, 1), (3, top - 10, top, 1)]
    assert sm.as_tuples(got.runs["kept"])[:3] == [(0, 900, 950, 1), (0, 950, 1_000, 2), (1, 0, 50, 1)]


def test_a_far_carry(sw):
    """10^5 records of one unit under one long record that KEPT does not have: one run for ALL, the carry over ~200 tiles."""
    n = 100_000
    rng = np.random.default_rng(91)
    s = np.concatenate([[0], rng.integers(1, 3_000_000_000, n - 1)])
    e = np.concatenate([[3_000_001_000], s[1:] + rng.integers(0, 1_000, n - 1)])
    ts = np.arange(n, dtype=np.int64) * 2_000
    te = ts + (e - s).clip(0, 1_500)
    cols = {"q_id": np.zeros(n), "t_id": np.ones(n), "q_start": s, "q_end": e, "t_start": ts, "t_end": te}
    cols = {k: np.asarray(v).astype(np.uint32) for k, v in cols.items()}
    status = np.ones(n, dtype=np.uint8)
    status[0] = 0
    perm = rng.permutation(n)
    got = check(sw, {c: v[perm] for c, v in cols.items()}, np.array([0, 1], dtype=np.uint32), None, status[perm], "long over short")
    assert sm.as_tuples(got.runs["all"])[0] == (0, 0, 3_000_001_000, 1) and int((got.runs["kept"]["seq"] == 0).sum()) > 50_000


def test_many_runs(sw):
    """More than 10^5 runs over 40 sequences and 5 genomes: both compactions and the run pass over many work-groups."""
    rng = np.random.default_rng(23)
    n, n_seq = 150_000, 40
    q, t = rng.integers(0, n_seq, n), rng.integers(0, n_seq, n)
    qs, ts = rng.integers(0, 4_000_000, n), rng.integers(0, 4_000_000, n)
    cols = {"q_id": q, "t_id": t, "q_start": qs, "q_end": qs + rng.integers(0, 900, n), "t_start": ts, "t_end": ts + rng.integers(0, 900, n)}
    cols = {k: np.asarray(v).astype(np.uint32) for k, v in cols.items()}
    seq_genome = (np.arange(n_seq) % 5).astype(np.uint32)
    status = (rng.random(n) < 0.5).astype(np.uint8)
    got = check(sw, cols, seq_genome, lengths_for(cols, n_seq), status, "many runs")
    assert len(got.runs["all"]) > 100_000 and int(got.runs["all"]["depth"].max()) >= 3


def test_the_hashed_segment_set_gives_the_same_answers(sw, shapes, monkeypatch):
    with sw.PafFile(text=shapes["pansn"]) as paf:
        cols, seq_genome = paf_columns(paf)
    seq_len = lengths_for(cols, len(seq_genome))
    status = (np.arange(len(cols["q_id"])) % 3 != 0).astype(np.uint8)
    plain = both_seams(sw, cols, seq_genome, seq_len, status)
    hand = hand_case()
    monkeypatch.setenv("SWG_BREADTH_HASH", "1")
    assert same_results(check(sw, cols, seq_genome, seq_len, status, "pansn, hashed"), plain)
    got = check(sw, hand[0], hand[1], hand[2], hand[3], "hand, hashed")
    check_hand(got.runs["all"], got.spectrum["all"], got.runs["kept"], got.spectrum["kept"], hand[4])


def test_a_real_filter_status(sw):
    FM = sw.FilterMode
    cfg = sw.FilterConfig(mapping_filter_mode=FM.OneToOne, mapping_max_per_query=1, mapping_max_per_target=1)   # --num-mappings 1:1
    text = gen_text(21, 20_000, n_genomes=4, chrs_per_genome=3, span=400_000)
    with sw.PafFile(text=text) as paf:
        status, _ = run_filter(sw, paf, cfg)
        cols, seq_genome = paf_columns(paf)
    assert 0 < int((status != 0).sum()) < len(status)
    got = check(sw, cols, seq_genome, lengths_for(cols, len(seq_genome)), status, "1:1")
    # without the model: the filter only takes away -- per genome, bases move towards lower depths
    a, k = got.spectrum["all"].astype(np.int64), got.spectrum["kept"].astype(np.int64)
    assert (np.cumsum(k, axis=1) >= np.cumsum(a, axis=1)).all() and (k[:, 0] > a[:, 0]).any() and got.bases["kept"] < got.bases["all"]


def test_the_capacity_protocol_and_the_want_bits(sw):
    from sweepga_amd._lib import SwgDepthRun, SwgSharingRequest
    from sweepga_amd.sharing import RUN_DTYPE
    ctx = sw.default_context()
    cols, seq_genome, seq_len, status, want = hand_case()
    rec = records_of(cols, len(seq_genome))
    call = lambda req: ctx.check(ctx.lib.swg_sharing_records(ctx.handle, C.byref(rec), seq_genome.ctypes.data, 3, seq_len.ctypes.data,
                                                             status.ctypes.data, C.byref(req)))
    req = SwgSharingRequest()
    req.want = 0x3
    poison = np.frombuffer(bytearray(b"\xab" * 16 * 4), dtype=RUN_DTYPE)
    before = poison.copy()
    req.set[1].capacity, req.set[1].rows = 4, C.cast(poison.ctypes.data, C.POINTER(SwgDepthRun))     # too small an array, and none
    call(req)
    assert poison.tobytes() == before.tobytes()
    bufs = {}
    for s, name in enumerate(SETS):
        lst = req.set[s]
        assert int(lst.n) == len(want["runs_" + name]) and int(lst.bases) == want["bases_" + name]
        bufs[name] = np.zeros(int(lst.n) + 1, dtype=RUN_DTYPE)
        bufs[name][-1] = (7, 7, 7, 7)
        lst.capacity, lst.rows = int(lst.n), C.cast(bufs[name].ctypes.data, C.POINTER(SwgDepthRun))
    call(req)
    for name, b in bufs.items():
        assert sm.as_tuples(b[:-1]) == want["runs_" + name] and sm.as_tuples(b[-1:]) == [(7, 7, 7, 7)], name
    # a clear bit leaves its part untouched, and the passes only it would need are not launched
    ctx.profile(True)
    try:
        for bits, launches in ((0x1, {"sharing_events": 1, "sharing_runs": 1, "sharing_bases": 1, "sharing_spectrum": 0, "sharing_lengths": 0}),
                               (0x2, {"sharing_events": 1, "sharing_runs": 1, "sharing_bases": 1, "sharing_spectrum": 0}),
                               (0x4, {"sharing_events": 1, "sharing_runs": 1, "sharing_bases": 0, "sharing_spectrum": 1, "sharing_private": 1}),
                               (0x8, {"sharing_runs": 1, "sharing_bases": 0, "sharing_spectrum": 1, "sharing_lengths": 1}),
                               (0xc, {"sharing_events": 1, "sharing_runs": 2, "sharing_bases": 0, "sharing_spectrum": 2}),
                               (0xf, {"sharing_keys": 1, "sharing_gather": 1, "sharing_count": 1, "sharing_events": 1, "sharing_runs": 2,
                                      "sharing_bases": 2, "sharing_spectrum": 2, "sharing_private": 2})):
            req = SwgSharingRequest()
            req.want = bits
            spectra = [np.full((3, 3), 99, dtype=np.uint64), np.full((3, 3), 99, dtype=np.uint64)]
            rows = [np.zeros(16, dtype=RUN_DTYPE), np.zeros(16, dtype=RUN_DTYPE)]
            for s in range(2):
                req.set[s].n = req.set[s].bases = 12345
                req.set[s].capacity, req.set[s].rows = 16, C.cast(rows[s].ctypes.data, C.POINTER(SwgDepthRun))
                req.set[s].spectrum = C.cast(spectra[s].ctypes.data, C.POINTER(C.c_uint64))
            ctx.profile_reset()
            call(req)
            table = ctx.profile_table()
            for name, count in launches.items():
                assert (table[name][0] if name in table else 0) == count, (bits, name, table)
            for s, name in enumerate(SETS):
                assert int(req.set[s].n) == (len(want["runs_" + name]) if bits >> s & 1 else 12345), (bits, name)
                assert sm.as_tuples(rows[s][:len(want["runs_" + name])]) == (want["runs_" + name] if bits >> s & 1 else [(0, 0, 0, 0)] * 11), (bits, name)
                assert spectra[s].tolist() == (want["spectrum_" + name] if bits >> (2 + s) & 1 else [[99] * 3] * 3), (bits, name)   # no row read back
    finally:
        ctx.profile(False)


def test_limits_and_ids_out_of_range(sw):
    from sweepga_amd.sharing import sharing_records
    ctx = sw.default_context()
    cols, seq_genome, seq_len, status, want = hand_case()
    # 4097 genomes: no spectrum, but the runs
    for bits in (0x4, 0x8, 0xf):
        with pytest.raises(sw.SwgError) as e:
            sharing_records(ctx, cols, seq_genome, seq_len, status, n_genome=4097, want=bits)
        assert e.value.code == -5 and "4096" in str(e.value)
    got = sharing_records(ctx, cols, seq_genome, seq_len, status, n_genome=4097, want=0x3)
    assert sm.as_tuples(got.runs["all"]) == want["runs_all"] and sm.as_tuples(got.runs["kept"]) == want["runs_kept"]
    got = sharing_records(ctx, cols, seq_genome, seq_len, status, n_genome=4096, want=0x4)
    assert got.spectrum["all"][:3, :3].tolist() == [[1_000, 400, 100], [1_870, 430, 0], [600, 200, 0]] and int(got.spectrum["all"].sum()) == 4_600
    bad = {c: v.copy() for c, v in cols.items()}
    bad["t_id"][3] = len(seq_genome)
    short = seq_len.copy()
    short[2] = 1_149        # record 1 ends at 1150 on b1
    for args, kw in (((bad, seq_genome, seq_len, status), {}), ((cols, seq_genome, seq_len, status), {"n_genome": 2}),
                     ((cols, seq_genome, short, status), {}), ((cols, seq_genome, seq_len, None), {"want": 0x2}),
                     ((cols, seq_genome, seq_len, status), {"want": 0x10})):
        with pytest.raises(sw.SwgError) as e:
            sharing_records(ctx, *args, **kw)
        assert e.value.code == -1
    # no records, but sequences: the lengths are all there is
    none = sharing_records(ctx, {c: np.zeros(0, dtype=np.uint32) for c in COLS}, seq_genome, seq_len, np.zeros(0, dtype=np.uint8))
    assert len(none.runs["all"]) == 0 and none.spectrum["kept"].tolist() == [[1_500, 0, 0], [2_300, 0, 0], [800, 0, 0]]


def test_a_memory_limit_too_small_is_a_clean_oom(sw):
    from sweepga_amd.sharing import sharing_records
    ctx = sw.Context(0)
    try:
        rng = np.random.default_rng(51)
        with sw.PafFile(text=gen_text(52, 100_000, n_genomes=4, chrs_per_genome=3, span=400_000)) as paf:
            cols, seq_genome = paf_columns(paf)
        seq_len = lengths_for(cols, len(seq_genome))
        status = (rng.random(len(cols["q_id"])) < 0.5).astype(np.uint8)
        ctx.set_memory_limit(1 << 20)       # the staged columns alone are 2.5 MB
        with pytest.raises(sw.SwgError) as e:
            sharing_records(ctx, cols, seq_genome, seq_len, status)
        assert e.value.code == -4
        ctx.set_memory_limit(0)             # ... and the context works on
        models = {"all": sm.sharing(cols, seq_genome, seq_len, None), "kept": sm.sharing(cols, seq_genome, seq_len, status != 0)}
        check(sw, cols, seq_genome, seq_len, status, "after the refusal", ctx=ctx, models=models)
        ctx.set_memory_limit(1 << 30)
        check(sw, cols, seq_genome, seq_len, status, "under a limit that holds it", ctx=ctx, models=models)
        assert ctx.memory_info()[0] <= 1 << 30
    finally:
        ctx.close()


# ---- the texts ---------------------------------------------------------------------------------------------------------------
def test_texts_of_an_open_paf_equal_the_model_rendering(sw):
    text, status = hand_paf()
    with sw.PafFile(text=text) as paf:
        s = sw.Sharing.from_paf(sw.default_context(), paf, status, detailed=True)
        assert s.table.decode() == HAND_TABLE + HAND_SPECTRUM and (s.table, s.bed) == sm.paf_texts(text, status != 0, detailed=True)
        assert sw.Sharing.from_paf(sw.default_context(), paf, status).table.decode() == HAND_TABLE
    text = gen_text(61, 12_000, n_genomes=4, chrs_per_genome=3, span=300_000)
    with sw.PafFile(text=text) as paf:
        status, _ = run_filter(sw, paf, filter_cfgs(sw)["one_to_one"])
        for detailed in (False, True):
            table, bed = sm.paf_texts(text, status != 0, detailed=detailed)
            s = sw.Sharing.from_paf(sw.default_context(), paf, status, detailed=detailed)
            assert s.table == table and s.bed == bed and len(bed) > 0 and table.count(b"\n") >= 6
        ctx = sw.default_context()      # one text alone, and only its passes
        ctx.profile(True)
        try:
            ctx.profile_reset()
            only = sw.Sharing.from_paf(ctx, paf, status, table=False)
            assert only.table is None and only.bed == bed and "sharing_spectrum" not in ctx.profile_table()
            ctx.profile_reset()
            only = sw.Sharing.from_paf(ctx, paf, status, bed=False)
            assert only.bed is None and only.table == sm.paf_texts(text, status != 0)[0] and "sharing_bases" not in ctx.profile_table()
        finally:
            ctx.profile(False)
    ln = "\t".join(["a#1#x", str(2**33), str(2**32), str(2**32 + 50), "+", "b#1#y", "900", "10", "60", "50", "50", "60"]) + "\n"
    with sw.PafFile(text=ln) as paf:
        with pytest.raises(sw.SwgError) as e:
            sw.Sharing.from_paf(sw.default_context(), paf, np.ones(1, dtype=np.uint8))
        assert e.value.code == -6 and "2^32" in str(e.value)


def test_cli_sharing(sw, tmp_path):
    from sweepga_amd import build
    text = gen_text(71, 15_000, n_genomes=4, chrs_per_genome=3, span=400_000)
    inp = tmp_path / "in.paf"
    inp.write_text(text, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-jump", "10k", "--scaffold-mass", "2k", "--quiet"]
    plain, out, table, bed = (tmp_path / x for x in ("plain.paf", "out.paf", "sharing.tsv", "sharing.bed"))
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), *flags], capture_output=True)
    assert r0.returncode == 0 and plain.stat().st_size > 0, r0.stderr
    kept = kept_mask(text, plain.read_bytes().decode())
    want = {d: sm.paf_texts(text, kept, detailed=d) for d in (False, True)}
    assert len(want[False][1]) > 0
    for given in (("table",), ("bed",), ("table", "bed"), ("table", "detailed", "bed")):
        for p in (out, table, bed):
            p.unlink(missing_ok=True)
        extra = (["--sharing", str(table)] if "table" in given else []) + (["--sharing-bed", str(bed)] if "bed" in given else [])
        extra += ["--sharing-detailed"] if "detailed" in given else []
        r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), *extra, *flags], capture_output=True)
        assert r.returncode == 0 and r.stdout == b"" and out.read_bytes() == plain.read_bytes(), r.stderr     # the PAF does not change
        assert table.exists() == ("table" in given) and bed.exists() == ("bed" in given)
        assert "table" not in given or table.read_bytes() == want["detailed" in given][0]
        assert "bed" not in given or bed.read_bytes() == want[False][1]
    # - : the text on standard error, the PAF alone on standard output
    r1 = subprocess.run([build.CLI, str(inp), *flags], capture_output=True)
    r2 = subprocess.run([build.CLI, str(inp), "--sharing", "-", *flags], capture_output=True)
    assert r1.returncode == r2.returncode == 0 and r2.stdout == r1.stdout == plain.read_bytes() and r2.stderr == want[False][0]
    # --no-filter: every line to standard output, the device is opened, kept = all
    r = subprocess.run([build.CLI, str(inp), "--no-filter", "--sharing", str(table), "--sharing-bed", str(bed)], capture_output=True)
    every = sm.paf_texts(text, np.ones(len(kept), dtype=bool))
    assert r.returncode == 0 and r.stdout == text.encode() and table.read_bytes() == every[0] and bed.read_bytes() == every[1]
    # --sparsify tree: all = the whole input, kept = what is written
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--sparsify", "tree:1", "--sharing", str(table), "--sharing-bed", str(bed), *flags],
                       capture_output=True)
    assert r.returncode == 0 and out.stat().st_size > 0, r.stderr
    again = sm.paf_texts(text, kept_mask(text, out.read_bytes().decode()))
    assert table.read_bytes() == again[0] and bed.read_bytes() == again[1]


def test_smallest_shapes_on_a_fresh_context(sw):
    """The seams around the kernels at the smallest shapes -- one record; three records of one sequence pair in one chain -- on a
    context of its own: its first call sizes the arena from the input, the later ones find it sized.  Each shape twice, host seam
    against device seam byte for byte and both against the model."""
    a = np.array([(0, 1, 10, 110, 20, 125), (0, 1, 200, 300, 210, 310), (0, 1, 400, 450, 420, 470)], dtype=np.uint32)
    seq_genome, seq_len = np.array([0, 1], dtype=np.uint32), np.array([1000, 1000], dtype=np.uint32)
    ctx = sw.Context(0)
    try:
        for n in (1, 3, 1, 3):
            cols = {c: a[:n, j].copy() for j, c in enumerate(("q_id", "t_id", "q_start", "q_end", "t_start", "t_end"))}
            for status in (None, np.ones(n, dtype=np.uint8)):   # (None: the optional columns stay NULL on their way to the device)
                got = check(sw, cols, seq_genome, seq_len, status, f"n = {n}", ctx=ctx)
                assert len(got.runs["all"]) == 2 * n
            without = both_seams(sw, cols, seq_genome, None, None, ctx=ctx)
            assert sm.same_rows(without.runs["all"], got.runs["all"]) and not without.spectrum["all"][:, 0].any()
    finally:
        ctx.close()
