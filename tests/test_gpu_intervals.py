"""Intervals on the device (sweepga_amd/csrc/swg_intervals.hip) against tests/intervals_model.py: the two record seams on the
shapes tests/test_gpu_breadth.py uses, the hand case of tests/test_intervals_cpu.py, the agreement with breadth, inputs built
around the edges of the 1024-record tile, a carry over 10^6 records, the LOST stage at a size that crosses many work-groups, the
hashed segment set, a real filter status, a memory limit, and the text of swg_paf_intervals / --lost / --covered byte for byte.
Every comparison is exact: integers and bytes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import intervals_model as im
from tests.test_gpu_alnstats import filter_cfgs, gen_text, records_of, run_filter
from tests.test_gpu_breadth import SHAPE_NAMES, one_pair_columns, paf_columns, shape_texts
from tests.test_gpu_wide import Hip
from tests.test_intervals_cpu import COLS, hand_case

pytestmark = pytest.mark.gpu
EVERY = [(s, a) for s in im.SETS for a in im.AXES]


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


@pytest.fixture(scope="module")
def shapes():
    return shape_texts()


def same_lists(a, b):
    return sorted(a) == sorted(b) and all(im.same_rows(a[k], b[k]) for k in a) and a.bases == b.bases


def both_seams(sw, cols, seq_genome, status, want=None, ctx=None):
    """The lists from the host seam, after checking that the device seam gives the same rows in the same order."""
    from sweepga_amd.intervals import _call, intervals_records
    ctx = ctx or sw.default_context()
    G = int(seq_genome.max()) + 1
    got = intervals_records(ctx, cols, seq_genome, status, n_genome=G, want=want)
    hip = Hip()
    try:
        dcols = {name: hip.up(np.ascontiguousarray(cols[name], dtype=np.uint32)) for name in COLS}
        rec = records_of(dcols, len(seq_genome), len(cols["q_id"]))
        d_status = hip.up(np.ascontiguousarray(status, dtype=np.uint8)) if status is not None else None
        mask = want if want is not None else (0x3f if status is not None else 0x3)
        dev = _call(ctx, ctx.lib.swg_intervals_records_device, rec, hip.up(seq_genome), G, d_status, mask)
    finally:
        hip.free()
    assert same_lists(dev, got)
    return got


def check(sw, cols, seq_genome, status, what="", ctx=None, model=None):
    got = both_seams(sw, cols, seq_genome, status, ctx=ctx)
    want = model or im.intervals(*[cols[c] for c in COLS], seq_genome, None if status is None else np.asarray(status) != 0)
    keys = EVERY if status is not None else [("all", "q"), ("all", "t")]
    assert sorted(got) == sorted(keys), what
    for k in keys:
        assert im.same_rows(got[k], want[k]), (what, k, len(got[k]), len(want[k]))
        assert got.bases[k] == int((want[k]["end"].astype(np.int64) - want[k]["start"]).sum()), (what, k)
    return got


@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_record_seams_against_the_model(sw, shapes, shape):
    rng = np.random.default_rng(len(shape))
    with sw.PafFile(text=shapes[shape]) as paf:
        cols, seq_genome = paf_columns(paf)
    n = len(cols["q_id"])
    status = (rng.random(n) < 0.4).astype(np.uint8) * rng.integers(1, 4, n).astype(np.uint8)
    got = check(sw, cols, seq_genome, status, shape)
    only_all = check(sw, cols, seq_genome, None, shape + " no status")
    assert all(im.same_rows(only_all["all", a], got["all", a]) for a in im.AXES) and len(got["all", "q"]) > 0 and len(got["lost", "t"]) > 0
    perm = rng.permutation(n)
    assert same_lists(both_seams(sw, {c: cols[c][perm] for c in COLS}, seq_genome, status[perm]), got)


def test_hand_case(sw):
    cols, seq_genome, status, want = hand_case()
    got = check(sw, cols, seq_genome, status, "hand")
    assert {k: im.as_tuples(v) for k, v in got.items()} == want


def test_the_two_call_capacity_protocol_and_the_want_bits(sw):
    from sweepga_amd._lib import SwgInterval, SwgIntervalRequest
    from sweepga_amd.intervals import INTERVAL_DTYPE, want_bits
    ctx = sw.default_context()
    cols, seq_genome, status, want = hand_case()
    rec = records_of(cols, len(seq_genome))
    req = SwgIntervalRequest()
    req.want = 0x3f
    poison = np.frombuffer(bytearray(b"\xab" * 16 * 4), dtype=INTERVAL_DTYPE)
    before = poison.copy()
    for s in range(3):
        for a in range(2):
            req.list[s][a].capacity = 0 if (s, a) != (2, 0) else 4          # one list with too small an array, the others with none
            req.list[s][a].rows = C.cast(poison.ctypes.data, C.POINTER(SwgInterval)) if (s, a) == (2, 0) else None
    ctx.check(ctx.lib.swg_intervals_records(ctx.handle, C.byref(rec), seq_genome.ctypes.data, 3, status.ctypes.data, C.byref(req)))
    assert poison.tobytes() == before.tobytes()
    bufs = {}
    for s, a in ((s, a) for s in range(3) for a in range(2)):
        key = (im.SETS[s], im.AXES[a])
        lst = req.list[s][a]
        assert int(lst.n) == len(want[key]) and int(lst.bases) == sum(r[3] - r[2] for r in want[key]), key
        bufs[key] = np.zeros(int(lst.n) + 1, dtype=INTERVAL_DTYPE)
        bufs[key][-1] = (7, 7, 7, 7)
        lst.capacity, lst.rows = int(lst.n), C.cast(bufs[key].ctypes.data, C.POINTER(SwgInterval))
    ctx.check(ctx.lib.swg_intervals_records(ctx.handle, C.byref(rec), seq_genome.ctypes.data, 3, status.ctypes.data, C.byref(req)))
    for key, b in bufs.items():
        assert im.as_tuples(b[:-1]) == want[key] and im.as_tuples(b[-1:]) == [(7, 7, 7, 7)], key
    # a clear bit leaves its list untouched, and the passes only it would need are not launched
    ctx.profile(True)
    try:
        for names, launches in (([("all", "q")], {"intervals_write": 1, "intervals_lost_flags": 0, "intervals_lost_write": 0}),
                                ([("lost", "t")], {"intervals_write": 1, "intervals_lost_flags": 1, "intervals_lost_write": 1}),
                                ([("kept", "q"), ("kept", "t")], {"intervals_write": 2, "intervals_lost_flags": 0})):
            req = SwgIntervalRequest()
            req.want = want_bits(names)
            for s in range(3):
                for a in range(2):
                    req.list[s][a].n = req.list[s][a].bases = 12345
            ctx.profile_reset()
            ctx.check(ctx.lib.swg_intervals_records(ctx.handle, C.byref(rec), seq_genome.ctypes.data, 3, status.ctypes.data, C.byref(req)))
            table = ctx.profile_table()
            for name, count in launches.items():
                assert (table[name][0] if name in table else 0) == count, (names, name, table)
            for s, a in ((s, a) for s in range(3) for a in range(2)):
                key = (im.SETS[s], im.AXES[a])
                assert int(req.list[s][a].n) == (len(want[key]) if key in names else 12345), (names, key)
    finally:
        ctx.profile(False)
    assert {k: im.as_tuples(v) for k, v in both_seams(sw, cols, seq_genome, status, want=want_bits([("lost", "q")])).items()} == {("lost", "q"): want["lost", "q"]}


def pair_sums(rows, axis, seq_genome, G):
    """{(q_genome, t_genome): bases} of a list."""
    mine = seq_genome[rows["seq"].astype(np.int64)].astype(np.int64)
    other = rows["other_genome"].astype(np.int64)
    key = mine * G + other if axis == "q" else other * G + mine
    sums = np.zeros(G * G, dtype=np.int64)
    np.add.at(sums, key, rows["end"].astype(np.int64) - rows["start"].astype(np.int64))
    return {(int(k) // G, int(k) % G): int(v) for k, v in enumerate(sums) if v}


def test_agreement_with_breadth(sw, shapes):
    from sweepga_amd.breadth import breadth_records
    rng = np.random.default_rng(17)
    with sw.PafFile(text=shapes["pansn"]) as paf:
        cols, seq_genome = paf_columns(paf)
    status = (rng.random(len(cols["q_id"])) < 0.4).astype(np.uint8)
    G = int(seq_genome.max()) + 1
    got = both_seams(sw, cols, seq_genome, status)
    a, k = breadth_records(sw.default_context(), cols, seq_genome, status, n_genome=G)
    for axis, field in (("q", "q_union"), ("t", "t_union")):
        all_ = {(int(p["q_genome"]), int(p["t_genome"])): int(p[field]) for p in a}
        kept = {(int(p["q_genome"]), int(p["t_genome"])): int(p[field]) for p in k}
        assert pair_sums(got["all", axis], axis, seq_genome, G) == {p: v for p, v in all_.items() if v}
        assert pair_sums(got["kept", axis], axis, seq_genome, G) == {p: v for p, v in kept.items() if v}
        assert pair_sums(got["lost", axis], axis, seq_genome, G) == {p: v - kept.get(p, 0) for p, v in all_.items() if v - kept.get(p, 0)}
        for s in im.SETS:
            assert got.bases[s, axis] == int((got[s, axis]["end"].astype(np.int64) - got[s, axis]["start"]).sum())
    assert sum(pair_sums(got["lost", "q"], "q", seq_genome, G).values()) > 0


def tile_edge_case():
    """Sequences 0 and 1 (genome 0) against sequence 2 (genome 1); in the query axis' sorted order: unit (0, 1) fills tile 0
    exactly, unit (1, 1) follows, a tail of intra-genome records closes.  -> (cols, seq_genome, status, facts to assert)."""
    rows = []   # (q, t, qs, qe)
    rows += [(0, 2, 10 * i, 10 * i + 10) for i in range(1023)]          # sorted 0..1022: touching, one interval
    rows += [(0, 2, 20_000, 20_010)]                                     # sorted 1023: a head, last record of tile 0 and of the unit
    rows += [(1, 2, 0, 5)]                                               # sorted 1024: the unit changes at the tile boundary; a head
    rows += [(1, 2, 100 + 10 * j, 105 + 10 * j) for j in range(1023)]    # sorted 1025..2047: apart, every one a head
    rows += [(1, 2, 20_000, 20_000)]                                     # sorted 2048: zero length, first record of tile 2, at ...
    rows += [(1, 2, 20_000, 20_100)]                                     # sorted 2049: ... the start of a true head after a gap
    rows += [(1, 2, 30_000, 1_000_000)]                                  # sorted 2050: one long record over ...
    rows += [(1, 2, 30_010 + 100 * j, 30_060 + 100 * j) for j in range(3_000)]   # ... 3000 short ones: its end is carried over tiles 2..4
    rows += [(1, 2, 2_000_000, 2_000_010)]                               # sorted 5051: the last counted record, a head after the carry
    n_counted = len(rows)
    rows += [(0, 1, 5 * j, 5 * j + 50) for j in range(100)]              # intra-genome: the sentinel region
    arr = np.array(rows, dtype=np.int64)
    n = len(arr)
    ts = np.arange(n, dtype=np.int64) * 100
    te = ts + np.where(arr[:, 3] > arr[:, 2], 7 + (np.arange(n) % 200), 0)     # (the target side: every record apart, some touching)
    cols = {k: v.astype(np.uint32) for k, v in zip(COLS, (arr[:, 0], arr[:, 1], arr[:, 2], arr[:, 3], ts, te))}
    status = (np.random.default_rng(5).random(n) < 0.5).astype(np.uint8)
    status[2050] = 0          # KEPT loses the long record: the short ones under it stand apart there
    status[2048] = 1          # the zero-length record is a KEPT record
    status[2049] = 1
    return cols, np.array([0, 0, 1], dtype=np.uint32), status, n_counted


def test_tile_edges(sw):
    cols, seq_genome, status, n_counted = tile_edge_case()
    # the construction is what it claims: the input order of the counted records IS the sorted order of the query axis
    q, s, e = (cols[c][:n_counted].astype(np.int64) for c in ("q_id", "q_start", "q_end"))
    assert np.array_equal(np.lexsort((s, q)), np.arange(n_counted)) and (q[:1024] == 0).all() and (q[1024:] == 1).all()
    assert s[2048] == e[2048] == s[2049] and s[2049] > e[2047] and n_counted == 5052 and 2050 // 1024 + 3 <= (n_counted - 1) // 1024 + 1
    got = check(sw, cols, seq_genome, status, "tile edges")
    rows = im.as_tuples(got["all", "q"])
    assert rows[:3] == [(0, 1, 0, 10_230), (0, 1, 20_000, 20_010), (1, 1, 0, 5)]
    assert rows[-3:] == [(1, 1, 20_000, 20_100), (1, 1, 30_000, 1_000_000), (1, 1, 2_000_000, 2_000_010)] and len(rows) == 3 + 1023 + 3
    kept = im.as_tuples(got["kept", "q"])
    assert (1, 1, 20_000, 20_100) in kept and len(kept) > 1_000
    perm = np.random.default_rng(6).permutation(len(status))
    assert same_lists(both_seams(sw, {c: cols[c][perm] for c in COLS}, seq_genome, status[perm]), got)


def test_tile_edges_with_one_set_scanned(sw):
    """The five tiles again, wanting only the KEPT lists and then only the ALL lists: the walk then carries one set across the
    tile edges and must leave the other set's carry alone.  The rows equal those of the all-six call, in both seams."""
    from sweepga_amd.intervals import want_bits
    cols, seq_genome, status, _ = tile_edge_case()
    every = both_seams(sw, cols, seq_genome, status)
    for name in ("kept", "all"):
        only = both_seams(sw, cols, seq_genome, status, want=want_bits([(name, "q"), (name, "t")]))
        assert sorted(only) == [(name, "q"), (name, "t")]
        for a in im.AXES:
            assert len(only[name, a]) > 1_000 and im.same_rows(only[name, a], every[name, a]), (name, a)
            assert only.bases[name, a] == every.bases[name, a], (name, a)


def test_a_far_carry(sw):
    """10^6 records of one unit under one long interval that KEPT does not have: 977 tiles of carry for ALL, none for KEPT."""
    n = 1_000_000
    rng = np.random.default_rng(91)
    s = np.concatenate([[0], rng.integers(1, 3_000_000_000, n - 1)])
    e = np.concatenate([[3_000_001_000], s[1:] + rng.integers(0, 1_000, n - 1)])
    ts = np.arange(n, dtype=np.int64) * 2_000
    te = ts + (e - s).clip(0, 1_500)
    status = np.ones(n, dtype=np.uint8)
    status[0] = 0
    cols, seq_genome = one_pair_columns(s, e, ts, te)
    perm = rng.permutation(n)
    got = check(sw, {c: v[perm] for c, v in cols.items()}, seq_genome, status[perm], "long over short")
    assert im.as_tuples(got["all", "q"]) == [(0, 1, 0, 3_000_001_000)] and len(got["kept", "q"]) > 100_000
    assert len(got["lost", "q"]) == len(got["kept", "q"]) + 1 and len(got["lost", "t"]) == 1


def test_the_lost_stage_across_many_work_groups(sw):
    rng = np.random.default_rng(23)
    n, n_units = 200_000, 2_000
    q = rng.integers(0, n_units, n)
    s = rng.integers(0, 290_000, n)
    e = s + rng.integers(1, 4_000, n)
    cols, seq_genome = one_pair_columns(s, e, s, e, q_seq=q)
    cols["t_start"], cols["t_end"] = (q * 300_000 + s).astype(np.uint32), (q * 300_000 + e).astype(np.uint32)
    status = (rng.random(n) < 0.3).astype(np.uint8)
    got = check(sw, cols, seq_genome, status, "lost at scale")
    assert 80_000 < len(got["all", "q"]) < 120_000 and 40_000 < len(got["kept", "q"]) < 60_000 and len(got["lost", "q"]) > 80_000
    only = both_seams(sw, cols, seq_genome, status, want=1 << 4)      # LOST of the query axis alone
    assert sorted(only) == [("lost", "q")] and im.same_rows(only["lost", "q"], got["lost", "q"])


def test_the_hashed_segment_set_gives_the_same_rows_in_the_same_order(sw, shapes, monkeypatch):
    with sw.PafFile(text=shapes["pansn"]) as paf:
        cols, seq_genome = paf_columns(paf)
    status = (np.arange(len(cols["q_id"])) % 3 != 0).astype(np.uint8)
    plain = both_seams(sw, cols, seq_genome, status)
    hand = hand_case()
    monkeypatch.setenv("SWG_BREADTH_HASH", "1")
    assert same_lists(check(sw, cols, seq_genome, status, "pansn, hashed"), plain)
    got = check(sw, hand[0], hand[1], hand[2], "hand, hashed")
    assert {k: im.as_tuples(v) for k, v in got.items()} == hand[3]


def test_a_real_filter_status(sw):
    FM = sw.FilterMode
    cfg = sw.FilterConfig(mapping_filter_mode=FM.OneToOne, mapping_max_per_query=1, mapping_max_per_target=1)   # --num-mappings 1:1
    text = gen_text(21, 20_000, n_genomes=4, chrs_per_genome=3, span=400_000)
    with sw.PafFile(text=text) as paf:
        status, _ = run_filter(sw, paf, cfg)
        cols, seq_genome = paf_columns(paf)
    assert 0 < int((status != 0).sum()) < len(status)
    got = check(sw, cols, seq_genome, status, "1:1")
    for axis in im.AXES:   # without the model: LOST and KEPT do not meet, and together they are ALL, unit by unit
        units = {}
        for s in im.SETS:
            for seq, other, a, b in im.as_tuples(got[s, axis]):
                units.setdefault((seq, other), {x: [] for x in im.SETS})[s].append((a, b))
        assert len(units) > 10
        for u, l in units.items():
            assert im.merged(l["kept"] + l["lost"]) == l["all"], (axis, u)
            assert sum(b - a for a, b in l["kept"] + l["lost"]) == sum(b - a for a, b in l["all"]), (axis, u)
        assert len(got["lost", axis]) > 0 and len(got["kept", axis]) > 0


def test_a_memory_limit_too_small_is_a_clean_oom(sw):
    from sweepga_amd.intervals import intervals_records
    ctx = sw.Context(0)
    try:
        rng = np.random.default_rng(51)
        with sw.PafFile(text=gen_text(52, 200_000, n_genomes=4, chrs_per_genome=3, span=400_000)) as paf:
            cols, seq_genome = paf_columns(paf)
        status = (rng.random(len(cols["q_id"])) < 0.5).astype(np.uint8)
        ctx.set_memory_limit(1 << 20)       # the staged columns alone are 5 MB
        with pytest.raises(sw.SwgError) as e:
            intervals_records(ctx, cols, seq_genome, status)
        assert e.value.code == -4
        ctx.set_memory_limit(0)             # ... and the context works on
        model = im.intervals(*[cols[c] for c in COLS], seq_genome, status != 0)
        check(sw, cols, seq_genome, status, "after the refusal", ctx=ctx, model=model)
        ctx.set_memory_limit(1 << 30)
        check(sw, cols, seq_genome, status, "under a limit that holds it", ctx=ctx, model=model)
        assert ctx.memory_info()[0] <= 1 << 30
    finally:
        ctx.close()


def test_ids_out_of_range(sw):
    from sweepga_amd.intervals import intervals_records
    ctx = sw.default_context()
    cols, seq_genome, status, _ = hand_case()
    bad = {c: v.copy() for c, v in cols.items()}
    bad["t_id"][3] = len(seq_genome)
    for args, kw in (((bad, seq_genome, status), {}), ((cols, seq_genome, status), {"n_genome": 2}), ((cols, seq_genome, None), {"want": 0x4}),
                     ((cols, seq_genome, status), {"want": 0x40})):
        with pytest.raises(sw.SwgError) as e:
            intervals_records(ctx, *args, **kw)
        assert e.value.code == -1


# ---- the text ----------------------------------------------------------------------------------------------------------------
def kept_mask(in_text, out_text):
    """Which input lines were written: the output holds them in input order, each with tags appended."""
    lines = [ln for ln in in_text.split("\n") if ln]
    mask = np.zeros(len(lines), dtype=bool)
    k = 0
    for out in (ln for ln in out_text.split("\n") if ln):
        while not out.startswith(lines[k]):
            k += 1
        mask[k] = True
        k += 1
    return mask


def model_texts(in_text, kept):
    cols, seq_genome, names, genomes = im.parse_paf(in_text)
    lists = im.intervals(*[cols[c] for c in COLS], seq_genome, kept)
    return {s: im.render(lists, s, names, genomes) for s in im.SETS}


def test_text_of_an_open_paf_equals_the_model_rendering(sw, tmp_path):
    text = gen_text(61, 12_000, n_genomes=4, chrs_per_genome=3, span=300_000)
    with sw.PafFile(text=text) as paf:
        status, chain = run_filter(sw, paf, filter_cfgs(sw)["one_to_one"])
        want = model_texts(text, status != 0)
        t = sw.Intervals.from_paf(sw.default_context(), paf, status)
        assert t.text == want and len(want["lost"]) > 0 and len(want["kept"]) > 0
        assert sw.Intervals.from_paf(sw.default_context(), paf).text == {"all": want["all"]}
        assert sw.Intervals.from_paf(sw.default_context(), paf, status, sets=("lost",)).text == {"lost": want["lost"]}
    ln = "\t".join(["a#1#x", str(2**33), str(2**32), str(2**32 + 50), "+", "b#1#y", "900", "10", "60", "50", "50", "60"]) + "\n"
    with sw.PafFile(text=ln) as paf:
        with pytest.raises(sw.SwgError) as e:
            sw.Intervals.from_paf(sw.default_context(), paf)
        assert e.value.code == -6 and "2^32" in str(e.value)


def test_cli_lost_and_covered(sw, tmp_path):
    from sweepga_amd import build
    text = gen_text(71, 15_000, n_genomes=4, chrs_per_genome=3, span=400_000)
    inp = tmp_path / "in.paf"
    inp.write_text(text, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-jump", "10k", "--scaffold-mass", "2k", "--quiet"]
    plain, out, lost, covered = (tmp_path / x for x in ("plain.paf", "out.paf", "lost.bed", "covered.bed"))
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), *flags], capture_output=True)
    assert r0.returncode == 0 and plain.stat().st_size > 0, r0.stderr
    want = model_texts(text, kept_mask(text, plain.read_bytes().decode()))
    assert len(want["lost"]) > 0 and len(want["kept"]) > 0
    for given in (("lost",), ("covered",), ("lost", "covered")):
        for p in (out, lost, covered):
            p.unlink(missing_ok=True)
        extra = (["--lost", str(lost)] if "lost" in given else []) + (["--covered", str(covered)] if "covered" in given else [])
        r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), *extra, *flags], capture_output=True)
        assert r.returncode == 0 and r.stdout == b"" and out.read_bytes() == plain.read_bytes(), r.stderr
        assert lost.exists() == ("lost" in given) and covered.exists() == ("covered" in given)
        assert "lost" not in given or lost.read_bytes() == want["lost"]
        assert "covered" not in given or covered.read_bytes() == want["kept"]
    # - : the text on standard error, the PAF alone on standard output
    r1 = subprocess.run([build.CLI, str(inp), *flags], capture_output=True)
    r2 = subprocess.run([build.CLI, str(inp), "--lost", "-", *flags], capture_output=True)
    assert r1.returncode == r2.returncode == 0 and r2.stdout == r1.stdout == plain.read_bytes() and r2.stderr == want["lost"]
    # --no-filter: every line to standard output, the device is opened, nothing is lost and --covered is ALL
    r = subprocess.run([build.CLI, str(inp), "--no-filter", "--lost", str(lost), "--covered", str(covered)], capture_output=True)
    assert r.returncode == 0 and r.stdout == text.encode() and lost.read_bytes() == b"" and covered.read_bytes() == want["all"]
    # --sparsify tree: all = the whole input, kept = what is written
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--sparsify", "tree:1", "--lost", str(lost), "--covered", str(covered), *flags],
                       capture_output=True)
    assert r.returncode == 0 and out.stat().st_size > 0, r.stderr
    want = model_texts(text, kept_mask(text, out.read_bytes().decode()))
    assert lost.read_bytes() == want["lost"] and covered.read_bytes() == want["kept"]


def test_smallest_shapes_on_a_fresh_context(sw):
    """The seams around the kernels at the smallest shapes -- one record; three records of one sequence pair in one chain -- on a
    context of its own: its first call sizes the arena from the input, the later ones find it sized.  Each shape twice, host seam
    against device seam byte for byte and both against the model."""
    a = np.array([(0, 1, 10, 110, 20, 125), (0, 1, 200, 300, 210, 310), (0, 1, 400, 450, 420, 470)], dtype=np.uint32)
    seq_genome = np.array([0, 1], dtype=np.uint32)
    ctx = sw.Context(0)
    try:
        for n in (1, 3, 1, 3):
            cols = {c: a[:n, j].copy() for j, c in enumerate(("q_id", "t_id", "q_start", "q_end", "t_start", "t_end"))}
            for status in (None, np.ones(n, dtype=np.uint8)):   # (None: the optional column stays NULL on its way to the device)
                got = check(sw, cols, seq_genome, status, f"n = {n}", ctx=ctx)
                assert len(got["all", "q"]) == n == len(got["all", "t"])
    finally:
        ctx.close()
