"""Breadth on the device (sweepga_amd/csrc/swg_breadth.hip) against tests/breadth_model.py: the two record seams on the shapes
tests/test_gpu_alnstats.py uses, the hand cases of tests/test_breadth_cpu.py, a real filter status, order independence, the
agreement with the alnstats seam, inputs that make the running maximum travel far, one case large enough for the hashed pair
table and multi-tile sorts, a memory limit, and the report of swg_paf_breadth / --breadth byte for byte.  Every comparison is
exact: integers and bytes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import breadth_model as bm
from tests.test_breadth_cpu import as_rows, hand_case
from tests.test_gpu_alnstats import filter_cfgs, gen_text, named_text, records_of, run_filter
from tests.test_gpu_wide import Hip

pytestmark = pytest.mark.gpu
COLS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


def both_seams(sw, cols, seq_genome, status, ctx=None):
    """(all, kept) from the host seam, after checking that the device seam gives the same."""
    from sweepga_amd.breadth import _call, breadth_records
    ctx = ctx or sw.default_context()
    G = int(seq_genome.max()) + 1
    a, k = breadth_records(ctx, cols, seq_genome, status, n_genome=G)
    hip = Hip()
    try:
        dcols = {name: hip.up(np.ascontiguousarray(cols[name], dtype=np.uint32)) for name in COLS}
        rec = records_of(dcols, len(seq_genome), len(cols["q_id"]))
        d_status = hip.up(np.ascontiguousarray(status, dtype=np.uint8)) if status is not None else None
        a2, k2 = _call(ctx, ctx.lib.swg_breadth_records_device, rec, hip.up(seq_genome), G, d_status)
    finally:
        hip.free()
    assert bm.same_pairs(a2, a) and (status is None or bm.same_pairs(k2, k))
    return a, k


def check(sw, cols, seq_genome, status, what="", ctx=None):
    a, k = both_seams(sw, cols, seq_genome, status, ctx)
    args = [cols[c] for c in COLS]
    assert bm.same_pairs(a, bm.breadth(*args, seq_genome)), (what, "all")
    if status is not None:
        assert bm.same_pairs(k, bm.breadth(*args, seq_genome, np.asarray(status) != 0)), (what, "kept")
    else:
        assert k is None
    assert (a["q_union"] <= a["q_bases"]).all() and (a["t_union"] <= a["t_bases"]).all(), what
    return a, k


def paf_columns(paf):
    return {c: paf.column(c).copy() for c in COLS}, paf.seq_genome_last.copy()


def shape_texts():
    return {
        "pansn": gen_text(1, 6_000, n_genomes=5, chrs_per_genome=4),
        "pansn_selfheavy": gen_text(2, 3_000, n_genomes=2, chrs_per_genome=2, self_frac=0.3),
        "one_hash": named_text(3, 4_000, ["g%d#chr%d" % (g, c) for g in range(6) for c in range(3)]),
        "three_hashes": named_text(4, 4_000, ["s%d#%d#x%d#chr%d" % (g, g % 2, g % 3, c) for g in range(7) for c in range(3)]),
        "no_hash_20000_contigs": named_text(5, 60_000, ["ctg%05d" % i for i in range(20_000)]),
        # 64 genomes of one contig, dense pair table: a sorted tile of 1024 records holds more pairs than the LDS table takes
        "no_hash_64_contigs": named_text(6, 8_192, ["ctg%02d" % i for i in range(64)]),
    }


SHAPE_NAMES = ("no_hash_20000_contigs", "no_hash_64_contigs", "one_hash", "pansn", "pansn_selfheavy", "three_hashes")


@pytest.fixture(scope="module")
def shapes():
    """The texts, built once when the first test asks for them: nothing at collection."""
    texts = shape_texts()
    assert sorted(texts) == list(SHAPE_NAMES)
    return texts


@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_record_seams_against_the_model(sw, shapes, shape):
    rng = np.random.default_rng(len(shape))
    with sw.PafFile(text=shapes[shape]) as paf:
        cols, seq_genome = paf_columns(paf)
    status = (rng.random(len(cols["q_id"])) < 0.4).astype(np.uint8) * rng.integers(1, 4, len(cols["q_id"])).astype(np.uint8)
    a, _ = check(sw, cols, seq_genome, status, shape)
    a1, none = check(sw, cols, seq_genome, None, shape + " no status")
    assert bm.same_pairs(a1, a) and len(a) > 0
    # a shuffled copy: the same values per pair, matched by key
    perm = rng.permutation(len(status))
    b, kb = both_seams(sw, {c: cols[c][perm] for c in COLS}, seq_genome, status[perm])
    a, k = both_seams(sw, cols, seq_genome, status)
    assert bm.by_key(b) == bm.by_key(a) and bm.by_key(kb) == bm.by_key(k)


def test_hand_cases(sw):
    cols, seq_genome, status, want_all, want_kept = hand_case()
    a, k = check(sw, cols, seq_genome, status, "hand")
    assert as_rows(a) == want_all and as_rows(k) == want_kept


def test_hashed_segments_and_pair_table_at_small_size(sw, shapes, monkeypatch):
    """SWG_BREADTH_HASH=1 sends a small input through the open-addressing segment set and the hashed pair table, which sizes alone
    select only beyond 2^32 (sequence, genome) products and 2^20 genome pairs."""
    monkeypatch.setenv("SWG_BREADTH_HASH", "1")
    cols, seq_genome, status, want_all, want_kept = hand_case()
    a, k = check(sw, cols, seq_genome, status, "hand, hashed")
    assert as_rows(a) == want_all and as_rows(k) == want_kept
    with sw.PafFile(text=shapes["pansn"]) as paf:
        cols, seq_genome = paf_columns(paf)
    check(sw, cols, seq_genome, (np.arange(len(cols["q_id"])) % 3 != 0).astype(np.uint8), "pansn, hashed")


@pytest.mark.parametrize("cfg_name", ["default", "one_to_one_scaffolds"])
def test_a_real_filter_status(sw, cfg_name):
    """KEPT under the status swg_filter leaves == the model on the mask == ALL of the compacted kept subset; q_bases and the listing
    order are those of the alnstats seam."""
    from sweepga_amd.alnstats import alnstats_counts
    FM = sw.FilterMode
    cfg = filter_cfgs(sw)["default"] if cfg_name == "default" else sw.FilterConfig(
        mapping_filter_mode=FM.OneToOne, mapping_max_per_query=1, mapping_max_per_target=1,
        scaffold_filter_mode=FM.OneToOne, scaffold_max_per_query=1, scaffold_max_per_target=1)   # --num-mappings 1:1 --scaffold-filter 1:1
    text = gen_text(21, 20_000, n_genomes=4, chrs_per_genome=3, span=400_000)
    with sw.PafFile(text=text) as paf:
        status, _ = run_filter(sw, paf, cfg)
        cols, seq_genome = paf_columns(paf)
        matches = paf.column("matches").copy()
    assert int((status != 0).sum()) > 0
    a, k = check(sw, cols, seq_genome, status, cfg_name)
    sel = status != 0
    sub, none = both_seams(sw, {c: cols[c][sel] for c in COLS}, seq_genome, None)
    assert bm.by_key(sub) == bm.by_key(k) and [(int(p["q_genome"]), int(p["t_genome"])) for p in sub] == [(int(p["q_genome"]), int(p["t_genome"])) for p in k]
    assert np.array_equal(np.flatnonzero(sel)[sub["first_record"].astype(np.int64)], k["first_record"].astype(np.int64))
    # the alnstats seam on the same input: same pairs, same order, bases = q_bases
    G = int(seq_genome.max()) + 1
    rec = records_of({"q_id": cols["q_id"], "t_id": cols["t_id"], "q_start": cols["q_start"], "q_end": cols["q_end"], "matches": matches}, len(seq_genome))
    sa, sk = alnstats_counts(sw.default_context(), rec, seq_genome, G, status)
    for mine, theirs in ((a, sa["pairs"]), (k, sk["pairs"])):
        assert len(mine) == len(theirs)
        for f_mine, f_theirs in (("q_genome", "q_genome"), ("t_genome", "t_genome"), ("q_bases", "bases"), ("first_record", "first_record")):
            assert np.array_equal(mine[f_mine].astype(np.uint64), theirs[f_theirs].astype(np.uint64)), (cfg_name, f_mine)


def one_pair_columns(q_start, q_end, t_start, t_end, q_seq=None):
    """Records of sequence 0 (genome 0) -- or of the sequences q_seq, each its own genome -- against the last sequence."""
    n = len(q_start)
    q = np.zeros(n, dtype=np.uint32) if q_seq is None else q_seq.astype(np.uint32)
    n_seq = int(q.max()) + 2
    cols = {"q_id": q, "t_id": np.full(n, n_seq - 1, dtype=np.uint32), "q_start": q_start.astype(np.uint32), "q_end": q_end.astype(np.uint32),
            "t_start": t_start.astype(np.uint32), "t_end": t_end.astype(np.uint32)}
    return cols, np.arange(n_seq, dtype=np.uint32)


def test_the_running_maximum_travels_far(sw):
    n = 1_000_000
    rng = np.random.default_rng(91)
    # one segment: a long first interval, 10^6 - 1 short ones inside it (query); on the target the same intervals sit apart
    s = np.concatenate([[0], rng.integers(1, 3_000_000_000, n - 1)])
    e = np.concatenate([[3_000_001_000], s[1:] + rng.integers(0, 1_000, n - 1)])
    ts = np.arange(n, dtype=np.int64) * 2_000
    te = ts + (e - s).clip(0, 1_500)
    status = np.ones(n, dtype=np.uint8)
    status[0] = 0                                     # KEPT loses the long one: two different running maxima in one pass
    cols, seq_genome = one_pair_columns(s, e, ts, te)
    perm = rng.permutation(n)
    cols = {c: v[perm] for c, v in cols.items()}
    a, k = check(sw, cols, seq_genome, status[perm], "long over short")
    assert int(a["q_union"][0]) == 3_000_001_000 and int(a["t_union"][0]) == int(a["t_bases"][0]) and int(k["q_union"][0]) < 3_000_001_000
    # one segment of 10^6 pairwise-overlapping intervals: each reaches a little further than the one before
    s = np.arange(n, dtype=np.int64) * 10
    cols, seq_genome = one_pair_columns(s, s + 15, s, s + 10)
    a, _ = check(sw, cols, seq_genome, (np.arange(n) % 2).astype(np.uint8), "chain")
    assert int(a["q_union"][0]) == 10 * n + 5 and int(a["t_union"][0]) == 10 * n
    # 10^6 segments of one record: nothing may be carried from one to the next
    cols, seq_genome = one_pair_columns(np.zeros(n, dtype=np.int64), np.full(n, 100), np.zeros(n, dtype=np.int64), np.full(n, 7),
                                        q_seq=np.arange(n))
    a, _ = check(sw, cols, seq_genome, None, "one-record segments")
    assert len(a) == n and (a["q_union"] == 100).all() and (a["t_union"] == 7).all()


def test_twenty_million_records_every_contig_its_own_genome(sw):
    """3000 one-sequence genomes (G * G beyond the dense limit: the hashed pair table, > 2^20 pairs), thousands of tiles per sort
    and of carry; device-resident columns, against the model."""
    from sweepga_amd.breadth import _call
    ctx = sw.default_context()
    rng = np.random.default_rng(81)
    n, n_seq = 20_000_000, 3_000
    q = rng.integers(0, n_seq, n).astype(np.uint32)
    t = np.where(rng.random(n) < 0.05, q, rng.integers(0, n_seq, n)).astype(np.uint32)
    qs = rng.integers(0, 1_000_000, n).astype(np.uint32)
    ts = rng.integers(0, 1_000_000, n).astype(np.uint32)
    cols = {"q_id": q, "t_id": t, "q_start": qs, "q_end": (qs + rng.integers(0, 200_000, n)).astype(np.uint32), "t_start": ts,
            "t_end": (ts + rng.integers(0, 200_000, n)).astype(np.uint32)}
    seq_genome = np.arange(n_seq, dtype=np.uint32)
    status = (rng.random(n) < 0.3).astype(np.uint8)
    hip = Hip()
    try:
        dcols = {name: hip.up(c) for name, c in cols.items()}
        d_genome, d_status = hip.up(seq_genome), hip.up(status)
        ctx.profile(True)
        ctx.profile_reset()
        a, k = _call(ctx, ctx.lib.swg_breadth_records_device, records_of(dcols, n_seq, n), d_genome, n_seq, d_status)
        table = ctx.profile_table()
        ctx.profile(False)
    finally:
        hip.free()
    for name in ("breadth_keys", "breadth_gather", "breadth_union", "breadth_collect"):
        assert table[name][0] >= 1, table
    print({name: round(v[1], 3) for name, v in table.items()})
    args = [cols[c] for c in COLS]
    want_all = bm.breadth(*args, seq_genome)
    assert len(want_all) > 1 << 20
    assert bm.same_pairs(a, want_all)
    assert bm.same_pairs(k, bm.breadth(*args, seq_genome, status != 0))
    assert (a["q_union"] < a["q_bases"]).any()


def test_a_memory_limit_too_small_is_a_clean_oom(sw):
    ctx = sw.Context(0)
    try:
        rng = np.random.default_rng(51)
        with sw.PafFile(text=gen_text(52, 200_000, n_genomes=4, chrs_per_genome=3, span=400_000)) as paf:
            cols, seq_genome = paf_columns(paf)
        status = (rng.random(len(cols["q_id"])) < 0.5).astype(np.uint8)
        from sweepga_amd.breadth import breadth_records
        ctx.set_memory_limit(1 << 20)       # the staged columns alone are 5 MB
        with pytest.raises(sw.SwgError) as e:
            breadth_records(ctx, cols, seq_genome, status)
        assert e.value.code == -4
        ctx.set_memory_limit(0)             # ... and the context works on
        check(sw, cols, seq_genome, status, "after the refusal", ctx=ctx)
        ctx.set_memory_limit(1 << 30)
        check(sw, cols, seq_genome, status, "under a limit that holds it", ctx=ctx)
        assert ctx.memory_info()[0] <= 1 << 30
    finally:
        ctx.close()


def test_ids_out_of_range_and_too_small_a_pair_array(sw):
    from sweepga_amd._lib import SwgBreadthCounts, SwgBreadthPair
    from sweepga_amd.breadth import BREADTH_PAIR_DTYPE, breadth_records
    ctx = sw.default_context()
    cols, seq_genome, status, want_all, _ = hand_case()
    bad = {c: v.copy() for c, v in cols.items()}
    bad["t_id"][3] = len(seq_genome)
    with pytest.raises(sw.SwgError) as e:
        breadth_records(ctx, bad, seq_genome, status)
    assert e.value.code == -1
    with pytest.raises(sw.SwgError) as e:
        breadth_records(ctx, cols, seq_genome, status, n_genome=2)      # genome id 2 >= n_genome
    assert e.value.code == -1
    # the capacity protocol: SWG_OK, n_pairs says how many there are, the array is left alone
    c = SwgBreadthCounts()
    pairs = np.frombuffer(bytearray(b"\xab" * 96), dtype=BREADTH_PAIR_DTYPE)
    before = pairs.copy()
    c.pair_capacity, c.pairs = 2, C.cast(pairs.ctypes.data, C.POINTER(SwgBreadthPair))
    rec = records_of(cols, len(seq_genome))
    ctx.check(ctx.lib.swg_breadth_records(ctx.handle, C.byref(rec), seq_genome.ctypes.data, 3, None, C.byref(c), None))
    assert int(c.n_pairs) == len(want_all) == 4 and pairs.tobytes() == before.tobytes()


# ---- the report ------------------------------------------------------------------------------------------------------------
def model_report(in_text, out_text, detailed):
    sets = []
    for label, text in (("all", in_text), ("kept", out_text)):
        cols, seq_genome, names, sizes = bm.parse_paf(text)
        pairs = bm.breadth(*[cols[c] for c in COLS], seq_genome) if len(cols["q_id"]) else np.zeros(0, dtype=bm.MODEL_DTYPE)
        # every set renders its own names and sizes: rows carry names, not ids
        sets.append(bm.render([(label, pairs, sizes)], names, detailed).decode().split("\n", 1))
    return (sets[0][0] + "\n" + sets[0][1] + sets[1][1]).encode()


def test_report_of_an_open_paf_equals_the_model_rendering(sw, tmp_path):
    text = gen_text(61, 12_000, n_genomes=4, chrs_per_genome=3, span=300_000)
    inp, outp = tmp_path / "in.paf", tmp_path / "out.paf"
    inp.write_text(text, newline="")
    with sw.PafFile(path=str(inp)) as paf:
        status, chain = run_filter(sw, paf, filter_cfgs(sw)["one_to_one"])
        paf.write(str(outp), status, chain)
        for detailed in (True, False):
            b = sw.Breadth.from_paf(sw.default_context(), paf, status, detailed=detailed)
            assert b.text == model_report(text, outp.read_bytes().decode(), detailed), detailed
        cols, seq_genome = paf_columns(paf)
        assert bm.same_pairs(b.all, bm.breadth(*[cols[c] for c in COLS], seq_genome))
        assert bm.same_pairs(b.kept, bm.breadth(*[cols[c] for c in COLS], seq_genome, status != 0))
        only_all = sw.Breadth.from_paf(sw.default_context(), paf)
        assert only_all.kept is None and only_all.text == b"".join(ln + b"\n" for ln in sw.Breadth.from_paf(
            sw.default_context(), paf, status).text.split(b"\n") if ln and not ln.startswith(b"kept"))


def test_a_coordinate_beyond_32_bits_is_refused(sw):
    ln = "\t".join(["a#1#x", str(2**33), str(2**32), str(2**32 + 50), "+", "b#1#y", "900", "10", "60", "50", "50", "60"]) + "\n"
    with sw.PafFile(text=ln) as paf:
        assert paf.is_rebased
        with pytest.raises(sw.SwgError) as e:
            sw.Breadth.from_paf(sw.default_context(), paf)
        assert e.value.code == -6 and "2^32" in str(e.value)


def test_cli_breadth(sw, tmp_path):
    from sweepga_amd import build
    text = gen_text(71, 15_000, n_genomes=4, chrs_per_genome=3, span=400_000)
    inp = tmp_path / "in.paf"
    inp.write_text(text, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-jump", "10k", "--scaffold-mass", "2k", "--quiet"]
    plain, out, rep, srep, srep0 = (tmp_path / x for x in ("plain.paf", "out.paf", "rep.tsv", "stats.txt", "stats0.txt"))
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), "--stats", str(srep0), *flags], capture_output=True)
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--breadth", str(rep), "--breadth-detailed", "--stats", str(srep), *flags],
                       capture_output=True)
    assert r0.returncode == r.returncode == 0, r.stderr
    assert out.read_bytes() == plain.read_bytes() and out.stat().st_size > 0 and r.stdout == r0.stdout == b""
    assert srep.read_bytes().replace(str(out).encode(), b"OUT") == srep0.read_bytes().replace(str(plain).encode(), b"OUT")   # --stats beside it
    assert rep.read_bytes() == model_report(text, out.read_bytes().decode(), True)
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--breadth", str(rep), *flags], capture_output=True)
    assert r.returncode == 0 and rep.read_bytes() == model_report(text, out.read_bytes().decode(), False) and out.read_bytes() == plain.read_bytes()
    # --breadth - : the report on standard error, the PAF alone on standard output
    r1 = subprocess.run([build.CLI, str(inp), *flags], capture_output=True)
    r2 = subprocess.run([build.CLI, str(inp), "--breadth", "-", "--breadth-detailed", *flags], capture_output=True)
    assert r1.returncode == r2.returncode == 0 and r2.stdout == r1.stdout == plain.read_bytes()
    assert r2.stderr == model_report(text, r1.stdout.decode(), True)
    # --no-filter: every line to standard output, the device is opened, kept = all
    r = subprocess.run([build.CLI, str(inp), "--no-filter", "--breadth", str(rep), "--breadth-detailed"], capture_output=True)
    assert r.returncode == 0 and r.stdout == text.encode() and rep.read_bytes() == model_report(text, text, True)
    # --sparsify tree: all = the whole input, kept = what is written
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--sparsify", "tree:1", "--breadth", str(rep), "--breadth-detailed", *flags],
                       capture_output=True)
    assert r.returncode == 0, r.stderr
    assert out.stat().st_size > 0 and rep.read_bytes() == model_report(text, out.read_bytes().decode(), True)


def test_smallest_shapes_on_a_fresh_context(sw):
    """The seams around the kernels at the smallest shapes -- one record; three records of one sequence pair in one chain -- on a
    context of its own: its first call sizes the arena from the input, the later ones find it sized.  Each shape twice, host seam
    against device seam byte for byte and both against the model."""
    a = np.array([(0, 1, 10, 110, 20, 125), (0, 1, 200, 300, 210, 310), (0, 1, 400, 450, 420, 470)], dtype=np.uint32)
    seq_genome = np.array([0, 1], dtype=np.uint32)
    ctx = sw.Context(0)
    try:
        for n in (1, 3, 1, 3):
            cols = {c: a[:n, j].copy() for j, c in enumerate(COLS)}
            for status in (None, np.ones(n, dtype=np.uint8)):   # (None: the optional column stays NULL on its way to the device)
                got, _ = check(sw, cols, seq_genome, status, f"n = {n}", ctx=ctx)
                assert len(got) == 1 and int(got["q_union"][0]) == int((a[:n, 3] - a[:n, 2]).sum())
    finally:
        ctx.close()
