"""Gaps on the device (sweepga_amd/csrc/swg_gaps.hip) against tests/gaps_model.py: the two record seams under synthetic status
and chain columns, inputs that make the predecessor travel across tiles, ties, coordinates at 2^32 - 1, sparse numbering, both
genome-pair tables, the request's variants and errors, a real filter's status and chain, and the texts of swg_paf_gaps / --gaps
byte for byte against the model's formatter.  Every comparison is exact: integers and bytes.  The tile of the sorted order is
1,024 records."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import gaps_model as gm
from tests.test_gaps_cpu import columns, hand_case
from tests.test_gpu_alnstats import gen_text, records_of
from tests.test_gpu_blocks import SEED_WITH_RESCUES, filter_with_stats, flag_sets, synthetic
from tests.test_gpu_wide import Hip

pytestmark = pytest.mark.gpu
S, R = 1, 2
TOP = 2**32 - 1


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


def prepared(cols, status, chain, genome):
    cols = {k: np.ascontiguousarray(cols[k], dtype=np.uint8 if k == "strand" else np.uint32) for k in gm.COLUMNS}
    return cols, np.ascontiguousarray(status, dtype=np.uint8), np.ascontiguousarray(chain, dtype=np.uint32), np.ascontiguousarray(genome, dtype=np.uint32)


def both_seams(sw, cols, status, chain, genome, min_size, n_genome=None, ctx=None, want=3):
    """The result of the host seam, after checking that the device seam gives the same bytes."""
    from sweepga_amd.gaps import _call, gaps_records
    ctx = ctx or sw.default_context()
    cols, status, chain, genome = prepared(cols, status, chain, genome)
    if n_genome is None:
        n_genome = int(genome.max()) + 1
    host = gaps_records(ctx, cols, status, chain, genome, min_size=min_size, n_genome=n_genome, want=want)
    hip = Hip()
    try:
        rec = records_of({k: hip.up(v) for k, v in cols.items()}, len(genome), len(status))
        dev = _call(ctx, ctx.lib.swg_gaps_records_device, rec, hip.up(status), hip.up(chain), hip.up(genome), n_genome, min_size, want)
    finally:
        hip.free()
    for a, b in ((host.rows, dev.rows), (host.pairs, dev.pairs), (host.spectrum, dev.spectrum)):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()
    return host


def check(sw, cols, status, chain, genome, min_sizes=(0, 50), what="", **kw):
    out = None
    for min_size in min_sizes:
        got = both_seams(sw, cols, status, chain, genome, min_size, **kw)
        want_rows = gm.gaps(cols, status, chain, min_size)
        assert gm.rows(got.rows) == gm.rows(want_rows), (what, min_size)
        assert (got.rows["reserved"] == 0).all(), what
        pairs, spectrum = gm.summary(cols, status, chain, genome, min_size)
        assert gm.pairs(got.pairs) == pairs, (what, min_size)
        assert got.spectrum.tolist() == spectrum, (what, min_size)
        out = out or (got, want_rows)
    return out   # (of the first min_size)


def genome_of(n_seq, per_genome=4):
    return (np.arange(n_seq) // per_genome).astype(np.uint32)


# ---- 1. the record seams against the model -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["pansn_6000", "many_small_chains", "one_chain", "no_chain"])
def test_record_seams_against_the_model(sw, shape):
    rng = np.random.default_rng(len(shape))
    if shape == "pansn_6000":            # 5 x 4 sequences, 300 chains
        cols, status, chain = synthetic(rng, 6_000, 300)
    elif shape == "many_small_chains":   # 2,000 chains of about 4 records: a tile holds more chains than any staging
        cols, status, chain = synthetic(rng, 8_192, 2_000)
    elif shape == "one_chain":
        cols, status, chain = synthetic(rng, 3_000, 1)
    else:
        cols, status, chain = synthetic(rng, 3_000, 40)
        chain[rng.random(len(chain)) < 0.5] = 0
        status[chain != 0] = R           # a number on a rescued record makes no chain that takes part
    got, want = check(sw, cols, status, chain, genome_of(20), what=shape)
    if shape == "no_chain":
        assert len(got.rows) == 0 and len(got.pairs) == 0 and not got.spectrum.any()
    else:
        kinds = set(got.rows["kind"].tolist())
        assert {gm.INS, gm.DEL} <= kinds and (gm.INV in kinds or shape == "one_chain") and int(got.pairs["links"].sum()) > 0


def test_hand_case(sw):
    cols, status, chain, genome, want = hand_case()
    got, _ = check(sw, cols, status, chain, genome, min_sizes=(0, 50, 100, 550, 551), what="hand")
    assert gm.rows(got.rows) == [w[:9] for w in want]


# ---- 2. the predecessor across tile seams ----------------------------------------------------------------------------------------
def test_one_chain_of_3000_core_records(sw):
    rng = np.random.default_rng(5)
    n = 3_000
    qs = np.sort(rng.integers(0, 3_000_000, n))
    ts = qs + rng.integers(-300, 300, n) + 1_000
    rec = [(0, 1, qs[i], qs[i] + 500, ts[i], ts[i] + 500, 0) for i in range(n)]
    order = rng.permutation(n)
    cols = columns([rec[i] for i in order])
    got, want = check(sw, cols, np.full(n, S, dtype=np.uint8), np.full(n, 1, dtype=np.uint32), genome_of(2, 1), what="3000 core")
    assert len(got.rows) == n - 1 and int(got.pairs["links"][0]) == n - 1     # a link at every position, the tile seams included


@pytest.mark.parametrize("second_chain", [False, True])
def test_the_carry_crosses_two_tiles_without_a_core_record(sw, second_chain):
    """core, 2,500 inverted, core: positions 0 and 2,501 of the sorted order, the tiles 1,024 .. 2,047 hold no core record.  With a
    second chain behind it: its first core record (behind five inverted ones of its own) must find no predecessor."""
    rec = [(0, 1, 0, 100, 0, 100, 0)]
    rec += [(0, 1, 200 + 10 * i, 205 + 10 * i, 50_000 - 10 * i, 50_005 - 10 * i, 1) for i in range(2_500)]
    rec += [(0, 1, 40_000, 40_100, 30_000, 30_100, 0)]
    chain = [1] * len(rec)
    if second_chain:
        rec += [(2, 3, 10 * i, 10 * i + 5, 900 - 10 * i, 905 - 10 * i, 1) for i in range(5)]
        rec += [(2, 3, 100, 200, 100, 200, 0), (2, 3, 300, 400, 250, 350, 0)]
        chain += [2] * 7
    rng = np.random.default_rng(8)
    order = rng.permutation(len(rec))
    cols = columns([rec[i] for i in order])
    chain = np.asarray(chain, dtype=np.uint32)[order]
    got, want = check(sw, cols, np.full(len(rec), S, dtype=np.uint8), chain, genome_of(4, 1), what=second_chain)
    where = {int(old): new for new, old in enumerate(order)}
    links = got.rows[got.rows["kind"] != gm.INV]
    first = links[0]
    assert (int(first["chain"]), int(first["left"]), int(first["right"])) == (1, where[0], where[2_501])
    assert (int(first["q_lo"]), int(first["q_hi"]), int(first["t_lo"]), int(first["t_hi"])) == (100, 40_000, 100, 30_000)
    assert int((got.rows["kind"] == gm.INV).sum()) == 2_500 + (5 if second_chain else 0)
    if second_chain:
        assert len(links) == 2 and (int(links[1]["chain"]), int(links[1]["left"]), int(links[1]["right"])) == (2, where[2_507], where[2_508])
    else:
        assert len(links) == 1


# ---- 3. ties ---------------------------------------------------------------------------------------------------------------------
def tie_preserving(rng, classes):
    """A random permutation under which records of one class keep their relative order.  perm[new] = old."""
    n = len(classes)
    where = rng.permutation(n)
    for c in np.unique(classes):
        idx = np.flatnonzero(classes == c)
        where[idx] = np.sort(where[idx])
    return np.argsort(where)


def test_ties_in_q_start_are_broken_by_index(sw):
    rng = np.random.default_rng(21)
    n = 2_000
    qs = rng.choice(np.array([100, 5_000, 5_001, 90_000]), n)
    rec = [(0, 1, qs[i], qs[i] + rng.integers(0, 3_000), rng.integers(0, 100_000), 100_000 + rng.integers(0, 3_000), 0) for i in range(n)]
    cols = columns(rec)
    status, chain, genome = np.full(n, S, dtype=np.uint8), np.full(n, 1, dtype=np.uint32), genome_of(2, 1)
    got, want = check(sw, cols, status, chain, genome, what="ties")
    assert len(got.rows) == n - 1
    # a permutation that keeps the order inside every tie: the same rows, record numbers mapped
    perm = tie_preserving(rng, qs)
    where = np.argsort(perm)
    moved, _ = check(sw, {k: v[perm] for k, v in cols.items()}, status, chain, genome, what="ties, permuted")
    mapped = got.rows.copy()
    mapped["left"], mapped["right"] = where[got.rows["left"]], where[got.rows["right"]]
    assert moved.rows.tobytes() == mapped.tobytes()
    assert moved.pairs.tobytes() == got.pairs.tobytes() and moved.spectrum.tobytes() == got.spectrum.tobytes()
    # any permutation: the index breaks the ties anew (check() holds it to the model)
    perm = rng.permutation(n)
    check(sw, {k: v[perm] for k, v in cols.items()}, status, chain, genome, what="ties, shuffled")


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------------
def test_coordinates_at_the_top_and_a_sparse_numbering(sw):
    rec = [
        # chain 1, '+': dq = +TOP and dt = -TOP (size 2 TOP, beyond 2^32), then dq = -TOP and dt = +TOP
        (0, 1, 0, 0, 0, TOP, 0),            # r0
        (0, 1, TOP, TOP, 0, 0, 0),          # r1: a = r0, dq = TOP - 0, dt = 0 - TOP
        (0, 1, TOP, TOP, TOP, TOP, 0),      # r2: a = r1 (tie, by index), dq = 0, dt = TOP - 0 = TOP
        # chain 7, '-': dq = -TOP, dt = t_start[a] - t_end[b] = TOP - 0 and then 0 - TOP
        (1, 2, 0, TOP, TOP, TOP, 1),        # r3
        (1, 2, 0, TOP, 0, 0, 1),            # r4: a = r3, dq = 0 - TOP, dt = TOP - 0
        (1, 2, TOP, TOP, 0, TOP, 1),        # r5: a = r4, dq = 0, dt = 0 - TOP
        # chain 2^20, '+': one inversion of TOP bases and one of none
        (2, 0, 5, 10, 5, 10, 0), (2, 0, 0, TOP, 0, TOP, 1), (2, 0, 7, 7, 9, 9, 1),
    ]
    status = np.full(len(rec), S, dtype=np.uint8)
    chain = np.array([1, 1, 1, 7, 7, 7, 1 << 20, 1 << 20, 1 << 20], dtype=np.uint32)
    cols = columns(rec)
    got, want = check(sw, cols, status, chain, genome_of(3, 1), min_sizes=(0, 50, TOP), what="edges")     # chain numbers {1, 7, 2^20} only
    assert [(e["dq"], e["dt"], e["size"]) for e in want] == [(TOP, -TOP, 2 * TOP), (0, TOP, -TOP), (-TOP, TOP, -2 * TOP), (0, -TOP, TOP),
                                                             (0, 0, TOP), (0, 0, 0)]
    assert got.rows["chain"].tolist() == [1, 1, 7, 7, 1 << 20, 1 << 20]
    assert got.rows["flags"].tolist() == [2, 0, 1, 2, 0, 0] and got.rows["kind"].tolist() == [gm.INS, gm.DEL, gm.DEL, gm.INS, gm.INV, gm.INV]
    assert ((got.rows["q_hi"] - got.rows["q_lo"])[:4].tolist(), (got.rows["t_hi"] - got.rows["t_lo"])[:4].tolist()) == ([TOP, 0, TOP, 0], [TOP] * 4)
    top = both_seams(sw, cols, status, chain, genome_of(3, 1), TOP)
    assert top.spectrum[0].tolist() == [0] * 32 + [2] and top.spectrum[1].tolist() == [0] * 32 + [2] and len(top.rows) == 5


def test_a_permutation_that_interleaves_the_chains(sw):
    rng = np.random.default_rng(3)
    cols, status, chain = synthetic(rng, 6_000, 300)
    a, _ = check(sw, cols, status, chain, genome_of(20), what="pair-major")
    perm = tie_preserving(rng, chain.astype(np.int64) << 32 | cols["q_start"])     # chains interleaved record by record
    where = np.argsort(perm)
    b, _ = check(sw, {k: v[perm] for k, v in cols.items()}, status[perm], chain[perm], genome_of(20), what="interleaved")
    mapped = a.rows.copy()
    mapped["left"], mapped["right"] = where[a.rows["left"]], where[a.rows["right"]]
    assert b.rows.tobytes() == mapped.tobytes() and b.pairs.tobytes() == a.pairs.tobytes() and b.spectrum.tobytes() == a.spectrum.tobytes()


@pytest.mark.parametrize("table", ["dense", "hashed"])
def test_both_genome_pair_tables(sw, table):
    rng = np.random.default_rng(13)
    n_seq = 40 if table == "dense" else 1_100     # one genome per sequence: 1,100^2 > 2^20 entries, the table is hashed
    cols, status, chain = synthetic(rng, 6_000, 1_500, n_seq=n_seq)
    got, _ = check(sw, cols, status, chain, genome_of(n_seq, 1), what=table)
    assert len(got.pairs) > 200 and (np.diff(got.pairs["q_genome"].astype(np.int64) * n_seq + got.pairs["t_genome"]) > 0).all()


# ---- 5. the request ------------------------------------------------------------------------------------------------------------------
def test_want_bits_and_min_sizes(sw):
    rng = np.random.default_rng(31)
    cols, status, chain = synthetic(rng, 6_000, 300)
    genome = genome_of(20)
    both = both_seams(sw, cols, status, chain, genome, 50)
    rows_only = both_seams(sw, cols, status, chain, genome, 50, want=1)
    summary_only = both_seams(sw, cols, status, chain, genome, 50, want=2)
    assert rows_only.pairs is None and rows_only.spectrum is None and rows_only.rows.tobytes() == both.rows.tobytes()
    assert summary_only.rows is None and summary_only.pairs.tobytes() == both.pairs.tobytes() and summary_only.spectrum.tobytes() == both.spectrum.tobytes()
    every, _ = check(sw, cols, status, chain, genome, min_sizes=(0,), what="0")
    none, _ = check(sw, cols, status, chain, genome, min_sizes=(TOP,), what="2^32 - 1")
    assert len(none.rows) == 0 and len(none.pairs) == len(every.pairs) and none.pairs["links"].tolist() == every.pairs["links"].tolist()
    assert not none.spectrum.any() and int(none.pairs["n_inv"].sum()) == 0
    assert 0 < len(both.rows) < len(every.rows)


def request(cols, status, chain, genome, want=3, min_size=0):
    from sweepga_amd._lib import SwgGapsRequest
    req = SwgGapsRequest()
    req.want, req.min_size = want, min_size
    rec = records_of(cols, len(genome))
    return rec, req


def test_input_errors_and_the_capacity_protocol(sw):
    from sweepga_amd._lib import SwgGapPair, SwgGapRow
    from sweepga_amd.gaps import PAIR_DTYPE, ROW_DTYPE, gaps_records
    ctx = sw.default_context()
    cols, status, chain, genome, want = hand_case()
    two = {k: v.copy() for k, v in cols.items()}
    two["t_id"][9] = 1                      # chain 6 over (4, 0) and (4, 1)
    with pytest.raises(sw.SwgError) as e:
        gaps_records(ctx, two, status, chain, genome)
    assert e.value.code == -1 and "chain 6" in str(e.value)
    two = {k: v.copy() for k, v in cols.items()}
    two["q_id"][12] = 3                     # ... and where only a captured inversion differs
    with pytest.raises(sw.SwgError) as e:
        gaps_records(ctx, two, status, chain, genome)
    assert e.value.code == -1 and "chain 8" in str(e.value)
    with pytest.raises(sw.SwgError) as e:
        gaps_records(ctx, cols, status, chain, genome[:5])              # sequence id 5 >= n_seq
    assert e.value.code == -1
    with pytest.raises(sw.SwgError) as e:
        gaps_records(ctx, cols, status, chain, genome, n_genome=2)      # genome id 2 >= n_genome
    assert e.value.code == -1
    top = chain.copy()
    top[chain == 9] = TOP
    with pytest.raises(sw.SwgError) as e:
        gaps_records(ctx, cols, status, top, genome)                    # a chain number of 2^32 - 1
    assert e.value.code == -5
    rec, req = request(cols, status, chain, genome)
    args = (status.ctypes.data, chain.ctypes.data, genome.ctypes.data, 3)
    for field, value in (("reserved", 1), ("want", 0), ("want", 4)):
        setattr(req, field, value)
        assert ctx.lib.swg_gaps_records(ctx.handle, C.byref(rec), *args, C.byref(req)) == -1, field
        setattr(req, field, 3 if field == "want" else 0)
    rec.n = 2**31                                                       # refused before a column is looked at
    assert ctx.lib.swg_gaps_records(ctx.handle, C.byref(rec), *args, C.byref(req)) == -5
    rec.n = len(status)
    rec.strand = None
    assert ctx.lib.swg_gaps_records(ctx.handle, C.byref(rec), *args, C.byref(req)) == -1
    # the capacity protocol: SWG_OK, the counts say how many there are, the arrays are left alone
    rec, req = request(cols, status, chain, genome)
    rows = np.frombuffer(bytearray(b"\xab" * 32 * 10), dtype=ROW_DTYPE)
    pairs = np.frombuffer(bytearray(b"\xcd" * 64 * 3), dtype=PAIR_DTYPE)
    spectrum = np.full(66, 7, dtype=np.uint64)
    before = rows.copy(), pairs.copy()
    req.capacity, req.rows = 10, C.cast(rows.ctypes.data, C.POINTER(SwgGapRow))
    req.pair_capacity, req.pairs = 3, C.cast(pairs.ctypes.data, C.POINTER(SwgGapPair))
    req.spectrum = C.cast(spectrum.ctypes.data, C.POINTER(C.c_uint64))
    ctx.check(ctx.lib.swg_gaps_records(ctx.handle, C.byref(rec), *args, C.byref(req)))
    assert (int(req.n_rows), int(req.n_pairs)) == (11, 4) and rows.tobytes() == before[0].tobytes() and pairs.tobytes() == before[1].tobytes()
    assert int(spectrum.sum()) == 8          # the spectrum has no capacity: fully written
    req.pair_capacity = 4                    # one array fits, the other does not
    pairs4 = np.zeros(4, dtype=PAIR_DTYPE)
    req.pairs = C.cast(pairs4.ctypes.data, C.POINTER(SwgGapPair))
    ctx.check(ctx.lib.swg_gaps_records(ctx.handle, C.byref(rec), *args, C.byref(req)))
    assert rows.tobytes() == before[0].tobytes() and gm.pairs(pairs4) == gm.summary(cols, status, chain, genome, 0)[0]
    got, _ = check(sw, cols, status, chain, genome, what="after the refusals")
    assert gm.rows(got.rows) == [w[:9] for w in want]


def test_a_memory_limit_too_small_is_a_clean_oom(sw):
    from sweepga_amd.gaps import gaps_records
    ctx = sw.Context(0)
    try:
        cols, status, chain = synthetic(np.random.default_rng(51), 200_000, 5_000)
        genome = genome_of(20)
        ctx.set_memory_limit(1 << 20)       # the staged columns alone are 6 MB
        with pytest.raises(sw.SwgError) as e:
            gaps_records(ctx, cols, status, chain, genome)
        assert e.value.code == -4
        ctx.set_memory_limit(0)             # ... and the context works on
        want = both_seams(sw, cols, status, chain, genome, 50)
        got = both_seams(sw, cols, status, chain, genome, 50, ctx=ctx)
        ctx.set_memory_limit(1 << 30)
        limited = both_seams(sw, cols, status, chain, genome, 50, ctx=ctx)
        for r in (got, limited):
            assert r.rows.tobytes() == want.rows.tobytes() and r.pairs.tobytes() == want.pairs.tobytes() and len(r.rows) > 10_000
        assert ctx.memory_info()[0] <= 1 << 30
    finally:
        ctx.close()


# ---- 6. a real filter ----------------------------------------------------------------------------------------------------------------
def genome_names(sw, paf):
    names, genome = paf.names, paf.seq_genome_last
    out = [None] * int(paf.records.n_genome_last)
    for s, name in enumerate(names):
        out[int(genome[s])] = sw.SequenceIndex.prefix_last(name)
    return out


@pytest.mark.parametrize("flags", ["default", "one_to_one_rescue"])
def test_the_status_and_chain_of_a_real_filter(sw, flags):
    from sweepga_amd.blocks import blocks_records
    text = gen_text(SEED_WITH_RESCUES, 6_000, n_genomes=4, chrs_per_genome=3, span=400_000)
    with sw.PafFile(text=text) as paf:
        cols = {k: paf.column(k).copy() for k in gm.COLUMNS}
        n_seq = int(paf.records.n_seq)
        genome = paf.seq_genome_last[:n_seq].copy()
        status, chain, stats = filter_with_stats(sw, paf, flag_sets(sw)[flags])
        got, want = check(sw, cols, status, chain, genome, n_genome=int(paf.records.n_genome_last), what=flags)
        blocks = blocks_records(sw.default_context(), paf.records, status, chain)
        links = got.rows[got.rows["kind"] != gm.INV]
        per_chain = np.bincount(links["chain"], minlength=int(blocks["chain"].max()) + 1)
        assert per_chain[blocks["chain"]].tolist() == (blocks["n_core"] - 1).tolist() and int(per_chain.sum()) == len(links) > 0
        inv = np.bincount(got.rows["chain"][got.rows["kind"] == gm.INV], minlength=int(blocks["chain"].max()) + 1)
        assert inv[blocks["chain"]].tolist() == blocks["n_inverted"].tolist()
        if flags == "one_to_one_rescue":
            assert int((status == R).sum()) >= 1     # (not vacuous: the seed was chosen for this)
        # the texts: one call for both, the model's formatter over the same status and chain
        names = list(paf.names)
        for min_size in (0, 50):
            g = sw.Gaps.from_paf(sw.default_context(), paf, status, chain, min_size=min_size)
            assert g.rows == gm.rows_text(gm.gaps(cols, status, chain, min_size), cols, names)
            pairs, spectrum = gm.summary(cols, status, chain, genome, min_size)
            assert g.summary == gm.summary_text(pairs, spectrum, genome_names(sw, paf))
            assert g.rows.count(b"\n") > 10 and b"#spectrum\t" in g.summary
            if min_size == 0:
                assert g.table.rows.tobytes() == got.rows.tobytes() and g.table.pairs.tobytes() == got.pairs.tobytes()


# ---- 7. the command line ----------------------------------------------------------------------------------------------------------------
def test_cli_gaps(sw, tmp_path):
    from sweepga_amd import build
    text = gen_text(SEED_WITH_RESCUES, 6_000, n_genomes=4, chrs_per_genome=3, span=400_000)
    inp = tmp_path / "in.paf"
    inp.write_text(text, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-filter", "1:1", "--scaffold-dist", "20k", "--quiet"]
    plain, out, rows, summ = (tmp_path / x for x in ("plain.paf", "out.paf", "g.tsv", "s.tsv"))
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), *flags], capture_output=True)
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--gaps", str(rows), "--gaps-summary", str(summ), "--gaps-min-size", "1k", *flags],
                       capture_output=True)
    assert r0.returncode == r.returncode == 0, r.stderr
    assert out.read_bytes() == plain.read_bytes() and out.stat().st_size > 0 and r.stdout == r0.stdout == b""
    with sw.PafFile(text=text) as paf:
        status, chain, _ = filter_with_stats(sw, paf, flag_sets(sw)["one_to_one_rescue"])
        g = sw.Gaps.from_paf(sw.default_context(), paf, status, chain, min_size=1_000, table=False)
        cols = {k: paf.column(k).copy() for k in gm.COLUMNS}
        genome = paf.seq_genome_last[:int(paf.records.n_seq)].copy()
        want_rows = gm.rows_text(gm.gaps(cols, status, chain, 1_000), cols, list(paf.names))
        want_summary = gm.summary_text(*gm.summary(cols, status, chain, genome, 1_000), genome_names(sw, paf))
        dflt = sw.Gaps.from_paf(sw.default_context(), paf, status, chain, table=False)
    assert rows.read_bytes() == g.rows == want_rows and summ.read_bytes() == g.summary == want_summary and want_rows.count(b"\n") > 3
    # --gaps - : the rows on standard error, the PAF alone on standard output; the default size cut is 50
    r2 = subprocess.run([build.CLI, str(inp), "--gaps", "-", *flags], capture_output=True)
    assert r2.returncode == 0 and r2.stdout == plain.read_bytes() and r2.stderr == dflt.rows and len(dflt.rows) > len(want_rows)
    # no chains: --scaffold-jump 0 writes the header lines
    rows.write_bytes(b"stale")
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--scaffold-jump", "0", "--gaps", str(rows), "--gaps-summary", str(summ), "--quiet"],
                       capture_output=True)
    assert r.returncode == 0 and out.stat().st_size > 0 and rows.read_bytes() == gm.ROWS_HEADER.encode() and summ.read_bytes() == gm.SUMMARY_HEADER.encode()


def test_smallest_shapes_on_a_fresh_context(sw):
    """The seams around the kernels at the smallest shapes -- one record; three records of one sequence pair in one chain -- on a
    context of its own: its first call sizes the arena from the input, the later ones find it sized.  Each shape twice, host seam
    against device seam byte for byte and both against the model."""
    rec = [(0, 1, 10, 110, 20, 125, 0), (0, 1, 200, 300, 210, 310, 0), (0, 1, 400, 450, 520, 570, 0)]
    genome = np.array([0, 1], dtype=np.uint32)
    ctx = sw.Context(0)
    try:
        for n in (1, 3, 1, 3):
            got, _ = check(sw, columns(rec[:n]), np.full(n, S, dtype=np.uint8), np.ones(n, dtype=np.uint32), genome, min_sizes=(0,), what=f"n = {n}", ctx=ctx)
            assert len(got.rows) == n - 1 and int(got.pairs["links"].sum()) == n - 1
    finally:
        ctx.close()
