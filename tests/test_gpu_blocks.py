"""Blocks on the device (sweepga_amd/csrc/swg_blocks.hip) against tests/blocks_model.py: the two record seams under synthetic
status and chain columns, inputs that make the running maximum travel across tiles, order independence, edges, the input errors,
a real filter's status and chain, and the text of swg_paf_blocks / --blocks byte for byte against the model's parser of the
output PAF.  Every comparison is exact: integers and bytes.  The tile of the cover passes is 1,024 sorted records."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import blocks_model as bm
from tests.test_blocks_cpu import columns, hand_case
from tests.test_gpu_alnstats import gen_text, records_of
from tests.test_gpu_wide import Hip

pytestmark = pytest.mark.gpu
S, R = bm.SCAFFOLD, bm.RESCUED
SEED_WITH_RESCUES = 101   # chosen with the oracle on the CPU: under the second flag set below it rescues hundreds of records


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


def both_seams(sw, cols, status, chain, n_seq=None, ctx=None):
    """The table from the host seam, after checking that the device seam gives the same."""
    from sweepga_amd.blocks import _call, blocks_records
    ctx = ctx or sw.default_context()
    cols = {k: np.ascontiguousarray(cols[k], dtype=np.uint8 if k == "strand" else np.uint32) for k in bm.COLUMNS}
    status, chain = np.ascontiguousarray(status, dtype=np.uint8), np.ascontiguousarray(chain, dtype=np.uint32)
    if n_seq is None:
        n_seq = int(max(cols["q_id"].max(), cols["t_id"].max())) + 1
    host = blocks_records(ctx, cols, status, chain, n_seq=n_seq)
    hip = Hip()
    try:
        rec = records_of({k: hip.up(v) for k, v in cols.items()}, n_seq, len(status))
        dev = _call(ctx, ctx.lib.swg_blocks_records_device, rec, hip.up(status), hip.up(chain))
    finally:
        hip.free()
    assert dev.tobytes() == host.tobytes()
    return host


def check(sw, cols, status, chain, what="", **kw):
    got = both_seams(sw, cols, status, chain, **kw)
    assert bm.rows(got) == bm.rows(bm.blocks(cols, status, chain)), what
    assert (got["reserved"] == 0).all() and (np.diff(got["chain"].astype(np.int64)) > 0).all(), what
    return got


def synthetic(rng, n, n_chains, n_seq=20, chain_numbers=None, span=1_000_000, max_len=5_000):
    """n records in pair-major order with status and chain as a filter could have left them: every chain on one sequence pair and
    one strand, SCAFFOLD members (on '+' chains some of them captured '-' ones), RESCUED ones, and records without a chain."""
    pair_of_chain = np.sort(rng.integers(0, n_seq * n_seq, n_chains))
    strand_of_chain = (rng.random(n_chains) < 0.3).astype(np.uint8)
    ch = np.sort(rng.integers(0, n_chains, n))
    ch[:n_chains] = np.arange(n_chains)           # every chain has a record ...
    ch = np.sort(ch)
    first = np.r_[True, np.diff(ch) != 0]         # ... and its first one is a core record
    u = rng.random(n)
    status = np.where(first | (u < 0.6), S, np.where(u < 0.8, R, 0)).astype(np.uint8)
    strand = strand_of_chain[ch].copy()
    flip = ~first & (rng.random(n) < 0.15)        # captured inversions on '+' chains, rescued records of either strand
    strand[flip & ((strand_of_chain[ch] == 0) | (status != S))] ^= 1
    numbers = np.arange(1, n_chains + 1) if chain_numbers is None else np.asarray(chain_numbers)
    chain = numbers[ch].astype(np.uint32)
    loose = ~first & (rng.random(n) < 0.1)        # kept or dropped records without a chain
    chain[loose] = 0
    status[loose] = rng.choice(np.array([0, 3], dtype=np.uint8), int(loose.sum()))
    qs, ts = rng.integers(0, span, n), rng.integers(0, span, n)
    ln = rng.integers(0, max_len, n)
    ln[rng.random(n) < 0.02] = 0
    block = np.maximum(ln, 1)
    cols = {"q_id": pair_of_chain[ch] // n_seq, "t_id": pair_of_chain[ch] % n_seq, "q_start": qs, "q_end": qs + ln, "t_start": ts,
            "t_end": ts + np.maximum(ln + rng.integers(-20, 20, n), 0), "matches": (block * rng.uniform(0.6, 1.0, n)).astype(np.int64),
            "block_len": block, "strand": strand}
    return {k: np.asarray(v) for k, v in cols.items()}, status, chain


# ---- 1. the record seams against the model -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["pansn_6000", "many_small_chains", "one_chain", "no_chain"])
def test_record_seams_against_the_model(sw, shape):
    rng = np.random.default_rng(len(shape))
    if shape == "pansn_6000":       # 5 x 4 sequences, some hundreds of chains
        cols, status, chain = synthetic(rng, 6_000, 300)
    elif shape == "many_small_chains":   # 2,000 chains of about 4 records: a tile holds more chains than any staging
        cols, status, chain = synthetic(rng, 8_192, 2_000)
    elif shape == "one_chain":
        cols, status, chain = synthetic(rng, 3_000, 1)
    else:
        cols, status, chain = synthetic(rng, 3_000, 40)
        chain[rng.random(len(chain)) < 0.5] = 0
        status[chain != 0] = 0           # a number on a dropped record is no chain
    got = check(sw, cols, status, chain, shape)
    want_blocks = {"pansn_6000": 300, "many_small_chains": 2_000, "one_chain": 1, "no_chain": 0}[shape]
    assert len(got) == want_blocks
    if want_blocks:
        assert got["n_inverted"].sum() > 0 or shape == "one_chain"
        assert got["n_rescued"].sum() > 0 and (got["q_cover"] <= got["q_bases"]).all() and (got["t_cover"] <= got["t_bases"]).all()


def test_hand_case(sw):
    cols, status, chain, want = hand_case()
    assert bm.rows(check(sw, cols, status, chain, "hand")) == want


# ---- 2. the carry across tiles --------------------------------------------------------------------------------------------------
def carry_case(long_last, second_chain):
    rng = np.random.default_rng(17)
    n = 5_000
    s = np.r_[0, np.sort(rng.integers(1, 999_000, n - 1))]
    e = np.r_[1_000_000, s[1:] + rng.integers(0, 500, n - 1)]
    rec = [(0, 1, s[i], e[i], 2 * s[i], 2 * s[i] + 1, 1, 1, 0) for i in range(n)]   # on the target: apart, one base each
    chain = [1] * n
    if second_chain:   # starts that fall between those of chain 1: sorted behind it, its cover must not inherit the long interval
        rec += [(2, 3, 100, 200, 100, 200, 1, 1, 0), (2, 3, 500_000, 500_010, 150, 250, 1, 1, 0), (2, 3, 900_000, 900_001, 0, 0, 1, 1, 0)]
        chain += [2, 2, 2]
    order = np.arange(len(rec))
    if long_last:
        order = np.r_[order[1:n], 0, order[n:]]
    cols = columns([rec[i] for i in order])
    return cols, np.full(len(rec), S, dtype=np.uint8), np.asarray(chain, dtype=np.uint32)[order]


@pytest.mark.parametrize("long_last,second_chain", [(False, False), (True, False), (False, True)])
def test_one_long_interval_over_five_tiles(sw, long_last, second_chain):
    cols, status, chain = carry_case(long_last, second_chain)
    got = check(sw, cols, status, chain, (long_last, second_chain))
    assert int(got["q_cover"][0]) == 1_000_000 and int(got["q_bases"][0]) > 1_000_000
    assert int(got["t_cover"][0]) == len(set(cols["t_start"][chain == 1].tolist()))
    if second_chain:
        assert (int(got["q_cover"][1]), int(got["t_cover"][1])) == (111, 150)


# ---- 3. order independence -----------------------------------------------------------------------------------------------------
def test_a_random_permutation_changes_only_first_record(sw):
    rng = np.random.default_rng(3)
    cols, status, chain = synthetic(rng, 6_000, 300)
    a = check(sw, cols, status, chain, "pair-major")
    perm = rng.permutation(len(status))          # chains interleaved record by record
    b = check(sw, {k: v[perm] for k, v in cols.items()}, status[perm], chain[perm], "shuffled")
    for f in a.dtype.names:
        assert f == "first_record" or np.array_equal(a[f], b[f]), f
    where = np.argsort(perm)                     # record i of the first order is record where[i] of the second
    for x, y in zip(a, b):                       # first_record maps through the permutation: the smallest NEW index of a core record
        core = np.flatnonzero((chain == x["chain"]) & (status == S) & (cols["strand"] == x["strand"]))
        assert int(x["first_record"]) == core.min() and int(y["first_record"]) == where[core].min()


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------------
def test_edges(sw):
    top = 2**32 - 1
    rec = [
        # chain 1: coordinates at 2^32 - 1
        (0, 1, top - 10, top, top - 5, top, 10, 10, 0), (0, 1, top, top, top, top, 0, 0, 0), (0, 1, top - 20, top - 10, 0, top, 7, top, 0),
        # chain 7: a '+' block whose only '-' records are a captured one and a rescued one
        (1, 2, 100, 200, 100, 200, 90, 100, 0), (1, 2, 120, 140, 150, 170, 19, 20, 1), (1, 2, 300, 350, 400, 450, 45, 50, 1),
        # chain 2^20: a '-' block
        (2, 0, 10, 20, 10, 20, 9, 10, 1), (2, 0, 15, 40, 30, 60, 20, 30, 1),
    ]
    status = np.array([S, S, S, S, S, R, S, S], dtype=np.uint8)
    chain = np.array([1, 1, 1, 7, 7, 7, 1 << 20, 1 << 20], dtype=np.uint32)
    got = check(sw, columns(rec), status, chain, "edges")     # chain numbers {1, 7, 2^20} only: a sparse table
    assert got["chain"].tolist() == [1, 7, 1 << 20] and got["strand"].tolist() == [0, 0, 1]
    assert (int(got["q_start"][0]), int(got["q_end"][0]), int(got["t_start"][0]), int(got["t_end"][0])) == (top - 20, top, 0, top)
    assert (int(got["q_cover"][0]), int(got["t_cover"][0]), int(got["t_bases"][0])) == (20, top, top + 5)
    assert (int(got["n_core"][1]), int(got["n_inverted"][1]), int(got["n_rescued"][1]), int(got["q_end"][1])) == (1, 1, 1, 200)
    assert (int(got["n_core"][2]), int(got["n_inverted"][2]), int(got["q_cover"][2]), int(got["t_cover"][2])) == (2, 0, 30, 40)


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------
def test_input_errors_and_the_capacity_protocol(sw):
    from sweepga_amd._lib import SwgBlock, SwgBlockTable
    from sweepga_amd.blocks import BLOCK_DTYPE, blocks_records
    ctx = sw.default_context()
    cols, status, chain, want = hand_case()
    two = {k: v.copy() for k, v in cols.items()}
    two["t_id"][2] = 2                      # chain 5 over (0, 1) and (0, 2)
    with pytest.raises(sw.SwgError) as e:
        blocks_records(ctx, two, status, chain, n_seq=4)
    assert e.value.code == -1 and "chain 5" in str(e.value)
    masked = status.copy()
    masked[[6, 8]] = R                      # chain 2 without a SCAFFOLD record
    with pytest.raises(sw.SwgError) as e:
        blocks_records(ctx, cols, masked, chain, n_seq=4)
    assert e.value.code == -1 and "chain 2" in str(e.value)
    with pytest.raises(sw.SwgError) as e:
        blocks_records(ctx, cols, status, chain, n_seq=3)    # sequence id 3 >= n_seq
    assert e.value.code == -1
    # the capacity protocol: SWG_OK, n_blocks says how many there are, the array is left alone
    t = SwgBlockTable()
    blocks = np.frombuffer(bytearray(b"\xab" * 208), dtype=BLOCK_DTYPE)
    before = blocks.copy()
    t.block_capacity, t.blocks = 2, C.cast(blocks.ctypes.data, C.POINTER(SwgBlock))
    rec = records_of(cols, 4)
    ctx.check(ctx.lib.swg_blocks_records(ctx.handle, C.byref(rec), status.ctypes.data, chain.ctypes.data, C.byref(t)))
    assert int(t.n_blocks) == len(want) == 3 and blocks.tobytes() == before.tobytes()
    assert bm.rows(check(sw, cols, status, chain, "after the refusals")) == want


def test_a_memory_limit_too_small_is_a_clean_oom(sw):
    from sweepga_amd.blocks import blocks_records
    ctx = sw.Context(0)
    try:
        cols, status, chain = synthetic(np.random.default_rng(51), 200_000, 5_000)
        ctx.set_memory_limit(1 << 20)       # the staged columns alone are 7 MB
        with pytest.raises(sw.SwgError) as e:
            blocks_records(ctx, cols, status, chain)
        assert e.value.code == -4
        ctx.set_memory_limit(0)             # ... and the context works on
        check(sw, cols, status, chain, "after the refusal", ctx=ctx)
        ctx.set_memory_limit(1 << 30)
        check(sw, cols, status, chain, "under a limit that holds it", ctx=ctx)
        assert ctx.memory_info()[0] <= 1 << 30
    finally:
        ctx.close()


# ---- 6. a real filter ----------------------------------------------------------------------------------------------------------------
def paf_columns(paf):
    return {k: paf.column(k).copy() for k in bm.COLUMNS}


def filter_with_stats(sw, paf, cfg, scaffolds_only=False):
    from sweepga_amd._lib import SwgStats
    ctx = sw.default_context()
    status, chain, stats = np.zeros(paf.n, dtype=np.uint8), np.zeros(paf.n, dtype=np.uint32), SwgStats()
    cc = cfg.to_c(False, scaffolds_only)
    ctx.check(ctx.lib.swg_filter(ctx.handle, C.byref(paf.records), C.byref(cc), status.ctypes.data, chain.ctypes.data, C.byref(stats)))
    return status, chain, stats


def flag_sets(sw):
    FM = sw.FilterMode
    return {"default": sw.FilterConfig(),
            # --num-mappings 1:1 --scaffold-filter 1:1 --scaffold-dist 20k
            "one_to_one_rescue": sw.FilterConfig(mapping_filter_mode=FM.OneToOne, mapping_max_per_query=1, mapping_max_per_target=1,
                                                 scaffold_filter_mode=FM.OneToOne, scaffold_max_per_query=1, scaffold_max_per_target=1,
                                                 scaffold_max_deviation=20_000)}


@pytest.mark.parametrize("flags", ["default", "one_to_one_rescue"])
def test_the_status_and_chain_of_a_real_filter(sw, flags):
    text = gen_text(SEED_WITH_RESCUES, 6_000, n_genomes=4, chrs_per_genome=3, span=400_000)
    with sw.PafFile(text=text) as paf:
        cols = paf_columns(paf)
        for scaffolds_only in (False, True):
            status, chain, stats = filter_with_stats(sw, paf, flag_sets(sw)[flags], scaffolds_only)
            got = check(sw, cols, status, chain, (flags, scaffolds_only), n_seq=int(paf.records.n_seq))
            assert len(got) == stats.n_chains_kept > 0
            assert int(got["n_core"].sum() + got["n_inverted"].sum() + got["n_rescued"].sum()) == int((chain != 0).sum())
            assert (got["q_cover"] <= got["q_bases"]).all() and (got["t_cover"] <= got["t_bases"]).all()
            for b in got:
                m = chain == b["chain"]
                assert int(b["q_cover"]) <= int(cols["q_end"][m].max()) - int(cols["q_start"][m].min())
            if scaffolds_only:
                assert got["n_inverted"].sum() == 0 and got["n_rescued"].sum() == 0
            elif flags == "one_to_one_rescue":
                assert got["n_rescued"].sum() >= 1 and int((status == R).sum()) >= 1    # (not vacuous: the seed was chosen for this)
            if not scaffolds_only:
                b = sw.Blocks.from_paf(sw.default_context(), paf, status, chain)
                assert b.table.tobytes() == got.tobytes() and b.text == bm.render(got, text.split("\n"))


# ---- 7. the command line ----------------------------------------------------------------------------------------------------------------
def test_cli_blocks(sw, tmp_path):
    from sweepga_amd import build
    text = gen_text(SEED_WITH_RESCUES, 6_000, n_genomes=4, chrs_per_genome=3, span=400_000)
    inp = tmp_path / "in.paf"
    inp.write_text(text, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-filter", "1:1", "--scaffold-dist", "20k", "--quiet"]
    plain, out, blk = (tmp_path / x for x in ("plain.paf", "out.paf", "b.paf"))
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), *flags], capture_output=True)
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--blocks", str(blk), *flags], capture_output=True)
    assert r0.returncode == r.returncode == 0, r.stderr
    assert out.read_bytes() == plain.read_bytes() and out.stat().st_size > 0 and r.stdout == r0.stdout == b""
    want = bm.render_from_output_paf(out.read_bytes().decode())      # from out.paf alone
    assert blk.read_bytes() == want and b"\tnr:i:0\t" in want and any(b"\tnr:i:0\t" not in ln for ln in want.splitlines())
    # --blocks - : the blocks on standard error, the PAF alone on standard output
    r1 = subprocess.run([build.CLI, str(inp), *flags], capture_output=True)
    r2 = subprocess.run([build.CLI, str(inp), "--blocks", "-", *flags], capture_output=True)
    assert r1.returncode == r2.returncode == 0 and r2.stdout == r1.stdout == plain.read_bytes() and r2.stderr == want
    # no chains: --no-filter (every line to standard output) and --scaffold-jump 0 write the file empty
    r = subprocess.run([build.CLI, str(inp), "--no-filter", "--blocks", str(blk)], capture_output=True)
    assert r.returncode == 0 and r.stdout == text.encode() and blk.read_bytes() == b""
    blk.write_bytes(b"stale")
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--scaffold-jump", "0", "--blocks", str(blk), "--quiet"], capture_output=True)
    assert r.returncode == 0 and out.stat().st_size > 0 and blk.read_bytes() == b""


def test_smallest_shapes_on_a_fresh_context(sw):
    """The seams around the kernels at the smallest shapes -- one record; three records of one sequence pair in one chain -- on a
    context of its own: its first call sizes the arena from the input, the later ones find it sized.  Each shape twice, host seam
    against device seam byte for byte and both against the model."""
    rec = [(0, 1, 10, 110, 20, 125, 90, 105, 0), (0, 1, 200, 300, 210, 310, 80, 100, 0), (0, 1, 400, 450, 420, 470, 50, 50, 0)]
    ctx = sw.Context(0)
    try:
        for n in (1, 3, 1, 3):
            got = check(sw, columns(rec[:n]), np.full(n, S, dtype=np.uint8), np.ones(n, dtype=np.uint32), f"n = {n}", ctx=ctx, n_seq=2)
            assert len(got) == 1 and int(got["n_core"][0]) == n
    finally:
        ctx.close()
