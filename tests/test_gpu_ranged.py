"""The ranged filter (csrc/swg_range.hip) at small sizes: a device-memory limit (Context.set_memory_limit) small enough that the
one-piece footprint does not fit makes swg_filter / swg_filter_device / the 64-bit entries cut the records into ranges of whole
genome pairs.  Status and chain numbers must equal the oracle, record for record, and the same call without a limit -- in
pair-major order (every range a slice of the caller's columns), by query genome and shuffled (ranges gathered)."""
import ctypes as C

import numpy as np
import pytest

from tests import gen, orc

pytestmark = pytest.mark.gpu

N = 120_000
MB = 1 << 20
CONFIGS = [
    ("sweep", dict(mapping_filter_mode="OneToOne", scaffold_gap=0)),
    ("full", dict(mapping_filter_mode="OneToOne", scaffold_filter_mode="OneToOne", scaffold_max_deviation=20_000)),
    ("default", dict()),
    ("k2_gap5k", dict(mapping_filter_mode="OneToMany", mapping_max_per_query=2, scaffold_gap=5_000, min_scaffold_length=2_000,
                      scaffold_max_deviation=3_000, overlap_threshold=0.5)),
]
RANGE_KERNELS = ("range_pair_insert", "range_plan", "range_plan_lds", "range_count", "range_index", "range_gather", "range_scatter", "range_chain_bounds", "range_chain_shift")


class Hip:
    """hipMalloc / hipMemcpy / hipFree of the runtime libsweepga_gpu.so is linked against."""

    def __init__(self):
        from sweepga_amd import _lib
        self.lib = _lib.load()
        self.lib.hipMalloc.restype = self.lib.hipMemcpy.restype = self.lib.hipFree.restype = C.c_int
        self.lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.lib.hipFree.argtypes = [C.c_void_p]
        self.held = []

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), max(a.nbytes, 8)) == 0
        assert self.lib.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        self.held.append(p)
        return p.value

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), max(nbytes, 8)) == 0
        self.held.append(p)
        return p.value

    def down(self, ptr, dtype, n):
        out = np.zeros(n, dtype=dtype)
        assert self.lib.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), out.nbytes, 2) == 0
        return out

    def free(self):
        for p in self.held:
            self.lib.hipFree(p)
        self.held = []


def _genome2(name):
    return "#".join(name.split("#")[:2])


def _reorder(rec, order):
    return orc.Records([rec.qname[i] for i in order], [rec.tname[i] for i in order],
                       *(np.ascontiguousarray(getattr(rec, f)[order]) for f in ("qs", "qe", "ts", "te", "block_length", "identity",
                                                                                "matches", "strand")),
                       np.arange(len(order), dtype=np.uint64))


def _ordered(rec, how, rng):
    n = len(rec.qname)
    if how == "pair_major":
        key = np.array([_genome2(q) + "|" + _genome2(t) for q, t in zip(rec.qname, rec.tname)])
        return _reorder(rec, np.argsort(key, kind="stable"))
    if how == "query_major":
        return _reorder(rec, np.argsort(np.array([_genome2(q) for q in rec.qname]), kind="stable"))
    return _reorder(rec, rng.permutation(n))


def _cfg(sw, kw):
    cfg = sw.FilterConfig(**{k: (getattr(sw.FilterMode, v) if isinstance(v, str) else v) for k, v in kw.items()})
    ocfg = orc.Config(**{k: (int(getattr(sw.FilterMode, v)) if isinstance(v, str) else v) for k, v in kw.items()})
    return cfg, ocfg


def _limit(n, kw):
    """About five ranges: the per-record budgets of a range (scratch + staging) times n / 5, plus the fixed 8 MB of scratch
    every call is budgeted and some slack."""
    per = 150 if kw.get("scaffold_gap", 1) == 0 else 350
    return 11 * MB + (n // 5) * per


def _device_records(hip, packed):
    from sweepga_amd._lib import SwgRecords
    r = SwgRecords()
    r.n = packed.n
    for k in ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end", "identity", "matches", "block_len", "strand"):
        setattr(r, k, hip.up(packed.cols[k]))
    r.n_seq = packed.n_seq
    r.seq_genome_last = hip.up(packed.seq_genome_last)
    r.n_genome_last = packed.n_genome_last
    r.seq_genome_two = hip.up(packed.seq_genome_two)
    r.n_genome_two = packed.n_genome_two
    return r


def _filter_device(ctx, hip, r, cfg, n, wide=False):
    from sweepga_amd._lib import SwgStats
    d_status, d_chain = hip.alloc(n), hip.alloc(4 * n)
    stats = SwgStats()
    cc = cfg.to_c(False, False)
    entry = ctx.lib.swg_filter_device64 if wide else ctx.lib.swg_filter_device
    ctx.check(entry(ctx.handle, C.byref(r), C.byref(cc), C.c_void_p(d_status), C.c_void_p(d_chain), C.byref(stats)))
    ctx.synchronize()
    return hip.down(d_status, np.uint8, n), hip.down(d_chain, np.uint32, n), stats


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    return sweepga_amd


@pytest.fixture(scope="module")
def base_records():
    return gen.random_records(np.random.default_rng(31337), N, n_genomes=4, chrs_per_genome=3, span=2_000_000)


@pytest.mark.parametrize("order", ["pair_major", "query_major", "shuffled"])
@pytest.mark.parametrize("cname", [c for c, _ in CONFIGS])
def test_ranged_matches_oracle_and_one_piece(sw, base_records, order, cname):
    kw = dict(CONFIGS)[cname]
    rec = _ordered(base_records, order, np.random.default_rng(7))
    packed = sw.pack_records(gen.records_to_meta(rec))
    cfg, ocfg = _cfg(sw, kw)
    ost, och = orc.apply_filters(ocfg, rec)
    free_ctx = sw.Context(0)
    st0, ch0 = sw.PafFilter(cfg, ctx=free_ctx).filter_columns(packed)   # no limit: one piece
    assert np.array_equal(st0, ost) and np.array_equal(ch0, och)
    limit = _limit(N, kw)

    # host columns: swg_filter
    hctx = sw.Context(0)
    hctx.set_memory_limit(limit)
    assert hctx.memory_limit() == limit
    f = sw.PafFilter(cfg, ctx=hctx)
    hctx.profile(True)
    st, ch = f.filter_columns(packed)
    htable = hctx.profile_table()
    assert np.array_equal(st, ost), int((st != ost).sum())
    assert np.array_equal(ch, och), int((ch != och).sum())
    assert f.last_stats.n_in == N and f.last_stats.n_out == int((ost != 0).sum())
    assert hctx.memory_info()[0] <= limit
    # the host path's ranges are one-piece device calls on gathered records: one `prepare` launch each
    assert 3 <= htable["prepare"][0] <= 10, htable
    assert not any(k in htable for k in RANGE_KERNELS), htable

    # device columns: swg_filter_device, ranges counted from the profile
    dctx = sw.Context(0)
    dctx.set_memory_limit(limit)
    hip = Hip()
    try:
        r = _device_records(hip, packed)
        dctx.profile(True)
        st, ch, stats = _filter_device(dctx, hip, r, cfg, N)
        table = dctx.profile_table()
    finally:
        hip.free()
    assert np.array_equal(st, ost), int((st != ost).sum())
    assert np.array_equal(ch, och), int((ch != och).sum())
    assert stats.n_in == N and stats.n_out == int((ost != 0).sum())
    ranges = table["range_chain_bounds"][0]
    assert 3 <= ranges <= 10, table
    if order == "pair_major":
        assert "range_gather" not in table and "range_scatter" not in table, table    # every range a slice
    elif order == "shuffled":
        assert table["range_gather"][0] == ranges and table["range_scatter"][0] == ranges, table
    if kw.get("scaffold_gap", 1) != 0:
        assert table["range_chain_shift"][0] == 1
    for c in (free_ctx, hctx, dctx):
        c.close()


@pytest.mark.parametrize("cname", ["default", "full", "sweep"])
def test_ranged_64bit_entries(sw, cname):
    """u64 columns with a sequence touched over 2^32 bases: swg_filter64 and swg_filter_device64 under a forcing limit
    (every gathered or sliced range is rebased on its own: it holds whole sweep segments)."""
    kw = dict(CONFIGS)[cname]
    rng = np.random.default_rng(4711)
    rec0 = gen.random_records(rng, 60_000, n_genomes=4, chrs_per_genome=2, span=1_500_000, minus_frac=0.3)
    rec = _ordered(gen.shifted_by_axis(rec0, rng), "shuffled", rng)
    spread = {}
    for q, a, b in zip(rec.qname, rec.qs, rec.qe):
        lo, hi = spread.get(q, (int(a), int(b)))
        spread[q] = (min(lo, int(a)), max(hi, int(b)))
    assert max(hi - lo for lo, hi in spread.values()) >= 2**32
    packed = sw.pack_records(gen.records_to_meta(rec))
    assert packed.wide
    n = len(rec.qname)
    cfg, ocfg = _cfg(sw, kw)
    ost, och = orc.apply_filters(ocfg, rec)
    limit = _limit(n, kw) + (n // 5) * 48
    hctx = sw.Context(0)
    hctx.set_memory_limit(limit)
    st, ch = sw.PafFilter(cfg, ctx=hctx).filter_columns(packed)          # swg_filter64
    assert np.array_equal(st, ost) and np.array_equal(ch, och)
    dctx = sw.Context(0)
    dctx.set_memory_limit(limit)
    hip = Hip()
    try:
        r = _device_records(hip, packed)
        dctx.profile(True)
        st, ch, _ = _filter_device(dctx, hip, r, cfg, n, wide=True)
        table = dctx.profile_table()
    finally:
        hip.free()
    assert np.array_equal(st, ost), int((st != ost).sum())
    assert np.array_equal(ch, och), int((ch != och).sum())
    assert 3 <= table["range_chain_bounds"][0] <= 10, table
    assert table["range_gather"][0] >= 1 and "axis_rebase" in table, table
    hctx.close()
    dctx.close()


def _one_big_pair(rng, n_big, n_small_pairs, per_small):
    """One genome pair of n_big records and n_small_pairs pairs of per_small records each, shuffled."""
    big = gen.random_records(rng, n_big, n_genomes=1, chrs_per_genome=3, span=2_000_000, self_frac=0.0)
    small = gen.random_records(rng, n_small_pairs * per_small, n_genomes=6, chrs_per_genome=2, span=500_000)
    qn = ["big" + q for q in big.qname] + ["s" + q for q in small.qname]
    tn = ["BIG" + t for t in big.tname] + ["s" + t for t in small.tname]
    cat = lambda f: np.concatenate([getattr(big, f), getattr(small, f)])
    rec = orc.Records(qn, tn, *(np.ascontiguousarray(cat(f)) for f in ("qs", "qe", "ts", "te", "block_length", "identity", "matches",
                                                                       "strand")), np.arange(len(qn), dtype=np.uint64))
    return _reorder(rec, rng.permutation(len(qn)))


def test_pair_larger_than_range_runs_alone(sw):
    """A genome pair larger than the range size R (from the per-record budgets) but within what the limit actually holds runs
    in a range of its own, with exact results."""
    rng = np.random.default_rng(99)
    rec = _one_big_pair(rng, 60_000, 12, 2_000)
    packed = sw.pack_records(gen.records_to_meta(rec))
    n = len(rec.qname)
    cfg, ocfg = _cfg(sw, {})
    ost, och = orc.apply_filters(ocfg, rec)
    # what the big pair needs: its own scratch high-water mark in one piece, plus its staging
    big_only = np.array([q.startswith("big") for q in rec.qname])
    sub = _reorder(rec, np.flatnonzero(big_only))
    probe = sw.Context(0)
    sw.PafFilter(cfg, ctx=probe).filter_columns(sw.pack_records(gen.records_to_meta(sub)))
    peak = probe.memory_info()[1]
    probe.close()
    limit = peak + 64 * int(big_only.sum()) + 2 * MB
    # every range of R records is budgeted at least 8 MB + 296 B per record of scratch: R < (limit - 8 MB) / 296 is smaller
    # than the pair, so the pair forms a range of its own (the packing rule, tests/native/range_plan_check.cpp)
    assert (limit - 8 * MB) // 296 < int(big_only.sum())
    dctx = sw.Context(0)
    dctx.set_memory_limit(limit)
    hip = Hip()
    try:
        r = _device_records(hip, packed)
        dctx.profile(True)
        st, ch, _ = _filter_device(dctx, hip, r, cfg, n)
        table = dctx.profile_table()
    finally:
        hip.free()
    assert np.array_equal(st, ost), int((st != ost).sum())
    assert np.array_equal(ch, och), int((ch != och).sum())
    assert table["range_chain_bounds"][0] >= 2, table
    assert dctx.profile_units()["range_chain_bounds"] == n    # every record in exactly one range
    dctx.close()


def test_pair_that_cannot_fit_is_an_oom_error(sw):
    rng = np.random.default_rng(98)
    rec = _one_big_pair(rng, 60_000, 12, 300)
    packed = sw.pack_records(gen.records_to_meta(rec))
    n = len(rec.qname)
    cfg, _ = _cfg(sw, {})
    dctx = sw.Context(0)
    dctx.set_memory_limit(10 * MB)
    hip = Hip()
    try:
        r = _device_records(hip, packed)
        from sweepga_amd._lib import SwgStats
        d_status, d_chain = hip.alloc(n), hip.alloc(4 * n)
        cc = cfg.to_c(False, False)
        rc = dctx.lib.swg_filter_device(dctx.handle, C.byref(r), C.byref(cc), C.c_void_p(d_status), C.c_void_p(d_chain),
                                        C.byref(SwgStats()))
        msg = dctx.lib.swg_last_error(dctx.handle).decode()
        assert rc == -4, (rc, msg)
        assert "genome pair of 60000 records" in msg and str(10 * MB) in msg, msg
        # no fault: the context and the device go on working
        dctx.set_memory_limit(0)
        st, ch, _ = _filter_device(dctx, hip, r, cfg, n)
        assert (st != 0).any()
    finally:
        hip.free()
    dctx.close()


def test_prefix_rules_that_disagree_are_unsupported_when_ranging(sw, base_records):
    packed = sw.pack_records(gen.records_to_meta(base_records))
    # every sequence its own genome under the last-'#' rule, grouped under the first-two-parts rule
    packed.seq_genome_last = np.arange(packed.n_seq, dtype=np.uint32)
    packed.n_genome_last = packed.n_seq
    cfg, _ = _cfg(sw, {})
    ctx = sw.Context(0)
    ctx.set_memory_limit(_limit(N, {}))
    with pytest.raises(sw.SwgError) as e:
        sw.PafFilter(cfg, ctx=ctx).filter_columns(packed)
    assert e.value.code == -6 and "partition" in str(e.value)
    hip = Hip()
    try:
        r = _device_records(hip, packed)
        from sweepga_amd._lib import SwgStats
        d_status, d_chain = hip.alloc(N), hip.alloc(4 * N)
        cc = cfg.to_c(False, False)
        rc = ctx.lib.swg_filter_device(ctx.handle, C.byref(r), C.byref(cc), C.c_void_p(d_status), C.c_void_p(d_chain),
                                       C.byref(SwgStats()))
        assert rc == -6, ctx.lib.swg_last_error(ctx.handle)
    finally:
        hip.free()
    ctx.close()


def test_no_limit_takes_no_range_kernel(sw, base_records):
    packed = sw.pack_records(gen.records_to_meta(base_records))
    ctx = sw.Context(0)
    assert ctx.memory_limit() == 0
    for _, kw in CONFIGS:
        cfg, _ = _cfg(sw, kw)
        ctx.profile(True)
        sw.PafFilter(cfg, ctx=ctx).filter_columns(packed)
        hip = Hip()
        try:
            _filter_device(ctx, hip, _device_records(hip, packed), cfg, N)
        finally:
            hip.free()
        table = ctx.profile_table()
        assert not any(k in table for k in RANGE_KERNELS), table
    ctx.close()


def test_more_than_2048_genomes_take_the_hashed_pair_table(sw):
    """Names without '#': every one of 2,400 sequences is its own genome, more than the dense G x G cell table takes; the device
    path's pairs then go through its hash table, with exact results."""
    rng = np.random.default_rng(2400)
    rec = _ordered(gen.random_records(rng, 60_000, n_genomes=60, chrs_per_genome=40, span=1_000_000, pansn=False), "shuffled", rng)
    packed = sw.pack_records(gen.records_to_meta(rec))
    assert packed.n_genome_two > 2048
    n = len(rec.qname)
    cfg, ocfg = _cfg(sw, {})
    ost, och = orc.apply_filters(ocfg, rec)
    G = packed.n_genome_two
    # the scaffold stage budgets two G x G genome tables per call on top of the per-record scratch
    limit = 11 * MB + 2 * G * G * 4 + 4 * MB + (n // 5) * 350
    dctx = sw.Context(0)
    dctx.set_memory_limit(limit)
    hip = Hip()
    try:
        r = _device_records(hip, packed)
        dctx.profile(True)
        st, ch, _ = _filter_device(dctx, hip, r, cfg, n)
        table = dctx.profile_table()
    finally:
        hip.free()
    assert np.array_equal(st, ost), int((st != ost).sum())
    assert np.array_equal(ch, och), int((ch != och).sum())
    assert table["range_pair_insert"][0] == 1 and table["range_chain_bounds"][0] >= 2, table
    dctx.close()
