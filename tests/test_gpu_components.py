"""Components on the device (sweepga_amd/csrc/swg_components.hip) against tests/components_model.py: the two record seams byte
for byte against each other and against the model -- runs longer than a thread, a wavefront and a work-group, graph shapes that
need several rounds, the thresholds, the hashed table, edges, the capacity protocol, the input errors, a memory limit, a real
filter's status with the text of swg_paf_components / --components, and one size leg.  Every comparison is exact."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import components_model as cm
from tests.test_components_cpu import columns, hand_case
from tests.test_gpu_alnstats import gen_text, records_of
from tests.test_gpu_wide import Hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


def par_of(min_bases=0, ppm=0):
    from sweepga_amd._lib import SwgComponentParams
    return SwgComponentParams(min_bases, ppm, 0)


def same(a, b):
    return (a.components.tobytes() == b.components.tobytes() and a.links.tobytes() == b.links.tobytes() and
            a.seq_component.tobytes() == b.seq_component.tobytes() and a.cross == b.cross)


def both_seams(sw, cols, status, seq_len, min_bases=0, ppm=0, ctx=None):
    """The result of the host seam, after checking that the device seam gives the same."""
    from sweepga_amd.components import _call, components_records
    ctx = ctx or sw.default_context()
    cols = {k: np.ascontiguousarray(cols[k], dtype=np.uint32) for k in cm.COLUMNS}
    seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
    status = None if status is None else np.ascontiguousarray(status, dtype=np.uint8)
    host = components_records(ctx, cols, seq_len, status, par_of(min_bases, ppm))
    hip = Hip()
    try:
        rec = records_of({k: hip.up(v) for k, v in cols.items()}, len(seq_len), len(cols["q_id"]))
        dev = _call(ctx, ctx.lib.swg_components_records_device, rec, hip.up(seq_len), None if status is None else hip.up(status), par_of(min_bases, ppm))
    finally:
        hip.free()
    assert same(dev, host)
    return host


def check(sw, cols, status, seq_len, min_bases=0, ppm=0, what="", want=None, **kw):
    got = both_seams(sw, cols, status, seq_len, min_bases, ppm, **kw)
    want = want or cm.components(cols, status, seq_len, min_bases, ppm)
    assert cm.as_model(got) == want, what
    return got


def edges_to_columns(pairs, rng=None):
    """One record per (q, t) pair with a length of its own."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n = len(pairs)
    ln = np.arange(n) % 97 + 1 if rng is None else rng.integers(0, 5_000, n)
    s = np.arange(n) % 1000
    return {"q_id": pairs[:, 0], "t_id": pairs[:, 1], "q_start": s, "q_end": s + ln, "t_start": 2 * s, "t_end": 2 * s + ln + 1}


def random_records(rng, n, n_seq, pair_major, max_len=5_000):
    q, t = rng.integers(0, n_seq, n), rng.integers(0, n_seq, n)
    if pair_major:
        order = np.lexsort((t, q))
        q, t = q[order], t[order]
    qs, ts, ln = rng.integers(0, 1_000_000, n), rng.integers(0, 1_000_000, n), rng.integers(0, max_len, n)
    ln[rng.random(n) < 0.02] = 0
    return {"q_id": q, "t_id": t, "q_start": qs, "q_end": qs + ln, "t_start": ts, "t_end": ts + np.maximum(ln + rng.integers(-20, 20, n), 0)}


# ---- 1. runs ---------------------------------------------------------------------------------------------------------------------
def test_runs_longer_than_a_thread_a_wavefront_and_a_work_group(sw):
    rng = np.random.default_rng(19)
    cols = random_records(rng, 1_000, 20, True)                       # 5 x 4 sequences, pair-major ...
    at = 400
    long = random_records(rng, 5_000, 20, True)
    long["q_id"][:], long["t_id"][:] = 7, 12                           # ... and one pair of 5,000 records in the middle of them,
    flip = rng.random(5_000) < 0.3                                     # both orientations interleaved
    long["q_id"][flip], long["t_id"][flip] = 12, 7
    cols = {k: np.r_[cols[k][:at], long[k], cols[k][at:]] for k in cols}
    status = (rng.random(6_000) < 0.8).astype(np.uint8) * 2
    seq_len = rng.integers(1, 2_000_000, 20)
    a = check(sw, cols, status, seq_len, what="pair-major")
    link = a.links[(a.links["a"] == 7) & (a.links["b"] == 12)]
    assert len(link) == 1 and int(link["n_records"][0]) > 3_500
    perm = rng.permutation(6_000)
    b = check(sw, {k: v[perm] for k, v in cols.items()}, status[perm], seq_len, what="shuffled")
    assert a.components.tobytes() == b.components.tobytes() and a.seq_component.tobytes() == b.seq_component.tobytes() and a.cross == b.cross
    for f in a.links.dtype.names:
        assert f == "first_record" or np.array_equal(a.links[f], b.links[f]), f
    c = check(sw, cols, None, seq_len, what="no status")              # every record takes part
    assert int(c.links["n_records"].sum()) == int((cols["q_id"] != cols["t_id"]).sum())


# ---- 2. graph shapes ---------------------------------------------------------------------------------------------------------------
def graph(shape):
    rng = np.random.default_rng(len(shape))
    n_seq = 3_000
    path = np.c_[np.arange(n_seq - 1), np.arange(1, n_seq)]
    if shape == "path":
        pairs = path
    elif shape == "path_permuted":
        pairs = rng.permutation(n_seq)[path]
    elif shape == "ring":
        p = rng.permutation(n_seq)
        pairs = np.r_[p[path], [[p[-1], p[0]]]]
    elif shape == "star_on_the_largest":      # every hook lands on one label
        n_seq = 2_001
        pairs = np.c_[np.full(2_000, 2_000), np.arange(2_000)]
    elif shape == "star_on_the_smallest":
        n_seq = 2_001
        pairs = np.c_[np.arange(1, 2_001), np.zeros(2_000, dtype=np.int64)]
    elif shape == "two_paths_tied_by_the_last_record":
        pairs = np.r_[path[:1_499], path[1_500:], [[2_999, 0]]]
    else:                                     # no link at all: self mappings
        pairs = np.c_[np.arange(n_seq), np.arange(n_seq)]
    return edges_to_columns(pairs), n_seq


@pytest.mark.parametrize("shape", ["path", "path_permuted", "ring", "star_on_the_largest", "star_on_the_smallest",
                                   "two_paths_tied_by_the_last_record", "no_link"])
def test_graph_shapes(sw, shape):
    cols, n_seq = graph(shape)
    seq_len = np.arange(n_seq) + 10
    got = check(sw, cols, None, seq_len, what=shape)
    if shape == "no_link":
        assert len(got.components) == n_seq and len(got.links) == 0 and got.seq_component.tolist() == list(range(1, n_seq + 1))
    else:
        assert len(got.components) == 1 and int(got.components["n_seq"][0]) == n_seq and int(got.components["first_seq"][0]) == 0
        assert int(got.components["n_links"][0]) == len(cols["q_id"]) and got.cross == (0, 0, 0)
    if shape == "two_paths_tied_by_the_last_record":   # without the tie: two components, the second numbered by sequence 1,500
        cut = {k: v[:-1] for k, v in cols.items()}
        got = check(sw, cut, None, seq_len, what="untied")
        assert got.components["first_seq"].tolist() == [0, 1_500] and got.components["n_seq"].tolist() == [1_500, 1_500]


# ---- 3. thresholds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_bases,ppm", [(0, 0), (0, 160_000), (0, 160_001), (0, 500_000), (0, 500_001), (150, 0), (151, 0)])
def test_hand_case_on_the_device(sw, min_bases, ppm):
    cols, status, seq_len = hand_case()
    got = check(sw, cols, status, seq_len, min_bases, ppm)
    joined = {(int(l["a"]), int(l["b"])): int(l["joined"]) for l in got.links}
    # By hand from hand_case(): links (0, 1): 160 / 140, (0, 4): 5 / 5, (1, 4): 150 / 150, (2, 3): 20 / 10; seq_len 1000, 1000, 500,
    # 2000, 300.  At 160,000 ppm need = 160, 160, 80, 320, 48: (0, 1) joins on a (160 >= 160), (1, 4) on b (150 >= 48), (0, 4) has
    # 5 < 48 and (2, 3) 20 < 80, 10 < 320.  One ppm more: need(0) = need(1) = 161 drops (0, 1), need(4) = 49 keeps (1, 4).  At
    # 500,000 ppm need(4) = 150 keeps (1, 4) alone; one ppm more, need(4) = 151, drops it.  min_bases 150: max(160, 140) and
    # max(150, 150) pass; 151 drops (1, 4).
    want = {(0, 0): (1, 1, 1, 1), (0, 160_000): (1, 0, 1, 0), (0, 160_001): (0, 0, 1, 0), (0, 500_000): (0, 0, 1, 0), (0, 500_001): (0, 0, 0, 0),
            (150, 0): (1, 0, 1, 0), (151, 0): (1, 0, 0, 0)}[(min_bases, ppm)]
    assert tuple(joined[k] for k in ((0, 1), (0, 4), (1, 4), (2, 3))) == want


@pytest.mark.parametrize("min_bases,ppm", [(0, 0), (20_000, 0), (0, 40_000), (20_000, 500_000), (0, 1_000_000)])
def test_random_records_under_thresholds(sw, min_bases, ppm):
    rng = np.random.default_rng(23)
    cols = random_records(rng, 3_000, 24, True)
    status = (rng.random(3_000) < 0.7).astype(np.uint8)
    seq_len = rng.integers(50_000, 3_000_000, 24)
    seq_len[5] = 0
    got = check(sw, cols, status, seq_len, min_bases, ppm)
    if (min_bases, ppm) != (0, 0):   # (not vacuous: each pair splits the links)
        assert 0 < int(got.links["joined"].sum()) < len(got.links)


# ---- 4. the hashed table ---------------------------------------------------------------------------------------------------------------
def test_two_hundred_thousand_pairs_hashed_and_dense(sw, monkeypatch):
    rng = np.random.default_rng(29)
    n_seq = 1_000                                    # 499,500 pairs possible; n_seq^2 <= 2^20: the default route is the dense table
    a, b = np.triu_indices(n_seq, 1)
    pick = rng.permutation(len(a))[:200_000]
    pairs = np.c_[a[pick], b[pick]]
    pairs = np.r_[pairs, pairs[:, ::-1]]             # every pair twice, once per orientation: 400,000 records
    pairs = pairs[rng.permutation(len(pairs))]
    cols = edges_to_columns(pairs, rng)
    seq_len = rng.integers(1_000, 100_000, n_seq)
    want = cm.components(cols, None, seq_len, 4_000, 0)
    assert len(want["links"]) == 200_000
    dense = check(sw, cols, None, seq_len, 4_000, 0, what="dense", want=want)
    monkeypatch.setenv("SWG_COMPONENTS_HASH", "1")   # 200,000 keys in 2^19 slots: probes collide
    hashed = check(sw, cols, None, seq_len, 4_000, 0, what="hashed", want=want)
    assert same(dense, hashed) and 0 < int(dense.links["joined"].sum()) < 200_000
    small = {k: v[:3_000] for k, v in cols.items()}
    check(sw, small, None, seq_len, what="hashed, few records")


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------------------
def test_edges(sw):
    none = columns(np.zeros((0, 6)))
    got = check(sw, none, np.zeros(0, dtype=np.uint8), [7, 0, 9, 11, 13])           # n = 0: n_seq singletons
    assert got.components["length"].tolist() == [7, 0, 9, 11, 13] and got.components["id"].tolist() == [1, 2, 3, 4, 5] and len(got.links) == 0
    check(sw, none, None, [5])
    got = check(sw, columns([(0, 0, 0, 10, 0, 10)] * 3), None, [100])               # n_seq = 1
    assert cm.as_model(got)["components"] == [(1, 0, 1, 0, 100, 0, 0)]
    selfs = columns([(i % 7, i % 7, 0, 10, 5, 15) for i in range(700)])              # every record a self mapping
    assert len(check(sw, selfs, np.ones(700, dtype=np.uint8), np.arange(7) + 1).links) == 0
    top = 2**32 - 1
    rec = [(0, 1, 5, 5, 9, 9), (1, 0, top, top, 0, 0),                               # zero-length records: a link of 0 bases
           (2, 3, 0, top, 0, top), (3, 2, 0, top, 1, top)]                           # sums beyond 2^32
    for ppm in (0, 1_000_000):
        got = check(sw, columns(rec), None, [0, 50, top, top], 0, ppm, what=ppm)
        assert [tuple(int(x) for x in (l["n_records"], l["a_bases"], l["b_bases"], l["joined"])) for l in got.links] == [
            (2, 0, 0, 1), (2, 2 * top - 1, 2 * top, 1)]                              # need(0) = 0: a zero seq_len joins under any share
    got = check(sw, columns(rec), None, [10, 50, top, top], 1, 1_000_000)            # min_bases = 1: the empty link does not join
    assert got.links["joined"].tolist() == [0, 1] and got.cross == (1, 2, 0)


# ---- 6. the capacity protocol and the errors -----------------------------------------------------------------------------------------------
def test_capacity_protocol_per_array(sw):
    from sweepga_amd._lib import SwgComponent, SwgComponentTable, SwgLink
    from sweepga_amd.components import COMPONENT_DTYPE, LINK_DTYPE
    ctx = sw.default_context()
    cols, status, seq_len = hand_case()
    want = cm.components(cols, status, seq_len)          # 3 components, 4 links
    rec = records_of(cols, 6)
    for cap_c, cap_l in ((2, 4), (3, 3), (3, 4), (0, 0)):
        comps = np.frombuffer(bytearray(b"\xab" * 40 * 3), dtype=COMPONENT_DTYPE)
        links = np.frombuffer(bytearray(b"\xcd" * 40 * 4), dtype=LINK_DTYPE)
        seq = np.zeros(6, dtype=np.uint32)
        c0, l0 = comps.copy(), links.copy()
        t = SwgComponentTable()
        t.component_capacity, t.components = cap_c, C.cast(comps.ctypes.data, C.POINTER(SwgComponent))
        t.link_capacity, t.links = cap_l, C.cast(links.ctypes.data, C.POINTER(SwgLink))
        t.seq_component = C.cast(seq.ctypes.data, C.POINTER(C.c_uint32))
        ctx.check(ctx.lib.swg_components_records(ctx.handle, C.byref(rec), seq_len.ctypes.data, status.ctypes.data, None, C.byref(t)))
        assert (int(t.n_components), int(t.n_links)) == (3, 4) and seq.tolist() == want["seq_component"]
        assert (comps.tobytes() == c0.tobytes()) == (cap_c < 3) and (links.tobytes() == l0.tobytes()) == (cap_l < 4), (cap_c, cap_l)
    t = SwgComponentTable()                              # NULL arrays: the counts alone
    ctx.check(ctx.lib.swg_components_records(ctx.handle, C.byref(rec), seq_len.ctypes.data, status.ctypes.data, None, C.byref(t)))
    assert (int(t.n_components), int(t.n_links), int(t.cross_links)) == (3, 4, 0)


def test_input_errors(sw):
    from sweepga_amd._lib import SwgComponentParams
    from sweepga_amd.components import components_records
    ctx = sw.default_context()
    cols, status, seq_len = hand_case()
    for bad, par in ((seq_len[:4], None), (seq_len, SwgComponentParams(0, 1_000_001, 0)), (seq_len, SwgComponentParams(0, 0, 1))):
        with pytest.raises(sw.SwgError) as e:           # sequence id 4 >= n_seq; min_share_ppm; reserved
            components_records(ctx, cols, bad, status, par)
        assert e.value.code == -1
    dropped = status.copy()
    dropped[5:] = 0                                      # ... an id out of range is refused on a record that takes no part, too
    with pytest.raises(sw.SwgError) as e:
        components_records(ctx, cols, seq_len[:4], dropped)
    assert e.value.code == -1
    check(sw, cols, status, seq_len, what="after the refusals")


def test_a_memory_limit_too_small_is_a_clean_oom(sw):
    from sweepga_amd.components import components_records
    ctx = sw.Context(0)
    try:
        rng = np.random.default_rng(51)
        cols = random_records(rng, 200_000, 40, True)
        seq_len = rng.integers(1_000, 1_000_000, 40)
        want = cm.components(cols, None, seq_len)
        ctx.set_memory_limit(1 << 20)       # the staged columns alone are 4.8 MB
        with pytest.raises(sw.SwgError) as e:
            components_records(ctx, cols, seq_len)
        assert e.value.code == -4
        ctx.set_memory_limit(0)             # ... and the context works on
        check(sw, cols, None, seq_len, what="after the refusal", want=want, ctx=ctx)
        ctx.set_memory_limit(1 << 30)
        check(sw, cols, None, seq_len, what="under a limit that holds it", want=want, ctx=ctx)
        assert ctx.memory_info()[0] <= 1 << 30
    finally:
        ctx.close()


# ---- 7. a real filter: the record seam, swg_paf_components and the command line --------------------------------------------------------------
def flag_sets(sw):
    FM = sw.FilterMode
    return {"default": (sw.FilterConfig(), []),
            "one_to_one": (sw.FilterConfig(mapping_filter_mode=FM.OneToOne, mapping_max_per_query=1, mapping_max_per_target=1,
                                           scaffold_filter_mode=FM.OneToOne, scaffold_max_per_query=1, scaffold_max_per_target=1),
                           ["--num-mappings", "1:1", "--scaffold-filter", "1:1"])}


@pytest.mark.parametrize("flags", ["default", "one_to_one"])
def test_the_status_of_a_real_filter_text_and_command_line(sw, tmp_path, flags):
    from sweepga_amd import build
    from sweepga_amd._lib import SwgStats
    text = gen_text(101, 6_000, n_genomes=4, chrs_per_genome=3, span=400_000)
    cfg, cli_flags = flag_sets(sw)[flags]
    ctx = sw.default_context()
    inp = tmp_path / "in.paf"
    inp.write_text(text, newline="")
    plain = tmp_path / "plain.paf"
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), "--quiet", *cli_flags], capture_output=True)
    assert r0.returncode == 0, r0.stderr
    with sw.PafFile(text=text) as paf:
        cols = {k: paf.column(k).copy() for k in cm.COLUMNS}
        status, chain, stats = np.zeros(paf.n, dtype=np.uint8), np.zeros(paf.n, dtype=np.uint32), SwgStats()
        cc = cfg.to_c(False, False)
        ctx.check(ctx.lib.swg_filter(ctx.handle, C.byref(paf.records), C.byref(cc), status.ctypes.data, chain.ctypes.data, C.byref(stats)))
        assert 0 < int((status != 0).sum()) < paf.n
        names = paf.names
        seq_len = cm.last_lengths(text, names)
        for min_bases, share, par_flags in ((0, 0.0, []), (20_000, 0.05, ["--component-min-bases", "20k", "--component-min-share", "0.05"])):
            ppm = int(round(share * 1e6))
            want = cm.components(cols, status, seq_len, min_bases, ppm)
            got = check(sw, cols, status, seq_len, min_bases, ppm, what=(flags, min_bases), want=want)
            assert len(got.links) > 0
            for detailed in (False, True):
                c = sw.Components.from_paf(ctx, paf, status, min_bases, share, detailed)
                assert c.text == cm.report(names, seq_len, want, detailed) and same(c, got), (flags, min_bases, detailed)
            # the command line: plain under the defaults, detailed under the thresholds; the output PAF is the same with the flag
            detailed = min_bases != 0
            out, rep = tmp_path / "out.paf", tmp_path / "c.tsv"
            r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--quiet", "--components", str(rep), *par_flags,
                                *(["--components-detailed"] if detailed else []), *cli_flags], capture_output=True)
            assert r.returncode == 0, r.stderr
            assert rep.read_bytes() == cm.report(names, seq_len, want, detailed) and out.read_bytes() == plain.read_bytes() and plain.stat().st_size > 0
        if flags == "default":
            # --components - : the report on standard error, the PAF alone on standard output
            r = subprocess.run([build.CLI, str(inp), "--quiet", "--components", "-"], capture_output=True)
            assert r.returncode == 0 and r.stdout == plain.read_bytes() and r.stderr == cm.report(names, seq_len, cm.components(cols, status, seq_len), False)
            # --no-filter: every record takes part
            r = subprocess.run([build.CLI, str(inp), "--no-filter", "--components", str(tmp_path / "n.tsv")], capture_output=True)
            assert r.returncode == 0 and r.stdout == text.encode()
            assert (tmp_path / "n.tsv").read_bytes() == cm.report(names, seq_len, cm.components(cols, None, seq_len), False)


# ---- 8. one size leg --------------------------------------------------------------------------------------------------------------------------
def test_a_million_records_pair_major_and_shuffled(sw):
    rng = np.random.default_rng(31)
    n, n_seq = 1_000_000, 60
    cols = random_records(rng, n, n_seq, True)
    status = (rng.random(n) < 0.5).astype(np.uint8)
    seq_len = rng.integers(1_000_000, 200_000_000, n_seq)
    want = cm.components(cols, status, seq_len, 700_000, 100_000)
    a = check(sw, cols, status, seq_len, 700_000, 100_000, what="pair-major", want=want)
    assert 0 < int(a.links["joined"].sum()) < len(a.links)
    perm = rng.permutation(n)
    where = np.empty(n, dtype=np.int64)
    where[perm] = np.arange(n)                        # record i of the first order is record where[i] of the second
    q, t = cols["q_id"], cols["t_id"]
    key = np.minimum(q, t) * n_seq + np.maximum(q, t)
    first = np.full(n_seq * n_seq, n, dtype=np.int64)
    part = (status != 0) & (q != t)
    np.minimum.at(first, key[part], where[part])
    want_shuffled = dict(want, links=[l[:6] + (int(first[l[0] * n_seq + l[1]]),) for l in want["links"]])
    check(sw, {k: v[perm] for k, v in cols.items()}, status[perm], seq_len, 700_000, 100_000, what="shuffled", want=want_shuffled)


def test_smallest_shapes_on_a_fresh_context(sw):
    """The seams around the kernels at the smallest shapes -- one record; three records of one sequence pair in one chain -- on a
    context of its own: its first call sizes the arena from the input, the later ones find it sized.  Each shape twice, host seam
    against device seam byte for byte and both against the model."""
    a = np.array([(0, 1, 10, 110, 20, 125), (0, 1, 200, 300, 210, 310), (0, 1, 400, 450, 420, 470)], dtype=np.uint32)
    seq_len = np.array([1000, 1000], dtype=np.uint32)
    ctx = sw.Context(0)
    try:
        for n in (1, 3, 1, 3):
            cols = {c: a[:n, j].copy() for j, c in enumerate(("q_id", "t_id", "q_start", "q_end", "t_start", "t_end"))}
            for status in (None, np.ones(n, dtype=np.uint8)):   # (None: the optional column stays NULL on its way to the device)
                got = check(sw, cols, status, seq_len, what=f"n = {n}", ctx=ctx)
                assert len(got.components) == 1 and len(got.links) == 1 and int(got.links["n_records"][0]) == n
    finally:
        ctx.close()
