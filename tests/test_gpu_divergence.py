"""The divergence track on the device (sweepga_amd/csrc/swg_divergence.hip) against tests/divergence_model.py: in every case the
host seam against the model field by field and the device seam against the host seam byte for byte.  The shapes are the smallest at
which each part can go wrong: window borders and points worked out by hand, the op pass's tile of 1,024 ops and its four ops per
thread, five scan tiles of windows, the fold along the wavefront at its extremes, M-only and =-only CIGARs, one long CIGAR; the
cross-checks against the windows, the difference list and the base-exact lift ON the device; the capacity protocol and every
refusal; a random case under a real filter status; the texts of swg_paf_divergence / Divergence.from_paf / --divergence for every
batch size.  Every comparison is exact: integers and bytes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import divergence_model as vm
from tests import lift_exact_model as em
from tests import lift_model as lm
from tests.test_divergence_cpu import HAND, check_hand_rows, hand_inputs
from tests.test_gpu_intervals import kept_mask
from tests.test_gpu_lift import Dev
from tests.test_gpu_lift_exact import corrupt, random_case, tagged_paf
from tests.test_gpu_place import FILTER_COLS
from tests.test_gpu_ucsc_chain import pairs, records_of
from tests.test_gpu_wide import Hip

pytestmark = pytest.mark.gpu
COLS = lm.COLS
FIELDS = ("n_rows", "n_seqs", "ops", "cigar_bad", "usable")
TOP = 2**32 - 1


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


def same(a, b):
    return ((a.rows is None) == (b.rows is None) and (a.seqs is None) == (b.seqs is None) and (a.rows is None or a.rows.tobytes() == b.rows.tobytes())
            and (a.seqs is None or a.seqs.tobytes() == b.seqs.tobytes()) and a.state.tobytes() == b.state.tobytes()
            and all(getattr(a, f) == getattr(b, f) for f in FIELDS))


def both_seams(sw, cols, strand, seq_len, genome, G_, cig, status=None, set_=0, axis=0, window=100, other=None, ctx=None, want=3, shift=0):
    """The result of the host seam, after checking that the device seam gives the same.  shift: the device text starts that many
    bytes behind a 16-byte boundary."""
    from sweepga_amd.divergence import divergence_records, divergence_records_device
    from sweepga_amd.lift import cigar_set
    ctx = ctx or sw.default_context()
    recs = sorted(cig)
    kw = dict(set=set_, axis=axis, window=window, other_genome=other, want=want)
    got = divergence_records(ctx, cols, strand, seq_len, genome, G_, recs, [cig[i] for i in recs], status=status, **kw)
    record, offset, text = cigar_set(recs, [cig[i] for i in recs])
    hip = Hip()
    try:
        dcols = {k: Dev(hip, cols[k], np.uint32) for k in COLS}
        dtext = Dev(hip, np.concatenate([np.zeros(shift, dtype=np.uint8), text, np.zeros(1, dtype=np.uint8)]))
        dtext.ptr += shift
        dev = divergence_records_device(ctx, dcols, Dev(hip, strand, np.uint8), Dev(hip, seq_len, np.uint32), Dev(hip, genome, np.uint32), G_, Dev(hip, record),
                                        Dev(hip, offset), dtext, len(recs), status=Dev(hip, status, np.uint8) if status is not None else None, **kw)
    finally:
        hip.free()
    assert same(dev, got)
    return got


def compare(got, want, what=""):
    assert got.state.tolist() == want["state"], (what, [(k, a, b) for k, (a, b) in enumerate(zip(got.state.tolist(), want["state"])) if a != b][:8])
    assert (got.ops, got.cigar_bad, got.usable) == (want["ops"], want["cigar_bad"], want["usable"]), what
    if got.rows is not None:
        vm.same(got.rows, want["rows"], (what, "rows"))
        assert got.n_rows == len(want["rows"])
    if got.seqs is not None:
        vm.same(got.seqs, want["seqs"], (what, "summary"))
        assert got.n_seqs == len(want["seqs"])


def check(sw, cols, strand, seq_len, genome, G_, cig, status=None, variants=((0, 0, 100, None),), what="", ctx=None, shift=0, model_checks=False):
    """Both seams against the model, for every (set, axis, window, other genome) of variants -> the last result."""
    cols = {k: np.asarray(cols[k]).astype(np.uint32) for k in COLS}
    strand, genome, seq_len = np.asarray(strand).astype(np.uint8), np.asarray(genome).astype(np.uint32), np.asarray(seq_len).astype(np.uint32)
    kept = None if status is None else np.asarray(status) != 0
    for set_, axis, window, other in variants:
        got = both_seams(sw, cols, strand, seq_len, genome, G_, cig, status, set_, axis, window, other, ctx, shift=shift)
        compare(got, vm.divergence(cols, strand, seq_len, genome, cig, kept, set_, axis, window, other, check=model_checks), (what, set_, axis, window, other))
    return got


def check_texts(sw, texts, what="", strands=None, windows=(100,), **kw):
    """One record per CIGAR text, query on sequence 0 (genome 0) and target on sequence 1 (genome 1), one behind the other; both axes."""
    cols, strand, seq_len = records_of(texts, strands)
    return check(sw, cols, strand, seq_len, [0, 1], 2, dict(enumerate(texts)), variants=[(0, axis, w, None) for w in windows for axis in (0, 1)], what=what, **kw)


# ---- window borders and points -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seq_len", [1_000, 1_050])
def test_hand_cases(sw, seq_len):
    for axis in (0, 1):
        for second in (False, True):
            cols, strand, lens, genome, cig, want = hand_inputs(axis, seq_len, second)
            got = check(sw, cols, strand, lens, genome, 3, cig, variants=((0, axis, 100, None),), what=(axis, second), model_checks=True)
            check_hand_rows(got.rows, want)
            assert got.usable == len(cig) and got.n_seqs == 1 + second and int(got.rows["end"][got.rows["seq"] == 0][-1]) == seq_len
    assert len(HAND) > 20


def test_extremes_of_the_window(sw):
    """W = 1, the sequence length, larger than every sequence, 2^32 - 1; a sequence of length 0 among the ids."""
    for axis in (0, 1):
        cols, strand, lens, genome, cig, _ = hand_inputs(axis, 1_000, True)
        lens, genome = lens + [0], genome + [1]
        got = check(sw, cols, strand, lens, genome, 3, cig, variants=[(0, axis, w, None) for w in (1, 1_000, 1_020, 5_000, TOP)], what=("extremes", axis))
        assert len(got.rows) == 2 and got.rows["end"].tolist() == [1_000, 1_020]
        one = check(sw, cols, strand, lens, genome, 3, cig, variants=((0, axis, 1, None),))
        assert len(one.rows) == 2_020 and int(one.rows["n"].max()) > 3 and (one.rows["end"] - one.rows["start"] == 1).all()
        assert int(one.rows["aligned"].sum()) == int(got.rows["aligned"].sum()) and int(one.rows["indels"].sum()) == int(got.rows["indels"].sum())


# ---- the op pass ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1_023, 1_024, 1_025])
def test_entries_around_one_tile_of_ops(sw, n):
    """Entries of n ops none of which is '=': the entry border falls in front of, on and behind the tile border."""
    for shift in (0, 5):
        got = check_texts(sw, [pairs(n, "1X", "2D"), "2=", pairs(n, "3I", "1M"), "1X", pairs(1_024, "1N", "2X"), pairs(n, "1X", "1I")], "n = %d" % n,
                          windows=(100, 7), shift=shift)
        assert got.ops == 3 * n + 1_024 + 2 and got.usable == 6


def test_four_ops_of_a_thread_in_four_entries(sw):
    """Entries of one op, so that every thread of the op pass meets four entries; empty and unusable entries between them."""
    unit = ("2X", "3D", "1I", "4M", "", "2N", "5=", "1X9", "3X", "1D")
    texts = [unit[k % len(unit)] for k in range(5_000)]
    for shift in (0, 9):
        got = check_texts(sw, texts, "one op per entry", windows=(100, 3), shift=shift)
        # (the last variant is the target axis: a record of `1I` has no target base and does not take part)
        assert got.usable == 3_500 and got.cigar_bad == 500 and got.state.tolist()[:10] == [0, 0, 0, 0, 16, 0, 0, 1, 0, 0]
    got = check_texts(sw, ["", "1X", "", "", "2I1=", "x", "5=1D", ""], "empty entries between")
    assert got.usable == 3 and got.state.tolist() == [16, 0, 16, 16, 0, 1, 0, 16]


def test_scan_tiles_one_M_and_one_N_over_20000_windows(sw):
    """Five scan tiles of windows: the differences of two long ops run through them under 3,000 short entries."""
    rng = np.random.default_rng(4)
    texts = ["2000000M", "10=2000000N10="] + ["%d=%dX%d=" % tuple(rng.integers(1, 40, 3)) for _ in range(3_000)]
    adv = np.array([em.advances(em.parse(t)[1]) for t in texts], dtype=np.int64)
    qs = np.concatenate([[50, 130], rng.integers(0, 2_000_000, 3_000)])
    ts = np.concatenate([[50, 130], rng.integers(0, 2_000_000, 3_000)])
    cols = {"q_id": np.zeros(3_002), "t_id": np.ones(3_002), "q_start": qs, "q_end": qs + adv[:, 0], "t_start": ts, "t_end": ts + adv[:, 1]}
    strand = rng.integers(0, 2, 3_002)
    got = check(sw, cols, strand, [2_100_000, 2_100_000], [0, 1], 2, dict(enumerate(texts)), variants=((0, 1, 100, None), (0, 0, 100, None)), what="scan tiles")
    assert len(got.rows) == 21_000 and got.usable == 3_002
    t = check(sw, cols, strand, [2_100_000, 2_100_000], [0, 1], 2, dict(enumerate(texts)), variants=((0, 1, 100, None),))
    assert int(t.rows["m_columns"][1:20_000].min()) == 100 and int(t.rows["unaligned"][2:20_001].min()) == 100 and int(t.rows["indels"].sum()) == 1


@pytest.mark.parametrize("shape", ["one window", "4096 ends", "every op its own slot", "alternating"])
def test_the_fold_along_the_wavefront(sw, shape):
    n = 4_096
    if shape == "one window":           # every lane of every wavefront hits one slot
        texts, window = ["1=1X1="] * n, 100
        q0 = t0 = np.full(n, 7) + np.arange(n) % 50
    elif shape == "4096 ends":          # one slot for the starts, 4,096 for the ends; runs of one lane
        texts, window = ["%d=1X" % (2 * i + 1) for i in range(n)], 2
        q0 = t0 = np.ones(n, dtype=np.int64)
    elif shape == "every op its own slot":
        texts, window = ["1=1X" * 2_000, "1X1=" * 2_000], 1
        q0 = t0 = np.array([0, 4_000])
    else:                               # neighbours alternate between two windows: no run is longer than one lane
        texts, window = ["2=1X1I1D"] * n, 100
        q0 = t0 = np.where(np.arange(n) % 2 == 0, 10, 510) + np.arange(n) % 3
    adv = np.array([em.advances(em.parse(t)[1]) for t in texts], dtype=np.int64)
    k = len(texts)
    cols = {"q_id": np.zeros(k), "t_id": np.ones(k), "q_start": q0, "q_end": q0 + adv[:, 0], "t_start": t0, "t_end": t0 + adv[:, 1]}
    got = check(sw, cols, np.arange(k) % 2, [8_200, 8_200], [0, 1], 2, dict(enumerate(texts)), variants=((0, 0, window, None), (0, 1, window, None)), what=shape)
    assert got.usable == k and int(got.rows["n"].max()) == {"one window": n, "4096 ends": n, "every op its own slot": 1, "alternating": n // 2}[shape]


def test_M_only_and_eq_only_cigars(sw):
    rng = np.random.default_rng(8)
    for letter in "M=":
        texts = ["%d%s" % (l, letter) for l in rng.integers(1, 900, 700)] + ["%d%s%d%s" % (a, letter, b, letter) for a, b in rng.integers(1, 300, (300, 2))]
        got = check_texts(sw, texts, letter, windows=(64,))
        assert got.usable == 1_000 and int(got.rows["aligned"].sum()) > 300_000
        assert not any(got.rows[f].any() for f in ("mismatches", "unaligned", "inserted", "mismatch_runs", "indels"))
        if letter == "M":
            assert not got.rows["matches"].any() and (got.rows["m_columns"] == got.rows["aligned"]).all()
        else:           # the op pass visits nothing: the rows come from the overlaps alone
            assert not got.rows["m_columns"].any() and (got.rows["matches"] == got.rows["aligned"]).all()


def test_one_cigar_of_100000_ops_on_both_strands(sw):
    long = "".join(("2=", "1X", "3=", "2I", "1=", "3D", "1M", "1N")[k % 8] for k in range(100_000))
    got = check_texts(sw, ["2=", long, long, "1X"], "10^5", strands=[0, 0, 1, 1], windows=(1_000,))
    assert got.ops == 200_002 and got.usable == 4 and int(got.rows["mismatch_runs"].sum()) == 25_001 and int(got.rows["indels"].sum()) == 75_000


# ---- the cross-checks on the device -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(7)
    cols, strand, texts = random_case(rng, 600, 4)
    seq_len = np.full(4, int(max(cols["q_end"].max(), cols["t_end"].max())) + 7, dtype=np.uint32)
    return cols, strand, texts, np.array([0, 1, 1, 2], dtype=np.uint32), (rng.random(600) < 0.6).astype(np.uint8), seq_len


def test_against_windows_diffs_and_the_exact_lift_on_the_device(sw, small):
    from sweepga_amd.diffs import diff_records
    from sweepga_amd.lift import lift_exact_records
    from sweepga_amd.windows import windows_records
    cols, strand, texts, genome, status, seq_len = small
    ctx = sw.default_context()
    every = dict(enumerate(texts))
    inter = np.flatnonzero(genome[cols["q_id"]] != genome[cols["t_id"]])
    for axis in (0, 1):
        for set_, window in ((0, 5_000), (1, 777)):
            got = check(sw, cols, strand, seq_len, genome, 3, every, status, ((set_, axis, window, None),), what=("cross", axis, set_))
            # the windows: depth and n of the same set (the windows list the sequences of ALL records)
            w = windows_records(ctx, dict(cols, matches=np.zeros(600, dtype=np.uint32)), seq_len, genome, status, axis=axis, window=window, n_genome=3).rows
            w = w[np.isin(w["seq"], got.rows["seq"])]
            assert (w["seq"] == got.rows["seq"]).all() and (w["start"] == got.rows["start"]).all() and len(w) > 40
            assert (w["depth"][:, set_] == got.rows["aligned"] + got.rows["unaligned"]).all() and (w["n"][:, set_] == got.rows["n"]).all()
            # the difference list: the pair sums of the inter-genome pairs
            on_axis = np.flatnonzero(cols[("q_end", "t_end")[axis]] > cols[("q_start", "t_start")[axis]]).tolist()      # (an empty axis side takes no part)
            d = diff_records(ctx, cols, strand, 4, genome, 3, on_axis, [texts[i] for i in on_axis], status=status, set=set_, kinds=15).pairs
            d = d[d["q_genome"] != d["t_genome"]]
            total = {f: int(got.rows[f].sum()) for f in vm.FIELDS}
            assert total["aligned"] == int(d["aligned"].sum()) and total["matches"] == int(d["eq"].sum()) and total["mismatches"] == int(d["snp_bases"].sum())
            assert total["m_columns"] == int(d["m_columns"].sum()) and total["mismatch_runs"] == int(d["snp_runs"].sum()) and int(d["entries"].sum()) == got.usable
            assert total["indels"] == int(d["n_ins"].sum() + d["n_del"].sum() + d["n_skip"].sum())
            assert total["unaligned"] + total["inserted"] == int(d["ins_bases"].sum() + d["del_bases"].sum() + d["skip_bases"].sum())
    # the base-exact lift with the windows as regions: aligned and matches per window, over the inter-genome records alone
    part = {k: v[inter] for k, v in cols.items()}
    cig = {j: texts[i] for j, i in enumerate(inter)}
    for axis in (0, 1):
        got = check(sw, part, strand[inter], seq_len, genome, 3, cig, variants=((0, axis, 5_000, None),), what=("lift", axis))
        regions = [(int(r["seq"]), int(r["start"]), int(r["end"])) for r in got.rows]
        lifted = lift_exact_records(ctx, part, strand[inter], 4, regions, sorted(cig), [cig[j] for j in sorted(cig)], axes=("query", "target")[axis])
        assert lifted.exact_rows == lifted.n >= got.usable > 300      # (every usable entry meets a window or more)
        for f in ("aligned", "matches"):
            assert (np.bincount(lifted.rows["region"], weights=lifted.rows[f], minlength=len(regions)).astype(np.uint64) == got.rows[f]).all()


# ---- the protocol ------------------------------------------------------------------------------------------------------------------------
def test_sets_genomes_a_partial_set_and_records_permuted(sw, small):
    cols, strand, texts, genome, status, seq_len = small
    every = dict(enumerate(texts))
    variants = [(set_, axis, 1_000, other) for set_ in (0, 1) for axis in (0, 1) for other in (None, 1)]
    base = check(sw, cols, strand, seq_len, genome, 3, every, status, variants, what="sets", model_checks=True)
    assert base.usable > 50
    none = check(sw, cols, strand, seq_len, genome, 3, every, np.zeros(600, dtype=np.uint8), ((1, 0, 1_000, None),), what="never in status")
    assert (none.n_rows, none.n_seqs, none.usable, len(none.rows)) == (0, 0, 0, 0) and none.ops == base.ops
    part = check(sw, cols, strand, seq_len, genome, 3, {i: texts[i] for i in range(0, 600, 3)}, status, ((1, 0, 1_000, None), (0, 1, 1_000, None)), what="a partial set")
    assert 0 < part.usable < 200 and (part.seqs["records"] > part.seqs["entries"]).all()
    listed = check(sw, cols, strand, seq_len, genome, 3, {}, status, ((0, 0, 1_000, None),), what="no entry at all")      # listed sequences with zero rows
    assert listed.n_rows == len(listed.rows) > 100 and not listed.rows["n"].any() and (listed.seqs["records"] > 0).all() and not listed.seqs["entries"].any()
    perm = np.random.default_rng(3).permutation(600)
    pcols = {k: v[perm] for k, v in cols.items()}
    for axis in (0, 1):
        in_order = both_seams(sw, cols, strand, seq_len, genome, 3, every, status, 1, axis, 333)
        moved = both_seams(sw, pcols, strand[perm], seq_len, genome, 3, {j: texts[i] for j, i in enumerate(perm)}, status[perm], 1, axis, 333)
        assert moved.rows.tobytes() == in_order.rows.tobytes() and moved.seqs.tobytes() == in_order.seqs.tobytes() and moved.usable == in_order.usable


def test_each_want_bit(sw, small):
    cols, strand, texts, genome, status, seq_len = small
    every = dict(enumerate(texts))
    both = both_seams(sw, cols, strand, seq_len, genome, 3, every, status, 1, 0, 500)
    rows = both_seams(sw, cols, strand, seq_len, genome, 3, every, status, 1, 0, 500, want=1)
    seqs = both_seams(sw, cols, strand, seq_len, genome, 3, every, status, 1, 0, 500, want=2)
    assert rows.seqs is None and seqs.rows is None and rows.rows.tobytes() == both.rows.tobytes() and seqs.seqs.tobytes() == both.seqs.tobytes()
    assert (rows.n_seqs, seqs.n_rows) == (0, 0) and rows.usable == seqs.usable == both.usable and rows.state.tobytes() == both.state.tobytes()


def raw_call(sw, fn, cols, strand, seq_len, genome, G_, cig, caps, set_=0, axis=0, window=500, other=TOP, want=3, status=None, ctx=None, null=(), reserved=0):
    """A record seam with caller arrays full of 0xAB -> (rc, request, rows bytes, seqs bytes, state bytes)"""
    from sweepga_amd import _lib
    from sweepga_amd.lift import cigar_set
    ctx = ctx or sw.default_context()
    rec = _lib.SwgRecords()
    rec.n = len(strand)
    keep = {k: np.ascontiguousarray(cols[k], dtype=np.uint32) for k in COLS}
    for k, a in keep.items():
        setattr(rec, k, a.ctypes.data)
    rec.strand, rec.n_seq = strand.ctypes.data, len(genome) if genome is not None else 4
    record, offset, text = cig if isinstance(cig, tuple) else cigar_set(sorted(cig), [cig[i] for i in sorted(cig)])
    cs = _lib.SwgCigarSet()
    cs.record, cs.offset, cs.text, cs.k = record.ctypes.data, offset.ctypes.data, text.ctypes.data, len(record)
    arrays = [np.full(size * max(c, 1), 0xab, dtype=np.uint8) for size, c in zip((80, 88), caps)]
    state = np.full(max(len(record), 1), 0xab, dtype=np.uint8)
    req = _lib.SwgDivergenceRequest()
    req.set, req.axis, req.window, req.other_genome, req.want, req.reserved, req.state, req.n_rows = set_, axis, window, other, want, reserved, state.ctypes.data, 99
    req.capacity, req.seq_capacity = caps
    req.rows, req.seqs = (None if k in null else a.ctypes.data for k, a in enumerate(arrays))
    rc = fn(ctx.handle, C.byref(rec), seq_len.ctypes.data if seq_len is not None else None, genome.ctypes.data if genome is not None else None, G_,
            status.ctypes.data if status is not None else None, C.byref(cs), C.byref(req))
    return (rc, req) + tuple(a.tobytes() for a in arrays) + (state.tobytes(),)


def test_capacities_with_poisoned_arrays(sw, small):
    cols, strand, texts, genome, _, seq_len = small
    lib = sw.default_context().lib
    cig = dict(enumerate(texts))
    want = vm.divergence(cols, strand, seq_len, genome, cig, window=500)
    counts = (len(want["rows"]), len(want["seqs"]))
    full = (want["rows"].tobytes(), want["seqs"].tobytes())
    assert counts[0] > 100 and counts[1] == 4
    for which in range(2):
        for cap in (0, counts[which] - 1, counts[which]):
            caps = tuple(cap if k == which else counts[k] for k in range(2))
            rc, req, *arrays, state = raw_call(sw, lib.swg_divergence_records, cols, strand, seq_len, genome, 3, cig, caps)
            assert rc == 0 and (req.n_rows, req.n_seqs, req.usable, req.ops) == (counts[0], counts[1], want["usable"], want["ops"]) and list(state) == want["state"]
            for k in range(2):
                if caps[k] < counts[k]:
                    assert set(arrays[k]) == {0xab}, (which, cap, k)      # an array that does not hold its count is left alone
                else:
                    assert arrays[k] == full[k], (which, cap, k)
    rc, req, *arrays, state = raw_call(sw, lib.swg_divergence_records, cols, strand, seq_len, genome, 3, cig, counts, null=(0, 1))
    assert rc == 0 and (req.n_rows, req.n_seqs, req.usable) == (counts[0], counts[1], want["usable"]) and all(set(a) == {0xab} for a in arrays)
    rc, req, *arrays, state = raw_call(sw, lib.swg_divergence_records, cols, strand, seq_len, genome, 3, cig, counts, want=2)      # the rows bit is not set
    assert rc == 0 and set(arrays[0]) == {0xab} and arrays[1] == full[1] and req.n_seqs == counts[1]


def test_refusals(sw, small):
    from sweepga_amd import _lib
    from sweepga_amd.divergence import divergence_records, divergence_records_device
    from sweepga_amd.lift import cigar_set
    cols, strand, texts, genome, status, seq_len = small
    ctx = sw.default_context()
    lib = ctx.lib
    good = cigar_set([3, 5, 9], ["1=", "2=", ""])
    bad_sets = [(np.array([3, 3, 9], dtype=np.uint32), good[1], good[2]), (np.array([5, 3, 9], dtype=np.uint32), good[1], good[2]),
                (np.array([3, 5, 600], dtype=np.uint32), good[1], good[2]), (good[0], np.array([0, 4, 2, 4], dtype=np.uint64), good[2]),
                (good[0], np.array([1, 2, 4, 4], dtype=np.uint64), good[2])]
    beyond = {k: v.copy() for k, v in cols.items()}
    first = int(np.flatnonzero(genome[cols["q_id"]] != genome[cols["t_id"]])[2])
    beyond["q_end"][first] = int(seq_len[0]) + 1
    beyond["q_end"][first + 50:] = int(seq_len[0]) + 1       # the smallest such record is named (an intra-genome one would not take part)
    later = [i for i in range(first + 50, 600) if genome[cols["q_id"][i]] != genome[cols["t_id"][i]]]
    assert later
    wrong_id = {k: v.copy() for k, v in cols.items()}
    wrong_id["t_id"][17] = 4
    hip = Hip()
    try:
        dcols = {k: Dev(hip, cols[k], np.uint32) for k in COLS}
        dstrand, dgenome, dlen = Dev(hip, strand, np.uint8), Dev(hip, genome, np.uint32), Dev(hip, seq_len, np.uint32)
        for record, offset, text in bad_sets:                  # the set, on both seams
            rc, req, rows, seqs, state = raw_call(sw, lib.swg_divergence_records, cols, strand, seq_len, genome, 3, (record, offset, text), (4, 4))
            assert rc == -1 and set(rows) == set(seqs) == set(state) == {0xab} and req.n_rows == 99, (record, offset)
            with pytest.raises(sw.SwgError) as e:
                divergence_records_device(ctx, dcols, dstrand, dlen, dgenome, 3, Dev(hip, record), Dev(hip, offset), Dev(hip, text), 3)
            assert e.value.code == -1, (record, offset)
        dset = [Dev(hip, a) for a in good]
        for kw, word in (({"window": 0}, "window size"), ({"axis": 2}, "axis"), ({"other_genome": 3}, "other_genome"), ({"set": 2}, "set"),
                         ({"set": 1}, "status"), ({"want": 0}, "want"), ({"want": 4}, "want")):
            with pytest.raises(sw.SwgError) as e:
                divergence_records_device(ctx, dcols, dstrand, dlen, dgenome, 3, *dset, 3, **kw)
            assert e.value.code == -1 and word in str(e.value), kw
            with pytest.raises(sw.SwgError) as e:
                divergence_records(ctx, cols, strand, seq_len, genome, 3, None, good, **kw)
            assert e.value.code == -1 and word in str(e.value), kw
        for name, c in (("beyond", beyond), ("id", wrong_id)):      # found on the device, before any write trusts it
            with pytest.raises(sw.SwgError) as e:
                divergence_records_device(ctx, {k: Dev(hip, c[k], np.uint32) for k in COLS}, dstrand, dlen, dgenome, 3, *dset, 3)
            assert e.value.code == -1 and (("record %d takes part and ends beyond" % first) if name == "beyond" else "sequence id") in str(e.value)
            rc, req, rows, seqs, state = raw_call(sw, lib.swg_divergence_records, c, strand, seq_len, genome, 3, good, (4, 4))
            assert rc == -1 and set(rows) == set(seqs) == {0xab}
        twos = np.full(4, 2, dtype=np.uint32)
        for n_genome in (2, 0):                    # a genome id >= n_genome, on both seams
            with pytest.raises(sw.SwgError) as e:
                divergence_records_device(ctx, dcols, dstrand, dlen, Dev(hip, twos), n_genome, *dset, 3)
            assert e.value.code == -1 and "genome" in str(e.value)
            rc, req, rows, *_ = raw_call(sw, lib.swg_divergence_records, cols, strand, seq_len, twos, n_genome, good, (4, 4))
            assert rc == -1 and set(rows) == {0xab} and b"genome" in lib.swg_last_error(ctx.handle)
    finally:
        hip.free()
    for fn in (lib.swg_divergence_records, lib.swg_divergence_records_device):      # k and n are looked at before any array
        for n, k in ((600, 2**31), (2**31, 3)):
            cs = _lib.SwgCigarSet()
            cs.record, cs.offset, cs.text, cs.k = good[0].ctypes.data, good[1].ctypes.data, good[2].ctypes.data, k
            rec = _lib.SwgRecords()
            rec.n, rec.n_seq = n, 4
            req = _lib.SwgDivergenceRequest()
            req.want, req.window, req.other_genome = 3, 100, TOP
            assert fn(ctx.handle, C.byref(rec), seq_len.ctypes.data, genome.ctypes.data, 3, None, C.byref(cs), C.byref(req)) == -5
    for kw, word in ((dict(genome=None), b"NULL column"), (dict(seq_len=None), b"NULL column"), (dict(reserved=1), b"reserved")):
        args = dict(seq_len=seq_len, genome=genome)
        reserved = kw.pop("reserved", 0)
        args.update(kw)
        rc, req, rows, *_ = raw_call(sw, lib.swg_divergence_records, cols, strand, args["seq_len"], args["genome"], 3, good, (4, 4), reserved=reserved)
        assert rc == -1 and set(rows) == {0xab} and word in lib.swg_last_error(ctx.handle), word
    with pytest.raises(sw.SwgError) as e:      # a set for no records
        divergence_records(ctx, {k: np.zeros(0, dtype=np.uint32) for k in COLS}, np.zeros(0, dtype=np.uint8), seq_len, genome, 3, [0], ["1="])
    assert e.value.code == -1
    empty = divergence_records(ctx, {k: np.zeros(0, dtype=np.uint32) for k in COLS}, np.zeros(0, dtype=np.uint8), seq_len, genome, 3, [], [])
    assert (empty.n_rows, empty.n_seqs, empty.usable, len(empty.rows), len(empty.seqs)) == (0, 0, 0, 0, 0)
    after = check(sw, cols, strand, seq_len, genome, 3, {3: texts[3]}, what="after the refusals")      # the context is as usable as before
    assert after.n_seqs == 4


def test_too_many_windows_are_refused_before_they_are_allocated(sw):
    """One listed sequence of 2^32 - 2 bases under W = 1 carries a single short record: 2^31 windows or more is SWG_ERR_RANGE.  The
    table would take hundreds of gigabytes; a context limited to 64 MB refuses with the RANGE code, not with OOM."""
    from sweepga_amd.divergence import divergence_records
    ctx = sw.Context(0)
    try:
        ctx.set_memory_limit(64 << 20)
        cols = {k: np.array([v], dtype=np.uint32) for k, v in zip(COLS, (0, 1, 5, 9, 50, 54))}
        for length, window in ((TOP - 1, 1), (TOP, 2)):
            with pytest.raises(sw.SwgError) as e:
                divergence_records(ctx, cols, [0], [length, 100], [0, 1], 2, [0], ["1=1X2="], window=window)
            assert e.value.code == -5 and "2^31 windows" in str(e.value)
        got = divergence_records(ctx, cols, [0], [2**31 - 1, 100], [0, 1], 2, [0], ["1=1X2="], window=2**20)      # ... and the context works on
        assert len(got.rows) == 2_048 and tuple(int(v) for v in got.seqs[0]) == (0, 2_048, 1, 1, 4, 3, 1, 0, 0, 0, 1, 0)
    finally:
        ctx.close()


def test_a_memory_limit_too_small_is_a_clean_oom(sw, small):
    from sweepga_amd.divergence import divergence_records
    cols, strand, texts, genome, _, seq_len = small
    ctx = sw.Context(0)
    try:
        long = "1=1I" * 100_000      # 400 kB of text, 2 * 10^5 ops: 32 bytes of prefix sums each, 6.4 MB
        c1 = {k: np.array([v], dtype=np.uint32) for k, v in zip(COLS, (0, 1, 0, 200_000, 0, 100_000))}
        ctx.set_memory_limit(4 << 20)
        with pytest.raises(sw.SwgError) as e:
            divergence_records(ctx, c1, [0], [200_000, 100_000], [0, 1], 2, [0], [long])
        assert e.value.code == -4
        got = divergence_records(ctx, cols, strand, seq_len, genome, 3, list(range(600)), texts, window=500)      # the same context, a call that fits
        compare(got, vm.divergence(cols, strand, seq_len, genome, dict(enumerate(texts)), window=500), "under the limit")
        ctx.set_memory_limit(0)
        got = divergence_records(ctx, c1, [0], [200_000, 100_000], [0, 1], 2, [0], [long])
        assert len(got.rows) == 20 and tuple(int(v) for v in got.seqs[0]) == (0, 20, 1, 1, 100_000, 100_000, 0, 0, 100_000, 0, 0, 100_000)
    finally:
        ctx.close()


def test_smallest_shapes_on_a_fresh_context(sw):
    """The seams around the kernels at the smallest shapes -- one record; three records -- with and without a status, on a context of
    its own: its first call sizes the arena from the input, the later ones find it sized."""
    texts = ["5=2I6=4D5X2=", "10M", "3I4=2I3D2=1I"]
    cols, strand, seq_len = records_of(texts)
    ctx = sw.Context(0)
    try:
        for n in (1, 3, 1, 3):
            part = {k: v[:n] for k, v in cols.items()}
            for status in (None, np.array([1, 0, 1], dtype=np.uint8)[:n]):
                got = check(sw, part, strand[:n], seq_len, [0, 1], 2, dict(enumerate(texts[:n])), status,
                            [(0 if status is None else 1, axis, 10, None) for axis in (0, 1)], what=f"n = {n}", ctx=ctx, model_checks=True)
                assert got.usable == (n if status is None else (n + 1) // 2) and got.n_seqs == 1
    finally:
        ctx.close()


# ---- the whole path ------------------------------------------------------------------------------------------------------------------------
def test_20000_records_under_the_status_of_a_real_filter_on_the_device(sw):
    """Random CIGARs, 5 % of the entries corrupted, 5 % of the records left out of the set; swg_filter_device writes the status where
    the device seam reads it."""
    from sweepga_amd.divergence import _call
    from sweepga_amd.lift import cigar_set
    from tests.test_gpu_alnstats import filter_cfgs
    from tests.test_gpu_place import filter_on_the_device
    rng = np.random.default_rng(9)
    n, n_seq = 20_000, 12
    cols, strand, texts = random_case(rng, n, n_seq)
    lines = []
    for i in range(n):
        lines.append("\t".join(["g%d#1#c" % cols["q_id"][i], "400000", str(cols["q_start"][i]), str(cols["q_end"][i]), "-" if strand[i] else "+",
                                "g%d#1#c" % cols["t_id"][i], "400000", str(cols["t_start"][i]), str(cols["t_end"][i]), "50", "60", "60"]))
    roll = rng.random(n)
    cig = {i: (corrupt(texts[i], rng) if roll[i] < 0.05 else texts[i]) for i in range(n) if roll[i] >= 0.10 or roll[i] < 0.05}
    recs = sorted(cig)
    record, offset, text = cigar_set(recs, [cig[i] for i in recs])
    ctx = sw.default_context()
    assert "strand" in FILTER_COLS
    with sw.PafFile(text="\n".join(lines) + "\n") as paf:
        pcols = {c: paf.column(c).copy() for c in COLS}      # (the handle's ids: names in order of first appearance)
        pstrand, p_seq = paf.column("strand").copy(), int(paf.records.n_seq)
        genome = (np.arange(p_seq) // 2).astype(np.uint32)
        seq_len = np.full(p_seq, 400_000, dtype=np.uint32)
        hip = Hip()
        try:
            rec, d_status, status = filter_on_the_device(sw, paf, filter_cfgs(sw)["one_to_one"], hip)
            assert 0 < int((status != 0).sum()) < n
            d = [hip.up(a) for a in (seq_len, genome, record, offset, np.concatenate([text, np.zeros(16, dtype=np.uint8)]))]
            usable = []
            for set_, axis, window in ((1, 0, 10_000), (0, 1, 4_096)):
                dev = _call(ctx, ctx.lib.swg_divergence_records_device, rec, d[0], d[1], (p_seq + 1) // 2, d_status, (d[2], d[3], d[4]), len(recs), set_, axis,
                            window, None, 3)
                want = vm.divergence(pcols, pstrand, seq_len, genome, cig, status != 0, set_, axis, window)
                compare(dev, want, ("filter", set_, axis))
                host = both_seams(sw, pcols, pstrand, seq_len, genome, (p_seq + 1) // 2, cig, status, set_, axis, window)
                assert same(dev, host) and dev.cigar_bad > 0.03 * len(cig) and len(dev.rows) > 400
                usable.append(dev.usable)
            assert usable[1] > 10_000 and 0 < usable[0] < usable[1]
        finally:
            hip.free()


def test_the_texts_the_python_class_and_the_command_line_for_every_batch_size(sw, tmp_path):
    from sweepga_amd import build
    rng = np.random.default_rng(10)
    text = tagged_paf(rng, 3_000)
    inp = tmp_path / "in.paf"
    inp.write_text(text, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-jump", "10k", "--scaffold-mass", "2k"]
    plain, out, rows, summ, w0, w1, d0, d1, r0_, r1_ = (tmp_path / x for x in ("plain.paf", "out.paf", "v.tsv", "vs.tsv", "w0.tsv", "w1.tsv", "d0.tsv", "d1.tsv",
                                                                                  "r0.tsv", "r1.tsv"))
    beside = lambda w, d, r: ["--windows", str(w), "--diffs-summary", str(d), "--diffs", str(r)]      # noqa: E731
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), *beside(w0, d0, r0_), *flags, "--quiet"], capture_output=True)
    assert r0.returncode == 0 and plain.stat().st_size > 0, r0.stderr
    kept = kept_mask(text, plain.read_bytes().decode())
    st = kept.astype(np.uint8)
    one_record = min(len(t) for t in (em.last_cigar_tag(ln) or "" for ln in text.split("\n") if ln) if t)
    with sw.PafFile(text=text) as paf:
        for set_, axis, window, genome in ((1, 0, 10_000, None), (0, 1, 777, "g2#1"), (0, 0, 50_000, "g4#1#")):
            want = vm.paf_texts(text, kept, set_, axis, window, genome)
            assert want[2]["usable"] > 20 and want[2]["bad"] > 0 and want[2]["untagged"] > 0 and want[2]["windows"] > 8
            got = [sw.Divergence.from_paf(paf, st, set=set_, axis=("query", "target")[axis], window=window, genome=genome, batch_bytes=b)
                   for b in (1, max(one_record, 2), 4_096, 0)]
            for g in got:
                assert (g.text, g.summary_text) == want[:2], (set_, axis)
                assert {k: v for k, v in g.counts.items() if k != "batches"} == want[2]
            batches = [g.counts["batches"] for g in got]
            # (one byte per batch: one record per batch, but for the empty entries that follow one another)
            assert want[2]["records"] >= batches[0] > 0.8 * want[2]["records"] and batches[0] >= batches[1] > batches[2] > batches[3] == 1
            assert len(got[0].rows) == want[2]["windows"] and len(got[0].summary) == want[2]["seqs"]
        with pytest.raises(sw.SwgError) as e:
            sw.Divergence.from_paf(paf, st, genome="nobody#0")
        assert e.value.code == -1 and "nobody#0" in str(e.value)
        assert sw.Divergence.from_paf(paf, None, set="all").text == vm.paf_texts(text, None, 0)[0]
    # the command line: after the filter; the PAF, the windows and the difference summary beside it do not change
    for extra, args in (([], (1, 0, 10_000, None)),
                        (["--divergence-set", "all", "--divergence-axis", "target", "--divergence-window", "5k", "--divergence-genome", "g3#1", "--divergence-batch", "2k"],
                         (0, 1, 5_000, "g3#1"))):
        want = vm.paf_texts(text, kept, *args)
        r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--divergence", str(rows), "--divergence-summary", str(summ), *beside(w1, d1, r1_),
                            *extra, *flags], capture_output=True)
        assert r.returncode == 0 and r.stdout == b"" and out.read_bytes() == plain.read_bytes(), r.stderr
        assert w1.read_bytes() == w0.read_bytes() and d1.read_bytes() == d0.read_bytes() and r1_.read_bytes() == r0_.read_bytes()
        assert w0.stat().st_size > 100 and d0.stat().st_size > 100 and r0_.stat().st_size > 1_000
        c = want[2]
        assert rows.read_text() == want[0] and summ.read_text() == want[1]
        assert ("--divergence: %d windows on %d sequences from %d usable entries of %d records, %d bad, %d without a cg:Z: tag\n"
                % (c["windows"], c["seqs"], c["usable"], c["records"], c["bad"], c["untagged"])) in r.stderr.decode()
    rows.unlink()
    r = subprocess.run([build.CLI, str(inp), "--divergence-summary", "-", "--no-filter", "--quiet", "--divergence-window", "50k"], capture_output=True)
    assert r.returncode == 0 and r.stderr.decode() == vm.paf_texts(text, None, 0, 0, 50_000)[1] and not rows.exists(), r.stderr
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--divergence", str(rows), "--divergence-genome", "nobody", *flags], capture_output=True)
    assert r.returncode == 3 and b"unknown genome 'nobody'" in r.stderr
