"""pair_sort over the third size class in two launches (csrc/swg_pair.hip): pair_order leaves the pairs of more
than T records as an exact prefix of the class's list; those and the very long pairs stay with pair_sort_big (1,024 threads, a CU
each), the pairs of at most T records go to pair_sort_mx (512 threads, two work-groups to a CU).  The chunk list of the walk is
written by a wavefront, a lane per cell.  What can go wrong: a pair on the wrong side of the cut, a pair sorted twice or not at all,
the second batch of a pair under the 512-thread instance (SWG_PAIR_MX_MAX=16384: members beyond its 8,192-member batch), and a
chunk with a wrong begin, end or strand bit around the '+' / '-' boundary.  (With the cut that ships, 8,192, a pair's members
fit one batch of the instance, so no coarse bin can be denser than its batch.)  Every case is held to the CPU oracle record for record and reads the launch table.
Inputs hold more than 65,536 records (the plan over runs, not the hash grouping) on 150 Mbp sequences.  -m gpu only."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import gen, orc
from tests.test_gpu_pair_columns import COLS, SPAN, launched, pairs_of
from tests.test_gpu_pairs import run_both

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 600
T = 8_192          # the cut that ships (PAIR_MX_CUT_DEFAULT)
T_MAX = 16_384     # what the 512-thread instance holds (PAIR_MX_MAX): two batches of 8,192 members
BATCH = 8_192
THREE_CONFIGS = [{}, {"scaffold_gap": 60_000, "min_scaffold_length": 3_000}, {"min_scaffold_identity": 0.9}]


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context(0)
    return sweepga_amd


def cut_sizes(t):
    sizes = sorted({4_097, 8_192, 8_193, t, t + 1, 32_768})
    return sizes if sum(sizes) > 65_536 else sizes + [20_000]


def cut_input(t=T):
    return pairs_of(np.random.default_rng(t), cut_sizes(t))


def sort_labels(table):
    return sorted(k for k in table if k.startswith("pair_sort"))


@pytest.mark.parametrize("cfg", THREE_CONFIGS)
def test_the_cut(sw, cfg):
    """Pairs of 4,097, 8,192, 8,193, T, T + 1 and 32,768 records in one input: both launches, the oracle's answers with three,
    three and five columns through the buffers."""
    run_both(sw, cut_input(), cfg, expect_pair_path=True)
    launched(sw, "pair_sort_big", "pair_sort_mx", "pair_order")


def test_only_small_side_pairs(sw):
    rec = pairs_of(np.random.default_rng(7000), [7_000] * 10)
    run_both(sw, rec, {}, expect_pair_path=True)
    table = launched(sw, "pair_sort_mx")
    assert "pair_sort_big" not in table, sort_labels(table)


def test_only_large_side_pairs(sw):
    rec = pairs_of(np.random.default_rng(20000), [20_000] * 4)
    run_both(sw, rec, {}, expect_pair_path=True)
    table = launched(sw, "pair_sort_big")
    assert "pair_sort_mx" not in table, sort_labels(table)


def test_cut_behind_a_mapping_sweep(sw):
    """Members are fewer than records; the alive non-members ride behind them."""
    rec = cut_input()
    for cfg in ({"mapping_filter_mode": "OneToOne"}, {"mapping_filter_mode": "OneToOne", "scaffold_gap": 40_000, "min_scaffold_length": 2_000}):
        _, _, stats = run_both(sw, rec, cfg, expect_pair_path=True)
        assert 0 < int(stats.n_swept) < int(stats.n_retained)
        launched(sw, "pair_sort_big", "pair_sort_mx")


# ---- the chunk list ------------------------------------------------------------------------------------------------------
def with_strands(rec, lo, hi, n_plus, rng):
    """Records [lo, hi) of rec: exactly n_plus of them on '+', the others on '-' (which ones: random)."""
    s = np.full(hi - lo, ord("-"), dtype=np.uint8)
    s[rng.choice(hi - lo, n_plus, replace=False)] = ord("+")
    rec.strand[lo:hi] = s
    return rec


def dense_pair(rng, n, k):
    """One pair whose records lie 1 kb apart on average: under a gap of 100 kb every start is within reach of an earlier end, so
    the strand's members are ONE unit (test_chunk_list checks that)."""
    r = gen.random_records(rng, n, n_genomes=1, chrs_per_genome=1, span=n * 1_000, minus_frac=0.0, zero_frac=0.0, self_frac=0.0)
    r.qname = [f"d{k}#1#c"] * n
    r.tname = [f"e{k}#1#c"] * n
    return r


def concat(parts):
    total = sum(len(r) for r in parts)
    return orc.Records(sum((r.qname for r in parts), []), sum((r.tname for r in parts), []),
                       *[np.concatenate([getattr(r, c) for r in parts]) for c in COLS], np.arange(total, dtype=np.uint64))


def units_of(qs, qe, gap):
    """Unit starts of one strand's members in q_start order: a start beyond every earlier end by more than the gap."""
    o = np.argsort(qs, kind="stable")
    qs, qe = qs[o].astype(np.int64), qe[o].astype(np.int64)
    reach = np.maximum.accumulate(qe)
    return np.flatnonzero(np.concatenate(([True], qs[1:] > reach[:-1] + gap)))


def test_chunk_list(sw):
    """Pair 0 (5,000 records): exactly 2,048 '+' members, so the first '-' member is the first member of cell 2 -- the cell's first
    unit start coincides with m_plus.  Pair 1 (7,000): 3,000 '+' members, the boundary inside cell 2.  Pair 2 (12,000, all '+', 1 kb
    apart): one unit of 12,000 members, at least the 9,216 of a long-list entry.  Pairs 3 and 4 fill the input."""
    rng = np.random.default_rng(2048)
    gap = 100_000
    a = pairs_of(rng, [5_000, 7_000])
    with_strands(a, 0, 5_000, 2_048, rng)
    with_strands(a, 5_000, 12_000, 3_000, rng)
    d = dense_pair(rng, 12_000, 0)
    assert units_of(d.qs, d.qe, gap).tolist() == [0] and len(d) >= 9_216      # (the docstring's long unit, checked here)
    rest = pairs_of(rng, [20_000, 30_000])
    rest.qname = [q.replace("a", "f") for q in rest.qname]
    rest.tname = [t.replace("b", "h") for t in rest.tname]
    rec = concat([a, d, rest])
    assert len(rec) > 65_536
    assert int((rec.strand[:5_000] == ord("+")).sum()) == 2_048 and int((rec.strand[5_000:12_000] == ord("+")).sum()) == 3_000
    for cfg in ({"scaffold_gap": gap}, {"scaffold_gap": gap, "min_scaffold_length": 2_000, "min_scaffold_identity": 0.8}):
        run_both(sw, rec, cfg, expect_pair_path=True)
        launched(sw, "pair_sort_big", "pair_sort_mx")


def test_chunk_list_of_a_very_long_pair(sw):
    """A pair of 70,000 records (the XL body: 256 cells, which the wavefront takes 64 at a time) with exactly 65,536 '+' members:
    the first '-' member is the first member of cell 64, so the chunk that ends at m_plus takes its begin from the carry across
    the first group of 64 cells; and one with 60,000 '+' members, the boundary inside cell 58.  (Three shorter pairs keep the
    average below the 32,768 records per pair that the pair path admits.)"""
    rng = np.random.default_rng(65536)
    rec = pairs_of(rng, [70_000, 5_000, 5_000, 300])
    for n_plus in (65_536, 60_000):
        with_strands(rec, 0, 70_000, n_plus, rng)
        run_both(sw, rec, {"scaffold_gap": 20_000}, expect_pair_path=True)
        launched(sw, "pair_sort_big", "pair_sort_mx", "pair_sort_s")


# ---- cases that need an environment knob: read once per process, so a child of its own ------------------------------------------
def two_batch_input():
    """Pairs under the 512-thread instance whose members do not fit its batch of 8,192: 8,193 and 16,384 members; 12,000 all on
    '-'; 14,000 all on '+' with 2,500 equal starts around the 8,192nd member, where the first batch ends; 16,000 to fill."""
    rng = np.random.default_rng(8193)
    rec = pairs_of(rng, [8_193, 16_384, 12_000, 14_000, 16_000], all_minus=2)
    lo = 8_193 + 16_384 + 12_000
    with_strands(rec, lo, lo + 14_000, 14_000, rng)
    ln = rec.qe[lo:lo + 14_000] - rec.qs[lo:lo + 14_000]
    o = np.argsort(rec.qs[lo:lo + 14_000], kind="stable")
    tie = rec.qs[lo + o[BATCH]]
    rec.qs[lo + o[7_000:9_500]] = tie
    rec.qe[lo:lo + 14_000] = rec.qs[lo:lo + 14_000] + ln
    assert int((rec.qs[lo:lo + 14_000] == tie).sum()) >= 2_500 and len(rec) > 65_536
    return rec


def child_two_batches(sw):
    rec = two_batch_input()
    for cfg in THREE_CONFIGS:
        run_both(sw, rec, cfg, expect_pair_path=True)
        table = launched(sw, "pair_sort_mx")
        assert "pair_sort_big" not in table, sort_labels(table)      # (every pair at most T_MAX records)
    run_both(sw, cut_input(T_MAX), {}, expect_pair_path=True)
    launched(sw, "pair_sort_mx", "pair_sort_big")


def child_single_launch(sw):
    for cfg in ({}, {"min_scaffold_identity": 0.9}):
        run_both(sw, cut_input(), cfg, expect_pair_path=True)
        table = launched(sw, "pair_sort_big")
        assert "pair_sort_mx" not in table, sort_labels(table)


CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import sweepga_amd
sweepga_amd.default_context(0)
from tests import test_gpu_pair_sort_split as T
for name in %(cases)r:
    getattr(T, name)(sweepga_amd)
print("ok")
"""


def in_child(env, *cases):
    out = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, cases=list(cases))], env=dict(os.environ, **env),
                         capture_output=True, text=True, cwd=ROOT, timeout=CHILD_TIMEOUT)
    assert out.returncode == 0 and "ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    return out.stderr


def child_cut(sw):
    run_both(sw, cut_input(), {}, expect_pair_path=True)


def test_which_pair_goes_where():
    """SWG_DEBUG=1 prints how many pairs each launch took: of 4,097, 8,192, 8,193, 20,000 and 32,768 records the first two go to
    pair_sort_mx and three stay (a pair on the wrong side, or a prefix off by a bin, would still be sorted correctly)."""
    sizes = cut_sizes(T)
    small = sum(1 for n in sizes if n <= T)
    err = in_child({"SWG_DEBUG": "1"}, "child_cut")
    assert f"pair_sort: {len(sizes) - small} pairs under pair_sort_big, {small} under pair_sort_mx (cut {T})" in err, err[-2000:]
    err = in_child({"SWG_DEBUG": "1", "SWG_PAIR_MX_MAX": "8400"}, "child_cut")      # rounded down to 65 x 128: 8,193 now on the short side
    assert f"pair_sort: {len(sizes) - small - 1} pairs under pair_sort_big, {small + 1} under pair_sort_mx (cut 8320)" in err, err[-2000:]


def test_two_batches_under_the_512_thread_instance():
    """SWG_PAIR_MX_MAX=16384: the instance's own limit as the cut."""
    in_child({"SWG_PAIR_MX_MAX": str(T_MAX)}, "child_two_batches")


def test_pair_order_off_keeps_the_single_launch():
    """SWG_PAIR_ORDER=0: list 2 has no ordered prefix, one pair_sort_big launch takes it all, same answers."""
    in_child({"SWG_PAIR_ORDER": "0"}, "child_single_launch")


def test_split_off_keeps_the_single_launch():
    in_child({"SWG_PAIR_MX_MAX": "0"}, "child_single_launch")
