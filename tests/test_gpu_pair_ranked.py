"""The ranked form of the pair stage (csrc/swg_pair.hip, csrc/swg_chain_table.hip): under the default flags a pair
whose chunks all fit the labelling's LDS layout (at most 1,536 elements each) has its kept chains ranked by chain_label where it
labels them, and pair_finish numbers the pair from the chunks' counts instead of ranking the chains again.  What can go wrong: a
pair marked that should not be (or the reverse), a rank off by a chunk's base, a '+' / '-' boundary in the wrong chunk, a chain
list of the inversion capture with a wrong or missing triple -- in LDS, or in memory beyond 4,096 kept '+' chains -- and a flag
set that takes the form although a passing chain is not a kept chain there.  Every case is held to the CPU oracle record for
record; which pairs are marked is worked out here from the records (chunks_of) and, in a child process with SWG_DEBUG, read back
from the device.  Inputs hold more than 65,536 records (the plan over runs) on 150 Mbp sequences.  -m gpu only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import orc
from tests.test_gpu_pair_columns import launched, pairs_of
from tests.test_gpu_pair_sort_split import concat, dense_pair, units_of, with_strands
from tests.test_gpu_pairs import run_both

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 600
GAP = 50_000          # FilterConfig's scaffold_gap
CELL = 1_024          # PAIR_CELL: the first unit start of every cell of this many members opens a chunk
FAST = 1_536          # LABEL_FAST: the longest chunk that is labelled in LDS
LONG = 9_216          # LABEL_CAP_ELEMS: a chunk of this many members is a long unit (the side stream's leg)
MAX_CHUNKS = 128      # RANKED_MAX_CHUNKS
KP = 4_096            # kept '+' chains that pair_finish's large class holds in LDS
MIXED_CONFIGS = [{}, {"scaffold_gap": 100_000, "min_scaffold_length": 2_000}]
OFF_CONFIGS = [{"scaffold_max_deviation": 20_000}, {"scaffold_filter_mode": "OneToOne"}, {"min_scaffold_identity": 0.9},
               {"mapping_filter_mode": "OneToOne"}]


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context(0)
    return sweepga_amd


# ---- inputs --------------------------------------------------------------------------------------------------------------
def named(rec, tag):
    rec.qname = [f"{tag}q#1#c"] * len(rec)
    rec.tname = [f"{tag}t#1#c"] * len(rec)
    return rec


def sparse(rng, sizes, tag, **kw):
    """Pairs of random records on 150 Mbp: 5,000 of them lie 30 kb apart, so units are a handful of members long."""
    return concat([named(pairs_of(rng, [n], **kw), f"{tag}{k}") for k, n in enumerate(sizes)])


def planted(qs, ln, diag, strand):
    """Records of given starts and lengths on the diagonal t = q + diag."""
    qs, ln = np.asarray(qs, dtype=np.uint64), np.asarray(ln, dtype=np.uint64) + np.zeros(len(qs), dtype=np.uint64)
    m = np.floor(0.9 * ln).astype(np.uint64)
    n = len(qs)
    return orc.Records([""] * n, [""] * n, qs, qs + ln, qs + np.uint64(diag), qs + np.uint64(diag) + ln, ln, m / ln, m,
                       np.full(n, ord(strand), dtype=np.uint8), np.arange(n, dtype=np.uint64))


def chain_at(q0, diag=500, links=6, ln=3_000, step=4_000):
    """Collinear '+' records 1 kb apart: one chain of links * step - 1,000 bases."""
    return planted(q0 + step * np.arange(links), ln, diag, "+")


def pair_bounds(rec):
    key = list(zip(rec.qname, rec.tname))
    cut = [0] + [i for i in range(1, len(key)) if key[i] != key[i - 1]] + [len(key)]
    return list(zip(cut[:-1], cut[1:]))


def chunks_of(rec, lo, hi, gap):
    """Chunk lengths of the pair [lo, hi) when every record is a member: '+' members first, each strand in q_start order; the
    first unit start of every 1,024-member cell opens a chunk, and so does the first '-' member."""
    plus = rec.strand[lo:hi] == ord("+")
    starts, off = [], 0
    for sel in (plus, ~plus):
        if sel.any():
            starts.append(off + units_of(rec.qs[lo:hi][sel], rec.qe[lo:hi][sel], gap))
            off += int(sel.sum())
    us = np.concatenate(starts)
    begins = us[np.concatenate(([True], us[1:] // CELL != us[:-1] // CELL))]
    m_plus = int(plus.sum())
    if 0 < m_plus < hi - lo:
        begins = np.union1d(begins, [m_plus])
    return np.diff(np.concatenate((begins, [hi - lo])))


def marked(rec, gap):
    """Per pair: every chunk at most 1,536 elements long, at most 128 of them."""
    out = []
    for lo, hi in pair_bounds(rec):
        c = chunks_of(rec, lo, hi, gap)
        out.append(bool(c.max() <= FAST and len(c) <= MAX_CHUNKS))
    return out


def mixed_input():
    """Thirteen sparse pairs of every size class, a pair that is one unit of 12,000 members (the long leg) and one that is one
    unit of 3,000 (a chunk between 1,537 and 9,215 elements: chain_label's path for long chunks)."""
    rng = np.random.default_rng(1536)
    a = sparse(rng, [5_000, 4_097, 4_096, 1_025, 1_024, 600, 5_000, 5_000, 4_800, 4_500, 5_000, 3_000, 5_000], "s")
    return concat([a, named(dense_pair(rng, 12_000, 0), "long"), named(dense_pair(rng, 3_000, 1), "mid"), sparse(rng, [5_000], "z")])


def check_mixed(rec, gap):
    assert len(rec) > 65_536
    bounds, mk = pair_bounds(rec), marked(rec, gap)
    assert len(bounds) == 16 and mk == [True] * 13 + [False, False, True], mk
    assert chunks_of(rec, *bounds[13], gap).max() >= LONG
    assert FAST < chunks_of(rec, *bounds[14], gap).max() < LONG
    return bounds, mk


@pytest.fixture(scope="module")
def mixed():
    return mixed_input()


# ---- the cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", MIXED_CONFIGS)
def test_mixed_input(sw, mixed, cfg):
    check_mixed(mixed, cfg.get("scaffold_gap", GAP))
    _, ch, _ = run_both(sw, mixed, cfg, expect_pair_path=True)
    assert len(np.unique(ch[ch != 0])) >= 10      # (chains are kept: the numbering is exercised)
    launched(sw, "chain_label", "chain_label_long", "pair_finish", "pair_finish_m", "pair_finish_s")


def edge_input():
    """Thirteen sparse pairs, then two pairs that are ONE '+' unit each (records 1 kb apart): 1,536 members and 1,537."""
    rng = np.random.default_rng(1537)
    rec = concat([sparse(rng, [5_000] * 13, "s"), named(dense_pair(rng, FAST, 0), "fits"), named(dense_pair(rng, FAST + 1, 1), "over")])
    bounds = pair_bounds(rec)
    assert len(rec) > 65_536 and len(bounds) == 15
    for (lo, hi), n in zip(bounds[13:], (FAST, FAST + 1)):
        assert (rec.strand[lo:hi] == ord("+")).all() and chunks_of(rec, lo, hi, GAP).tolist() == [n]
    assert marked(rec, GAP) == [True] * 14 + [False]
    return rec


def test_the_1536_1537_edge(sw):
    rec = edge_input()
    run_both(sw, rec, {}, expect_pair_path=True)
    err = in_child({"SWG_DEBUG": "1"}, "child_edge")
    assert f"ranked form: 14 of 15 pairs, {len(rec) - FAST - 1} of {len(rec)} records" in err, err[-2000:]


def strands_input():
    """Pair 0: exactly 2,048 '+' members (the first '-' member opens cell 2).  1: 3,000 '+' members (the boundary inside a cell).
    2: the first record is on '-' while most are on '+' (the '-' chains are numbered first).  3: all '+'.  4: all '-'.  5: 120
    records of 2 kb, 1 Mbp apart: no chain passes.  6: the same with one planted chain of 23 kb.  7-14 fill the input."""
    rng = np.random.default_rng(2048)
    a = sparse(rng, [5_000, 5_000, 5_000, 4_000, 4_000], "s", minus_frac=0.4)
    with_strands(a, 0, 5_000, 2_048, rng)
    with_strands(a, 5_000, 10_000, 3_000, rng)
    a.strand[10_000] = ord("-")
    with_strands(a, 15_000, 19_000, 4_000, rng)
    with_strands(a, 19_000, 23_000, 0, rng)
    lone = planted(1_000_000 * np.arange(1, 121), 2_000, 500, "+")
    lone.strand[::3] = ord("-")
    none = named(concat([lone]), "none")
    one = named(concat([lone, chain_at(70_500_000)]), "one")
    rec = concat([a, none, one, sparse(rng, [5_000] * 9, "z", minus_frac=0.3)])
    assert len(rec) > 65_536 and all(marked(rec, GAP))
    b = pair_bounds(rec)
    assert [int((rec.strand[lo:hi] == ord("+")).sum()) for lo, hi in b[:5]][:2] == [2_048, 3_000]
    assert rec.strand[10_000] == ord("-") and (rec.strand[10_000:15_000] == ord("+")).sum() > 2_000
    assert (rec.strand[15_000:19_000] == ord("+")).all() and (rec.strand[19_000:23_000] == ord("-")).all()
    return rec, b


def test_strands_and_order(sw):
    rec, b = strands_input()
    _, ch, _ = run_both(sw, rec, {}, expect_pair_path=True)
    per_pair = [len(np.unique(ch[lo:hi][ch[lo:hi] != 0])) for lo, hi in b]
    assert per_pair[5] == 0 and per_pair[6] == 1, per_pair[:8]
    assert ch[b[6][1] - 6:b[6][1]].min() > 0                                # (the planted chain is the one)
    lo, hi = b[2]
    both = ch[lo:hi] != 0
    assert (both & (rec.strand[lo:hi] == ord("-"))).any() and (both & (rec.strand[lo:hi] == ord("+"))).any()   # chains on both strands
    _, ch, _ = run_both(sw, rec, {"min_scaffold_length": 3_000}, expect_pair_path=True)
    assert all(len(np.unique(ch[lo:hi][ch[lo:hi] != 0])) > 10 for lo, hi in b[:5])


def capture_input():
    """Pair 0: sixty planted '+' chains 2 Mbp apart, a 600-base '-' record on the diagonal inside each: nothing else, 64-thread
    class.  Pair 1: the same among 4,000 scattered records (the large class).  The rest fills the input."""
    rng = np.random.default_rng(60)
    q0 = 1_000_000 + 2_000_000 * np.arange(60)
    chains = concat([chain_at(int(q)) for q in q0])
    inv = planted(q0 + 11_200, 600, 500, "-")
    p0 = named(concat([chains, inv]), "cap")
    p1 = named(concat([pairs_of(rng, [4_000]), chains, inv]), "capl")
    rec = concat([p0, p1, sparse(rng, [5_000] * 13, "z")])
    assert len(rec) > 65_536 and all(marked(rec, GAP))
    return rec, [np.arange(360, 420), len(p0) + 4_000 + np.arange(360, 420)]


def test_inversion_capture_in_marked_pairs(sw):
    rec, inv = capture_input()
    st, ch, _ = run_both(sw, rec, {}, expect_pair_path=True)
    for idx in inv:      # (run_both: st / ch are the oracle's)
        assert (rec.strand[idx] == ord("-")).all()
        assert int((st[idx] != 0).sum()) >= 36, int((st[idx] != 0).sum())
    idx = inv[0]         # (nothing but the planted chains in pair 0: record 360 + j joins chain j, whose third link is record 6 j + 2)
    assert (ch[idx] == ch[6 * np.arange(60) + 2]).all() and (ch[idx] != 0).all()


def test_more_kept_plus_chains_than_the_lds_list(sw):
    """20,000 records, every chain passes (min_scaffold_length 1) and few records are within 5 kb of another: more than 4,096 kept
    '+' chains in one pair, whose list for the inversion capture then lives in memory."""
    rng = np.random.default_rng(4096)
    cfg = {"scaffold_gap": 5_000, "min_scaffold_length": 1}
    rec = concat([sparse(rng, [20_000], "big"), sparse(rng, [5_000] * 10, "z")])
    plus = rec.strand[:20_000] == ord("+")
    assert len(units_of(rec.qs[:20_000][plus], rec.qe[:20_000][plus], 5_000)) > KP      # every unit holds a chain, every chain passes
    assert len(rec) > 65_536 and all(marked(rec, 5_000)) and chunks_of(rec, 0, 20_000, 5_000).max() <= FAST
    st, ch, _ = run_both(sw, rec, cfg, expect_pair_path=True)
    assert len(np.unique(ch[:20_000][plus])) > KP
    assert (~plus).any() and (st[:20_000][~plus] != 0).all()


def counts(sw):
    return {k: int(v[0]) for k, v in sw.default_context(0).profile_table().items()}


def test_flag_sets_that_do_not_take_the_form(sw, mixed):
    """Rescue, a scaffold filter with limits, an identity floor, a 1:1 mapping sweep: the oracle's answers, and the launch labels
    and counts of a process in which the form is switched off."""
    check_mixed(mixed, GAP)
    got = []
    for cfg in OFF_CONFIGS:
        run_both(sw, mixed, cfg, expect_pair_path=True)
        got.append(counts(sw))
    off = json.loads(in_child({"SWG_PAIR_RANKED": "0"}, "child_off_configs", want="RESULT "))
    assert got == off, [sorted(set(g.items()) ^ set(o.items())) for g, o in zip(got, off)]


def test_knob_off_gives_the_same(sw, mixed):
    """SWG_PAIR_RANKED=0: every pair takes pair_finish's own ranking -- same columns, same launch table."""
    got = []
    for cfg in MIXED_CONFIGS:
        st, ch, _ = run_both(sw, mixed, cfg, expect_pair_path=True)
        got.append([counts(sw), st.tolist(), ch.tolist()])
    off = json.loads(in_child({"SWG_PAIR_RANKED": "0"}, "child_mixed", want="RESULT "))
    for g, o in zip(got, off):
        assert g[0] == o[0], sorted(set(g[0].items()) ^ set(o[0].items()))
        assert g[1] == o[1] and g[2] == o[2]
    err = in_child({"SWG_PAIR_RANKED": "0", "SWG_DEBUG": "1"}, "child_edge")
    assert "ranked form: off" in err and "ranked form: 1" not in err, err[-2000:]


# ---- child processes (the knobs are read once per process) ----------------------------------------------------------------------
def child_edge(sw):
    run_both(sw, edge_input(), {}, expect_pair_path=True)


def child_off_configs(sw):
    rec, out = mixed_input(), []
    for cfg in OFF_CONFIGS:
        run_both(sw, rec, cfg, expect_pair_path=True)
        out.append(counts(sw))
    print("RESULT " + json.dumps(out))


def child_mixed(sw):
    rec, out = mixed_input(), []
    for cfg in MIXED_CONFIGS:
        st, ch, _ = run_both(sw, rec, cfg, expect_pair_path=True)
        out.append([counts(sw), st.tolist(), ch.tolist()])
    print("RESULT " + json.dumps(out))


CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import sweepga_amd
sweepga_amd.default_context(0)
from tests import test_gpu_pair_ranked as T
for name in %(cases)r:
    getattr(T, name)(sweepga_amd)
print("ok")
"""


def in_child(env, *cases, want=None):
    out = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, cases=list(cases))], env=dict(os.environ, **env),
                         capture_output=True, text=True, cwd=ROOT, timeout=CHILD_TIMEOUT)
    assert out.returncode == 0 and "ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    if want is None:
        return out.stderr
    return next(line[len(want):] for line in out.stdout.splitlines() if line.startswith(want))
