"""pair_finish with its loads requested ahead (csrc/swg_pair.hip): the ranked body asks for the chunk stretch, its
first round of hd and its first capture positions at the kernel's top, for round r + 1 of the anchors loop before round r is
turned into results, for the '+' triples of every round together, and for the capture's positions one round ahead.  What can go
wrong is a round boundary, a clamp or a value requested before the store it should have seen -- so the shapes are the rounds of
the three size classes (4,096 / 1,024 / 256 positions) with and without dead records, '-' counts around the thread counts, kept
'+' chain counts around a round of the triples and around the LDS list, chunk stretches around the first wavefront's 64 and the
form's 128, and the flag sets under which the other body runs in the same launch.  Every case is held to the CPU oracle record
for record by run_both; inputs hold more than 65,536 records (the plan over runs), 5,000-record pairs fill them.  -m gpu only."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import gen, orc
from tests.test_gpu_pair_columns import SPAN, launched
from tests.test_gpu_pair_ranked import (GAP, KP, MAX_CHUNKS, chain_at, check_mixed, chunks_of, marked, mixed_input, named, pair_bounds,
                                        planted, sparse)
from tests.test_gpu_pair_sort_split import concat, with_strands
from tests.test_gpu_pairs import run_both

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 600
FLOOR = {"min_identity": 0.8}                                   # records below it are dead: m < n
MANY_CHAINS = {"scaffold_gap": 5_000, "min_scaffold_length": 1}  # every chain passes
ROUND_SIZES = {
    "large": [4_097, 8_192, 8_193, 12_288],                      # rounds of 4,096 positions (512 threads, 8 rows)
    "middle": [1_025, 2_048, 2_049, 4_096],                      # 1,024 (256 threads, 4 rows)
    "small": [1, 2, 63, 64, 65, 256, 257, 1_024],                # 256 (64 threads, 4 rows)
}
LABELS = {"large": "pair_finish", "middle": "pair_finish_m", "small": "pair_finish_s"}


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context(0)
    return sweepga_amd


# ---- inputs --------------------------------------------------------------------------------------------------------------
def filled(rng, parts, front=False, fill_pairs=1):
    """parts, and 5,000-record pairs -- at least fill_pairs of them -- until the input holds more than 65,536 records (behind the
    parts, or in front of them)."""
    have = sum(len(p) for p in parts)
    fill = sparse(rng, [5_000] * max(fill_pairs, -(-(65_537 - have) // 5_000)), "fill")
    rec = concat([fill] + parts if front else parts + [fill])
    assert len(rec) > 65_536
    return rec


def rounds_input(cls):
    rng = np.random.default_rng(len(cls) + 4_096)
    rec = filled(rng, [sparse(rng, ROUND_SIZES[cls], cls)])
    assert [hi - lo for lo, hi in pair_bounds(rec)][:len(ROUND_SIZES[cls])] == ROUND_SIZES[cls]
    return rec


def strands_input():
    """Pairs of 1,000 / 4,000 / 5,000 records (64, 256 and 512 threads) with NT - 1, NT and NT + 1 '-' records; a pair that is all
    '+' (no capture position, although the first ones were requested), one that is all '-' (no kept '+' chain), one whose only
    '-' record is its last position; the LAST pair of the input has 513 '-' records."""
    rng = np.random.default_rng(513)
    sizes, minus = [], []
    for n, nt in ((1_000, 64), (4_000, 256), (5_000, 512)):
        for k in (nt - 1, nt, nt + 1):
            sizes.append(n)
            minus.append(k)
    sizes += [5_000, 5_000, 5_000]
    minus += [0, 5_000, 1]
    a = sparse(rng, sizes, "s")
    last = sparse(rng, [5_000], "last")
    lo = 0
    for n, k in zip(sizes, minus):
        with_strands(a, lo, lo + n, n - k, rng)
        lo += n
    with_strands(last, 0, 5_000, 5_000 - 513, rng)
    rec = filled(rng, [a, last], front=True)
    b = pair_bounds(rec)
    got = [int((rec.strand[lo:hi] == ord("-")).sum()) for lo, hi in b[-len(sizes) - 1:]]
    assert got == minus + [513], got
    return rec


def chains_pair(n_chains, links, tag, inv_every=1):
    """n_chains planted '+' chains of `links` collinear records, 60 kb apart, and a 600-base '-' record on the diagonal of every
    inv_every-th chain, between its first two links (capture_input's construction)."""
    step = 60_000 if links > 2 else 30_000
    q0 = 1_000_000 + step * np.arange(n_chains)
    assert n_chains == 0 or int(q0[-1]) + 40_000 < SPAN
    parts = [chain_at(int(q), links=links) for q in q0]
    parts.append(planted(q0[::inv_every] + 3_200, 600, 500, "-"))
    return named(concat(parts), tag)


KEPT_COUNTS = [(1, 2), (511, 9), (512, 9), (513, 9), (4_096, 2), (4_097, 2)]   # kept '+' chains of a pair, links per chain


def kept_chains_input():
    """Pairs with exactly 1, 511, 512, 513 (a round of 512 threads; nine links each, so the pair is of the large class), 4,096 and
    4,097 (the LDS list) planted '+' chains and nothing else on '+', '-' records on the chains' diagonals; in front a pair that
    is all '-' (no kept '+' chain with '-' records present)."""
    rng = np.random.default_rng(4_097)
    none = sparse(rng, [5_000], "none")
    with_strands(none, 0, 5_000, 0, rng)
    parts = [none] + [chains_pair(n, links, f"k{n}", inv_every=1 if n <= 513 else 8) for n, links in KEPT_COUNTS]
    rec = filled(rng, parts)
    sizes = [hi - lo for lo, hi in pair_bounds(rec)]
    assert sizes[2] > 4_096 and sizes[5] > 4_096, sizes[:8]     # the large class
    return rec, pair_bounds(rec)[1:1 + len(KEPT_COUNTS)]


def short_records(rng, n, n_plus, tag):
    """n records of at most 400 bases on 150 Mbp, n_plus of them on '+': at a gap of 100 bases units are a few members long
    whatever n is."""
    r = gen.random_records(rng, n, n_genomes=1, chrs_per_genome=1, span=SPAN, max_len=400, minus_frac=0.0, zero_frac=0.0, self_frac=0.0)
    with_strands(r, 0, n, n_plus, rng)
    return named(r, tag)


STRETCH_CFG = {"scaffold_gap": 100, "min_scaffold_length": 1}
STRETCHES = {                                                    # (records, '+' records) per pair -> chunks per pair
    "up_to_65": ([(1_000, 1_000), (800, 500), (65_536, 65_536), (65_537, 65_537)], [1, 2, 64, 65]),
    "128_129": ([(131_072, 131_072), (131_073, 131_073)], [128, 129]),
}


def stretch_input(key):
    rng = np.random.default_rng(129)
    shapes, want = STRETCHES[key]
    # (the pair stage takes an input whose pairs hold at most 32,768 records on average: eight filling pairs bring the two long ones there)
    rec = filled(rng, [short_records(rng, n, n_plus, f"c{k}") for k, (n, n_plus) in enumerate(shapes)], fill_pairs=8)
    b = pair_bounds(rec)
    assert len(rec) // len(b) <= 32_768
    b = b[:len(shapes)]
    got = [len(chunks_of(rec, lo, hi, STRETCH_CFG["scaffold_gap"])) for lo, hi in b]
    assert got == want, got
    mk = marked(rec, STRETCH_CFG["scaffold_gap"])
    assert mk[:len(shapes)] == [c <= MAX_CHUNKS for c in want] and all(mk[len(shapes):]), mk
    return rec


@pytest.fixture(scope="module")
def mixed():
    return mixed_input()


# ---- the cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [{}, FLOOR, dict(MANY_CHAINS, **FLOOR)], ids=["default", "floor", "many_floor"])
@pytest.mark.parametrize("cls", list(ROUND_SIZES))
def test_rounds_of_the_anchors_loop(sw, cls, cfg):
    rec = rounds_input(cls)
    assert all(marked(rec, cfg.get("scaffold_gap", GAP)))
    if "min_identity" in cfg:                                    # (dead records in the pairs of the class: m < n)
        lo, hi = pair_bounds(rec)[len(ROUND_SIZES[cls]) - 1]
        assert (rec.identity[lo:hi] < cfg["min_identity"]).any() and (rec.identity[lo:hi] >= cfg["min_identity"]).any()
    _, ch, _ = run_both(sw, rec, cfg, expect_pair_path=True)
    assert (ch != 0).any()
    launched(sw, LABELS[cls], "pair_finish")


@pytest.mark.parametrize("cfg", [{}, MANY_CHAINS], ids=["default", "many"])
def test_minus_counts_around_the_thread_counts(sw, cfg):
    rec = strands_input()
    assert all(marked(rec, cfg.get("scaffold_gap", GAP)))
    st, _, _ = run_both(sw, rec, cfg, expect_pair_path=True)
    lo, hi = pair_bounds(rec)[-1]
    assert (st[lo:hi] != 0).any()                               # (the last pair of the input keeps something)
    launched(sw, "pair_finish", "pair_finish_m", "pair_finish_s")


@pytest.mark.parametrize("cfg", [MANY_CHAINS, dict(MANY_CHAINS, min_scaffold_length=1_000)], ids=["every_chain", "capture"])
def test_kept_plus_chain_counts(sw, cfg):
    """min_scaffold_length 1: every chain passes, the '-' records are chains of their own (anchors: the capture skips them all).
    min_scaffold_length 1,000: the same '+' chains, and the 600-base '-' records are left to the capture, which takes them."""
    rec, bounds = kept_chains_input()
    assert all(marked(rec, cfg["scaffold_gap"]))
    st, ch, _ = run_both(sw, rec, cfg, expect_pair_path=True)    # (st / ch are the oracle's too)
    for (lo, hi), (n, _) in zip(bounds, KEPT_COUNTS):
        plus = rec.strand[lo:hi] == ord("+")
        assert len(np.unique(ch[lo:hi][plus])) == n and (ch[lo:hi][plus] != 0).all(), n
        assert (~plus).any() and (st[lo:hi][~plus] != 0).all(), n
        if cfg["min_scaffold_length"] > 600:                     # captured: each '-' record carries the number of a '+' chain
            assert np.isin(ch[lo:hi][~plus], ch[lo:hi][plus]).all(), n
    assert KEPT_COUNTS[-1][0] > KP >= KEPT_COUNTS[-2][0]
    launched(sw, "pair_finish", "pair_finish_s")


@pytest.mark.parametrize("key", list(STRETCHES))
def test_chunk_stretches(sw, key):
    rec = stretch_input(key)
    _, ch, _ = run_both(sw, rec, STRETCH_CFG, expect_pair_path=True)
    for lo, hi in pair_bounds(rec)[:len(STRETCHES[key][0])]:
        assert len(np.unique(ch[lo:hi])) > (hi - lo) // 4         # (chains are kept all along the stretch)
    launched(sw, "pair_finish")


OTHER_BODY = [{}, {"scaffold_max_deviation": 20_000}, {"scaffold_filter_mode": "OneToOne"}, {"mapping_filter_mode": "OneToOne"}]


@pytest.mark.parametrize("cfg", OTHER_BODY, ids=["default", "rescue", "chain_table", "mapping_sweep"])
def test_the_other_body_in_the_same_launch(sw, mixed, cfg):
    check_mixed(mixed, GAP)
    run_both(sw, mixed, cfg, expect_pair_path=True)
    launched(sw, "pair_finish", "pair_finish_m", "pair_finish_s")


def test_form_off_gives_the_same_columns(sw):
    """A child process with SWG_PAIR_RANKED=0 (the knob is read once per process): every pair takes the first body."""
    got = []
    for rec, cfg in child_inputs():
        st, ch, _ = run_both(sw, rec, cfg, expect_pair_path=True)
        got.append([st.tolist(), ch.tolist()])
    out = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT)], env=dict(os.environ, SWG_PAIR_RANKED="0"),
                         capture_output=True, text=True, cwd=ROOT, timeout=CHILD_TIMEOUT)
    assert out.returncode == 0 and "ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    off = json.loads(next(line[7:] for line in out.stdout.splitlines() if line.startswith("RESULT ")))
    assert got == off


def test_the_ranked_body_ran_on_the_device(sw):
    """marked() is a model of pair_sort's marks; what pair_finish did is read back from the device: a child process with SWG_DEBUG
    counts the pairs and records that took the ranked body -- all of them, in both inputs."""
    out = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT)], env=dict(os.environ, SWG_DEBUG="1"),
                         capture_output=True, text=True, cwd=ROOT, timeout=CHILD_TIMEOUT)
    assert out.returncode == 0 and "ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    got = [tuple(map(int, g)) for g in re.findall(r"ranked form: (\d+) of (\d+) pairs, (\d+) of (\d+) records", out.stderr)]
    want = [(len(pair_bounds(rec)),) * 2 + (len(rec),) * 2 for rec, _ in child_inputs()]
    assert got == want, (got, want, out.stderr[-2000:])


# ---- the child process ----------------------------------------------------------------------------------------------------
def child_inputs():
    return [(strands_input(), {}), (kept_chains_input()[0], dict(MANY_CHAINS, min_scaffold_length=1_000))]


def child_columns(sw):
    out = []
    for rec, cfg in child_inputs():
        st, ch, _ = run_both(sw, rec, cfg, expect_pair_path=True)
        out.append([st.tolist(), ch.tolist()])
    print("RESULT " + json.dumps(out))


CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import sweepga_amd
sweepga_amd.default_context(0)
from tests import test_gpu_pair_finish_loads as T
T.child_columns(sweepga_amd)
print("ok")
"""
