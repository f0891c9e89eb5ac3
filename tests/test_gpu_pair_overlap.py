"""The pair-resident stage runs its long-unit leg (pair_long_plan, the speculative rounds, chain_label_long) on a side stream beside
the short-unit kernels (chain_walk, chain_label): csrc/swg_pair.hip, DESIGN.md 3.5b.  SWG_PAIR_OVERLAP=0 keeps one leg after the
other on one stream.  Under both settings -- each in a fresh child process, the knob is read once per process -- status and chain
numbers must equal the CPU oracle's and each other's: on inputs with long units (a unit of 9,216 members or more), on inputs with
large pairs but no long unit, on inputs without large pairs, and on a call the long leg hands over to the global-sort stage on the
device's word.  The launch table must name the long leg's kernels under both settings, and 20 calls in a row on one context must
give the same answer every time, the last one -- made without the profiler's events -- the oracle's again (the join orders the legs).  -m gpu only."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import gen, orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 900   # seconds for one child process (records -> device, up to 20 filter calls)
GLOBAL_STAGE = ("chain_cuts", "cuts_from_scan", "sortA_keys", "sortA_keys_hist", "sortA_words")   # (as tests/test_gpu_pairs.py tells the paths apart)


def _concat(parts):
    rec = parts[0]
    for r in parts[1:]:
        rec = orc.Records(rec.qname + r.qname, rec.tname + r.tname,
                          *[np.concatenate([getattr(rec, c), getattr(r, c)])
                            for c in ("qs", "qe", "ts", "te", "block_length", "identity", "matches", "strand")],
                          np.arange(len(rec) + len(r), dtype=np.uint64))
    return rec


def size_class_pairs():
    """tests/test_gpu_pairs.py::test_one_pair_per_size_class: pairs of 900 .. 40,000 records 3 kb apart, 75,400 records in all (beyond
    the hash grouping: the pairs are the runs of the input).  Under a gap limit of 5 kb and more every pair is one unit: three
    of them have 14,000 to 40,000 members."""
    rng = np.random.default_rng(77)
    parts = []
    for k, n in enumerate([900, 3_500, 14_000, 40_000, 17_000]):
        r = gen.random_records(rng, n, n_genomes=1, chrs_per_genome=1, span=int(n * 3000), minus_frac=0.15, zero_frac=0.0, self_frac=0.0)
        r.qname = [f"a{k}#1#c" for _ in range(n)]
        r.tname = [f"b{k}#1#c" for _ in range(n)]
        parts.append(r)
    return _concat(parts)


def small_pairs():
    """400 pairs of ~225 records: no pair large enough to hold a long unit (the long leg is not enqueued at all)."""
    from tests.test_gpu_pairs import pair_major
    rng = np.random.default_rng(4100)
    return pair_major(gen.random_records(rng, 90_000, n_genomes=5, chrs_per_genome=4, span=300_000, zero_frac=0.0), rng)


def deep_pairs():
    """tests/fuzz/fuzz_large.py's giant_pair_deep (100,000 records over four chromosome pairs of 3 Mb, records of up to 20 kb: hundreds
    of members inside one gap limit), grouped by pair: the long leg finds units it does not take and raises the hand-over flag."""
    from tests.test_gpu_pairs import pair_major
    rng = np.random.default_rng(1000)
    rec = gen.random_records(rng, 100_000, n_genomes=2, chrs_per_genome=1, span=3_000_000, max_len=20_000, syntenic_frac=0.9, zero_frac=0.0)
    return pair_major(rec, rng)


# name -> (records, [(config, what the launch table must show)])
#   "long": long units are walked and labelled;  "no_long": large pairs, no long unit;  "small": no large pair;
#   "handover": started on the pair path, finished by the global-sort stage
CASES = {
    "size_classes": (size_class_pairs, [
        ({}, "long"),
        ({"scaffold_gap": 9_000, "min_scaffold_length": 20_000, "min_scaffold_identity": 0.8}, "long"),          # the weighted identity's columns
        ({"scaffold_filter_mode": "OneToOne", "scaffold_gap": 6_000, "min_scaffold_length": 8_000, "scaffold_max_deviation": 20_000}, "long"),   # the join in front of pair_chains
        ({"scaffold_gap": 400, "min_scaffold_length": 0}, "no_long"),
    ]),
    "small_pairs": (small_pairs, [({"scaffold_gap": 3_000, "min_scaffold_length": 1_000}, "small")]),
    "deep_pairs": (deep_pairs, [({}, "handover")]),
}
REPEATS = 20

CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(root)r)
import sweepga_amd as sw
from tests import gen
from tests.test_gpu_pair_overlap import CASES, REPEATS
name, out_dir = %(name)r, %(out)r
make, configs = CASES[name]
rec = make()
packed = sw.pack_records(gen.records_to_meta(rec))
ctx = sw.default_context(0)
report = []
for k, (kw, kind) in enumerate(configs):
    kwg = {a: (getattr(sw.FilterMode, v) if isinstance(v, str) else v) for a, v in kw.items()}
    f = sw.PafFilter(sw.FilterConfig(**kwg))
    ctx.profile_reset()
    ctx.profile(True)
    st, ch = f.filter_columns(packed)
    ctx.profile(False)
    table = ctx.profile_table()
    np.save(f"{out_dir}/st{k}.npy", st)
    np.save(f"{out_dir}/ch{k}.npy", ch)
    differing = 0
    if kind == "long":                       # the same call again and again on this context
        for _ in range(REPEATS - 1):
            st2, ch2 = f.filter_columns(packed)
            differing += int(not (np.array_equal(st, st2) and np.array_equal(ch, ch2)))
        np.save(f"{out_dir}/st{k}_last.npy", st2)     # (the last call, made without the profiler's events: held to the oracle too)
        np.save(f"{out_dir}/ch{k}_last.npy", ch2)
    report.append({"launches": {a: int(v[0]) for a, v in table.items()}, "differing_repeats": differing})
json.dump(report, open(f"{out_dir}/report.json", "w"))
print("ok")
"""


def _child(name, overlap, out_dir):
    code = CHILD % dict(root=ROOT, name=name, out=out_dir)
    env = dict(os.environ, SWG_PAIR_OVERLAP=overlap)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=ROOT, timeout=CHILD_TIMEOUT)
    assert out.returncode == 0 and "ok" in out.stdout, (name, overlap, out.returncode, out.stderr[-2000:])
    report = json.load(open(os.path.join(out_dir, "report.json")))
    res = []
    for k in range(len(report)):
        last = os.path.join(out_dir, f"st{k}_last.npy")
        res.append((np.load(os.path.join(out_dir, f"st{k}.npy")), np.load(os.path.join(out_dir, f"ch{k}.npy")),
                    np.load(last) if os.path.exists(last) else None,
                    np.load(os.path.join(out_dir, f"ch{k}_last.npy")) if os.path.exists(last) else None))
    return report, res


@pytest.mark.parametrize("name", sorted(CASES))
def test_both_orders_give_the_oracles_answer(name):
    import sweepga_amd as sw
    make, configs = CASES[name]
    rec = make()
    runs = {}
    for overlap in ("1", "0"):
        with tempfile.TemporaryDirectory() as d:
            runs[overlap] = _child(name, overlap, d)
    for k, (kw, kind) in enumerate(configs):
        okw = {a: (int(getattr(sw.FilterMode, v)) if isinstance(v, str) else v) for a, v in kw.items()}
        ost, och = orc.apply_filters(orc.Config(**okw), rec)
        for overlap in ("1", "0"):
            report, res = runs[overlap]
            st, ch, st_last, ch_last = res[k]
            assert (st_last is not None) == (kind == "long")
            if st_last is not None:   # call 20 of 20, profiler off
                assert np.array_equal(st_last, ost) and np.array_equal(ch_last, och), (name, kw, overlap, "last of the repeated calls")
            launches = report[k]["launches"]
            bad = np.flatnonzero((st != ost) | (ch != och))
            print(name, kw, "SWG_PAIR_OVERLAP=" + overlap, "records differing from the oracle:", int(bad.size), "repeats differing:",
                  report[k]["differing_repeats"], "long-leg launches:", {a: launches.get(a, 0) for a in ("chain_walk_spec", "chain_label_long", "pair_gate")})
            assert bad.size == 0, (name, kw, overlap, int(bad.size), bad[:10].tolist())
            assert report[k]["differing_repeats"] == 0, (name, kw, overlap, report[k]["differing_repeats"])
            on_global = any(a in launches for a in GLOBAL_STAGE)
            if kind in ("long", "no_long"):
                assert "pair_renumber" in launches and not on_global, (name, kw, overlap, sorted(launches))
                assert launches.get("chain_walk_spec", 0) == 4 and launches.get("chain_label_long", 0) == 1, (name, kw, overlap, launches)
                assert launches.get("chain_walk", 0) == 1 and launches.get("chain_label", 0) == 1 and launches.get("pair_gate", 0) == 2, (name, kw, overlap, launches)
            elif kind == "small":
                assert "pair_renumber" in launches and not on_global, (name, kw, overlap, sorted(launches))
                assert "chain_walk_spec" not in launches and "chain_label_long" not in launches, (name, kw, overlap, launches)
            else:
                assert "chain_walk_spec" in launches and "chain_label_long" in launches and on_global, (name, kw, overlap, sorted(launches))
        # the two orders against each other (implied by the oracle, spelled out)
        assert np.array_equal(runs["1"][1][k][0], runs["0"][1][k][0]) and np.array_equal(runs["1"][1][k][1], runs["0"][1][k][1]), (name, kw)
        assert runs["1"][0][k]["launches"] == runs["0"][0][k]["launches"], (name, kw, runs["1"][0][k]["launches"], runs["0"][0][k]["launches"])
