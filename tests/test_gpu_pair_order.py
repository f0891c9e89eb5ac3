"""Which pair runs when in the pair-resident stage (csrc/swg_pair.hip): the two largest size classes share one
pair_finish launch and one pair_chains launch per phase, the very long pairs first; pair_order brings the two classes' lists into
longest-first order before anything reads them; the numbering of up to 12,288 pairs counts from LDS.  None of it may change an
answer: every case is held to the CPU oracle record for record (status and chain numbers), on inputs beyond 65,536 records
grouped by pair (below that the hash-table plan runs, which has no class 3 and no lists in run order), and every case shows from
the launch table that the pair-resident path ran.  -m gpu only."""
import functools
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
GLOBAL_STAGE = ("chain_cuts", "cuts_from_scan", "sortA_keys", "sortA_keys_hist", "sortA_words")   # (as tests/test_gpu_pairs.py tells the paths apart)
CHILD_TIMEOUT = 600

# the issue's flag sets: the CLI defaults; --scaffold-filter 1:1 --scaffold-dist 20000 (pair_chains, both phases); the same behind --num-mappings 1:1
FLAGS = {
    "default": {},
    "scaffold_1to1": {"scaffold_filter_mode": "OneToOne", "scaffold_max_deviation": 20_000},
    "mapping_1to1_scaffold_1to1": {"mapping_filter_mode": "OneToOne", "scaffold_filter_mode": "OneToOne", "scaffold_max_deviation": 20_000},
}


def _pairs(sizes, seed, names=None):
    """One chromosome pair per entry of `sizes`, in that order: records 3 kb apart on tests/gen.py's coordinates (dense enough to
    chain under every gap limit used here), a (query, target) of its own per pair."""
    rng = np.random.default_rng(seed)
    cols = ("qs", "qe", "ts", "te", "block_length", "identity", "matches", "strand")
    parts, qn, tn = [], [], []
    for k, n in enumerate(sizes):
        r = gen.random_records(rng, n, n_genomes=1, chrs_per_genome=1, span=int(n * 3000), minus_frac=0.15, zero_frac=0.0, self_frac=0.0)
        q, t = names[k] if names else (f"a{k}#1#c", f"b{k}#1#c")
        qn += [q] * n
        tn += [t] * n
        parts.append(r)
    total = sum(sizes)
    return orc.Records(qn, tn, *[np.concatenate([getattr(r, c) for r in parts]) for c in cols], np.arange(total, dtype=np.uint64))


def _numbering_names(reverse):
    """600 chromosome pairs over 5 genomes of 5 chromosomes (genome pair = the first two '#' parts, chromosome pair inside it: both
    of the numbering's first-appearance tables matter), in genome order or in reverse."""
    seqs = [f"g{g}#1#chr{c}" for g in range(5) for c in range(5)]
    names = [(q, t) for q in seqs for t in seqs][:600]
    return names[::-1] if reverse else names


# name -> (sizes in input order, seed, names): the 40,000-record pair in the MIDDLE and the 32,768-record pair LAST, so that the
# lists' order after pair_order differs from the input's
INPUTS = {
    "class_edges": ([300, 1_024, 1_025, 4_096, 40_000, 4_097, 20_000, 32_769, 32_768], 501, None),   # all four classes, every edge
    # no class-2 work-group in the merged launch.  (Two pairs of 33,000 and 36,000 records alone average more than 32,768 records,
    # which the pair path does not admit -- csrc/swg_pair.hip, pair_plan -- so a pair of 300 records lowers the average.)
    "class3_only": ([33_000, 300, 36_000], 502, None),
    "class2_only": ([12_000] * 6, 503, None),                           # no very long pair
    "equal_lengths": ([8_192] * 12, 504, None),                         # one length bin, ties
    "numbering": ([128] * 600, 505, _numbering_names(False)),           # 76,800 records: above NUMBER_SMALL, below 12,288 pairs
    "numbering_reversed": ([128] * 600, 505, _numbering_names(True)),   # the genome pairs' first appearances in reverse order
}


@functools.lru_cache(maxsize=None)
def records(name):
    sizes, seed, names = INPUTS[name]
    rec = _pairs(sizes, seed, names)
    assert len(rec) > 65_536
    return rec


@functools.lru_cache(maxsize=None)
def oracle(name, flags):
    import sweepga_amd as sw
    okw = {a: (int(getattr(sw.FilterMode, v)) if isinstance(v, str) else v) for a, v in FLAGS[flags].items()}
    return orc.apply_filters(orc.Config(**okw), records(name))


@functools.lru_cache(maxsize=None)
def packed(name):
    import sweepga_amd as sw
    return sw.pack_records(gen.records_to_meta(records(name)))


def call(name, flags):
    """One filter call under the profiler -> (status, chain, {label: launches})."""
    import sweepga_amd as sw
    kw = {a: (getattr(sw.FilterMode, v) if isinstance(v, str) else v) for a, v in FLAGS[flags].items()}
    ctx = sw.default_context(0)
    ctx.profile_reset()
    ctx.profile(True)
    st, ch = sw.PafFilter(sw.FilterConfig(**kw)).filter_columns(packed(name))
    ctx.profile(False)
    return st, ch, {a: int(v[0]) for a, v in ctx.profile_table().items()}


def check(name, flags, st, ch, launches):
    """The oracle's answer, record for record, and the pair-resident path."""
    ost, och = oracle(name, flags)
    bad = np.flatnonzero((st != ost) | (ch != och))
    print(name, flags, "records differing from the oracle:", int(bad.size), "kept:", int((ost != 0).sum()), "chains:", int(len(set(och[ost != 0].tolist()))),
          {a: launches.get(a, 0) for a in ("pair_order", "pair_finish", "pair_finish_m", "pair_finish_s", "pair_chains", "pair_number")})
    assert bad.size == 0, (name, flags, int(bad.size), bad[:10].tolist(), st[bad[:10]].tolist(), ost[bad[:10]].tolist(), ch[bad[:10]].tolist(), och[bad[:10]].tolist())
    assert "pair_renumber" in launches and not any(a in launches for a in GLOBAL_STAGE), (name, flags, sorted(launches))


def run(name, flags):
    st, ch, launches = call(name, flags)
    check(name, flags, st, ch, launches)
    return st, ch, launches


@pytest.mark.parametrize("flags", sorted(FLAGS))
def test_every_class_edge(flags):
    st, ch, launches = run("class_edges", flags)
    # one launch for the two largest classes, the middle and small classes their own
    assert launches.get("pair_finish", 0) == 1 and launches.get("pair_finish_m", 0) == 1 and launches.get("pair_finish_s", 0) == 1, launches
    if flags != "default":   # both phases of pair_chains: one launch each for the two largest classes
        assert launches.get("pair_chains", 0) == 2 and launches.get("pair_chains_m", 0) == 2 and launches.get("pair_chains_s", 0) == 2, launches
    assert launches.get("pair_order", 0) == 1, launches


@pytest.mark.parametrize("name", ["class3_only", "class2_only", "equal_lengths"])
@pytest.mark.parametrize("flags", ["default", "scaffold_1to1"])
def test_one_class_alone(name, flags):
    st, ch, launches = run(name, flags)
    assert launches.get("pair_finish", 0) == 1 and "pair_finish_m" not in launches, launches
    assert launches.get("pair_finish_s", 0) == (1 if name == "class3_only" else 0), launches


@pytest.mark.parametrize("name", ["numbering", "numbering_reversed"])
def test_numbering_of_a_few_hundred_pairs(name):
    """Chain NUMBERS equal to the oracle's, not only the partition (run() compares the chain column itself)."""
    ost, och = oracle(name, "default")
    assert len(set(och[ost != 0].tolist())) > 300   # (the numbering has something to order: chains in most of the 600 pairs)
    st, ch, launches = run(name, "default")
    assert launches.get("pair_number", 0) == 4, launches   # key1, rank_count, key2, base_count: the counting form


CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(root)r)
from tests import test_gpu_pair_order as T
out = {}
for flags in sorted(T.FLAGS):
    st, ch, out[flags] = T.call("class_edges", flags)
    np.save(%(out)r + "/st_" + flags + ".npy", st)
    np.save(%(out)r + "/ch_" + flags + ".npy", ch)
json.dump(out, open(%(out)r + "/launches.json", "w"))
print("ok")
"""


def test_launch_counts_do_not_depend_on_the_overlap_knob():
    """SWG_PAIR_OVERLAP=0 (read once per process: a child of its own) against this process's setting: the same launches per label,
    one pair_finish launch, and the oracle's answer (computed once, here)."""
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, out=d)], env=dict(os.environ, SWG_PAIR_OVERLAP="0"),
                             capture_output=True, text=True, cwd=ROOT, timeout=CHILD_TIMEOUT)
        assert out.returncode == 0 and "ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
        serial = json.load(open(os.path.join(d, "launches.json")))
        for flags in sorted(FLAGS):
            check("class_edges", flags, np.load(os.path.join(d, f"st_{flags}.npy")), np.load(os.path.join(d, f"ch_{flags}.npy")), serial[flags])
    for flags in sorted(FLAGS):
        st, ch, launches = call("class_edges", flags)
        assert launches == serial[flags], (flags, launches, serial[flags])
        assert serial[flags].get("pair_finish", 0) == 1, serial[flags]
