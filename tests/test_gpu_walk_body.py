"""The body of the fused walk (csrc/swg_chain.hip, chain_walk_kernel / walk_key_loop): the packed-key loop with its
one counter, the strand compiled in and the ring of two columns in the pair-resident path, three columns and the strand per lane
in the global-sort stage and in the blocks of long units.  What can go wrong: a window one element short or long -- at a batch's
first and last lane, where the ring wraps, beyond the ring --, a tie taken by the wrong j, a list that is exhausted without the
whole-window pass, a limit off by one on either axis or either side, a difference near 2^32 taken for a small one, the wrong
target column on the '-' strand.  Every input is ONE planted pair among sparse filler pairs (more than 65,536 records on 150 Mbp:
the plan over runs and the benchmark's size classes), once as planted and once mirrored onto the '-' strand, and is held to the
CPU oracle record for record (status and chain numbers) on the pair path (this process), in the global-sort stage (a child
process with SWG_GROUP_FUSED=0) and, cases 1-3, with the plain candidate lists (a child with SWG_WALK_PLAIN=1).  -m gpu only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import orc
from tests.test_gpu_pair_columns import pairs_of
from tests.test_gpu_pair_ranked import planted
from tests.test_gpu_pair_sort_split import concat, dense_pair
from tests.test_gpu_pairs import run_both

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 600
GAP = 50_000              # FilterConfig's scaffold_gap
SPAN = 150_000_000
TOP = 2**32 - 1
BIGW = 256                # the fused walk's ring
LONG = 9_216              # LABEL_CAP_ELEMS: a chunk of this many members is walked in blocks (chain_walk_spec)
WINDOWS = [1, 63, 64, 65, 255, 256, 257, 300]
GAPS = [1, 50_000, 2**22, 2**22 + 1]
EVERY_CHAIN = {"min_scaffold_length": 1}     # every chain passes: the chain numbers show every link


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context(0)
    return sweepga_amd


# ---- inputs --------------------------------------------------------------------------------------------------------------
def records(qs, qe, ts, te, strand="+"):
    u = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.uint64))
    qs, qe, ts, te = u(qs), u(qe), u(ts), u(te)
    n = len(qs)
    ln = np.maximum(qe - qs, te - ts)
    m = np.floor(0.9 * ln).astype(np.uint64)
    return orc.Records([""] * n, [""] * n, qs, qe, ts, te, ln, m / np.maximum(ln, 1), m, np.full(n, ord(strand), dtype=np.uint8),
                       np.arange(n, dtype=np.uint64))


def mirrored(rec, top):
    """The same records on the '-' strand: target coordinates mirrored about top / 2, so that d(i, j) of every pair of records --
    t_start[i] against t_end[j] there -- is what t_end[i] against t_start[j] was."""
    out = concat([rec])
    out.ts, out.te = np.uint64(top) - rec.te, np.uint64(top) - rec.ts
    out.strand = np.full(len(rec), ord("-"), dtype=np.uint8)
    return out


_FILLER = []


def filler():
    """Fourteen sparse pairs, 66,000 records: a handful of members per unit."""
    if not _FILLER:
        _FILLER.append(pairs_of(np.random.default_rng(255), [5_000] * 13 + [1_000]))
    return _FILLER[0]


def whole(pair, minus, top=SPAN):
    """The planted pair (mirrored: minus) in front of the filler, shuffled inside itself like the filler's pairs are."""
    pair = mirrored(pair, top) if minus else concat([pair])
    o = np.random.default_rng(len(pair)).permutation(len(pair))
    for c in ("qs", "qe", "ts", "te", "block_length", "identity", "matches", "strand"):
        setattr(pair, c, np.ascontiguousarray(getattr(pair, c)[o]))
    pair.qname, pair.tname = ["plant#1#c"] * len(pair), ["plant#1#d"] * len(pair)
    rec = concat([pair, filler()])
    assert len(rec) > 65_536
    return rec


def lone(n, q0, step=150_000):
    """n records of 1 kb, `step` apart: every one a unit of its own, no window holds anything."""
    return planted(q0 + step * np.arange(n), 1_000, 500, "+")


def window_block(rng, w, q0, ln=60_000):
    """A long record at q0 whose q_end + GAP reaches exactly w later starts -- the last of them AT q_end + GAP, the next record one
    base beyond.  Most of the w start inside the long record's first 40 kb (an overlap of more than GAP / 5: no candidates), the
    others between its end - 5 kb and its reach: the candidates lie at the window's far end."""
    reach = q0 + ln + GAP
    early = (w * 9) // 10 if w >= 200 else w // 2
    q = np.concatenate((np.sort(rng.choice(np.arange(q0 + 1, q0 + 40_000), early, replace=False)),
                        np.sort(rng.choice(np.arange(q0 + ln - 5_000, reach), w - early - 1, replace=False)) if w - early > 1 else [],
                        [reach, reach + 1, reach + 700])).astype(np.int64)
    t = q + 500 + rng.integers(-3_000, 3_000, len(q))
    t[-3:] = q[-3:] + 500
    fol = records(q, q + 100, t, t + 100)
    return concat([records([q0], [q0 + ln], [q0 + 500], [q0 + 500 + ln]), fol]), reach + 1_000


def window_pair(w):
    """Case 1.  One chunk: 64 lone records, the long record at position 64 (lane 0 of the second batch, the ring's first slot),
    its w + 2 followers, lone records up to a position = 255 (mod 256), and there -- lane 63, the ring's last slot before it
    wraps -- a second long record with its followers."""
    rng = np.random.default_rng(1_000 + w)
    a = lone(64, 1_000_000)
    b, end = window_block(rng, w, 1_000_000 + 64 * 150_000)
    n = len(a) + len(b)
    pad = (BIGW - 1 - n) % BIGW
    c = lone(pad, end + 150_000)
    d, end2 = window_block(rng, w, end + 150_000 * (pad + 2))
    e = lone(200, end2 + 150_000)
    pair = concat([a, b, c, d, e])
    o = np.argsort(pair.qs, kind="stable")
    first, second = int(np.flatnonzero(o == 64)[0]), int(np.flatnonzero(o == n + pad)[0])
    assert first == 64 and second % BIGW == BIGW - 1 and second % 64 == 63 and second + w + 3 < 1_024 + 256, (first, second)
    for i in (first, second):    # exactly w later starts within reach
        assert int((pair.qs[o][i + 1:] <= pair.qe[o][i] + GAP).sum()) == w and pair.qs[o][i + w] == pair.qe[o][i] + GAP
    assert int(pair.qe.max()) < SPAN
    return pair


def ties_pair():
    """Case 2.  Six successors at one distance from one element (552,500 = 70^2 + 740^2 = ... = 500^2 + 550^2), two at one distance
    (3,000 / 4,000 and 4,000 / 3,000), and two elements at one distance from one successor; lone records around them."""
    parts, q0 = [lone(70, 1_000_000)], 20_000_000
    six = [(70, 740), (140, 730), (220, 710), (250, 700), (410, 620), (500, 550)]
    for k, gaps in enumerate((six, [(3_000, 4_000), (4_000, 3_000)], six[::-1][:2] + six[:2])):
        qe = q0 + 1_000_000 * k
        te = qe + 700
        parts.append(records([qe - 6_000], [qe], [te - 6_000], [te]))
        parts.append(records([qe + g for g, _ in gaps], [qe + g + 6_000 for g, _ in gaps], [te + r for _, r in gaps],
                             [te + r + 6_000 for _, r in gaps]))
    sq, st = 40_000_000, 40_000_700      # one successor, two elements whose ends lie (3,000, 4,000) and (4,000, 3,000) before it
    parts.append(records([sq - 3_000 - 6_000, sq - 4_000 - 6_000, sq], [sq - 3_000, sq - 4_000, sq + 6_000],
                         [st - 4_000 - 6_000, st - 3_000 - 6_000, st], [st - 4_000, st - 3_000, st + 6_000]))
    parts.append(lone(500, 50_000_000))
    return concat(parts)


def exhausted_pair():
    """Case 3.  Twelve records that end at one point, then six successors at growing distances: the first takes the nearest, the
    second finds it taken at an equal distance and takes the next, ... the fifth finds all four of its list taken while its window
    held six: the whole window.  Twice: at the start of a batch (positions 64-75) and across a batch's end (122-133)."""
    parts = [lone(64, 1_000_000)]
    for k, n_before in enumerate((0, 40)):
        q0 = 30_000_000 + 10_000_000 * k
        parts.append(lone(n_before, q0 - 150_000 * (n_before + 1)))
        qe, te = q0 + 20_000, q0 + 20_500
        st = qe - 30_000 - 10 * np.arange(12)[::-1]      # (they overlap one another by more than GAP / 5: no candidates)
        parts.append(records(st, np.full(12, qe), st + 500, np.full(12, te)))
        g = 1_000 * np.arange(1, 7)
        parts.append(records(qe + g, qe + g + 300, te + 2 * g, te + 2 * g + 300))
    parts.append(lone(500, 60_000_000))
    return concat(parts)


def limits_pair(gap):
    """Case 4.  Two-record groups 12 Mbp apart: a gap of exactly `gap` and of gap + 1 on the query axis, on the target axis and
    on both; an overlap of exactly gap / 5 and of gap / 5 + 1 on either axis."""
    fifth = gap // 5
    ln = max(6_000, fifth + 5_000)
    parts, q0 = [lone(64, 1_000)], 12_000_000
    for dq, dt in ((gap, 0), (gap + 1, 0), (0, gap), (0, gap + 1), (gap, gap), (gap + 1, gap + 1), (-fifth, 0), (-fifth - 1, 0),
                   (0, -fifth), (0, -fifth - 1), (-fifth, -fifth)):
        qe, te = q0 + ln, q0 + 700 + ln
        parts.append(records([q0, qe + dq], [qe, qe + dq + ln], [q0 + 700, te + dt], [te, te + dt + ln]))
        q0 += 12_000_000
    assert q0 - 12_000_000 + 3 * ln + gap < SPAN
    return concat(parts)


def edges_pair():
    """Case 5.  Target starts at 10 and at 2^32 - 20,000 under neighbouring query starts (in either order), the same on the query
    axis with records that end at 2^32 - 1, and a record from 5,000 to 2^32 - 1 whose window is the rest of the pair: every
    difference near 2^32 is a small one modulo 2^32."""
    hi = TOP - 20_000
    parts = [lone(64, 1_000_000),
             records([20_000_000, 20_007_000], [20_006_000, 20_013_000], [10, hi], [6_010, hi + 6_000]),
             records([21_000_000, 21_007_000], [21_006_000, 21_013_000], [hi, 10], [hi + 6_000, 6_010]),
             records([22_000_000, 22_007_000], [22_006_000, 22_013_000], [TOP - 6_000, 2_000], [TOP, 8_000]),
             records([23_000_000, 23_007_000], [23_006_000, 23_013_000], [2_000, TOP - 6_000], [8_000, TOP]),
             records([5_000], [TOP], [5_700], [TOP]),                                   # its q_end + GAP is beyond u32
             records([10_000, 30_000, 56_000], [16_000, 36_000, 62_000], [10_700, 30_700, 56_700], [16_700, 36_700, 62_700]),
             lone(300, 100_000_000),
             records([TOP - 13_000, TOP - 6_000, TOP - 5_000], [TOP - 7_000, TOP, TOP], [TOP - 13_000, TOP - 6_000, 10],
                     [TOP - 7_000, TOP, 5_010])]
    return concat(parts)


def long_pair():
    """Case 6.  12,000 records 1 kb apart: one unit, walked in blocks."""
    return dense_pair(np.random.default_rng(12_000), 12_000, 0)


def cases():
    """name -> (planted pair, the flag sets, the coordinate the '-' version is mirrored about)"""
    out = {}
    for w in WINDOWS:
        out[f"window{w}"] = (window_pair(w), [{}, EVERY_CHAIN], SPAN)
    out["ties"] = (ties_pair(), [{}, EVERY_CHAIN], SPAN)
    out["exhausted"] = (exhausted_pair(), [EVERY_CHAIN], SPAN)
    for gap in GAPS:
        out[f"limits{gap}"] = (limits_pair(gap), [{"scaffold_gap": gap}, {"scaffold_gap": gap, "min_scaffold_length": 1}], SPAN)
    out["edges"] = (edges_pair(), [{}, EVERY_CHAIN], TOP + 10)
    out["long"] = (long_pair(), [{}], SPAN)
    return out


NAMES = [f"window{w}" for w in WINDOWS] + ["ties", "exhausted"] + [f"limits{g}" for g in GAPS] + ["edges", "long"]
PLAIN_NAMES = [n for n in NAMES if n.startswith("window") or n in ("ties", "exhausted")]      # case 7


def run_case(sw, name, minus, expect_pair_path, last_only=False):
    pair, cfgs, top = cases_cached()[name]
    rec = whole(pair, minus, top)
    out = []
    for cfg in cfgs[-1:] if last_only else cfgs:
        st, ch, _ = run_both(sw, rec, cfg, expect_pair_path=expect_pair_path)
        out.append((st, ch))
    return rec, out


_CASES = {}


def cases_cached():
    if not _CASES:
        _CASES.update(cases())
    return _CASES


# ---- the pair path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("minus", [False, True], ids=["plus", "minus"])
@pytest.mark.parametrize("name", NAMES)
def test_pair_path(sw, name, minus):
    rec, out = run_case(sw, name, minus, True)
    n = len(cases_cached()[name][0])
    st, ch = out[-1]
    table = sw.default_context(0).profile_table()
    assert "chain_walk" in table
    if name == "edges":                 # nothing chains across the 2^32 difference: no chain holds a low and a high coordinate
        for c in np.unique(ch[:n][ch[:n] != 0]):
            for col in (rec.ts[:n][ch[:n] == c], rec.qe[:n][ch[:n] == c]):
                assert int(col.max()) - int(col.min()) < 2**31, (int(c), col.tolist())
    if name == "long":
        assert n >= LONG and "chain_walk_spec" in table, sorted(table)


def test_the_limits_bind_where_they_should(sw):
    """Case 4 read without the oracle: of the eleven two-record groups the ones at the limit chain and the ones beyond do not."""
    for gap in GAPS:
        pair = limits_pair(gap)
        rec = whole(pair, False)
        _, ch, _ = run_both(sw, rec, {"scaffold_gap": gap, "min_scaffold_length": 1}, expect_pair_path=True)
        n = len(pair)
        o = np.argsort(rec.qs[:n], kind="stable")[64:]
        assert len(o) == 22
        same = [bool(ch[o[2 * k]] == ch[o[2 * k + 1]]) for k in range(11)]
        assert same == [True, False, True, False, True, False, True, False, True, False, True], (gap, same)


# ---- the global-sort stage and the plain lists: child processes (the knobs are read once per process) -----------------------
CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
import sweepga_amd
sweepga_amd.default_context(0)
from tests import test_gpu_walk_body as T
done = []
for name in %(names)r:
    for minus in (False, True):
        T.run_case(sweepga_amd, name, minus, %(pair_path)r, last_only=True)
        done.append([name, minus])
print("RESULT " + json.dumps(done))
"""


def in_child(env, names, pair_path):
    out = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, names=names, pair_path=pair_path)], env=dict(os.environ, **env),
                         capture_output=True, text=True, cwd=ROOT, timeout=CHILD_TIMEOUT)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    line = next(ln for ln in out.stdout.splitlines() if ln.startswith("RESULT "))
    return json.loads(line[len("RESULT "):])


GROUPS = {"windows_to_65": NAMES[:4], "windows_from_255": NAMES[4:8], "ties_exhausted_limits": NAMES[8:14], "edges_long": NAMES[14:]}


@pytest.mark.parametrize("group", list(GROUPS))
def test_global_sort_stage(group):
    """SWG_GROUP_FUSED=0: the same inputs through the three-column ring with the strand per lane (run_both asserts the path; each
    input under the flag set that shows every link)."""
    names = GROUPS[group]
    done = in_child({"SWG_GROUP_FUSED": "0"}, names, False)
    assert done == [[n, m] for n in names for m in (False, True)]


@pytest.mark.parametrize("group", list(GROUPS)[:3])
def test_plain_lists(group):
    """Case 7.  SWG_WALK_PLAIN=1: the inputs of cases 1-3 with the per-lane candidate lists instead of the packed-key loop."""
    names = [n for n in GROUPS[group] if n in PLAIN_NAMES]
    done = in_child({"SWG_WALK_PLAIN": "1"}, names, True)
    assert done == [[n, m] for n in names for m in (False, True)]
