"""Named, deterministic record sets at the edges of the u64 -> u32 rebasing rule (tests/wide_model.py states the rule).  Every case
carries the answer its construction is meant to produce (`expect`, a prefix of the model's answer) and asserts that premise
against the model when it is built: a case that does not hit the edge it was written for fails here, not silently.

Used by tests/test_wide_edges_cpu.py (rebase.h through tests/native/rebase_check, the PAF and .1aln front ends) and
tests/test_gpu_wide_edges.py (swg_filter64 and swg_filter_device64)."""
import os
import re

from tests import wide_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = wm.LIMIT   # 2^32
TOP = (1 << 64) - 1


def kernel_group_size():
    """EW, the work-group size of the rebasing kernels (nblk(n) launches EW threads), read from the source."""
    src = open(os.path.join(ROOT, "sweepga_amd", "csrc", "swg_filter.hip")).read()
    m = re.search(r"constexpr\s+int\s+EW\s*=\s*(\d+)\s*;", src)
    assert m and "nblk(n), EW" in src
    return int(m.group(1))


EW = kernel_group_size()


def genome_of(name):
    return name.rsplit("#", 1)[0] + "#" if "#" in name else name


class Case:
    """recs: (query name, target name, q_start, q_end, t_start, t_end, matches, block_len).  Ids are given in first-appearance
    order, query before target, genomes likewise over the sequence table (what pack_records and the front ends do).
    pad: names of further sequences that no record names.  bad_id = (record, axis): that id becomes n_seq.  bad_genome = name of a
    sequence whose genome table entry becomes n_genome_last.  modelled = False: a record has start > end, which the filter itself
    does not model; the rebasing is checked, the filter's answer only between the two entry points."""

    def __init__(self, name, group, recs, expect, pad=(), bad_id=None, bad_genome=None, modelled=True, step2=None):
        self.name, self.group, self.expect, self.modelled = name, group, tuple(expect), modelled
        ids = {}
        for r in recs:
            for nm in r[:2]:
                ids.setdefault(nm, len(ids))
        for nm in pad:
            assert nm not in ids
            ids[nm] = len(ids)
        self.names = list(ids)
        self.n = len(recs)
        self.n_seq = max(len(ids), 1)
        gid = {}
        self.genome = [gid.setdefault(genome_of(nm), len(gid)) for nm in self.names] or [0]
        self.n_genome = max(len(gid), 1)
        self.qname = [r[0] for r in recs]
        self.tname = [r[1] for r in recs]
        self.q_id = [ids[r[0]] for r in recs]
        self.t_id = [ids[r[1]] for r in recs]
        self.cols = [[int(r[2 + f]) for r in recs] for f in range(6)]
        for c in self.cols:
            assert all(0 <= v <= TOP for v in c)
        self.text = bad_id is None and bad_genome is None and not pad   # expressible as a PAF / as .1aln input
        if bad_id is not None:
            (self.q_id if bad_id[1] == 0 else self.t_id)[bad_id[0]] = self.n_seq
        if bad_genome is not None:
            self.genome[ids[bad_genome]] = self.n_genome
        self.result = wm.rebase(self.q_id, self.t_id, self.cols, self.n_seq, self.genome, self.n_genome)
        assert self.result[:len(self.expect)] == self.expect, (name, self.result[:3], self.expect)
        if step2 is not None:   # what the per-sequence attempt alone names (must differ from the final answer where the case says so)
            self.step2 = step2
            alone = wm.rebase(self.q_id, self.t_id, self.cols, self.n_seq, self.genome, wm.MAX_CELLS + 1)
            assert alone == ("range",) + tuple(step2), (name, alone, step2)
            assert alone != self.result[:3], name


def filler(k, base=1 << 40):
    """An ordinary record on its own pair of sequences, far beyond 2^32 (and narrow)."""
    return ("F#1#f", "G#1#g", base + 1000 * k, base + 1000 * k + 500, base + 1000 * k + 7, base + 1000 * k + 507, 450, 500)


def with_fillers(n, placed):
    """n records: `placed` = {index: record}, fillers everywhere else."""
    assert all(0 <= i < n for i in placed)
    return [placed.get(i, filler(i)) for i in range(n)]


SIZES = [1, 63, 64, 65, EW - 1, EW, EW + 1, 3 * EW + 7]


def positions(n):
    return sorted({p for p in (0, 63, 64, n - 1) if 0 <= p < n})


def edge_records(n, pos, f, width, lo=5 * W + 11):
    """n records; the one at `pos` has field f exactly `width` above its sequence's smallest coordinate."""
    other = (lo + 3, lo + 9)
    if f in (1, 3):      # an end: the record itself spans the stretch
        mine = (lo, lo + width)
        anchor = None
    elif n == 1:         # a start, alone: only a reversed interval puts the minimum into the end column
        mine = (lo + width, lo)
        anchor = None
    else:                # a start: a zero-length record, the sequence's smallest coordinate is another record's
        mine = (lo + width, lo + width)
        anchor = (lo, lo + 100)
    q, t = (mine, other) if f < 2 else (other, mine)
    placed = {pos: ("X#1#x", "Y#1#y", q[0], q[1], t[0], t[1], 90, 100)}
    if anchor is not None:
        a = (pos + 1) % n
        qa, ta = (anchor, other) if f < 2 else (other, anchor)
        placed[a] = ("X#1#x", "Y#1#y", qa[0], qa[1], ta[0], ta[1], 90, 100)
    return with_fillers(n, placed), not (n == 1 and f in (0, 2))


def boundary_cases():
    out = []
    grid = [(n, p) for n in SIZES for p in positions(n)]
    for k, (n, p) in enumerate(grid):
        for f in range(4):
            recs, modelled = edge_records(n, p, f, W)
            out.append(Case(f"refuse_f{f}_n{n}_p{p}", "boundary", recs, ("range", p, f), modelled=modelled))
        # accepted: every (n, position) with one field in turn, and every field at one (n, position) below
        f = k % 4
        recs, modelled = edge_records(n, p, f, W - 1)
        c = Case(f"accept_f{f}_n{n}_p{p}", "boundary", recs, ("ok", "seq"), modelled=modelled)
        assert c.result[4][f][p] == 0xFFFFFFFF
        out.append(c)
    for f in range(4):
        recs, modelled = edge_records(EW + 1, 64, f, W - 1)
        c = Case(f"accept_f{f}_every_field", "boundary", recs, ("ok", "seq"), modelled=modelled)
        assert c.result[4][f][64] == 0xFFFFFFFF
        out.append(c)
    # reversed intervals (start > end): the minimum comes from the end column
    lo = 9 * W
    for f, nm in ((0, "query"), (2, "target")):
        for width, expect in ((W - 1, ("ok", "seq")), (W, ("range", 1, f))):
            r = [lo + width, lo, lo + 3, lo + 9] if f == 0 else [lo + 3, lo + 9, lo + width, lo]
            recs = [filler(0), ("X#1#x", "Y#1#y", *r, 90, 100), filler(2)]
            c = Case(f"reversed_{nm}_{'accept' if expect[0] == 'ok' else 'refuse'}", "boundary", recs, expect, modelled=False)
            if expect[0] == "ok":
                assert c.result[4][f][1] == 0xFFFFFFFF and c.result[4][f + 1][1] == 0
            out.append(c)
    # matches and block length: not rebased, 2^32 - 1 is the last value that fits
    for f, nm in ((4, "matches"), (5, "block_len")):
        for v, expect in ((W - 1, ("ok", "seq")), (W, ("range", 65, f))):
            x = ["X#1#x", "Y#1#y", lo + 10, lo + 510, lo + 20, lo + 520, 450, 500]
            x[2 + f] = v
            if f == 4:
                x[7] = W - 1   # (matches <= block length, as in any PAF line)
            recs = with_fillers(EW + 1, {65: tuple(x)})
            out.append(Case(f"{nm}_{'accept' if expect[0] == 'ok' else 'refuse'}", "boundary", recs, expect))
    # the top of u64
    recs = [filler(0), ("X#1#x", "Y#1#y", TOP - 1000, TOP, TOP - (W - 1), TOP, 900, 1000), filler(2)]
    c = Case("top_of_u64", "boundary", recs, ("ok", "seq"))
    assert c.result[4][1][1] == 1000 and c.result[4][3][1] == 0xFFFFFFFF
    out.append(c)
    recs = [filler(0), ("X#1#x", "Y#1#y", TOP - 1000, TOP, TOP - W, TOP, 900, 1000), filler(2)]
    out.append(Case("top_of_u64_refuse", "boundary", recs, ("range", 1, 3)))
    out.append(Case("empty", "boundary", [], ("ok", "seq")))
    return out


def wavefront_cases():
    """Each named sequence's stretch is exactly 2^32 - 1 wide, so a constant that is off by one in either direction turns an
    accepted case into a refusal (too small: the largest value no longer fits; too large: the smallest wraps)."""
    out = []
    lo_q, lo_t = 3 * W + 5, 7 * W + 1

    def rec(q, t, a, b, ln=200):
        return (q, t, a, a + ln, b, b + ln, 180, 200)

    for lane in (0, 31, 63):
        # 64 records of one (query, target): the minimum in `lane`, the maximum end (lo + 2^32 - 1) in the lane after it
        recs = []
        for k in range(64):
            a, b = lo_q + 1000 * (k + 1), lo_t + 1000 * (k + 1)
            if k == lane:
                a, b = lo_q, lo_t
            if k == (lane + 1) % 64:
                a, b = lo_q + W - 1 - 200, lo_t + W - 1 - 200
            recs.append(rec("X#1#x", "Y#1#y", a, b))
        c = Case(f"uniform_min_lane{lane}", "wavefronts", recs, ("ok", "seq"))
        assert c.result[2] == [lo_q] * 64 and c.result[3] == [lo_t] * 64
        assert max(c.result[4][1]) == 0xFFFFFFFF and max(c.result[4][3]) == 0xFFFFFFFF
        out.append(c)
        # the same wavefront behind one of mixed records, and before a partial one
        c = Case(f"uniform_min_lane{lane}_second_wavefront", "wavefronts", [filler(k) for k in range(64)] + recs + [filler(k) for k in range(5)],
                 ("ok", "seq"))
        out.append(c)
    for axis, nm in ((0, "q_uniform_t_mixed"), (1, "t_uniform_q_mixed")):
        recs = []
        for k in range(64):
            j = k % 3   # three sequences on the mixed axis: their minima in lanes 61, 62, 63, their maxima in lanes 0, 1, 2
            u = lo_q if k == 40 else (lo_q + W - 1 - 200 if k == 41 else lo_q + 500 * (k + 1))
            base = lo_t + j * 11 * W
            m = base if k >= 61 else (base + W - 1 - 200 if k < 3 else base + 700 * (k + 1))
            mixed = f"M{j}#1#m"
            recs.append(rec("U#1#u", mixed, u, m) if axis == 0 else rec(mixed, "U#1#u", m, u))
        c = Case(nm, "wavefronts", recs, ("ok", "seq"))
        assert max(c.result[4][1]) == 0xFFFFFFFF and max(c.result[4][3]) == 0xFFFFFFFF
        assert len(set(c.result[2 if axis == 0 else 3])) == 1 and len(set(c.result[3 if axis == 0 else 2])) == 3
        out.append(c)
    # a last wavefront with one live lane, which alone names its two sequences
    for n in (65, EW + 1):
        recs = with_fillers(n, {n - 1: ("X#1#x", "Y#1#y", lo_q, lo_q + W - 1, lo_t, lo_t + W - 1, 90, 100)})
        c = Case(f"one_live_lane_n{n}", "wavefronts", recs, ("ok", "seq"))
        assert c.result[4][1][n - 1] == 0xFFFFFFFF and c.result[4][3][n - 1] == 0xFFFFFFFF
        out.append(c)
    # a sequence named only as a target: its constant comes from the target columns alone
    recs = [rec("X#1#x", "T#1#t", lo_q + 1000 * k, lo_t + 1000 * (64 - k)) for k in range(64)]
    recs += [("X#1#x", "T#1#t", lo_q + 5, lo_q + 6, lo_t, lo_t + W - 1, 1, 1)]
    c = Case("target_only", "wavefronts", recs, ("ok", "seq"))
    assert "T#1#t" not in c.qname and set(c.result[3]) == {lo_t} and c.result[4][3][64] == 0xFFFFFFFF
    out.append(c)
    # sequences that no record names (ids beyond every named one, and the table still has them)
    recs = [rec("X#1#x", "Y#1#y", lo_q + 1000 * k, lo_t + 1000 * k) for k in range(70)]
    c = Case("unnamed_sequences", "wavefronts", recs, ("ok", "seq"), pad=["P#1#p", "Q#1#q", "X#1#z"])
    assert c.n_seq == 5 and wm.seq_constants(c.q_id, c.t_id, c.n_seq, c.result)[2:] == [wm.UNNAMED] * 3
    out.append(c)
    return out


def _pads(k, shared_genome=0):
    """k - shared_genome sequences of a genome of their own each, then shared_genome sequences of genome A."""
    return [f"P{i}#1#p" for i in range(k - shared_genome)] + [f"A#1#extra{i}" for i in range(shared_genome)]


def two_axis_cases():
    out = []
    far = 2 * W   # 2^33

    def rec(q, t, a, b, ln=1000):
        return (q, t, a, a + ln, b, b + ln, 900, 1000)

    # a sequence mapped onto itself: its query stretch near 0, its target stretch near 2^33
    recs = [rec("S#1#s", "S#1#s", 100 + 2000 * k, far + 100 + 2000 * k) for k in range(70)]
    c = Case("self_mapping_apart", "two_axes", recs, ("ok", "axis"), step2=(0, 2))
    assert set(c.result[2]) == {100} and set(c.result[3]) == {far + 100}
    out.append(c)
    # A against genome B near 0 and against genome C near 2^33
    ab = [rec("A#1#a", "B#1#b", 50 + 3000 * k, 10 + 3000 * k) for k in range(40)]
    ac = [rec("A#1#a", "C#1#c", far + 70 + 3000 * k, 20 + 3000 * k) for k in range(40)]
    c = Case("two_genomes_apart", "two_axes", ab + ac, ("ok", "axis"), step2=(40, 0))
    assert set(c.result[2]) == {50, far + 70}
    out.append(c)
    # ... and the C segment itself 2^32 wide: refused, and not at the record the per-sequence attempt names
    wide_c = ac + [rec("A#1#a", "C#1#c", far + 70 + W, 999_000)]
    out.append(Case("two_genomes_one_too_wide", "two_axes", ab + wide_c, ("range", 80, 0), step2=(40, 0)))
    # the tables' limit: n_seq * n_genome_last = 2^24 exactly (4096 sequences, every one a genome of its own) still takes the axis path
    c = Case("cells_exactly_2_24", "two_axes", ab + ac, ("ok", "axis"), pad=_pads(4096 - 3), step2=(40, 0))
    assert c.n_seq * c.n_genome == wm.MAX_CELLS
    out.append(c)
    # one row more: the per-sequence attempt's record stands
    c = Case("cells_one_row_over", "two_axes", ab + ac, ("range", 40, 0), pad=_pads(4097 - 3, shared_genome=1))
    assert c.n_seq * c.n_genome == wm.MAX_CELLS + 4096 and c.n_genome == 4096
    out.append(c)
    # a named sequence whose genome entry is n_genome_last, met on the axis path only
    out.append(Case("genome_entry_out_of_range", "two_axes", ab + ac, ("invalid", 40), bad_genome="C#1#c"))
    return out


def precedence_cases():
    """Order matters to tests/test_gpu_wide_edges.py: of the two cases with an id out of range BEHIND a wide record, the one whose
    wide segment cannot be fixed comes first."""
    out = []
    far = 2 * W

    def rec(q, t, a, b, ln=1000, m=900):
        return (q, t, a, a + ln, b, b + ln, m, 1000)

    ab = [rec("A#1#a", "B#1#b", 50 + 3000 * k, 10 + 3000 * k) for k in range(40)]
    ac = [rec("A#1#a", "C#1#c", far + 70 + 3000 * k, 20 + 3000 * k) for k in range(40)]       # fixable per genome
    unfixable = ac + [rec("A#1#a", "C#1#c", far + 70 + W, 999_000)]
    for axis in (0, 1):
        recs = ab + unfixable + [rec("A#1#a", "B#1#b", 400_000, 400_000)]
        out.append(Case(f"bad_id_behind_unfixable_wide_axis{axis}", "precedence", recs, ("invalid", 81), bad_id=(81, axis)))
    for axis in (0, 1):
        out.append(Case(f"bad_id_behind_fixable_wide_axis{axis}", "precedence", ab + ac, ("invalid", 70), bad_id=(70, axis)))
    out.append(Case("bad_id_before_wide", "precedence", ab + ac, ("invalid", 3), bad_id=(3, 0)))
    out.append(Case("bad_id_first_and_last", "precedence", ab + ac, ("invalid", 0), bad_id=(0, 1)))
    big_m = list(ab)
    big_m[5] = rec("A#1#a", "B#1#b", 50 + 3000 * 5, 10 + 3000 * 5, m=W)
    out.append(Case("bad_id_behind_wide_matches", "precedence", big_m, ("invalid", 30), bad_id=(30, 1)))
    # matches >= 2^32 at a lower index than a fixable wide span: the per-sequence attempt already stops at it
    out.append(Case("matches_before_fixable_wide", "precedence", big_m + ac, ("range", 5, 4)))
    # the other way round: the span is fixed per genome, and that attempt finds the matches
    late_m = list(ab + ac)
    late_m[60] = rec("A#1#a", "C#1#c", far + 70 + 3000 * 20, 20 + 3000 * 20, m=W)
    out.append(Case("fixable_wide_before_matches", "precedence", late_m, ("range", 60, 4), step2=(40, 0)))
    # one record failing both field 0 and field 4
    both = list(ab + ac)
    both[40] = rec("A#1#a", "C#1#c", far + 70, 20, m=W)
    out.append(Case("one_record_span_fixable_and_matches", "precedence", both, ("range", 40, 4), step2=(40, 0)))
    both = ab + [rec("A#1#a", "B#1#b", 50 + W, 77, ln=0, m=W)]
    out.append(Case("one_record_span_and_matches", "precedence", both, ("range", 40, 0)))
    return out


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = boundary_cases() + wavefront_cases() + two_axis_cases() + precedence_cases()
        assert len({c.name for c in _CASES}) == len(_CASES)
        assert all(c.n <= 3 * EW + 7 for c in _CASES)
    return _CASES


def group(name):
    return [c for c in all_cases() if c.group == name]
