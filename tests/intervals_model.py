"""The interval lists restated independently of sweepga_amd/csrc/swg_intervals.hip: per unit (one sequence of the axis against one
genome of the other side, inter-genome records only) the maximal intervals covered by ALL records, by the KEPT ones, and LOST =
covered by some record and by no kept one.  Two formulations, neither the device's (no combined sort key of unit and start, no
running maximum, no "gaps of the kept intervals clipped to an all interval"):

  plain       per unit in plain Python: ALL and KEPT by sort and merge; LOST by an event sweep with two depth counters -- a stretch
              is lost while depth_all > 0 and depth_kept == 0;
  vectorised  all units at once in numpy: every interval is a +1 event at its start and a -1 event at its end, for either
              counter; the three lists are the runs of the three conditions over the positions of a unit.

intervals() returns {(set, axis): rows} with set in SETS, axis in AXES and rows an array of ROW_DTYPE ordered by (seq,
other_genome, start); render() writes the text of swg_paf_intervals."""
import numpy as np

SETS = ("all", "kept", "lost")
AXES = ("q", "t")
ROW_DTYPE = np.dtype([("seq", "<u4"), ("other_genome", "<u4"), ("start", "<u4"), ("end", "<u4")])
FIELDS = ("seq", "other_genome", "start", "end")


def merged(intervals):
    """The maximal pieces of the union of half-open [s, e): sort, merge; zero-length intervals add nothing, touching ones join."""
    out = []
    for s, e in sorted((int(s), int(e)) for s, e in intervals):
        if e <= s:
            continue
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return [(s, e) for s, e in out]


def lost_by_depth(all_intervals, kept_intervals):
    """The maximal stretches with depth_all > 0 and depth_kept == 0: one walk over the positions where a depth changes."""
    events = {}
    for which, ivs in ((0, all_intervals), (1, kept_intervals)):
        for s, e in ivs:
            s, e = int(s), int(e)
            if e <= s:
                continue
            events.setdefault(s, [0, 0])[which] += 1
            events.setdefault(e, [0, 0])[which] -= 1
    out, depth, begun = [], [0, 0], None
    for pos in sorted(events):
        depth[0] += events[pos][0]
        depth[1] += events[pos][1]
        lost = depth[0] > 0 and depth[1] == 0
        if lost and begun is None:
            begun = pos
        elif not lost and begun is not None:
            out.append((begun, pos))
            begun = None
    assert begun is None and depth == [0, 0]
    return out


def _counted(q_id, t_id, seq_genome):
    seq_genome = np.asarray(seq_genome).astype(np.int64)
    q, t = np.asarray(q_id).astype(np.int64), np.asarray(t_id).astype(np.int64)
    return q, t, seq_genome[q], seq_genome[t]


def _rows(tuples):
    out = np.zeros(len(tuples), dtype=ROW_DTYPE)
    for k, r in enumerate(tuples):
        out[k] = r
    return out


def _plain_axis(seq, other, start, end, kept):
    units = {}
    for k in range(len(seq)):
        units.setdefault((int(seq[k]), int(other[k])), []).append((int(start[k]), int(end[k]), bool(kept[k])))
    lists = {s: [] for s in SETS}
    for (sq, og) in sorted(units):
        every = [(s, e) for s, e, _ in units[sq, og]]
        held = [(s, e) for s, e, k in units[sq, og] if k]
        for name, ivs in (("all", merged(every)), ("kept", merged(held)), ("lost", lost_by_depth(every, held))):
            lists[name] += [(sq, og, s, e) for s, e in ivs]
    return {s: _rows(v) for s, v in lists.items()}


def _vector_axis(seq, other, start, end, kept):
    live = end > start
    seq, other, start, end, kept = seq[live], other[live], start[live], end[live], kept[live]
    if len(seq) == 0:
        return {s: np.zeros(0, dtype=ROW_DTYPE) for s in SETS}
    units, unit_of = np.unique(np.stack([seq, other], axis=1), axis=0, return_inverse=True)   # rows ascending by (seq, other)
    unit_of = unit_of.reshape(-1)
    m = len(seq)
    u = np.concatenate([unit_of, unit_of])
    pos = np.concatenate([start, end])
    d_all = np.concatenate([np.ones(m, dtype=np.int64), -np.ones(m, dtype=np.int64)])
    d_kept = d_all * np.concatenate([kept, kept])
    order = np.lexsort((pos, u))
    u, pos = u[order], pos[order]
    depth_all, depth_kept = np.cumsum(d_all[order]), np.cumsum(d_kept[order])
    last = np.append((u[1:] != u[:-1]) | (pos[1:] != pos[:-1]), True)   # the last event at its position: every change applied
    u, pos, depth_all, depth_kept = u[last], pos[last], depth_all[last], depth_kept[last]
    out = {}
    for name, state in (("all", depth_all > 0), ("kept", depth_kept > 0), ("lost", (depth_all > 0) & (depth_kept == 0))):
        before = np.concatenate([[False], state[:-1]])   # (both depths are 0 behind a unit's last position: nothing leaks into the next)
        begins, ends = state & ~before, ~state & before
        rows = np.zeros(int(begins.sum()), dtype=ROW_DTYPE)
        assert int(ends.sum()) == len(rows) and np.array_equal(u[begins], u[ends])
        rows["seq"], rows["other_genome"] = units[u[begins], 0], units[u[begins], 1]
        rows["start"], rows["end"] = pos[begins], pos[ends]
        out[name] = rows
    return out


def intervals(q_id, t_id, q_start, q_end, t_start, t_end, seq_genome, kept=None, vectorised=None):
    """{(set, axis): rows}.  kept: a boolean mask (None: no record is kept -- "kept" comes out empty and "lost" equals "all")."""
    q, t, gq, gt = _counted(q_id, t_id, seq_genome)
    inter = gq != gt
    k = np.zeros(len(q), dtype=bool) if kept is None else np.asarray(kept).astype(bool)
    if vectorised is None:
        vectorised = int(inter.sum()) > 5_000
    one = _vector_axis if vectorised else _plain_axis
    out = {}
    for axis, (seq, other, s, e) in (("q", (q, gt, q_start, q_end)), ("t", (t, gq, t_start, t_end))):
        s, e = np.asarray(s).astype(np.int64), np.asarray(e).astype(np.int64)
        for name, rows in one(seq[inter], other[inter], s[inter], e[inter], k[inter]).items():
            out[name, axis] = rows
    return out


def as_tuples(rows):
    return [tuple(int(r[f]) for f in FIELDS) for r in rows]


def same_rows(got, want):
    return len(got) == len(want) and all(np.array_equal(np.asarray(got[f]).astype(np.uint64), np.asarray(want[f]).astype(np.uint64)) for f in FIELDS)


def render(lists, which, seq_names, genome_names):
    """The text of one set: the query-axis list, then the target-axis list; `name start end other_genome q|t`."""
    lines = []
    for axis in AXES:
        for r in lists[which, axis]:
            lines.append("%s\t%d\t%d\t%s\t%s\n" % (seq_names[int(r["seq"])], int(r["start"]), int(r["end"]), genome_names[int(r["other_genome"])], axis))
    return "".join(lines).encode("utf-8", errors="surrogateescape")


def parse_paf(text):
    """PAF text -> (columns dict, seq_genome, sequence names, genome names): lines with at least 11 fields; names interned in
    order of first appearance (a line's query before its target); genome = the name up to and including its last '#'."""
    ids, gids = {}, {}
    cols = {k: [] for k in ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")}
    for ln in text.split("\n"):
        if ln.endswith("\r"):
            ln = ln[:-1]
        f = ln.split("\t")
        if len(f) < 11:
            continue
        for nm in (f[0], f[5]):
            ids.setdefault(nm, len(ids))
        for k, v in zip(cols, (ids[f[0]], ids[f[5]], int(f[2]), int(f[3]), int(f[7]), int(f[8]))):
            cols[k].append(v)
    seq_genome = np.zeros(max(len(ids), 1), dtype=np.uint32)
    for nm, i in ids.items():
        p = nm.rfind("#")
        seq_genome[i] = gids.setdefault(nm if p < 0 else nm[:p + 1], len(gids))
    return {k: np.array(v, dtype=np.uint32) for k, v in cols.items()}, seq_genome, list(ids), list(gids)
