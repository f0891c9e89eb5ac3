"""Breadth restated independently of sweepga_amd/csrc/swg_breadth.hip: per ordered genome pair, the bases of each side under at
least one inter-genome mapping.  Two formulations, neither the device's (no sort key of segment and start, no running maximum):

  union_length      one segment in plain Python: sort the intervals, merge them, add up the merged pieces;
  covered_by_depth  many segments at once in numpy: every interval is a +1 event at its start and a -1 event at its end, the
                    events of a segment are walked in position order and a stretch counts while the depth is positive.

breadth() groups the records into segments (one sequence against one genome of the other side) and uses the first for small inputs,
the second for large ones; tests/test_breadth_cpu.py holds the two against each other.  render() writes the --breadth report
from (integers, sizes, names)."""
import numpy as np

PAIR_FIELDS = ("q_genome", "t_genome", "q_bases", "t_bases", "q_union", "t_union", "first_record")
MODEL_DTYPE = np.dtype([("q_genome", "<u4"), ("t_genome", "<u4"), ("q_bases", "<u8"), ("t_bases", "<u8"), ("q_union", "<u8"),
                        ("t_union", "<u8"), ("first_record", "<u8")])
HEADER = ("set", "query_genome", "target_genome", "q_bases", "q_union", "q_size", "q_breadth_pct", "q_depth", "t_bases", "t_union",
          "t_size", "t_breadth_pct", "t_depth")


def union_length(intervals):
    """|union of half-open [s, e)| by sort and merge."""
    total, cur_s, cur_e = 0, None, None
    for s, e in sorted((int(s), int(e)) for s, e in intervals):
        if e <= s:
            continue                      # zero length: nothing
        if cur_e is None or s > cur_e:    # a gap: close the piece (touching, s == cur_e, extends it)
            if cur_e is not None:
                total += cur_e - cur_s
            cur_s, cur_e = s, e
        elif e > cur_e:
            cur_e = e
    if cur_e is not None:
        total += cur_e - cur_s
    return total


def covered_by_depth(group, start, end, n_groups):
    """Per group id, the length of the positions covered by at least one of its intervals (event sweep, vectorised)."""
    m = len(group)
    out = np.zeros(n_groups, dtype=np.int64)
    if m == 0:
        return out
    g = np.concatenate([group, group]).astype(np.int64)
    pos = np.concatenate([start, end]).astype(np.int64)
    delta = np.concatenate([np.ones(m, dtype=np.int64), -np.ones(m, dtype=np.int64)])
    # by group, then position, starts ahead of ends at one position (one integer per event when it fits: a single-key sort is
    # what makes 10^7 records affordable)
    span = int(pos.max()) + 1
    if (int(n_groups) + 1) * span * 2 < 2**62:
        order = np.argsort((g * span + pos) * 2 + (delta < 0), kind="stable")
    else:
        order = np.lexsort((-delta, pos, g))
    g, pos, delta = g[order], pos[order], delta[order]
    depth = np.cumsum(delta)                   # returns to 0 at the end of every group
    step = np.diff(pos, append=pos[-1])
    same = np.append(g[1:] == g[:-1], False)
    np.add.at(out, g, np.where(same & (depth > 0), step, 0))
    return out


def _groups(a, b):
    """Distinct (a, b) rows in ascending order and, per element, the row it belongs to."""
    if len(a) == 0:
        return np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.int64)
    width = int(b.max()) + 1
    codes, inverse = np.unique(a * width + b, return_inverse=True)   # (a, b < 2^32: the code fits 64 bits)
    return np.stack([codes // width, codes % width], axis=1), inverse.reshape(-1)


def breadth(q_id, t_id, q_start, q_end, t_start, t_end, seq_genome, sel=None, vectorised=None):
    """The pairs of the records `sel` selects (a boolean mask; None = all) as MODEL_DTYPE, in order of first record."""
    n = len(q_id)
    idx = np.arange(n, dtype=np.int64) if sel is None else np.flatnonzero(sel).astype(np.int64)
    seq_genome = np.asarray(seq_genome).astype(np.int64)
    q, t = np.asarray(q_id)[idx].astype(np.int64), np.asarray(t_id)[idx].astype(np.int64)
    gq, gt = seq_genome[q], seq_genome[t]
    inter = gq != gt
    idx, q, t, gq, gt = idx[inter], q[inter], t[inter], gq[inter], gt[inter]
    cols = [np.asarray(c)[idx].astype(np.int64) for c in (q_start, q_end, t_start, t_end)]
    pair_rows, pair_of = _groups(gq, gt)
    n_pairs = len(pair_rows)
    out = np.zeros(n_pairs, dtype=MODEL_DTYPE)
    if n_pairs == 0:
        return out
    if vectorised is None:
        vectorised = len(idx) > 20_000
    first = np.full(n_pairs, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(first, pair_of, idx)
    sums = {}
    for side, (seq, s, e) in (("q", (q, cols[0], cols[1])), ("t", (t, cols[2], cols[3]))):
        bases = np.zeros(n_pairs, dtype=np.int64)
        np.add.at(bases, pair_of, e - s)
        union = np.zeros(n_pairs, dtype=np.int64)
        # a segment: one sequence of this side within one ordered genome pair (the pair fixes the genome of the other side)
        seg_rows, seg_of = _groups(pair_of, seq)
        if vectorised:
            per_seg = covered_by_depth(seg_of, s, e, len(seg_rows))
        else:
            members = [[] for _ in range(len(seg_rows))]
            for k, sg in enumerate(seg_of):
                members[int(sg)].append((s[k], e[k]))
            per_seg = np.array([union_length(mm) for mm in members], dtype=np.int64)
        np.add.at(union, seg_rows[:, 0], per_seg)
        sums[side] = (bases, union)
    order = np.argsort(first, kind="stable")
    out["q_genome"], out["t_genome"] = pair_rows[order, 0], pair_rows[order, 1]
    out["q_bases"], out["q_union"] = sums["q"][0][order], sums["q"][1][order]
    out["t_bases"], out["t_union"] = sums["t"][0][order], sums["t"][1][order]
    out["first_record"] = first[order]
    return out


def same_pairs(got, want):
    """Field by field (the two dtypes may come from different modules)."""
    return got is not None and len(got) == len(want) and all(np.array_equal(np.asarray(got[f]).astype(np.uint64),
                                                                               np.asarray(want[f]).astype(np.uint64)) for f in PAIR_FIELDS)


def by_key(pairs):
    """{(q_genome, t_genome): (q_bases, t_bases, q_union, t_union)}: what does not depend on the record order."""
    return {(int(p["q_genome"]), int(p["t_genome"])): tuple(int(p[f]) for f in PAIR_FIELDS[2:6]) for p in pairs}


# ---- the report ------------------------------------------------------------------------------------------------------------
def _ratio(num, den, scale):
    return "-" if den == 0 else "%.4f" % (scale * float(num) / float(den))


def _side(bases, union, size):
    return [str(bases), str(union), str(size), _ratio(union, size, 100.0), _ratio(bases, union, 1.0)]


def render(sets, genome_names, detailed):
    """sets: [(label, pairs, genome_sizes)] with genome_sizes indexable by genome id; -> the report as bytes."""
    lines = ["\t".join(HEADER)]
    for label, pairs, sizes in sets:
        tot = [0] * 6
        for p in pairs:
            gq, gt = int(p["q_genome"]), int(p["t_genome"])
            vals = [int(p["q_bases"]), int(p["q_union"]), int(sizes[gq]), int(p["t_bases"]), int(p["t_union"]), int(sizes[gt])]
            tot = [a + b for a, b in zip(tot, vals)]
            if detailed:
                lines.append("\t".join([label, genome_names[gq], genome_names[gt]] + _side(*vals[:3]) + _side(*vals[3:])))
        lines.append("\t".join([label, "*", "*"] + _side(*tot[:3]) + _side(*tot[3:])))
    return ("\n".join(lines) + "\n").encode("utf-8", errors="surrogateescape")


def parse_paf(text):
    """What the report needs of PAF text, as alnstats reads it: lines with at least 11 fields; names interned in order of first
    appearance; genome = the name up to and including its last '#'; a sequence's size = the length on the last line that names
    it (the target's after the query's on one line); a genome's size = the sum over its sequences.
    -> (columns dict, seq_genome, genome names, genome sizes)."""
    ids, gids, size = {}, {}, {}
    cols = {k: [] for k in ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")}
    for ln in text.split("\n"):
        if ln.endswith("\r"):
            ln = ln[:-1]
        f = ln.split("\t")
        if len(f) < 11:
            continue
        for nm in (f[0], f[5]):
            ids.setdefault(nm, len(ids))
        size[f[0]] = int(f[1])
        size[f[5]] = int(f[6])
        for k, v in zip(cols, (ids[f[0]], ids[f[5]], int(f[2]), int(f[3]), int(f[7]), int(f[8]))):
            cols[k].append(v)
    seq_genome = np.zeros(max(len(ids), 1), dtype=np.uint32)
    for nm, i in ids.items():
        p = nm.rfind("#")
        seq_genome[i] = gids.setdefault(nm if p < 0 else nm[:p + 1], len(gids))
    gsize = [0] * len(gids)
    for nm, i in ids.items():
        gsize[int(seq_genome[i])] += size[nm]
    return {k: np.array(v, dtype=np.uint32) for k, v in cols.items()}, seq_genome, list(gids), gsize
