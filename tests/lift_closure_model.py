"""Brute-force model of the transitive lift with Python integers: per region a dict of sequence -> list of
disjoint intervals, tests.lift_model.project for the projection, no index and no sort beyond sorted().  Everything it makes is
checked against the consequences of the definition: with one hop the rows of hop 1 are the merged dst of the lift's rows minus the
region itself, raising max_hops never touches a row of an earlier hop, V only grows, the rows of a region never overlap."""
import numpy as np

from tests import lift_model as lm

UNKNOWN = lm.UNKNOWN
SUMMARY_HEADER = "label\tsequence\tstart\tend\tpieces\tsequences\tgenomes\tbases\thops\tstate\n"
CUT = 1


def merged(ivs):
    """The maximal intervals of a union: touching intervals are one, a gap of one base separates."""
    out = []
    for a, b in sorted(ivs):
        assert a < b
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [tuple(v) for v in out]


def minus(ivs, cut):
    """ivs \\ cut, both disjoint and sorted: point by point in spirit, interval by interval in practice."""
    out = []
    for a, b in ivs:
        at = a
        for c, d in cut:
            if d <= at or c >= b:
                continue
            if c > at:
                out.append((at, c))
            at = max(at, d)
        if at < b:
            out.append((at, b))
    return out


def hits_of(c, strand, kept_arr, set_, axes, seq, x, y):
    """The non-empty dst intervals (dst_seq, start, end) of the region (seq, x, y) over the wanted axes: section 23's hits."""
    out = []
    for axis in (0, 1):
        if not (axes >> axis & 1):
            continue
        sid, ss, se, did, ds, de = (c[k] for k in lm.SIDES[axis])
        hit = (sid == seq) & (se > ss) & (np.maximum(x, ss) < np.minimum(y, se))
        if set_ == 1:
            hit &= kept_arr
        for i in np.flatnonzero(hit):
            i = int(i)
            _, _, t0, t1 = lm.project(x, y, int(ss[i]), int(se[i]), int(ds[i]), int(de[i]), int(strand[i] != 0))
            if t0 < t1:
                out.append((int(did[i]), t0, t1))
    return out


def closure(cols, strand, kept, regions, max_hops, min_len=100, set_=0, axes=3, check=True):
    """-> (rows: (region, seq, start, end, hop, 0) in row order, summary: (bases, pieces, sequences, hops, flags) per region,
    info: hops_run, projections, candidates [query axis, target axis])."""
    assert 1 <= max_hops <= 65535
    c = {k: np.asarray(cols[k]).astype(np.int64) for k in lm.COLS}
    strand = np.asarray(strand)
    kept_arr = np.zeros(len(strand), dtype=bool) if kept is None else np.asarray(kept, dtype=bool)
    rows, summary = [], []
    walked_per_hop = [[] for _ in range(max_hops + 1)]
    hops_run = projections = 0
    for r, (seq, a, b) in enumerate(regions):
        seq, a, b = int(seq), int(a), int(b)
        assert a <= b
        mine = []
        if seq != UNKNOWN and a < b and len(strand):
            visited = {seq: [(a, b)]}
            frontier = [(seq, a, b)]
            mine.append((r, seq, a, b, 0, 0))
            for hop in range(1, max_hops + 1):
                if not frontier:
                    break
                hops_run = max(hops_run, hop)
                walked = [p for p in frontier if hop == 1 or p[2] - p[1] >= min_len]
                walked_per_hop[hop] += walked
                made = {}
                for s, x, y in walked:
                    for dseq, t0, t1 in hits_of(c, strand, kept_arr, set_, axes, s, x, y):
                        made.setdefault(dseq, []).append((t0, t1))
                        projections += 1
                frontier = []
                for dseq in sorted(made):
                    before = visited.get(dseq, [])
                    p = merged(made[dseq])
                    new = minus(p, before)
                    after = merged(before + p)
                    assert minus(before, after) == [] and minus(new, before) == new          # V only grows; F_h lies outside V_{h-1}
                    assert merged(new) == new
                    visited[dseq] = after
                    frontier += [(dseq, x, y) for x, y in new]
                mine += [(r, s, x, y, hop, 0) for s, x, y in frontier]
        elif seq != UNKNOWN and a < b:
            mine.append((r, seq, a, b, 0, 0))                                                  # no records: hop 0 is all there is
        mine.sort(key=lambda w: (w[1], w[2]))
        for u, w in zip(mine, mine[1:]):
            assert u[1] != w[1] or u[3] <= w[2], (u, w)                                        # the rows of a region never overlap
        top = max((w[4] for w in mine), default=0)
        cut = any(w[4] == max_hops and w[3] - w[2] >= max(min_len, 1) for w in mine)
        summary.append((sum(w[3] - w[2] for w in mine), len(mine), len({w[1] for w in mine}), top, CUT if cut else 0))
        rows += mine
    cand = [0, 0]
    for walked in walked_per_hop:
        got = lm.candidates(cols, walked, axes) if walked else [0, 0]
        cand = [cand[0] + got[0], cand[1] + got[1]]
    if check and len(strand):
        one = [w for w in rows if w[4] <= 1] if max_hops > 1 else rows
        if max_hops > 1:                                                                       # raising max_hops touches no earlier row
            fewer = closure(cols, strand, kept, regions, max_hops - 1, min_len, set_, axes, check=False)[0]
            assert fewer == [w for w in rows if w[4] < max_hops]
            one = closure(cols, strand, kept, regions, 1, min_len, set_, axes, check=False)[0] if max_hops > 2 else fewer
        lifted, _ = lm.lift(cols, strand, kept, [tuple(int(v) for v in g) for g in regions], set_, axes)
        want = {}
        for r, _i, _ca, _cb, dseq, t0, t1, _f in lifted:
            if t0 < t1:
                want.setdefault((r, dseq), []).append((t0, t1))
        hop1 = {}
        for r, s, x, y, hop, _ in one:
            if hop == 1:
                hop1.setdefault((r, s), []).append((x, y))
        for (r, dseq), ivs in want.items():
            own = [(int(regions[r][1]), int(regions[r][2]))] if int(regions[r][0]) == dseq else []
            assert minus(merged(ivs), own) == hop1.pop((r, dseq), []), (r, dseq)
        assert not hop1
    return rows, summary, {"hops_run": hops_run, "projections": projections, "candidates": cand}


def rows_array(rows):
    from sweepga_amd.lift import CLOSURE_ROW_DTYPE
    out = np.zeros(len(rows), dtype=CLOSURE_ROW_DTYPE)
    for k, row in enumerate(rows):
        out[k] = row
    return out


def summary_array(summary):
    from sweepga_amd.lift import CLOSURE_SUMMARY_DTYPE
    out = np.zeros(len(summary), dtype=CLOSURE_SUMMARY_DTYPE)
    for k, row in enumerate(summary):
        out[k] = row
    return out


def genome_of(name):
    return name[:name.rfind("#") + 1] if "#" in name else name


def paf_texts(paf_text, kept, bed_text, max_hops, min_len=100, set_=1, axes=3):
    """(rows text, summary text) as swg_paf_lift_closure gives them; kept None = no status."""
    cols, strand, names = lm.parse_paf(paf_text)
    bed = lm.parse_bed(bed_text, {nm: i for i, nm in enumerate(names)})
    if not bed:
        return "", SUMMARY_HEADER
    rows, summary, _ = closure(cols, strand, kept, [b[:3] for b in bed], max_hops, min_len, set_, axes)
    out = ["\t".join([names[s], str(x), str(y), bed[r][3], str(hop)]) + "\n" for r, s, x, y, hop, _ in rows]
    genomes = [set() for _ in bed]
    for r, s, *_ in rows:
        genomes[r].add(genome_of(names[s]))
    summ = [SUMMARY_HEADER]
    for r, (seq, a, b, label, name) in enumerate(bed):
        bases, pieces, sequences, hops, flags = summary[r]
        state = "unknown" if seq == UNKNOWN else "none" if hops == 0 else "cut" if flags & CUT else "closed"
        summ.append("\t".join([label, name, str(a), str(b), str(pieces), str(sequences), str(len(genomes[r])), str(bases), str(hops), state]) + "\n")
    return "".join(out), "".join(summ)
