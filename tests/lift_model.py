"""Brute-force model of the lift: a loop over regions x records with Python integers, no index, no sort
beyond sorted() of the finished rows by the defined key.  Every row it makes is checked against the four consequences of the
projection rule.  `candidates` restates the prune (prefix maximum of ends per sequence) to give the number the device reports."""
import numpy as np

COLS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")
UNKNOWN = 2**32 - 1
ROW_FIELDS = ("region", "record", "src_start", "src_end", "dst_seq", "dst_start", "dst_end", "flags")
SUMMARY_HEADER = "label\tsequence\tstart\tend\tall_q\tall_t\tkept_q\tkept_t\tstate\n"
SIDES = (("q_id", "q_start", "q_end", "t_id", "t_start", "t_end"), ("t_id", "t_start", "t_end", "q_id", "q_start", "q_end"))


def project(a, b, s0, s1, d0, d1, minus):
    """The clip and the destination interval of a hit: (ca, cb, dst_start, dst_end)."""
    L, D = s1 - s0, d1 - d0
    ca, cb = max(a, s0), min(b, s1)
    o0, o1 = ca - s0, cb - s0
    assert 0 <= o0 < o1 <= L
    f0, c1 = o0 * D // L, -((-o1 * D) // L)
    dst = (d1 - c1, d1 - f0) if minus else (d0 + f0, d0 + c1)
    assert d0 <= dst[0] <= dst[1] <= d1                                   # inside [d0, d1]
    assert dst[0] < dst[1] if D > 0 else dst == (d0, d0)                  # non-empty whenever D > 0
    if a <= s0 and b >= s1:
        assert dst == (d0, d1)                                            # the whole source side gives exactly the other side
    return ca, cb, dst[0], dst[1]


def lift(cols, strand, kept, regions, set_=0, axes=3):
    """cols: numpy columns; strand: 0 = '+'; kept: a boolean per record or None; regions: (seq, start, end) triples.
    -> (rows: list of ROW_FIELDS tuples in row order, summary: (m, 2, 2) array of hits[region][set][axis])."""
    c = {k: np.asarray(cols[k]).astype(np.int64) for k in COLS}
    strand = np.asarray(strand)
    n = len(strand)
    kept_arr = np.zeros(n, dtype=bool) if kept is None else np.asarray(kept, dtype=bool)
    summary = np.zeros((len(regions), 2, 2), dtype=np.uint32)
    keyed = []
    for r, (seq, a, b) in enumerate(regions):
        seq, a, b = int(seq), int(a), int(b)
        assert a <= b
        for axis in (0, 1):
            if not (axes >> axis & 1) or seq == UNKNOWN:
                continue
            sid, ss, se, did, ds, de = (c[k] for k in SIDES[axis])
            hit = (sid == seq) & (se > ss) & (np.maximum(a, ss) < np.minimum(b, se))
            for i in np.flatnonzero(hit):
                i = int(i)
                s0, s1, d0, d1, minus = int(ss[i]), int(se[i]), int(ds[i]), int(de[i]), int(strand[i] != 0)
                summary[r, 0, axis] += 1
                summary[r, 1, axis] += int(kept_arr[i])
                if set_ == 1 and not kept_arr[i]:
                    continue
                ca, cb, t0, t1 = project(a, b, s0, s1, d0, d1, minus)
                if b < 2**32 - 1:                                         # growing the region never shrinks dst
                    _, _, g0, g1 = project(max(a - 1, 0), b + 1, s0, s1, d0, d1, minus)
                    assert g0 <= t0 and t1 <= g1
                keyed.append(((r, axis, s0, i), (r, i, ca, cb, int(did[i]), t0, t1, minus | axis << 1)))
    return [row for _, row in sorted(keyed)], summary


def candidates(cols, regions, axes=3):
    """[query axis, target axis]: per region, hi - p0 over the records of non-zero length of its sequence in (start, record) order:
    hi = those with start < end of the region, p0 = the first whose prefix maximum of ends exceeds the region's start.  Empty and
    unknown regions have none."""
    c = {k: np.asarray(cols[k]).astype(np.int64) for k in COLS}
    out = [0, 0]
    for axis in (0, 1):
        if not (axes >> axis & 1):
            continue
        sid, ss, se = (c[k] for k in SIDES[axis][:3])
        per_seq = {}
        for seq, a, b in regions:
            seq, a, b = int(seq), int(a), int(b)
            if seq == UNKNOWN or a == b:
                continue
            if seq not in per_seq:
                idx = np.flatnonzero((sid == seq) & (se > ss))
                idx = idx[np.argsort(ss[idx], kind="stable")]
                per_seq[seq] = (ss[idx], np.maximum.accumulate(se[idx]) if len(idx) else se[idx])
            starts, pmax = per_seq[seq]
            hi = int(np.searchsorted(starts, b, side="left"))
            p0 = int(np.searchsorted(pmax, a, side="right"))
            out[axis] += max(hi - p0, 0)
    return out


def rows_array(rows):
    from sweepga_amd.lift import ROW_DTYPE
    out = np.zeros(len(rows), dtype=ROW_DTYPE)
    for k, row in enumerate(rows):
        out[k] = row
    return out


# ---- the texts of swg_paf_lift ----------------------------------------------------------------------------------------------------
class BedError(ValueError):
    def __init__(self, line):
        super().__init__("BED line %d" % line)
        self.line = line


def parse_bed(text, ids):
    """-> [(seq or UNKNOWN, start, end, label, name)] in line order; BedError(line number) on a malformed line."""
    out = []
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    for no, ln in enumerate(lines, 1):
        if ln.endswith("\r"):
            ln = ln[:-1]
        if not ln or ln[0] == "#" or ln.startswith("track") or ln.startswith("browser"):
            continue
        f = ln.split("\t")
        if len(f) < 3 or not f[0]:
            raise BedError(no)
        vals = []
        for t in f[1:3]:
            if not t or len(t) > 10 or any(ch not in "0123456789" for ch in t) or int(t) >= 2**32:
                raise BedError(no)
            vals.append(int(t))
        if vals[0] > vals[1]:
            raise BedError(no)
        label = f[3] if len(f) > 3 and f[3] else "%s:%d-%d" % (f[0], vals[0], vals[1])
        out.append((ids.get(f[0], UNKNOWN), vals[0], vals[1], label, f[0]))
    return out


def parse_paf(text):
    """PAF text -> (columns, strand, sequence names): lines with at least 11 fields, names interned in order of first appearance
    (a line's query before its target)."""
    ids = {}
    cols = {k: [] for k in COLS}
    strand = []
    for ln in text.split("\n"):
        if ln.endswith("\r"):
            ln = ln[:-1]
        f = ln.split("\t")
        if len(f) < 11:
            continue
        for nm in (f[0], f[5]):
            ids.setdefault(nm, len(ids))
        for k, v in zip(COLS, (ids[f[0]], ids[f[5]], int(f[2]), int(f[3]), int(f[7]), int(f[8]))):
            cols[k].append(v)
        strand.append(1 if f[4] == "-" else 0)
    return {k: np.array(v, dtype=np.uint32) for k, v in cols.items()}, np.array(strand, dtype=np.uint8), list(ids)


def paf_texts(paf_text, kept, bed_text, set_=1, axes=3):
    """(rows text, summary text) as swg_paf_lift gives them; kept None = no status."""
    cols, strand, names = parse_paf(paf_text)
    bed = parse_bed(bed_text, {nm: i for i, nm in enumerate(names)})
    if not bed or not len(strand):
        return "", SUMMARY_HEADER
    rows, summary = lift(cols, strand, kept, [b[:3] for b in bed], set_, axes)
    out = []
    for r, i, ca, cb, dseq, t0, t1, flags in rows:
        out.append("\t".join([names[dseq], str(t0), str(t1), bed[r][3], bed[r][4], str(ca), str(cb), "-" if flags & 1 else "+",
                              "t" if flags & 2 else "q", str(i)]) + "\n")
    summ = [SUMMARY_HEADER]
    for r, (seq, a, b, label, name) in enumerate(bed):
        h = summary[r]
        any_all, any_kept = int(h[0].sum()) > 0, int(h[1].sum()) > 0
        state = "unknown" if seq == UNKNOWN else "none" if not any_all else "all" if kept is None else "kept" if any_kept else "lost"
        k = ["-", "-"] if kept is None else [str(h[1, 0]), str(h[1, 1])]
        summ.append("\t".join([label, name, str(a), str(b), str(h[0, 0]), str(h[0, 1]), *k, state]) + "\n")
    return "".join(out), "".join(summ)
