"""The mosaic restated independently of sweepga_amd/csrc/swg_mosaic.hip: at every base of a sequence the winner is the counted
record of the set that lies over the base with the largest P = weight << 32 | (0xffffffff - record).  Two formulations, neither
the device's (no boundary entries, no slots, no tiles, no sparse tables):

  per base   a u64 array per sequence, np.maximum of P over every record's slice, then run-length encoding.  Coordinates up to a
             few 10^5.
  heap       per sequence one walk over the positions where a record begins or ends with a heap of the open records, closed ones
             dropped lazily.  Any coordinates.

mosaic() gives the rows (ROW_DTYPE, ordered by (seq, start)), share_of() the [G, G] table from rows, rows_text() / share_text()
the two texts of swg_paf_mosaic, paf_texts() both from a PAF text."""
import heapq

import numpy as np

ROW_DTYPE = np.dtype([("seq", "<u4"), ("start", "<u4"), ("end", "<u4"), ("record", "<u4")])
FIELDS = ("seq", "start", "end", "record")
COLS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")
PER_BASE_LIMIT = 300_000   # bases per sequence up to which the per-base form is the default
TOP = 0xffffffff


def axis_columns(cols, axis):
    """(own sequence, other sequence, start, end) on the axis, as int64."""
    names = ("q_id", "t_id", "q_start", "q_end") if axis == 0 else ("t_id", "q_id", "t_start", "t_end")
    return tuple(np.asarray(cols[k]).astype(np.int64) for k in names)


def weights(cols, axis, weight=None, by_length=False):
    if by_length:
        _, _, s, e = axis_columns(cols, axis)
        return e - s
    return np.asarray(cols["matches"] if weight is None else weight).astype(np.int64)


def competitors(cols, seq_genome, mask, w, axis):
    """{seq: [(start, end, P)]} of the counted records of the set with non-zero length on the axis."""
    g = np.asarray(seq_genome).astype(np.int64)
    seq, other, s, e = axis_columns(cols, axis)
    use = (g[seq] != g[other]) & (e > s)
    if mask is not None:
        use &= np.asarray(mask).astype(bool)
    out = {}
    for r in np.flatnonzero(use):
        out.setdefault(int(seq[r]), []).append((int(s[r]), int(e[r]), (int(w[r]) << 32) | (TOP - int(r))))
    return out


def winners_per_base(ivs):
    top = max(e for _, e, _ in ivs)
    best = np.zeros(top, dtype=np.uint64)
    for s, e, p in ivs:
        np.maximum(best[s:e], np.uint64(p), out=best[s:e])
    cut = np.flatnonzero(best[1:] != best[:-1]) + 1
    begins, ends = np.concatenate([[0], cut]), np.concatenate([cut, [top]])
    return [(int(a), int(b), int(best[a])) for a, b in zip(begins, ends) if best[a]]


def winners_by_heap(ivs):
    at = {}
    for s, e, p in ivs:
        at.setdefault(s, []).append((-p, e))
        at.setdefault(e, [])
    heap, out, positions = [], [], sorted(at)
    for x, nxt in zip(positions, positions[1:] + [None]):
        for item in at[x]:
            heapq.heappush(heap, item)
        while heap and heap[0][1] <= x:
            heapq.heappop(heap)
        if nxt is None:
            assert not heap
        elif heap:
            p = -heap[0][0]
            if out and out[-1][1] == x and out[-1][2] == p:
                out[-1] = (out[-1][0], nxt, p)
            else:
                out.append((x, nxt, p))
    return out


def mosaic(cols, seq_genome, mask=None, weight=None, axis=0, by_length=False, per_base=None):
    """The rows of one set on one axis.  mask: the kept records (None = all); weight: None = cols["matches"]."""
    w = weights(cols, axis, weight, by_length)
    rows = []
    for seq, ivs in sorted(competitors(cols, seq_genome, mask, w, axis).items()):
        top = max(e for _, e, _ in ivs)
        use_base = (top <= PER_BASE_LIMIT and len(ivs) * 2_000 >= top) if per_base is None else per_base   # (few records: the walk is quicker)
        rows += [(seq, a, b, TOP - (p & TOP)) for a, b, p in (winners_per_base(ivs) if use_base else winners_by_heap(ivs))]
    return np.array(rows, dtype=ROW_DTYPE) if rows else np.zeros(0, dtype=ROW_DTYPE)


def bases_of(rows):
    return int((rows["end"].astype(np.int64) - rows["start"]).sum())


def share_of(rows, cols, seq_genome, axis, G=None):
    g = np.asarray(seq_genome).astype(np.int64)
    G = G or int(g.max()) + 1
    other = np.asarray(cols["t_id" if axis == 0 else "q_id"]).astype(np.int64)
    out = np.zeros((G, G), dtype=np.uint64)
    for r in rows:
        out[g[int(r["seq"])], g[other[int(r["record"])]]] += np.uint64(int(r["end"]) - int(r["start"]))
    return out


def as_tuples(rows):
    return [tuple(int(r[f]) for f in FIELDS) for r in rows]


def same_rows(got, want):
    return len(got) == len(want) and all(np.array_equal(np.asarray(got[f]).astype(np.uint64), np.asarray(want[f]).astype(np.uint64)) for f in FIELDS)


def check_rows(rows, cols, axis):
    """Every row's record covers the row on the axis; the rows of a sequence do not overlap and are ordered."""
    seq, _, s, e = axis_columns(cols, axis)
    r = rows["record"].astype(np.int64)
    assert (seq[r] == rows["seq"]).all() and (s[r] <= rows["start"]).all() and (rows["end"] <= e[r]).all() and (rows["start"] < rows["end"]).all()
    same = rows["seq"][1:] == rows["seq"][:-1]
    assert (rows["seq"][1:] >= rows["seq"][:-1]).all() and (rows["start"][1:][same] >= rows["end"][:-1][same]).all()
    touch = same & (rows["start"][1:] == rows["end"][:-1])
    assert (rows["record"][1:][touch] != rows["record"][:-1][touch]).all()      # maximal


def rows_text(seq_names, rows, cols, strand, w, axis):
    other = np.asarray(cols["t_id" if axis == 0 else "q_id"]).astype(np.int64)
    os_, oe = (cols["t_start"], cols["t_end"]) if axis == 0 else (cols["q_start"], cols["q_end"])
    out = []
    for seq, a, b, r in as_tuples(rows):
        out.append("%s\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\n" % (seq_names[seq], a, b, seq_names[int(other[r])], "-" if strand[r] else "+", r, int(w[r]),
                                                             int(os_[r]), int(oe[r])))
    return "".join(out).encode("utf-8", errors="surrogateescape")


def share_text(genome_names, share, bases):
    lines = ["genome\tother_genome\tbases\n"]
    G = len(genome_names)
    lines += ["%s\t%s\t%d\n" % (genome_names[g], genome_names[h], int(share[g, h])) for g in range(G) for h in range(G) if share[g, h]]
    lines.append("#total\t%d\n" % bases)
    return "".join(lines).encode("utf-8", errors="surrogateescape")


def parse_paf(text):
    """PAF text -> (columns dict with matches, strand, seq_genome, sequence names, genome names): lines with at least 11 fields;
    names interned in order of first appearance (a line's query before its target); genome = the name up to its last '#'."""
    ids, gids = {}, {}
    cols = {k: [] for k in COLS + ("matches",)}
    strand = []
    for ln in text.split("\n"):
        f = ln.rstrip("\r").split("\t")
        if len(f) < 11:
            continue
        for nm in (f[0], f[5]):
            ids.setdefault(nm, len(ids))
        for k, v in zip(cols, (ids[f[0]], ids[f[5]], int(f[2]), int(f[3]), int(f[7]), int(f[8]), int(f[9]))):
            cols[k].append(v)
        strand.append(f[4] == "-")
    seq_genome = np.zeros(max(len(ids), 1), dtype=np.uint32)
    for nm, i in ids.items():
        p = nm.rfind("#")
        seq_genome[i] = gids.setdefault(nm if p < 0 else nm[:p + 1], len(gids))
    return {k: np.array(v, dtype=np.uint32) for k, v in cols.items()}, np.array(strand, dtype=bool), seq_genome, list(ids), list(gids)


def paf_texts(text, kept, axis=0, set_="kept", by="matches"):
    """(rows text, share text) of a PAF text under its last-'#' genome map; kept: a boolean mask over its records."""
    cols, strand, seq_genome, names, genomes = parse_paf(text)
    if len(cols["q_id"]) == 0:
        return b"", share_text([], None, 0)
    w = weights(cols, axis, None, by == "length")
    rows = mosaic(cols, seq_genome, kept if set_ == "kept" else None, w, axis)
    return rows_text(names, rows, cols, strand, w, axis), share_text(genomes, share_of(rows, cols, seq_genome, axis, len(genomes)), bases_of(rows))
