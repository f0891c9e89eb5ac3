"""The windows report, written from its definitions (include/sweepga_gpu.h): the yardstick of
csrc/swg_windows.hip.  All values are integers and every comparison is exact.

  axis        on axis 0 record r lies on s = q_id[r] over [a, b) = [q_start, q_end) and its other sequence is o = t_id[r]; on axis 1
              the roles and the columns swap.  m = weight[r]; weight None: the matches column.
  takes part  (set ALL) genome[s] != genome[o], a < b, and other_genome is None or genome[o] == other_genome.
  set KEPT    the records of ALL with status != 0; status None: no KEPT set, every [1] entry is 0.
  windows     sequence s has K_s = ceil(seq_len[s] / W) windows, window k = [k W, min((k + 1) W, seq_len[s])); a record that takes
              part with b > seq_len[s] is an error (ValueError naming the smallest such record); a sequence is listed when a record of
              ALL lies on it.
  per window and set, ov(r, k) = the length of [a, b) in window k: n = the records with ov > 0, depth = sum of ov, covered = the bases
              under at least one record (by sorting and merging the intervals), matches = sum of floor(ov * m / (b - a)).
  rows        one per window of every listed sequence, (seq, k) ascending.
  summary     one entry per listed sequence: windows, empty[set] (windows with covered == 0; 0 for KEPT without a status), covered,
              depth and matches summed over its windows, records[set] = the records that take part on it.

Here the work is per record and window (numpy over the windows one record touches): nothing of the device's differences and
prefix sums."""
import numpy as np

ROW_DTYPE = np.dtype([(k, "<u4") for k in ("seq", "index", "start", "end")] + [("n", "<u4", (2,)), ("covered", "<u4", (2,)), ("depth", "<u8", (2,)),
                                                                                ("matches", "<u8", (2,))])
SEQ_DTYPE = np.dtype([("seq", "<u4"), ("windows", "<u4"), ("empty", "<u4", (2,))] + [(k, "<u8", (2,)) for k in ("covered", "depth", "matches", "records")])
ROWS_HEADER = "#sequence\tstart\tend\tn_all\tdepth_all\tcovered_all\tmatches_all\tn_kept\tdepth_kept\tcovered_kept\tmatches_kept\n"
SUMMARY_HEADER = ("#sequence\tlength\twindows\tempty_all\tempty_kept\tcovered_all\tcovered_kept\tdepth_all\tdepth_kept\tmatches_all\tmatches_kept\t"
                  "records_all\trecords_kept\n")


def by_role(cols, axis):
    """-> s, o, a, b of every record as int64 arrays."""
    q, t = np.asarray(cols["q_id"], dtype=np.int64), np.asarray(cols["t_id"], dtype=np.int64)
    if axis:
        return t, q, np.asarray(cols["t_start"], dtype=np.int64), np.asarray(cols["t_end"], dtype=np.int64)
    return q, t, np.asarray(cols["q_start"], dtype=np.int64), np.asarray(cols["q_end"], dtype=np.int64)


def taking(cols, seq_len, genome, status=None, axis=0, other_genome=None):
    """-> (the records of ALL, the records of KEPT), ascending; ValueError for one that ends beyond its sequence."""
    s, o, a, b = by_role(cols, axis)
    genome = np.asarray(genome, dtype=np.int64)
    sets = ([], [])
    for r in range(len(s)):
        if genome[s[r]] == genome[o[r]] or a[r] >= b[r] or (other_genome is not None and genome[o[r]] != other_genome):
            continue
        if b[r] > int(seq_len[s[r]]):
            raise ValueError(f"record {r} takes part and ends beyond its sequence")
        sets[0].append(r)
        if status is not None and status[r] != 0:
            sets[1].append(r)
    return sets


def overlaps(a, b, W):
    """The windows [a, b) touches and its overlap with each: (k as int64 [..], ov as uint64 [..]); a < b."""
    k = np.arange(a // W, (b - 1) // W + 1, dtype=np.int64)
    lo, hi = np.maximum(k * W, a), np.minimum((k + 1) * W, b)
    return k, (hi - lo).astype(np.uint64)


def merged(intervals):
    """The union of half-open intervals as disjoint ones, by sorting; touching intervals join."""
    out = []
    for a, b in sorted(intervals):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def windows(cols, seq_len, genome, status=None, axis=0, window=10_000, other_genome=None, weight=None):
    """-> (rows as ROW_DTYPE, seqs as SEQ_DTYPE)."""
    W = int(window)
    s, _, a, b = by_role(cols, axis)
    m = np.asarray(weight if weight is not None else cols["matches"], dtype=np.uint64)
    sets = taking(cols, seq_len, genome, status, axis, other_genome)
    listed = sorted({int(s[r]) for r in sets[0]})
    table = {}
    for q in listed:
        K = (int(seq_len[q]) + W - 1) // W
        table[q] = {k: np.zeros((2, K), dtype=np.uint64) for k in ("n", "depth", "covered", "matches")}
        table[q]["records"] = [0, 0]
    for which, records in enumerate(sets):
        intervals = {}
        for r in records:
            t = table[int(s[r])]
            k, ov = overlaps(int(a[r]), int(b[r]), W)
            t["n"][which, k] += np.uint64(1)
            t["depth"][which, k] += ov
            t["matches"][which, k] += ov * m[r] // np.uint64(int(b[r] - a[r]))      # (the product is below 2^64)
            t["records"][which] += 1
            intervals.setdefault(int(s[r]), []).append((int(a[r]), int(b[r])))
        for q, iv in intervals.items():
            for lo, hi in merged(iv):
                k, ov = overlaps(lo, hi, W)
                table[q]["covered"][which, k] += ov
    rows = np.zeros(sum(t["n"].shape[1] for t in table.values()), dtype=ROW_DTYPE)
    seqs = np.zeros(len(listed), dtype=SEQ_DTYPE)
    at = 0
    for j, q in enumerate(listed):
        t, length = table[q], int(seq_len[q])
        K = t["n"].shape[1]
        part = rows[at:at + K]
        index = np.arange(K, dtype=np.int64)
        part["seq"], part["index"], part["start"], part["end"] = q, index, index * W, np.minimum((index + 1) * W, length)
        for k in ("n", "depth", "covered", "matches"):
            part[k] = t[k].T
        at += K
        seqs[j]["seq"], seqs[j]["windows"] = q, K
        for which in range(2):
            seqs[j]["empty"][which] = int((t["covered"][which] == 0).sum()) if which == 0 or status is not None else 0
            for k in ("covered", "depth", "matches"):
                seqs[j][k][which] = int(t[k][which].sum(dtype=np.uint64))
            seqs[j]["records"][which] = t["records"][which]
    return rows, seqs


def rows_text(rows, names):
    out = [ROWS_HEADER]
    for r in rows:
        f = [names[int(r["seq"])], int(r["start"]), int(r["end"])]
        for which in range(2):
            f += [int(r[k][which]) for k in ("n", "depth", "covered", "matches")]
        out.append("\t".join(str(x) for x in f) + "\n")
    return "".join(out).encode()


def summary_text(seqs, names, seq_len):
    out = [SUMMARY_HEADER]
    for e in seqs:
        f = [names[int(e["seq"])], int(seq_len[int(e["seq"])]), int(e["windows"])]
        for k in ("empty", "covered", "depth", "matches", "records"):
            f += [int(e[k][0]), int(e[k][1])]
        out.append("\t".join(str(x) for x in f) + "\n")
    return "".join(out).encode()


def same(got, want, what):
    """Two structured arrays field by field, so that a difference names its row and field."""
    assert len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() == want.tobytes():
        return
    for name in want.dtype.names:
        bad = np.flatnonzero((got[name] != want[name]).reshape(len(want), -1).any(axis=1))
        assert len(bad) == 0, (what, name, int(bad[0]), got[bad[0]], want[bad[0]])
    raise AssertionError((what, "bytes differ where no field does"))
