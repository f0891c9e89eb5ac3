"""The rule by which u64 coordinates reach the 32-bit device layout, stated once in plain Python integers (nothing here can
wrap, and nothing is shared with sweepga_amd/csrc/host/rebase.h or the kernels of swg_filter.hip, which are held to it).

A constant is taken off every coordinate: one per sequence, or -- when some sequence is touched over 2^32 bases or more -- one
per (sequence, genome of the other side) and axis.  `rebase` answers what a front end must answer for a record set:

    ("ok", "seq" | "axis", off_q, off_t, cols32)   off_q[i] / off_t[i]: what was taken off record i's query / target coordinates
    ("invalid", record)                            a sequence id, or the genome table's entry of a named sequence, out of range
    ("range", record, field)                       a value that does not fit 32 bits after all; FIELDS[field] names it

Precedence:
 1. a q_id or t_id >= n_seq: invalid, the lowest such record, whatever else is wrong with the records;
 2. per-sequence constants lo[s] = min over every appearance of s, on either axis, of min(start, end); the first failure is the
    lowest record and in it the lowest field whose rebased value is >= 2^32 (matches and block length, fields 4 and 5, are not
    rebased); none: ok / seq;
 3. a first failure in field 4 or 5: range, that record and field;
 4. a first failure in field 0..3: when n_seq * n_genome_last > 2^24 the same record and field; else constants per
    (q_id, genome(t_id)) for the query axis and (t_id, genome(q_id)) for the target axis; a record naming a sequence whose genome
    entry is >= n_genome_last: invalid (the lowest such record); else the first failure under the new constants (all six fields
    again): range; none: ok / axis."""

LIMIT = 1 << 32
MAX_CELLS = 1 << 24
FIELDS = ("query_start", "query_end", "target_start", "target_end", "matches", "block_length")
UNNAMED = (1 << 64) - 1   # the constant of a sequence that no record names


def _too_wide(v):
    return v >= LIMIT


def _first_failure(n, cols, off_q, off_t):
    for i in range(n):
        vals = (cols[0][i] - off_q[i], cols[1][i] - off_q[i], cols[2][i] - off_t[i], cols[3][i] - off_t[i], cols[4][i], cols[5][i])
        for f, v in enumerate(vals):
            assert v >= 0
            if _too_wide(v):
                return i, f
    return None


def _ok(kind, n, cols, off_q, off_t):
    c32 = [[cols[0][i] - off_q[i] for i in range(n)], [cols[1][i] - off_q[i] for i in range(n)],
           [cols[2][i] - off_t[i] for i in range(n)], [cols[3][i] - off_t[i] for i in range(n)], list(cols[4]), list(cols[5])]
    return ("ok", kind, off_q, off_t, c32)


def rebase(q_id, t_id, cols, n_seq, seq_genome_last, n_genome_last):
    """q_id, t_id: sequences of ints; cols: the six u64 columns in the order of FIELDS, as sequences of Python ints."""
    q_id = [int(x) for x in q_id]
    t_id = [int(x) for x in t_id]
    cols = [[int(x) for x in c] for c in cols]
    n = len(q_id)
    # 1. ids
    for i in range(n):
        if q_id[i] >= n_seq or t_id[i] >= n_seq:
            return ("invalid", i)
    # 2. one constant per sequence
    lo = {}
    for i in range(n):
        lo[q_id[i]] = min(lo.get(q_id[i], UNNAMED), cols[0][i], cols[1][i])
        lo[t_id[i]] = min(lo.get(t_id[i], UNNAMED), cols[2][i], cols[3][i])
    off_q = [lo[q] for q in q_id]
    off_t = [lo[t] for t in t_id]
    first = _first_failure(n, cols, off_q, off_t)
    if first is None:
        return _ok("seq", n, cols, off_q, off_t)
    # 3. / 4.
    if first[1] >= 4 or n_seq * n_genome_last > MAX_CELLS:
        return ("range", first[0], first[1])
    genome = [int(g) for g in seq_genome_last]
    for i in range(n):
        if genome[q_id[i]] >= n_genome_last or genome[t_id[i]] >= n_genome_last:
            return ("invalid", i)
    lo_q, lo_t = {}, {}
    for i in range(n):
        kq, kt = (q_id[i], genome[t_id[i]]), (t_id[i], genome[q_id[i]])
        lo_q[kq] = min(lo_q.get(kq, UNNAMED), cols[0][i], cols[1][i])
        lo_t[kt] = min(lo_t.get(kt, UNNAMED), cols[2][i], cols[3][i])
    off_q = [lo_q[(q_id[i], genome[t_id[i]])] for i in range(n)]
    off_t = [lo_t[(t_id[i], genome[q_id[i]])] for i in range(n)]
    first = _first_failure(n, cols, off_q, off_t)
    if first is None:
        return _ok("axis", n, cols, off_q, off_t)
    return ("range", first[0], first[1])


def seq_constants(q_id, t_id, n_seq, result):
    """The per-sequence table of an ok / seq result: [n_seq], UNNAMED for a sequence no record names."""
    assert result[0] == "ok" and result[1] == "seq"
    lo = [UNNAMED] * n_seq
    for i, (q, t) in enumerate(zip(q_id, t_id)):
        lo[int(q)] = result[2][i]
        lo[int(t)] = result[3][i]
    return lo
