"""Brute-force model of the base-exact lift.  Per record the CIGAR is expanded to its aligned columns and
the definitions are applied literally: no prefix sums, no searches.  Hits, clips, order and the interpolated rows come from
tests/lift_model.py.  Every exact row is checked against the four consequences of the definitions."""
import numpy as np

from tests import lift_model as lm

EXACT = 4
SYNTAX, VALUE, Q_SUM, T_SUM, EMPTY = 1, 2, 4, 8, 16
LETTERS = "MIDNSHP=X"
ROW_FIELDS = lm.ROW_FIELDS + ("aligned", "matches")


def parse(text):
    """-> (state bits 1 | 2, ops as (length, letter)).  An op is 1 to 10 digits with a value below 2^32 and one letter of LETTERS; a
    foreign byte, a letter without digits, more than 10 digits and trailing digits are syntax errors (1), a value >= 2^32 in at
    most 10 digits is a value error (2).  A faulty op is left out of the list, its neighbours stay."""
    if isinstance(text, bytes):
        text = text.decode("latin-1")
    state, ops, digits = 0, [], ""
    for ch in text:
        if ch in "0123456789":
            digits += ch
            continue
        if ch not in LETTERS or not digits or len(digits) > 10:
            state |= SYNTAX
        elif int(digits) >= 2**32:
            state |= VALUE
        else:
            ops.append((int(digits), ch))
        digits = ""
    if digits:
        state |= SYNTAX
    return state, ops


def advances(ops):
    """(sum of the query advance, sum of the target advance) in Python integers"""
    return (sum(l for l, ch in ops if ch in "M=XI"), sum(l for l, ch in ops if ch in "M=XDN"))


def entry_state(text, Lq, Lt):
    """The state byte of an entry for a record of query length Lq and target length Lt.  The sums are looked at only when the
    text parsed (neither 1 nor 2 is set)."""
    if len(text) == 0:
        return EMPTY
    state, ops = parse(text)
    if state:
        return state
    x, y = advances(ops)
    return (Q_SUM if x != Lq else 0) | (T_SUM if y != Lt else 0)


def columns(ops):
    """The aligned columns in text order: (x, y, is_eq) as int64 arrays of walk offsets"""
    xs, ys, eq = [], [], []
    x = y = 0
    for l, ch in ops:
        if ch in "M=X":
            xs.append(np.arange(x, x + l, dtype=np.int64))
            ys.append(np.arange(y, y + l, dtype=np.int64))
            eq.append(np.full(l, ch == "=", dtype=bool))
            x += l
            y += l
        elif ch == "I":
            x += l
        elif ch in "DN":
            y += l
    if not xs:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)
    return np.concatenate(xs), np.concatenate(ys), np.concatenate(eq)


def exact_row(cols3, axis, minus, ca, cb, q_start, q_end, t_start, t_end):
    """The definitions, literally: (dst_start, dst_end, aligned, matches) of the clip [ca, cb) on the source side (axis 0: the
    query is the source)."""
    x, y, eq = cols3
    qc = (q_end - 1 - x) if minus else (q_start + x)      # the columns' query and target coordinates
    tc = t_start + y
    src, dst = (qc, tc) if axis == 0 else (tc, qc)
    d0, d1 = (t_start, t_end) if axis == 0 else (q_start, q_end)
    inside = (src >= ca) & (src < cb)
    aligned, matches = int(inside.sum()), int((inside & eq).sum())
    if aligned:
        return int(dst[inside].min()), int(dst[inside].max()) + 1, aligned, matches
    before = src < ca
    if minus:
        p = int(dst[before].min()) if before.any() else d1
    else:
        p = int(dst[before].max()) + 1 if before.any() else d0
    return p, p, 0, 0


def lift_exact(cols, strand, kept, regions, cigars, set_=0, axes=3):
    """cigars: {record: CIGAR text (str or bytes)}, the set.  -> (rows: list of ROW_FIELDS tuples in row order, summary, states:
    {record: state byte})."""
    rows, summary = lm.lift(cols, strand, kept, regions, set_, axes)
    c = {k: np.asarray(cols[k]).astype(np.int64) for k in lm.COLS}
    states, expanded = {}, {}
    for i, text in cigars.items():
        states[i] = entry_state(text, int(c["q_end"][i] - c["q_start"][i]), int(c["t_end"][i] - c["t_start"][i]))
    out = []
    for r, i, ca, cb, dseq, t0, t1, flags in rows:
        if states.get(i, -1) != 0:
            out.append((r, i, ca, cb, dseq, t0, t1, flags, 0, 0))
            continue
        if i not in expanded:
            ops = parse(cigars[i])[1]
            expanded[i] = columns(ops) + (len(ops) == 1 and ops[0][1] == "M",)
        rec = tuple(int(c[k][i]) for k in ("q_start", "q_end", "t_start", "t_end"))
        axis, minus = flags >> 1 & 1, flags & 1
        e0, e1, aligned, matches = exact_row(expanded[i][:3], axis, minus, ca, cb, *rec)
        d0, d1 = (rec[2], rec[3]) if axis == 0 else (rec[0], rec[1])
        assert d0 <= e0 <= e1 <= d1                                              # dst inside [d0, d1]
        assert 0 <= matches <= aligned <= min(cb - ca, e1 - e0)
        s0, s1 = (rec[0], rec[1]) if axis == 0 else (rec[2], rec[3])
        g0, g1, ga, gm = exact_row(expanded[i][:3], axis, minus, max(ca - 1, s0), min(cb + 1, s1), *rec)
        assert ga >= aligned and gm >= matches
        if aligned:                                                              # growing the region never shrinks dst.  (A clip
            assert g0 <= e0 and e1 <= g1                                         # without columns is the point p on ONE flank of its
        #                                                                          gap; grown by a base it may catch only the column on
        #                                                                          the other flank, a deletion away: no such promise.)
        if expanded[i][3] and rec[1] - rec[0] == rec[3] - rec[2]:
            assert (e0, e1) == (t0, t1) and aligned == cb - ca                   # a single M: the interpolated interval
        out.append((r, i, ca, cb, dseq, e0, e1, flags | EXACT, aligned, matches))
    return out, summary, states


def hit_records(rows):
    return sorted({row[1] for row in rows})


def rows_array(rows):
    from sweepga_amd.lift import EXACT_ROW_DTYPE
    out = np.zeros(len(rows), dtype=EXACT_ROW_DTYPE)
    for k, row in enumerate(rows):
        out[k] = row
    return out


# ---- the texts of swg_paf_lift_exact ----------------------------------------------------------------------------------------------
def last_cigar_tag(line):
    """The value of the last cg:Z: tag among the fields behind the twelfth, or None"""
    if line.endswith("\r"):
        line = line[:-1]
    found = None
    for f in line.split("\t")[12:]:
        if f.startswith("cg:Z:"):
            found = f[5:]
    return found


def paf_cigars(paf_text, records):
    """{record: text} for the records given: the last tag of the record's line, "" without one"""
    lines = [ln for ln in paf_text.split("\n") if len((ln[:-1] if ln.endswith("\r") else ln).split("\t")) >= 11]
    return {i: last_cigar_tag(lines[i]) or "" for i in records}


def paf_texts(paf_text, kept, bed_text, set_=1, axes=3):
    """(rows text, summary text, (records hit, exact, bad, without a tag)) as swg_paf_lift_exact gives them"""
    cols, strand, names = lm.parse_paf(paf_text)
    bed = lm.parse_bed(bed_text, {nm: i for i, nm in enumerate(names)})
    summary_text = lm.paf_texts(paf_text, kept, bed_text, set_, axes)[1]
    if not bed or not len(strand):
        return "", summary_text, (0, 0, 0, 0)
    plain, _ = lm.lift(cols, strand, kept, [b[:3] for b in bed], set_, axes)
    cig = paf_cigars(paf_text, hit_records(plain))
    rows, _, states = lift_exact(cols, strand, kept, [b[:3] for b in bed], cig, set_, axes)
    out = []
    for r, i, ca, cb, dseq, t0, t1, flags, aligned, matches in rows:
        out.append("\t".join([names[dseq], str(t0), str(t1), bed[r][3], bed[r][4], str(ca), str(cb), "-" if flags & 1 else "+",
                              "t" if flags & 2 else "q", str(i), str(aligned), str(matches), "exact" if flags & EXACT else "interp"]) + "\n")
    st = list(states.values())
    lines = [ln for ln in paf_text.split("\n") if len((ln[:-1] if ln.endswith("\r") else ln).split("\t")) >= 11]
    counts = (len(st), sum(s == 0 for s in st), sum(0 < s < EMPTY for s in st), sum(last_cigar_tag(lines[i]) is None for i in states))
    return "".join(out), summary_text, counts
