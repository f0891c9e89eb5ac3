"""Brute-force model of the lift slices.  Every CIGAR is expanded into its list of columns op by op, the ones
whose source coordinate lies in the clip are taken, and the slice's text is rebuilt op by op from them: no prefix sums, no binary
search.  (An op's columns are a Python `range`, so that a 10-digit op costs nothing; `slice_expanded` is the same with every column
listed in numpy arrays, for CIGARs small enough.)  Hits, clips and order come from tests/lift_model.py, entry states from
tests/lift_exact_model.py.  Every slice is checked against the first two consequences of the definitions."""
import re

import numpy as np

from tests import lift_exact_model as lem
from tests import lift_model as lm

HAS_EQ = 8
SLICE_FIELDS = ("region", "record", "q_start", "q_end", "t_start", "t_end", "flags", "aligned", "matches", "text_len", "block", "text_first")
TOKEN = re.compile(r"(\d+)(\D)")


def tokens(text):
    """A state-0 entry as [(digits as written, letter)]"""
    if isinstance(text, bytes):
        text = text.decode("latin-1")
    return TOKEN.findall(text)


def slice_row(text, axis, minus, ca, cb, q_start, q_end, t_start, t_end):
    """The slice of the clip [ca, cb) on the source side (axis 0: the query) of a record with a state-0 entry `text`: None without an
    aligned column in the clip, else a dict with the four coordinates, aligned, matches, block, cigar and has_eq."""
    toks = tokens(text)
    x = y = 0
    per_op = []          # per op: (first column inside, columns inside, x of the op's first column, y of it), or None
    for digits, ch in toks:
        l = int(digits)
        inside = None
        if ch in "M=X" and l:
            cols = range(l)                                  # column i of the op: walk offsets (x + i, y + i)
            if axis == 1:
                lo, hi = ca - (t_start + y), cb - (t_start + y)              # t_start + y + i in [ca, cb)
            elif minus:
                lo, hi = (q_end - 1 - x) - cb + 1, (q_end - 1 - x) - ca + 1  # q_end - 1 - x - i in [ca, cb)
            else:
                lo, hi = ca - (q_start + x), cb - (q_start + x)
            take = cols[max(lo, 0):max(hi, 0)]
            if len(take):
                inside = (take[0], len(take), x, y)
        per_op.append(inside)
        if ch in "M=XI":
            x += l
        if ch in "M=XDN":
            y += l
    hit = [r for r, v in enumerate(per_op) if v is not None]
    if not hit:
        return None
    i0, i1 = hit[0], hit[-1]
    aligned = sum(per_op[r][1] for r in hit)
    matches = sum(per_op[r][1] for r in hit if toks[r][1] == "=")
    f0, n0, ox0, oy0 = per_op[i0]
    f1, n1, ox1, oy1 = per_op[i1]
    x0, y0 = ox0 + f0, oy0 + f0
    x1, y1 = ox1 + f1 + n1 - 1, oy1 + f1 + n1 - 1
    if i0 == i1:
        cigar = "%d%s" % (n0, toks[i0][1])
    else:
        cigar = "%d%s" % (n0, toks[i0][1]) + "".join(d + ch for d, ch in toks[i0 + 1:i1]) + "%d%s" % (n1, toks[i1][1])
    q = (q_end - 1 - x1, q_end - x0) if minus else (q_start + x0, q_start + x1 + 1)
    return {"q_start": q[0], "q_end": q[1], "t_start": t_start + y0, "t_end": t_start + y1 + 1, "aligned": aligned, "matches": matches,
            "block": (x1 - x0 + 1) + (y1 - y0 + 1) - aligned, "cigar": cigar, "has_eq": any(ch == "=" and int(d) for d, ch in toks)}


def slice_expanded(text, axis, minus, ca, cb, q_start, q_end, t_start, t_end):
    """The same from every column listed: (q_start, q_end, t_start, t_end, aligned, matches, block) or None"""
    xs, ys, eq = lem.columns(lem.parse(text)[1])
    qc = (q_end - 1 - xs) if minus else (q_start + xs)
    tc = t_start + ys
    src = tc if axis else qc
    inside = (src >= ca) & (src < cb)
    if not inside.any():
        return None
    aligned = int(inside.sum())
    block = int(xs[inside].max() - xs[inside].min() + 1) + int(ys[inside].max() - ys[inside].min() + 1) - aligned
    return (int(qc[inside].min()), int(qc[inside].max()) + 1, int(tc[inside].min()), int(tc[inside].max()) + 1, aligned, int((inside & eq).sum()), block)


def check_slice(s, axis, minus):
    """The first two consequences: the slice's text is a state-0 entry of a record with the slice's coordinates, and lifting the
    slice's source interval through that record gives the slice again."""
    assert lem.entry_state(s["cigar"], s["q_end"] - s["q_start"], s["t_end"] - s["t_start"]) == 0, s
    src = (s["t_start"], s["t_end"]) if axis else (s["q_start"], s["q_end"])
    again = slice_row(s["cigar"], axis, minus, src[0], src[1], s["q_start"], s["q_end"], s["t_start"], s["t_end"])
    for key in ("q_start", "q_end", "t_start", "t_end", "aligned", "matches", "block", "cigar"):
        assert again[key] == s[key], (key, again, s)


def lift_slices(cols, strand, kept, regions, cigars, set_=0, axes=3, min_aligned=1):
    """cigars: {record: CIGAR text}, the set.  -> (slices: list of SLICE_FIELDS tuples in slice order, their CIGARs, counts: a dict with
    n_rows, n_slices, n_interp, n_empty, n_short, text_bytes, cigar_bad, states: {record: state byte})."""
    rows, _ = lm.lift(cols, strand, kept, regions, set_, axes)
    c = {k: np.asarray(cols[k]).astype(np.int64) for k in lm.COLS}
    states = {i: lem.entry_state(t, int(c["q_end"][i] - c["q_start"][i]), int(c["t_end"][i] - c["t_start"][i])) for i, t in cigars.items()}
    counts = {"n_rows": len(rows), "n_slices": 0, "n_interp": 0, "n_empty": 0, "n_short": 0, "text_bytes": 0,
              "cigar_bad": sum(0 < s < lem.EMPTY for s in states.values())}
    out, texts = [], []
    for r, i, ca, cb, dseq, t0, t1, flags in rows:
        if states.get(i, -1) != 0:
            counts["n_interp"] += 1
            continue
        axis, minus = flags >> 1 & 1, flags & 1
        s = slice_row(cigars[i], axis, minus, ca, cb, *(int(c[k][i]) for k in ("q_start", "q_end", "t_start", "t_end")))
        if s is None:
            counts["n_empty"] += 1
            continue
        if s["aligned"] < min_aligned:
            counts["n_short"] += 1
            continue
        check_slice(s, axis, minus)
        out.append((r, i, s["q_start"], s["q_end"], s["t_start"], s["t_end"], (flags & 3) | (HAS_EQ if s["has_eq"] else 0), s["aligned"], s["matches"],
                    len(s["cigar"]), s["block"], counts["text_bytes"]))
        texts.append(s["cigar"])
        counts["text_bytes"] += len(s["cigar"])
    counts["n_slices"] = len(out)
    return out, texts, counts, states


def slices_array(slices):
    from sweepga_amd.lift import SLICE_DTYPE
    out = np.zeros(len(slices), dtype=SLICE_DTYPE)
    for k, row in enumerate(slices):
        out[k] = row
    return out


# ---- the text of swg_paf_lift_paf_text --------------------------------------------------------------------------------------------
def paf_text(paf_text_, kept, bed_text, set_=1, axes=3, min_aligned=1):
    """(text, counts: rows slices interp empty too_short) as swg_paf_lift_paf_text gives them"""
    cols, strand, names = lm.parse_paf(paf_text_)
    bed = lm.parse_bed(bed_text, {nm: i for i, nm in enumerate(names)})
    zero = {"rows": 0, "slices": 0, "interp": 0, "empty": 0, "too_short": 0}
    if not bed or not len(strand):
        return "", zero
    lines = [(ln[:-1] if ln.endswith("\r") else ln).split("\t") for ln in paf_text_.split("\n")]
    lines = [f for f in lines if len(f) >= 11]
    plain, _ = lm.lift(cols, strand, kept, [b[:3] for b in bed], set_, axes)
    cig = lem.paf_cigars(paf_text_, lem.hit_records(plain))
    slices, texts, counts, _ = lift_slices(cols, strand, kept, [b[:3] for b in bed], cig, set_, axes, min_aligned)
    out = []
    for (r, i, q0, q1, t0, t1, flags, aligned, matches, _, block, _), cigar in zip(slices, texts):
        f = lines[i]
        out.append("\t".join([f[0], f[1], str(q0), str(q1), "-" if flags & 1 else "+", f[5], f[6], str(t0), str(t1),
                              str(matches if flags & HAS_EQ else aligned), str(block), f[11], "cg:Z:" + cigar, "rn:Z:" + bed[r][3], "ri:i:%d" % i]) + "\n")
    return "".join(out), {"rows": counts["n_rows"], "slices": counts["n_slices"], "interp": counts["n_interp"], "empty": counts["n_empty"],
                          "too_short": counts["n_short"]}


# ---- hand-worked lines ------------------------------------------------------------------------------------------------------------
# record 0: columns '=' x0-9 y0-9; I x10-11; X x12-16 y10-14; D y15-17; '=' x17-29 y18-30.  record 1 ('-'): M x0-3 y0-3; D y4-5; M x4-9 y6-11.
HAND_PAF = ("qA\t1000\t100\t130\t+\ttB\t2000\t500\t531\t23\t35\t60\tcg:Z:10=2I5X3D13=\n"
            "qA\t1000\t200\t210\t-\ttB\t2000\t800\t812\t10\t12\t30\tcg:Z:4M2D6M\n")
# tB 505-520: y in [5, 20) -> columns 5 .. 16 (five '=', five X, two '='), the D inside; x 5 .. 18
# qA 110-113: x 10, 11 are inserted bases, x 12 the first X column (y 10)
# tB 802-809: y 2, 3 and 6, 7, 8 -> x 2 .. 6, on '-' the query [210 - 1 - 6, 210 - 2)
# qA 110-112: inserted bases only -> empty
HAND_BED = "tB\t505\t520\tgeneT\nqA\t110\t113\ntB\t802\t809\tr2\nqA\t110\t112\tnone\n"
HAND_TEXT = ("qA\t1000\t105\t119\t+\ttB\t2000\t505\t520\t7\t17\t60\tcg:Z:5=2I5X3D2=\trn:Z:geneT\tri:i:0\n"
             "qA\t1000\t112\t113\t+\ttB\t2000\t510\t511\t0\t1\t60\tcg:Z:1X\trn:Z:qA:110-113\tri:i:0\n"
             "qA\t1000\t203\t208\t-\ttB\t2000\t802\t809\t5\t7\t30\tcg:Z:2M2D3M\trn:Z:r2\tri:i:1\n")
HAND_COUNTS = {"rows": 4, "slices": 3, "interp": 0, "empty": 1, "too_short": 0}


def random_cigar(rng, n_ops, max_len=9, letters="M=XIDN", extras=True):
    """A random state-0 CIGAR of n_ops advancing ops (lengths 1 .. max_len, no two neighbours alike), with zero-length ops and S, H, P
    strewn in when `extras` -> (text, query advance, target advance)"""
    out, x, y, last = [], 0, 0, ""
    for _ in range(n_ops):
        ch = letters[int(rng.integers(len(letters)))]
        while ch == last:
            ch = letters[int(rng.integers(len(letters)))]
        last = ch
        l = int(rng.integers(1, max_len + 1))
        if extras and rng.random() < 0.15:
            out.append("%d%s" % (0 if rng.random() < 0.6 else int(rng.integers(1, 30)), "MIDNSHP=X"[int(rng.integers(9))] if rng.random() < 0.5 else "SHP"[int(rng.integers(3))]))
            d, e = TOKEN.match(out[-1]).groups()
            x += int(d) if e in "M=XI" else 0
            y += int(d) if e in "M=XDN" else 0
        out.append(("%d%s" if rng.random() < 0.9 else "0%d%s") % (l, ch))
        x += l if ch in "M=XI" else 0
        y += l if ch in "M=XDN" else 0
    return "".join(out), x, y
