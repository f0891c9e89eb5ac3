"""The divergence track, written from its definitions (include/sweepga_gpu.h): the yardstick of
csrc/swg_divergence.hip.  Per usable entry the CIGAR is walked op by op with tests/lift_exact_model.py's parser and every aligned
column and every base facing a gap is placed by its own axis coordinate: no prefix sums, no searches, and none of the device's
`aligned = ov - unaligned` shortcut.  All values are integers and every comparison is exact.

  axis, windows, who takes part, listed   as tests/windows_model.py, for ONE set (all records, or those with status != 0); a
              sequence is listed when a record of the set that takes part lies on it, with or without an entry.
  usable      an entry of state 0 whose record is in the set; only those whose records take part add anything.
  coordinate  of a column or of a base facing a gap: t_start + y on axis 1; on axis 0 q_start + x on '+', q_end - 1 - x on '-'.
  point       of an op without axis extent (I on axis 1, D / N on axis 0): p = t_start + y, q_start + x or q_end - x; it belongs
              to the window of base min(p, b - 1).

Every entry is checked against the invariants of the definitions (check_entry); check_windows, check_diffs and check_lift compare
whole results with the windows, the difference list and the base-exact lift."""
import numpy as np

from tests import diffs_model as dm
from tests import lift_exact_model as em
from tests import lift_model as lm
from tests import windows_model as wm

FIELDS = ("aligned", "matches", "mismatches", "m_columns", "unaligned", "inserted", "mismatch_runs", "indels")
ROW_DTYPE = np.dtype([(k, "<u4") for k in ("seq", "start", "end", "n")] + [(k, "<u8") for k in FIELDS])
SEQ_DTYPE = np.dtype([("seq", "<u4"), ("windows", "<u4"), ("records", "<u8"), ("entries", "<u8")] + [(k, "<u8") for k in FIELDS])
ROWS_HEADER = "#sequence\tstart\tend\tn\t" + "\t".join(FIELDS) + "\n"
SUMMARY_HEADER = "#sequence\tlength\twindows\trecords\tentries\t" + "\t".join(FIELDS) + "\n"
COLUMN_FIELD = {"=": "matches", "X": "mismatches", "M": "m_columns"}


def entry_arrays(text, axis, minus, q_start, q_end, t_start, t_end, W):
    """One usable entry (state 0) whose axis side is not empty -> (k0, {field: uint64 array over the windows k0 .. of [a, b)}), by
    walking the text."""
    ops = em.parse(text)[1]
    a, b = (t_start, t_end) if axis else (q_start, q_end)
    k0 = a // W
    acc = {f: np.zeros((b - 1) // W - k0 + 1, dtype=np.uint64) for f in FIELDS}

    def add(field, base, amount=1):
        assert a <= base < b
        acc[field][int(base) // W - k0] += np.uint64(amount)

    def add_bases(field, bases):
        """every base on its own: one by one while they are few, by a histogram of their windows beyond that"""
        if len(bases) <= 32:
            for base in bases.tolist():
                add(field, base)
            return
        assert a <= bases.min() and bases.max() < b
        k = bases // W
        first = int(k.min())
        count = np.bincount(k - first).astype(np.uint64)
        acc[field][first - k0:first - k0 + len(count)] += count

    def coordinates(x, y, l):
        """the axis coordinates of l consecutive walk steps from (x, y)"""
        step = np.arange(l, dtype=np.int64)
        if axis:
            return t_start + y + step
        return q_end - 1 - (x + step) if minus else q_start + x + step

    x = y = 0
    for l, ch in ops:
        if l and ch in "=XM":
            at = coordinates(x, y, l)
            add_bases("aligned", at)
            add_bases(COLUMN_FIELD[ch], at)
            if ch == "X":
                add("mismatch_runs", at.min())
        elif l and ch in "IDN":
            if (ch == "I") == (axis == 0):          # the op consumes bases of this axis against a gap
                at = coordinates(x, y, l)
                add_bases("unaligned", at)
                add("indels", at.min())
            else:                                   # bases of the other sequence at a point of this axis
                p = t_start + y if axis else (q_end - x if minus else q_start + x)
                assert a <= p <= b
                add("inserted", min(p, b - 1), l)
                add("indels", min(p, b - 1))
        if ch in "M=XI":
            x += l
        if ch in "M=XDN":
            y += l
    return k0, acc


def cells_of(k0, acc):
    """{window index: {field: value}} of one entry's arrays"""
    return {k0 + j: {f: int(acc[f][j]) for f in FIELDS} for j in range(len(acc["aligned"]))}


def entry_table(text, axis, minus, q_start, q_end, t_start, t_end, W):
    """One usable entry -> {window index: {field: value}} over the windows of its axis side."""
    return cells_of(*entry_arrays(text, axis, minus, q_start, q_end, t_start, t_end, W))


def check_arrays(k0, acc, a, b, W):
    """Per entry the sum of aligned + unaligned is b - a, and per window it is the overlap of [a, b) with the window."""
    k, ov = wm.overlaps(a, b, W)
    assert int(k[0]) == k0 and len(k) == len(acc["aligned"])
    assert (acc["aligned"] + acc["unaligned"] == ov).all(), (a, b, W)
    assert int(ov.sum()) == b - a
    assert (acc["aligned"] == acc["matches"] + acc["mismatches"] + acc["m_columns"]).all()


def check_entry(table, a, b, W):
    """The same for an entry's {window: fields}."""
    k, ov = wm.overlaps(a, b, W)
    got = {kk: c["aligned"] + c["unaligned"] for kk, c in table.items() if c["aligned"] + c["unaligned"]}
    assert got == dict(zip(k.tolist(), (int(v) for v in ov))), (a, b, W)
    assert sum(got.values()) == b - a
    for c in table.values():
        assert c["aligned"] == c["matches"] + c["mismatches"] + c["m_columns"]


def divergence(cols, strand, seq_len, genome, cigars, kept=None, set_=0, axis=0, window=10_000, other_genome=None, check=True):
    """cigars: {record: text}.  kept: a mask per record (set_ 1).  -> dict: rows (ROW_DTYPE), seqs (SEQ_DTYPE), state (per entry, in
    set order), ops, cigar_bad, usable, `takes` (the records that take part) and `arrays`: {record: (k0, {field: array over its
    windows})} of the usable entries that take part."""
    W = int(window)
    c = {k: np.asarray(cols[k]).astype(np.int64) for k in lm.COLS}
    s, o, a, b = wm.by_role(c, axis)
    genome = np.asarray(genome, dtype=np.int64)
    n = len(s)
    in_set = [set_ == 0 or bool(kept[r]) for r in range(n)]
    takes = []
    for r in range(n):
        if not in_set[r] or genome[s[r]] == genome[o[r]] or a[r] >= b[r] or (other_genome is not None and genome[o[r]] != other_genome):
            continue
        if b[r] > int(seq_len[s[r]]):
            raise ValueError(f"record {r} takes part and ends beyond its sequence")
        takes.append(r)
    taking = set(takes)
    listed = sorted({int(s[r]) for r in takes})
    table = {q: {f: np.zeros((int(seq_len[q]) + W - 1) // W, dtype=np.uint64) for f in FIELDS + ("n",)} for q in listed}
    records = dict.fromkeys(listed, 0)
    entries = dict.fromkeys(listed, 0)
    for r in takes:
        records[int(s[r])] += 1
    states, arrays = [], {}
    usable = bad = 0
    for i in sorted(cigars):
        rec = tuple(int(c[k][i]) for k in ("q_start", "q_end", "t_start", "t_end"))
        state = em.entry_state(cigars[i], rec[1] - rec[0], rec[3] - rec[2])
        states.append(state)
        bad += bool(state & 15)
        if state or i not in taking:
            continue
        usable += 1
        q = int(s[i])
        entries[q] += 1
        k0, acc = entry_arrays(cigars[i], axis, int(strand[i]) != 0, *rec, W)
        if check:
            check_arrays(k0, acc, int(a[i]), int(b[i]), W)
        arrays[i] = (k0, acc)
        K = len(acc["aligned"])
        table[q]["n"][k0:k0 + K] += np.uint64(1)
        for f in FIELDS:
            table[q][f][k0:k0 + K] += acc[f]
    rows = np.zeros(sum(len(t["n"]) for t in table.values()), dtype=ROW_DTYPE)
    seqs = np.zeros(len(listed), dtype=SEQ_DTYPE)
    at = 0
    for j, q in enumerate(listed):
        t, length = table[q], int(seq_len[q])
        K = len(t["n"])
        part = rows[at:at + K]
        index = np.arange(K, dtype=np.int64)
        part["seq"], part["start"], part["end"], part["n"] = q, index * W, np.minimum((index + 1) * W, length), t["n"]
        for f in FIELDS:
            part[f] = t[f]
            seqs[j][f] = int(t[f].sum(dtype=np.uint64))
        at += K
        seqs[j]["seq"], seqs[j]["windows"], seqs[j]["records"], seqs[j]["entries"] = q, K, records[q], entries[q]
    text_ops = sum(sum(ch not in "0123456789" for ch in (t.decode("latin-1") if isinstance(t, bytes) else t)) for t in cigars.values())
    return {"rows": rows, "seqs": seqs, "state": states, "ops": text_ops, "cigar_bad": bad, "usable": usable, "arrays": arrays, "takes": takes}


# ---- the three cross-checks ----------------------------------------------------------------------------------------------------------
def check_windows(got, cols, seq_len, genome, kept, set_, axis, window, other_genome=None):
    """When every record of the set that takes part has a usable entry: aligned + unaligned and n are the windows' depth and n."""
    assert got["usable"] == len(got["takes"])
    status = None if set_ == 0 else np.asarray(kept).astype(np.uint8)
    cols = dict(cols, matches=np.zeros(len(cols["q_id"]), dtype=np.uint32))
    rows, _ = wm.windows(cols, seq_len, genome, status, axis, window, other_genome)
    which = 0 if set_ == 0 else 1
    if set_ == 1:      # the windows list the sequences of ALL records: those of the kept ones are among them
        keep = np.isin(rows["seq"], got["rows"]["seq"])
        assert not rows["n"][~keep, 1].any()
        rows = rows[keep]
    assert (rows["seq"] == got["rows"]["seq"]).all() and (rows["start"] == got["rows"]["start"]).all() and (rows["end"] == got["rows"]["end"]).all()
    assert (rows["depth"][:, which] == got["rows"]["aligned"] + got["rows"]["unaligned"]).all()
    assert (rows["n"][:, which] == got["rows"]["n"]).all()


def check_diffs(got, cols, strand, genome, n_genome, cigars):
    """The sums over all rows are the difference list's summary summed over the genome pairs, for the entries that take part."""
    takes = set(got["takes"])
    part = {i: cigars[i] for k, i in enumerate(sorted(cigars)) if got["state"][k] == 0 and i in takes}
    d = dm.diff_records(cols, strand, genome, n_genome, part, check=False)
    total = {name: sum(p[2 + k] for p in d["pairs"]) for k, name in enumerate(dm.SUMS)}
    rows = got["rows"]
    sums = {f: int(rows[f].sum(dtype=np.uint64)) for f in FIELDS}
    assert total["entries"] == got["usable"]
    assert sums["aligned"] == total["aligned"] and sums["matches"] == total["eq"] and sums["mismatches"] == total["snp_bases"]
    assert sums["m_columns"] == total["m_columns"] and sums["mismatch_runs"] == total["snp_runs"]
    assert sums["indels"] == total["n_ins"] + total["n_del"] + total["n_skip"]
    assert sums["unaligned"] + sums["inserted"] == total["ins_bases"] + total["del_bases"] + total["skip_bases"]


def check_lift(got, cols, strand, cigars, axis, window):
    """Each (entry, window) with ov > 0, lifted as a clip through the base-exact lift on this axis, gives the entry's aligned and
    matches in that window."""
    W = int(window)
    c = {k: np.asarray(cols[k]).astype(np.int64) for k in lm.COLS}
    seen = 0
    for i in sorted(got["arrays"]):
        rec = tuple(int(c[k][i]) for k in ("q_start", "q_end", "t_start", "t_end"))
        cols3 = em.columns(em.parse(cigars[i])[1])
        a, b = (rec[2], rec[3]) if axis else (rec[0], rec[1])
        cells = cells_of(*got["arrays"][i])
        for k in range(a // W, (b - 1) // W + 1):
            ca, cb = max(a, k * W), min(b, (k + 1) * W)
            _, _, aligned, matches = em.exact_row(cols3, axis, int(strand[i]) != 0, ca, cb, *rec)
            cell = cells[k]
            assert (aligned, matches) == (cell["aligned"], cell["matches"]), (i, k, cigars[i])
            seen += 1
    return seen


# ---- the texts of swg_paf_divergence --------------------------------------------------------------------------------------------------
def rows_text(rows, names):
    out = [ROWS_HEADER]
    for r in rows:
        out.append("\t".join([names[int(r["seq"])]] + [str(int(r[k])) for k in ("start", "end", "n") + FIELDS]) + "\n")
    return "".join(out)


def summary_text(seqs, names, seq_len):
    out = [SUMMARY_HEADER]
    for e in seqs:
        out.append("\t".join([names[int(e["seq"])], str(int(seq_len[int(e["seq"])]))] + [str(int(e[k])) for k in ("windows", "records", "entries") + FIELDS]) + "\n")
    return "".join(out)


def prefix_last(name):
    """The genome prefix up to and including the last '#'; the whole name without one."""
    return name[:name.rindex("#") + 1] if "#" in name else name


def last_lengths(paf_text, names):
    """Per sequence the length on the line that mentions it last (target column after query column)."""
    length = {}
    for ln in paf_text.split("\n"):
        f = (ln[:-1] if ln.endswith("\r") else ln).split("\t")
        if len(f) >= 11:
            length[f[0]] = int(f[1])
            length[f[5]] = int(f[6])
    return [length[nm] for nm in names]


def paf_texts(paf_text, kept, set_=1, axis=0, window=10_000, genome=None):
    """(rows text, summary text, counts without `batches`) as swg_paf_divergence gives them; kept None = no status."""
    cols, strand, names = lm.parse_paf(paf_text)
    lines = [ln for ln in paf_text.split("\n") if len((ln[:-1] if ln.endswith("\r") else ln).split("\t")) >= 11]
    sel = [i for i in range(len(strand)) if set_ == 0 or kept[i]]
    counts = dict.fromkeys(("records", "usable", "bad", "untagged", "windows", "seqs"), 0)
    counts["records"] = len(sel)
    if not sel:
        return ROWS_HEADER, SUMMARY_HEADER, counts
    genomes, seq_genome = [], []
    for nm in names:
        g = prefix_last(nm)
        if g not in genomes:
            genomes.append(g)
        seq_genome.append(genomes.index(g))
    other = None
    if genome is not None:
        other = genomes.index(genome if genome in genomes else genome + "#")
    seq_len = last_lengths(paf_text, names)
    tags = {i: em.last_cigar_tag(lines[i]) for i in sel}
    got = divergence(cols, strand, seq_len, seq_genome, {i: tags[i] or "" for i in sel}, kept, set_, axis, window, other, check=False)
    counts.update(usable=got["usable"], bad=got["cigar_bad"], untagged=sum(tags[i] is None for i in sel), windows=len(got["rows"]), seqs=len(got["seqs"]))
    return rows_text(got["rows"], names), summary_text(got["seqs"], names, seq_len), counts


def same(got, want, what):
    wm.same(got, want, what)
