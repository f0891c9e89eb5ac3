"""A plain numpy / Python restatement of the placement report (include/sweepga_gpu.h `swg_placement`) with
dictionaries and `sorted`: the candidate table (`candidates`), the rows (`place`), the summary per ordered genome pair (`summary`)
and the two texts (`rows_text`, `summary_text`).  Nothing here shares code with the library.

  axis        0: record r places s = q_id[r] on p = t_id[r] with weight q_end - q_start; 1: the roles and columns swap.
  anchor      '+': partner start - own start; '-': partner end + own start.
  takes part  a record of the set (all, or status != 0) whose two sequences are of different genomes; zero length counts, weight 0.
  candidate   (s, p): fwd / rev = the weights of its '+' / '-' records, n_records, bases = fwd + rev.
  winner      of (s, g = genome of p): largest bases, then smaller p; total_bases over the group, runner_bases of the second.
  orientation '+' when fwd >= rev and the winner has a '+' record, else '-'; the deciding records are the winner's on that strand.
  offset      weighted median of the anchors of the deciding records: by (anchor, index), the first whose inclusive prefix of
              weights reaches half = max(1, ceil(W / 2)); W == 0: the first one's.
  span        min of the starts / max of the ends of the deciding records on either axis; start = offset ('+') or offset - len ('-').
  rows        winners with bases >= min_bases in (genome of s, g, p, start, s) order; rank counts along (genome of s, p).
"""
FIELDS = ("seq", "partner", "genome", "partner_genome", "offset", "start", "bases", "fwd", "rev", "total_bases", "runner_bases", "n_records",
          "q_lo", "q_hi", "t_lo", "t_hi", "rank", "orient")
PAIR_FIELDS = ("genome", "partner_genome", "rows", "reversed", "length", "bases", "total_bases")
ROWS_HEADER = "#sequence\tlength\tpartner\tpartner_length\torient\tstart\tend\trank\tbases\tfwd\trev\ttotal\trunner\trecords\tq_lo\tq_hi\tt_lo\tt_hi\n"
SUMMARY_HEADER = "#genome\tpartner_genome\tsequences\treversed\tlength\tbases\ttotal_bases\n"


def _views(cols, axis):
    """-> per record (s, p, own start, own end, partner start, partner end, strand) as Python ints."""
    own, other = ("q", "t") if axis == 0 else ("t", "q")
    names = (own + "_id", other + "_id", own + "_start", own + "_end", other + "_start", other + "_end", "strand")
    return list(zip(*[[int(x) for x in cols[k]] for k in names]))


def taking(cols, seq_genome, status, axis, kept):
    """The indices of the records that take part."""
    out = []
    for i, (s, p, *_rest) in enumerate(_views(cols, axis)):
        if kept and int(status[i]) == 0:
            continue
        if int(seq_genome[s]) != int(seq_genome[p]):
            out.append(i)
    return out


def candidates(cols, seq_genome, status=None, axis=0, kept=False):
    """-> {(s, p): {"fwd", "rev", "n_records", "bases", "records": ([+ indices], [- indices])}}"""
    v = _views(cols, axis)
    table = {}
    for i in taking(cols, seq_genome, status, axis, kept):
        s, p, a, e, _, _, strand = v[i]
        c = table.setdefault((s, p), {"fwd": 0, "rev": 0, "n_records": 0, "bases": 0, "records": ([], [])})
        c["rev" if strand else "fwd"] += e - a
        c["bases"] += e - a
        c["n_records"] += 1
        c["records"][1 if strand else 0].append(i)
    return table


def anchor(view):
    _, _, a, _, pa, pe, strand = view
    return pe + a if strand else pa - a


def weighted_median(items):
    """items: (anchor, index, weight) -> the anchor of the definition."""
    items = sorted(items)
    total = sum(w for _, _, w in items)
    half = max(1, -(-total // 2))
    run = 0
    for off, _, w in items:
        run += w
        if run >= half:
            return off
    return items[0][0]   # W == 0


def place(cols, seq_len, seq_genome, status=None, axis=0, kept=False, min_bases=0):
    """-> the rows as dicts of FIELDS, in layout order."""
    v = _views(cols, axis)
    table = candidates(cols, seq_genome, status, axis, kept)
    groups = {}
    for (s, p), c in table.items():
        groups.setdefault((s, int(seq_genome[p])), []).append((-c["bases"], p))
    rows = []
    for (s, g), members in groups.items():
        members.sort()
        p = members[0][1]
        c = table[(s, p)]
        if c["bases"] < min_bases:
            continue
        plus = c["fwd"] >= c["rev"] and len(c["records"][0]) > 0
        deciding = c["records"][0 if plus else 1]
        offset = weighted_median([(anchor(v[i]), i, v[i][3] - v[i][2]) for i in deciding])
        rows.append({"seq": s, "partner": p, "genome": int(seq_genome[s]), "partner_genome": g, "offset": offset,
                     "start": offset if plus else offset - int(seq_len[s]), "bases": c["bases"], "fwd": c["fwd"], "rev": c["rev"],
                     "total_bases": sum(-b for b, _ in members), "runner_bases": -members[1][0] if len(members) > 1 else 0,
                     "n_records": c["n_records"], "q_lo": min(v[i][2] for i in deciding), "q_hi": max(v[i][3] for i in deciding),
                     "t_lo": min(v[i][4] for i in deciding), "t_hi": max(v[i][5] for i in deciding), "rank": 0, "orient": 0 if plus else 1})
    rows.sort(key=lambda r: (r["genome"], r["partner_genome"], r["partner"], r["start"], r["seq"]))
    seen = {}
    for r in rows:
        key = (r["genome"], r["partner"])
        r["rank"] = seen.get(key, 0)
        seen[key] = r["rank"] + 1
    return rows


def summary(rows, seq_len):
    """-> dicts of PAIR_FIELDS in (genome, partner_genome) order."""
    out = {}
    for r in rows:
        e = out.setdefault((r["genome"], r["partner_genome"]), dict.fromkeys(PAIR_FIELDS, 0))
        e["genome"], e["partner_genome"] = r["genome"], r["partner_genome"]
        e["rows"] += 1
        e["reversed"] += r["orient"]
        e["length"] += int(seq_len[r["seq"]])
        e["bases"] += r["bases"]
        e["total_bases"] += r["total_bases"]
    return [out[k] for k in sorted(out)]


def rows_text(rows, names, seq_len):
    out = [ROWS_HEADER]
    for r in rows:
        length = int(seq_len[r["seq"]])
        f = [names[r["seq"]], length, names[r["partner"]], int(seq_len[r["partner"]]), "-" if r["orient"] else "+", r["start"], r["start"] + length,
             r["rank"], r["bases"], r["fwd"], r["rev"], r["total_bases"], r["runner_bases"], r["n_records"], r["q_lo"], r["q_hi"], r["t_lo"], r["t_hi"]]
        out.append("\t".join(str(x) for x in f) + "\n")
    return "".join(out).encode()


def summary_text(pairs, genome_names):
    out = [SUMMARY_HEADER]
    for e in pairs:
        out.append("\t".join([genome_names[e["genome"]], genome_names[e["partner_genome"]]] +
                             [str(e[k]) for k in ("rows", "reversed", "length", "bases", "total_bases")]) + "\n")
    return "".join(out).encode()


def as_model(result):
    """A sweepga_amd.place.PlaceResult in the model's form: (rows, pairs), None where the result has none."""
    rows = None if result.rows is None else [{k: int(r[k]) for k in FIELDS} for r in result.rows]
    pairs = None if result.pairs is None else [{k: int(p[k]) for k in PAIR_FIELDS} for p in result.pairs]
    return rows, pairs
