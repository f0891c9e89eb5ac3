"""Brute-force model of the difference list.  Per entry the CIGAR is walked op by op with
tests/lift_exact_model.py's parser, and the definitions are applied literally: no prefix sums, no searches.  Every case is
checked against the consequences the definitions have: the sums' invariant, the walked lengths, every mismatched base as a
one-base exact lift, the flanks as matches, and the gaps of the chain file's blocks."""
import numpy as np

from tests import lift_exact_model as em
from tests import lift_model as lm
from tests import ucsc_chain_model as um

SNP, INS, DEL, SKIP = 1, 2, 4, 8
MINUS = 256
BINS = 33
KIND_OF = {"X": SNP, "I": INS, "D": DEL, "N": SKIP}
KIND_NAME = {SNP: "SNP", INS: "INS", DEL: "DEL", SKIP: "SKIP"}
SUMS = ("entries", "aligned", "eq", "m_columns", "snp_runs", "snp_bases", "n_ins", "ins_bases", "n_del", "del_bases", "n_skip", "skip_bases")
ROW_FIELDS = ("record", "kind_flags", "t_start", "t_end", "q_start", "q_end", "left", "right")
COUNTS = ("records", "usable", "bad", "untagged", "rows", "snp_runs", "snp_bases", "n_ins", "ins_bases", "n_del", "del_bases", "n_skip", "skip_bases",
          "m_columns", "batches")
ROWS_HEADER = "#target\tt_start\tt_end\tquery\tq_start\tq_end\tstrand\tkind\tlen\tleft\tright\trecord\n"
SUMMARY_HEADER = "#query_genome\ttarget_genome\tentries\taligned\teq\tm_columns\tsnp_runs\tsnp_bases\tins\tins_bases\tdel\tdel_bases\tskip\tskip_bases\n"


def entry_diffs(text, minus, q_start, q_end, t_start, t_end, record=0, check=True):
    """One usable entry (state 0) -> (rows of ALL kinds as (ROW_FIELDS tuple, length), sums as a dict without `entries`)."""
    ops = em.parse(text)[1]
    rows, sums = [], dict.fromkeys(SUMS[1:], 0)
    x = y = 0
    for k, (l, ch) in enumerate(ops):
        if ch in "M=X":
            sums["aligned"] += l
            sums["eq"] += l if ch == "=" else 0
            sums["m_columns"] += l if ch == "M" else 0
        if ch in KIND_OF and l > 0:
            kind = KIND_OF[ch]
            name = {SNP: ("snp_runs", "snp_bases"), INS: ("n_ins", "ins_bases"), DEL: ("n_del", "del_bases"), SKIP: ("n_skip", "skip_bases")}[kind]
            sums[name[0]] += 1
            sums[name[1]] += l
            lt, lq = (0 if kind == INS else l), (l if kind in (SNP, INS) else 0)
            qi = (q_end - x - lq, q_end - x) if minus else (q_start + x, q_start + x + lq)
            left = ops[k - 1][0] if k > 0 and ops[k - 1][1] == "=" else 0
            right = ops[k + 1][0] if k + 1 < len(ops) and ops[k + 1][1] == "=" else 0
            rows.append(((record, kind | (MINUS if minus else 0), t_start + y, t_start + y + lt, qi[0], qi[1], left, right), l))
        if ch in "M=XI":
            x += l
        if ch in "M=XDN":
            y += l
    if check:
        check_entry(text, ops, rows, sums, minus, q_start, q_end, t_start, t_end)
    return rows, sums


def check_entry(text, ops, rows, sums, minus, q_start, q_end, t_start, t_end):
    """The assertions of the definitions for one usable entry."""
    assert sums["aligned"] == sums["eq"] + sums["snp_bases"] + sums["m_columns"]
    assert sums["ins_bases"] + sums["aligned"] == q_end - q_start
    assert sums["del_bases"] + sums["skip_bases"] + sums["aligned"] == t_end - t_start
    cols3 = em.columns(ops)
    rec = (q_start, q_end, t_start, t_end)

    def lift(t):
        return em.exact_row(cols3, 1, minus, t, t + 1, *rec)

    for (record, kf, ts, te, qs, qe, left, right), l in rows:
        kind = kf & 255
        if kind == SNP:
            assert te - ts == qe - qs == l
            for i in range(l):          # every mismatched base alone: one column, no match, on the row's query base
                d0, d1, aligned, matches = lift(ts + i)
                assert (aligned, matches) == (1, 0) and d1 == d0 + 1 and d0 == (qe - 1 - i if minus else qs + i), (text, minus, ts + i)
        if left:                        # the base just outside, on a side with a flank, is a match
            assert lift(ts - 1)[2:] == (1, 1), (text, minus, ts)
        if right:
            assert lift(te)[2:] == (1, 1), (text, minus, te)
    # the gaps of the chain file's blocks are the indels strictly between the first and the last aligned op
    aligned_ops = [k for k, (l, ch) in enumerate(ops) if ch in "M=X" and l > 0]
    if aligned_ops:
        _, chain, _ = um.chain_of(text, minus, q_start, q_end, t_start, t_end, q_end + 5, t_end + 5, um.FROM_TARGET)
        inner = ops[aligned_ops[0]:aligned_ops[-1] + 1]
        assert sum(dq for _, _, dq in chain[7]) == sum(l for l, ch in inner if ch == "I")
        assert sum(dt for _, dt, _ in chain[7]) == sum(l for l, ch in inner if ch in "DN")


def diff_records(cols, strand, seq_genome, n_genome, cigars, kept=None, set_=0, kinds=7, min_indel=1, check=True):
    """cigars: {record: text}.  -> dict: rows (ROW_FIELDS tuples in row order), pairs [(q_genome, t_genome) + the twelve sums, ascending],
    spectrum (uint64 [4][33]), state (per entry), and the request's counts."""
    c = {k: np.asarray(cols[k]).astype(np.int64) for k in lm.COLS}
    rows, states, pairs = [], [], {}
    spectrum = np.zeros((4, BINS), dtype=np.uint64)
    usable = bad = 0
    for i in sorted(cigars):
        rec = tuple(int(c[k][i]) for k in ("q_start", "q_end", "t_start", "t_end"))
        state = em.entry_state(cigars[i], rec[1] - rec[0], rec[3] - rec[2])
        states.append(state)
        bad += bool(state & 15)
        if state or not (set_ == 0 or bool(kept[i])):
            continue
        usable += 1
        minus = int(strand[i]) != 0
        got, sums = entry_diffs(cigars[i], minus, *rec, record=i, check=check)
        key = (int(seq_genome[int(c["q_id"][i])]), int(seq_genome[int(c["t_id"][i])]))
        assert key[0] < n_genome and key[1] < n_genome
        acc = pairs.setdefault(key, dict.fromkeys(SUMS, 0))
        acc["entries"] += 1
        for name, v in sums.items():
            acc[name] += v
        for row, l in got:
            kind = row[1] & 255
            spectrum[{SNP: 0, INS: 1, DEL: 2, SKIP: 3}[kind], int(l).bit_length()] += 1
            if kind & kinds and (kind == SNP or l >= min_indel):
                rows.append(row)
    plist = [key + tuple(acc[s] for s in SUMS) for key, acc in sorted(pairs.items())]
    assert not spectrum[:, 0].any()
    text_ops = sum(sum(ch not in "0123456789" for ch in (t.decode("latin-1") if isinstance(t, bytes) else t)) for t in cigars.values())
    return {"rows": rows, "pairs": plist, "spectrum": spectrum, "state": states, "n_rows": len(rows), "n_pairs": len(plist), "ops": text_ops,
            "cigar_bad": bad, "usable": usable}


def rows_array(rows):
    from sweepga_amd.diffs import ROW_DTYPE
    out = np.zeros(len(rows), dtype=ROW_DTYPE)
    for k, row in enumerate(rows):
        out[k] = row
    return out


def pairs_array(pairs):
    from sweepga_amd.diffs import PAIR_DTYPE
    out = np.zeros(len(pairs), dtype=PAIR_DTYPE)
    for k, row in enumerate(pairs):
        out[k] = row
    return out


# ---- the texts of swg_paf_diffs_text -----------------------------------------------------------------------------------------------
def prefix_two(name):
    """The two-part genome prefix: the first two '#' parts and a '#'; the whole name without a '#'."""
    parts = name.split("#")
    return name if len(parts) == 1 else parts[0] + "#" + parts[1] + "#"


def row_text(t_name, q_name, row):
    record, kf, ts, te, qs, qe, left, right = row
    kind = kf & 255
    return "\t".join([t_name, str(ts), str(te), q_name, str(qs), str(qe), "-" if kf & MINUS else "+", KIND_NAME[kind],
                      str(qe - qs if kind == INS else te - ts), str(left), str(right), str(record)]) + "\n"


def summary_text(genome_name, pairs, spectrum):
    out = [SUMMARY_HEADER]
    for p in pairs:
        out.append("\t".join([genome_name[p[0]], genome_name[p[1]]] + [str(v) for v in p[2:]]) + "\n")
    for kind in range(4):
        for b in range(BINS):
            if spectrum[kind][b]:
                out.append("#spectrum\t%s\t%d\t%d\t%d\n" % (("SNP", "INS", "DEL", "SKIP")[kind], 1 << (b - 1) if b else 0, (1 << b) - 1 if b else 0,
                                                            int(spectrum[kind][b])))
    return "".join(out)


def paf_texts(paf_text, kept, set_=1, kinds=7, min_indel=1):
    """(rows text, summary text, counts without `batches`) as swg_paf_diffs_text gives them; kept None = no status.  A PAF without
    records of the set gives two empty texts."""
    cols, strand, names = lm.parse_paf(paf_text)
    lines = um.paf_lines(paf_text)
    sel = [i for i in range(len(strand)) if set_ == 0 or kept[i]]
    counts = dict.fromkeys(COUNTS[:-1], 0)
    counts["records"] = len(sel)
    if not sel:
        return "", "", counts
    genomes, seq_genome = [], []
    for nm in names:
        g = prefix_two(nm)
        if g not in genomes:
            genomes.append(g)
        seq_genome.append(genomes.index(g))
    tags = {i: em.last_cigar_tag(lines[i]) for i in sel}
    got = diff_records(cols, strand, seq_genome, len(genomes), {i: tags[i] or "" for i in sel}, None, 0, kinds, min_indel)
    rows = [ROWS_HEADER] + [row_text(names[int(cols["t_id"][r[0]])], names[int(cols["q_id"][r[0]])], r) for r in got["rows"]]
    counts.update(usable=got["usable"], bad=got["cigar_bad"], untagged=sum(tags[i] is None for i in sel), rows=got["n_rows"])
    for p in got["pairs"]:
        for name, v in zip(SUMS, p[2:]):
            if name in counts:
                counts[name] += v
    return "".join(rows), summary_text(genomes, got["pairs"], got["spectrum"]), counts
