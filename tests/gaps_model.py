"""A plain numpy / Python restatement of the gaps report (include/sweepga_gpu.h `swg_gap_row`): per chain
a sort and a walk.  Four parts: the rows (`gaps`), the summary per ordered genome pair and the spectrum (`summary`), and the two
texts (`rows_text`, `summary_text`).  Nothing here shares code with the library."""
import numpy as np

SCAFFOLD = 1
EVEN, INS, DEL, INV = 0, 1, 2, 3
KIND = {EVEN: "EVEN", INS: "INS", DEL: "DEL", INV: "INV"}
FIELDS = ("chain", "left", "right", "q_lo", "q_hi", "t_lo", "t_hi", "kind", "flags")
COLUMNS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end", "strand")
BINS = 33
SUM_FIELDS = ("links", "n_ins", "ins_bases", "n_del", "del_bases", "n_inv", "inv_bases")


class GapError(ValueError):
    """The input error of the record seam that the model knows: a chain over two sequence pairs."""


def chains(cols, status, chain):
    """-> [(chain number, strand, core records in order, inverted records)], ascending chain; order = (q_start, index)."""
    status, chain = np.asarray(status), np.asarray(chain)
    c = {k: [int(x) for x in cols[k]] for k in COLUMNS}
    members = {}
    for i in range(len(status)):
        if int(status[i]) == SCAFFOLD and int(chain[i]) != 0:
            members.setdefault(int(chain[i]), []).append(i)
    out = []
    for n_ch in sorted(members):
        idx = sorted(members[n_ch], key=lambda i: (c["q_start"][i], i))
        if len({(c["q_id"][i], c["t_id"][i]) for i in idx}) != 1:
            raise GapError(f"chain {n_ch}: two sequence pairs")
        strand = 0 if any(c["strand"][i] == 0 for i in idx) else 1
        out.append((n_ch, strand, [i for i in idx if c["strand"][i] == strand], [i for i in idx if c["strand"][i] != strand]))
    return out


def links(cols, status, chain):
    """Every link, whatever its size: dicts with chain, left, right, dq, dt, size and the row's fields."""
    c = {k: [int(x) for x in cols[k]] for k in COLUMNS}
    out = []
    for n_ch, strand, core, _ in chains(cols, status, chain):
        for a, b in zip(core, core[1:]):
            qa, qb = c["q_end"][a], c["q_start"][b]
            if strand == 0:
                ta, tb = c["t_end"][a], c["t_start"][b]
                dt = tb - ta
            else:
                ta, tb = c["t_start"][a], c["t_end"][b]
                dt = ta - tb
            dq = qb - qa
            size = dq - dt
            out.append(dict(chain=n_ch, left=a, right=b, q_lo=min(qa, qb), q_hi=max(qa, qb), t_lo=min(ta, tb), t_hi=max(ta, tb),
                            kind=INS if size > 0 else DEL if size < 0 else EVEN, flags=(1 if dq < 0 else 0) | (2 if dt < 0 else 0),
                            dq=dq, dt=dt, size=size))
    return out


def inversions(cols, status, chain):
    c = {k: [int(x) for x in cols[k]] for k in COLUMNS}
    return [dict(chain=n_ch, left=r, right=r, q_lo=c["q_start"][r], q_hi=c["q_end"][r], t_lo=c["t_start"][r], t_hi=c["t_end"][r], kind=INV,
                 flags=0, dq=0, dt=0, size=c["q_end"][r] - c["q_start"][r])
            for n_ch, _, _, inverted in chains(cols, status, chain) for r in inverted]


def gaps(cols, status, chain, min_size):
    """The rows: links with |size| >= min_size and inversions with a query length >= min_size, by (chain, q_start[right], right)."""
    qs = [int(x) for x in cols["q_start"]]
    rows = [e for e in links(cols, status, chain) + inversions(cols, status, chain) if abs(e["size"]) >= min_size]
    return sorted(rows, key=lambda e: (e["chain"], qs[e["right"]], e["right"]))


def rows(table):
    """A structured array of the library (ROW_DTYPE) or a list of model dicts -> list of tuples in FIELDS order."""
    return [tuple(int(r[f]) for f in FIELDS) for r in table]


def bit_length_bin(magnitude):
    return min(int(magnitude).bit_length(), BINS - 1)


def summary(cols, status, chain, seq_genome, min_size):
    """-> (pairs, spectrum): pairs = [(q_genome, t_genome, links, n_ins, ins_bases, n_del, del_bases, n_inv, inv_bases)] ascending,
    an entry where links or n_inv is non-zero; spectrum = [2][BINS] counts of the emitted INS and DEL by the bit length of |size|."""
    g = [int(x) for x in seq_genome]
    q_id, t_id = [int(x) for x in cols["q_id"]], [int(x) for x in cols["t_id"]]
    table, spectrum = {}, [[0] * BINS for _ in range(2)]
    for e in links(cols, status, chain):
        s = table.setdefault((g[q_id[e["right"]]], g[t_id[e["right"]]]), [0] * 7)
        s[0] += 1
        if abs(e["size"]) >= min_size and e["size"] != 0:
            k = 0 if e["size"] > 0 else 1
            s[1 + 2 * k] += 1
            s[2 + 2 * k] += abs(e["size"])
            spectrum[k][bit_length_bin(abs(e["size"]))] += 1
    for e in inversions(cols, status, chain):
        if e["size"] >= min_size:
            s = table.setdefault((g[q_id[e["right"]]], g[t_id[e["right"]]]), [0] * 7)
            s[5] += 1
            s[6] += e["size"]
    return [k + tuple(v) for k, v in sorted(table.items()) if v[0] or v[5]], spectrum


def pairs(table):
    """A structured array of the library (PAIR_DTYPE) -> list of tuples like summary()'s."""
    return [tuple(int(p[f]) for f in ("q_genome", "t_genome") + SUM_FIELDS) for p in table]


ROWS_HEADER = "#query\tq_start\tq_end\ttarget\tt_start\tt_end\tkind\tsize\tchain\tdq\tdt\tleft\tright\n"
SUMMARY_HEADER = "#query_genome\ttarget_genome\tlinks\tins\tins_bases\tdel\tdel_bases\tinv\tinv_bases\n"


def rows_text(table, cols, names):
    """The rows text: `table` as gaps() gives it, names[sequence id]."""
    out = [ROWS_HEADER]
    for e in table:
        r = e["right"]
        out.append("\t".join([names[int(cols["q_id"][r])], str(e["q_lo"]), str(e["q_hi"]), names[int(cols["t_id"][r])], str(e["t_lo"]),
                              str(e["t_hi"]), KIND[e["kind"]], str(e["size"]), str(e["chain"]), str(e["dq"]), str(e["dt"]), str(e["left"]),
                              str(r)]) + "\n")
    return "".join(out).encode()


def summary_text(pair_list, spectrum, genome_names):
    out = [SUMMARY_HEADER]
    for p in pair_list:
        out.append("\t".join([genome_names[p[0]], genome_names[p[1]]] + [str(v) for v in p[2:]]) + "\n")
    for k, kind in enumerate(("INS", "DEL")):
        for b in range(BINS):
            if spectrum[k][b]:
                lo = 2 ** (b - 1) if b else 0
                hi = 2 ** 33 - 2 if b == BINS - 1 else 2 ** b - 1 if b else 0
                out.append(f"#spectrum\t{kind}\t{lo}\t{hi}\t{spectrum[k][b]}\n")
    return "".join(out).encode()
