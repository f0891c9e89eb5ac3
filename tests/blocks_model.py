"""A plain numpy / Python restatement of the block table (include/sweepga_gpu.h `swg_block`): sort and
merge per chain.  Three parts: the table from record columns plus status and chain (`blocks`), the PAF line of a block
(`format_line`, `render`), and an independent parser that rebuilds the table from an OUTPUT PAF's text alone -- columns 1-12
plus the ch:Z: and st:Z: tags (`blocks_of_output_paf`).  Nothing here shares code with the library."""
import numpy as np

SCAFFOLD, RESCUED = 1, 2
FIELDS = ("chain", "q_id", "t_id", "strand", "q_start", "q_end", "t_start", "t_end", "n_core", "n_inverted", "n_rescued", "matches",
          "block_len", "q_bases", "t_bases", "q_cover", "t_cover", "first_record")
COLUMNS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end", "matches", "block_len", "strand")


class BlockError(ValueError):
    """The input errors of the record seam: a chain over two sequence pairs, a chain without a SCAFFOLD record."""


def union_length(starts, ends):
    """|union of [start, end)|: half-open, zero-length intervals add nothing, touching ones join."""
    total, reach = 0, None
    for s, e in sorted(zip((int(x) for x in starts), (int(x) for x in ends))):
        if e <= s:
            continue
        if reach is None or s > reach:
            total += e - s
            reach = e
        elif e > reach:
            total += e - reach
            reach = e
    return total


def blocks(cols, status, chain):
    """cols: dict of the COLUMNS (strand 0 = '+', 1 = '-'); status, chain: per record.  A list of dicts with FIELDS, ascending chain."""
    status, chain = np.asarray(status), np.asarray(chain)
    c = {k: np.asarray(cols[k]).astype(np.int64) for k in COLUMNS}
    part = np.flatnonzero((status != 0) & (chain != 0))
    out = []
    order = part[np.argsort(chain[part], kind="stable")]
    bounds = np.flatnonzero(np.diff(chain[order].astype(np.int64))) + 1
    for idx in np.split(order, bounds) if len(order) else []:
        n_ch = int(chain[idx[0]])
        if len(set(zip(c["q_id"][idx].tolist(), c["t_id"][idx].tolist()))) != 1:
            raise BlockError(f"chain {n_ch}: two sequence pairs")
        scaffold = idx[status[idx] == SCAFFOLD]
        if len(scaffold) == 0:
            raise BlockError(f"chain {n_ch}: no SCAFFOLD record")
        strand = 0 if (c["strand"][scaffold] == 0).any() else 1
        core = scaffold[c["strand"][scaffold] == strand]
        out.append(dict(
            chain=n_ch, q_id=int(c["q_id"][idx[0]]), t_id=int(c["t_id"][idx[0]]), strand=strand,
            q_start=int(c["q_start"][core].min()), q_end=int(c["q_end"][core].max()),
            t_start=int(c["t_start"][core].min()), t_end=int(c["t_end"][core].max()),
            n_core=len(core), n_inverted=len(scaffold) - len(core) if strand == 0 else 0, n_rescued=int((status[idx] == RESCUED).sum()),
            matches=int(c["matches"][idx].sum()), block_len=int(c["block_len"][idx].sum()),
            q_bases=int(np.maximum(c["q_end"][idx] - c["q_start"][idx], 0).sum()),
            t_bases=int(np.maximum(c["t_end"][idx] - c["t_start"][idx], 0).sum()),
            q_cover=union_length(c["q_start"][idx], c["q_end"][idx]), t_cover=union_length(c["t_start"][idx], c["t_end"][idx]),
            first_record=int(core.min())))
    return out


def rows(table):
    """A structured array of the library (BLOCK_DTYPE) or a list of model dicts -> list of tuples in FIELDS order."""
    return [tuple(int(b[f]) for f in FIELDS) for b in table]


def format_line(b, qname, qlen, tname, tlen):
    ident = b["matches"] / max(b["block_len"], 1)
    return "\t".join([qname, qlen, str(b["q_start"]), str(b["q_end"]), "-" if b["strand"] else "+", tname, tlen, str(b["t_start"]),
                      str(b["t_end"]), str(b["matches"]), str(b["block_len"]), "255", "ch:Z:chain_%d" % b["chain"], "nc:i:%d" % b["n_core"],
                      "ni:i:%d" % b["n_inverted"], "nr:i:%d" % b["n_rescued"], "qc:i:%d" % b["q_cover"], "tc:i:%d" % b["t_cover"],
                      "id:f:%.6f" % ident]) + "\n"


def render(table, lines):
    """The blocks text of a table over the PAF records `lines` (one string per record, in record order)."""
    out = []
    for b in table:
        f = lines[int(b["first_record"])].split("\t")
        out.append(format_line({k: int(b[k]) for k in FIELDS}, f[0], f[1], f[5], f[6]))
    return "".join(out).encode()


def blocks_of_output_paf(text):
    """The table rebuilt from a filtered PAF alone.  Ids are positions in the order of first appearance (queries and targets in
    one space); first_record counts the OUTPUT's lines.  Returns (table, lines)."""
    lines = [ln for ln in text.split("\n") if ln]
    ids, cols, status, chain = {}, {k: [] for k in COLUMNS}, [], []
    for ln in lines:
        f = ln.split("\t")
        tags = {t[:5]: t[5:] for t in f[12:]}
        for k, v in (("q_id", ids.setdefault(f[0], len(ids))), ("t_id", ids.setdefault(f[5], len(ids))), ("q_start", int(f[2])),
                     ("q_end", int(f[3])), ("t_start", int(f[7])), ("t_end", int(f[8])), ("matches", int(f[9])), ("block_len", int(f[10])),
                     ("strand", 0 if f[4] == "+" else 1)):
            cols[k].append(v)
        status.append({"scaffold": SCAFFOLD, "rescued": RESCUED}.get(tags.get("st:Z:"), 3))
        ch = tags.get("ch:Z:", "")
        chain.append(int(ch[len("chain_"):]) if ch.startswith("chain_") else 0)
    if not lines:
        return [], lines
    return blocks(cols, np.asarray(status), np.asarray(chain)), lines


def render_from_output_paf(text):
    table, lines = blocks_of_output_paf(text)
    return render(table, lines)
