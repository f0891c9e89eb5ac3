"""Brute-force model of the UCSC chain files.  Per record the CIGAR is expanded to its aligned columns with
tests/lift_exact_model.py's parser and expansion; the blocks come from scanning the columns for breaks -- no prefix sums, no
searches.  Every chain is walked back from its start and must reproduce the literal column set, in the coordinates of its
orientation; on the '-' strand seen from the query that set is the reverse complement's."""
import numpy as np

from tests import lift_exact_model as em
from tests import lift_model as lm

BEYOND = 32
FROM_TARGET, FROM_QUERY = 0, 1
MINUS = 1
COUNTS = ("records", "chains", "bad", "beyond", "untagged", "empty", "blocks", "batches")


def blocks_of(x, y):
    """The ungapped blocks of the columns (x, y) in text order: [(x_first, y_first, size)]"""
    out = []
    if not len(x):
        return out
    brk = np.flatnonzero((np.diff(x) != 1) | (np.diff(y) != 1)) + 1
    first = np.concatenate([[0], brk])
    last = np.concatenate([brk, [len(x)]])
    return [(int(x[a]), int(y[a]), int(b - a)) for a, b in zip(first, last)]


def swap(chain):
    """The same alignment with the two sides exchanged: chain = (ref_start, ref_end, ref_size, minus, oth_start, oth_end, oth_size,
    [(size, dt, dq)]) with (size, 0, 0) last."""
    rs, re, rsize, minus, os_, oe, osize, blocks = chain
    if not minus:
        return (os_, oe, osize, 0, rs, re, rsize, [(s, dq, dt) for s, dt, dq in blocks])
    B = len(blocks)
    rev = [(blocks[B - 1 - j][0],) + ((blocks[B - 2 - j][2], blocks[B - 2 - j][1]) if j < B - 1 else (0, 0)) for j in range(B)]
    return (osize - oe, osize - os_, osize, 1, rsize - re, rsize - rs, rsize, rev)


def walk(chain):
    """The columns a chain covers, block by block: (reference coordinates, other coordinates in their strand's coordinates)"""
    rs, re, _, _, os_, oe, _, blocks = chain
    r, o, rr, oo = rs, os_, [], []
    for size, dt, dq in blocks:
        assert size > 0
        rr.append(np.arange(r, r + size, dtype=np.int64))
        oo.append(np.arange(o, o + size, dtype=np.int64))
        r, o = r + size + dt, o + size + dq
    assert blocks[-1][1:] == (0, 0) and (r, o) == (re, oe)
    assert all((dt, dq) != (0, 0) for _, dt, dq in blocks[:-1])
    return np.concatenate(rr), np.concatenate(oo)


def same_columns(got, ref, oth):
    return np.array_equal(got[0], ref) and np.array_equal(got[1], oth)


def chain_of(text, minus, q_start, q_end, t_start, t_end, q_size, t_size, from_=FROM_TARGET):
    """-> (state, chain or None, score).  state: lift_exact_model's, with 32 when the record ends beyond a sequence.  A chain only
    for state 0 with at least one aligned column."""
    state = em.entry_state(text, q_end - q_start, t_end - t_start)
    if q_end > q_size or t_end > t_size:
        state |= BEYOND
    if state:
        return state, None, 0
    ops = em.parse(text)[1]
    x, y, eq = em.columns(ops)
    if not len(x):
        return 0, None, 0
    bl = blocks_of(x, y)
    blocks = [(s, bl[j + 1][1] - (yy + s), bl[j + 1][0] - (xx + s)) if j + 1 < len(bl) else (s, 0, 0) for j, (xx, yy, s) in enumerate(bl)]
    x0, y0 = bl[0][0], bl[0][1]
    x1, y1 = bl[-1][0] + bl[-1][2], bl[-1][1] + bl[-1][2]
    qbase = q_size - q_end if minus else q_start
    chain = (t_start + y0, t_start + y1, t_size, int(minus), qbase + x0, qbase + x1, q_size, blocks)
    assert same_columns(walk(chain), t_start + y, qbase + x)          # the blocks reproduce the literal expansion
    swapped = swap(chain)
    if minus:                                                          # the reverse-complemented column set, walked the other way
        assert same_columns(walk(swapped), (q_end - 1 - x)[::-1], (t_size - 1 - (t_start + y))[::-1])
    else:
        assert same_columns(walk(swapped), qbase + x, t_start + y)
    assert swap(swapped) == chain                                      # swap applied twice is the identity
    score = int(eq.sum()) or len(x)
    return 0, swapped if from_ == FROM_QUERY else chain, score


def block_text(blocks):
    return "".join("%d\t%d\t%d\n" % b for b in blocks[:-1]) + "%d\n\n" % blocks[-1][0]


def header_text(score, ref_name, oth_name, chain, id_):
    rs, re, rsize, minus, os_, oe, osize, _ = chain
    return "chain %d %s %d + %d %d %s %d %s %d %d %d\n" % (score, ref_name, rsize, rs, re, oth_name, osize, "-" if minus else "+", os_, oe, id_)


def chain_records(cols, strand, seq_len, cigars, kept=None, set_=0, from_=FROM_TARGET):
    """cigars: {record: text}.  -> dict: rows (one tuple per entry in record order: record, flags, ref_start, ref_end, oth_start,
    oth_end, score, n_blocks, first_block, text_first), blocks [(size, dt, dq)], text (bytes), states, and the request's counts."""
    c = {k: np.asarray(cols[k]).astype(np.int64) for k in lm.COLS}
    rows, blocks, text, text_len, states = [], [], [], 0, []
    n_chains = beyond = empty = bad = 0
    for i in sorted(cigars):
        minus = int(strand[i]) != 0
        q, t = int(c["q_id"][i]), int(c["t_id"][i])
        state, chain, score = chain_of(cigars[i], minus, int(c["q_start"][i]), int(c["q_end"][i]), int(c["t_start"][i]), int(c["t_end"][i]),
                                       int(seq_len[q]), int(seq_len[t]), from_)
        states.append(state)
        beyond += bool(state & BEYOND)
        bad += bool(state & 15)
        in_set = set_ == 0 or bool(kept[i])
        flags = int(minus) | state << 8
        if chain is None or not in_set:
            empty += state == 0 and in_set
            rows.append((i, flags, 0, 0, 0, 0, 0, 0, 0, 0))
            continue
        n_chains += 1
        rows.append((i, flags, chain[0], chain[1], chain[4], chain[5], score, len(chain[7]), len(blocks), text_len))
        blocks += chain[7]
        text.append(block_text(chain[7]))
        text_len += len(text[-1])
    return {"rows": rows, "blocks": blocks, "text": "".join(text).encode(), "state": states, "n_chains": n_chains, "n_blocks": len(blocks),
            "text_bytes": text_len, "cigar_bad": bad, "beyond": beyond, "empty_chains": empty,
            "ops": sum(sum(ch not in "0123456789" for ch in (t.decode("latin-1") if isinstance(t, bytes) else t)) for t in cigars.values())}


def rows_array(rows):
    from sweepga_amd.ucsc import CHAIN_DTYPE
    out = np.zeros(len(rows), dtype=CHAIN_DTYPE)
    for k, row in enumerate(rows):
        out[k] = row
    return out


def paf_lines(paf_text):
    return [ln[:-1] if ln.endswith("\r") else ln for ln in paf_text.split("\n") if len((ln[:-1] if ln.endswith("\r") else ln).split("\t")) >= 11]


def paf_chain_text(paf_text, kept, set_=1, from_=FROM_TARGET):
    """(the chain file, counts without `batches`) as swg_paf_ucsc_chain_text gives them; kept None = no status.  A sequence's size is
    the length on the line that mentions it last (its target column after its query column)."""
    cols, strand, names = lm.parse_paf(paf_text)
    lines = paf_lines(paf_text)
    size = {}
    for ln in lines:
        f = ln.split("\t")
        size[f[0]] = int(f[1])
        size[f[5]] = int(f[6])
    seq_len = [size[nm] for nm in names]
    sel = [i for i in range(len(strand)) if set_ == 0 or kept[i]]
    tags = {i: em.last_cigar_tag(lines[i]) for i in sel}
    got = chain_records(cols, strand, seq_len, {i: tags[i] or "" for i in sel}, None, 0, from_)
    out, id_ = [], 0
    for row in got["rows"]:
        i, flags, rs, re, os_, oe, score, nb, fb, _ = row
        if not nb:
            continue
        id_ += 1
        q, t = int(cols["q_id"][i]), int(cols["t_id"][i])
        ref, oth = (q, t) if from_ == FROM_QUERY else (t, q)
        chain = (rs, re, seq_len[ref], flags & MINUS, os_, oe, seq_len[oth], None)
        out.append(header_text(score, names[ref], names[oth], chain, id_) + block_text(got["blocks"][fb:fb + nb]))
    counts = {"records": len(sel), "chains": got["n_chains"], "bad": got["cigar_bad"], "beyond": got["beyond"],
              "untagged": sum(tags[i] is None for i in sel), "empty": got["empty_chains"], "blocks": got["n_blocks"]}
    return "".join(out), counts


def plan_batches(lens, batch_bytes):
    """The number of batches: consecutive entries whose lengths add up to at most batch_bytes, a longer entry alone; 0 = no bound
    but the call's (fewer than 2^32 bytes)"""
    top = 2**32 - 1
    bound = batch_bytes if 0 < batch_bytes < top else top
    batches, held = 0, 0
    for j, n in enumerate(lens):
        if j == 0 or held + n > bound:
            batches, held = batches + 1, 0
        held += n
    return batches


def paf_batches(paf_text, kept, set_, batch_bytes):
    """... of swg_paf_ucsc_chain_text over the records of the set"""
    lines = paf_lines(paf_text)
    return plan_batches([len(em.last_cigar_tag(ln) or "") for i, ln in enumerate(lines) if set_ == 0 or kept[i]], batch_bytes)


def lift_base(chain, ref_pos):
    """The other-side coordinate (in the chain's other-side strand coordinates) of reference base ref_pos, or None in a gap"""
    rs, _, _, _, os_, _, _, blocks = chain
    r, o = rs, os_
    for size, dt, dq in blocks:
        if r <= ref_pos < r + size:
            return o + ref_pos - r
        r, o = r + size + dt, o + size + dq
    return None
