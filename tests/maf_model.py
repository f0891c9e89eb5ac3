"""Literal model of the alignment blocks, written from the definitions in include/sweepga_gpu.h: per usable
entry the text is cut into its ops as they stand, the ops are walked one by one, breakers close the run that is open, and the two
rows of every block are put together op by op from slices of the sequences (numpy: 2 * 10^6 columns take milliseconds) -- no
prefix sums, no searches, no flags.  Everything it produces is held against the properties at the end of `entry_blocks` and of
`maf_records`.  Inputs come from tests/variants_model.py's generator.  Below the model: the text of the PAF seam."""
import numpy as np

from tests import eqx_model as xm
from tests import lift_exact_model as em
from tests import lift_model as lm

MINUS = 1
BLOCK_FIELDS = ("record", "entry", "op_first", "op_end", "t_start", "t_bases", "q_start", "q_bases", "aligned", "columns", "flags", "walk_x", "text_first",
                "reserved")
FIELDS = ("ops", "cigar_bad", "empty", "usable", "no_sequence", "out_of_sequence", "n_blocks", "gap_only", "breakers", "skipped_t", "skipped_q", "columns",
          "aligned", "text_bytes")
COUNTS = ("records", "usable", "bad", "untagged", "no_sequence", "out_of_sequence", "length_mismatch", "blocks", "gap_only", "breakers", "skipped_t",
          "skipped_q", "columns", "aligned", "file_bytes", "batches")
HEADER = "##maf version=1\n"
DASH = 45


def _comp_raw():
    t = list(range(256))
    for a, b in ("AT", "CG", "RY", "KM", "BV", "DH"):
        for x, y in ((a, b), (b, a)):
            t[ord(x)], t[ord(x.lower())] = ord(y), ord(y.lower())
    t[ord("U")], t[ord("u")] = ord("A"), ord("a")
    return np.array(t, dtype=np.uint8)


COMP_RAW = _comp_raw()


def comp_raw(b):
    return int(COMP_RAW[b])


def _bytes(a):
    return np.frombuffer(a, dtype=np.uint8) if isinstance(a, (bytes, bytearray)) else np.asarray(a, dtype=np.uint8)


def entry_blocks(text, minus, q_start, q_end, t_start, T, Q, g=0):
    """One usable entry -> (blocks, sums).  A block is a dict: op_first, op_end (from the entry's first op), t_start, t_bases, q_start
    (forward strand), q_bases, aligned, columns, walk_x, rows (target row + query row, bytes).  sums: gap_only, breakers, skipped_t,
    skipped_q, and lost_t, lost_q: the bases of the gap-only candidates, which appear in no block either.  T, Q: the target's and the
    query's bytes."""
    T, Q = _bytes(T), _bytes(Q)
    ops = [(int(d), ch) for d, ch in xm.raw_ops(text)]
    blocks = []
    sums = dict.fromkeys(("gap_only", "breakers", "skipped_t", "skipped_q", "lost_t", "lost_q"), 0)
    x = y = 0
    run = None      # the open candidate: first op, walk offsets there, the pieces of the two rows, advances

    def close(end):
        nonlocal run
        if run is None:
            return
        if run["aligned"] == 0:
            sums["gap_only"] += 1
            sums["lost_t"] += run["t_bases"]
            sums["lost_q"] += run["q_bases"]
        else:
            t_row = np.concatenate(run["t"]) if run["t"] else np.zeros(0, dtype=np.uint8)
            q_row = np.concatenate(run["q"]) if run["q"] else np.zeros(0, dtype=np.uint8)
            qb, tb = run["q_bases"], run["t_bases"]
            blocks.append(dict(op_first=run["first"], op_end=end, t_start=t_start + run["y0"], t_bases=tb,
                               q_start=q_end - run["x0"] - qb if minus else q_start + run["x0"], q_bases=qb, aligned=run["aligned"],
                               columns=qb + tb - run["aligned"], walk_x=run["x0"], rows=t_row.tobytes() + q_row.tobytes()))
        run = None

    for k, (l, ch) in enumerate(ops):
        if g > 0 and ch in "IDN" and l >= g:      # a breaker: its bases appear in no block
            close(k)
            sums["breakers"] += 1
            if ch == "I":
                sums["skipped_q"] += l
                x += l
            else:
                sums["skipped_t"] += l
                y += l
            continue
        if run is None:
            run = dict(first=k, x0=x, y0=y, t=[], q=[], q_bases=0, t_bases=0, aligned=0)
        if ch in "M=XIDN" and l:
            on_t, on_q = ch != "I", ch not in "DN"
            run["t"].append(T[t_start + y:t_start + y + l] if on_t else np.full(l, DASH, dtype=np.uint8))
            if not on_q:
                run["q"].append(np.full(l, DASH, dtype=np.uint8))
            elif minus:      # walk offset x + b is Q[q_end - 1 - (x + b)], complemented
                run["q"].append(COMP_RAW[Q[q_end - x - l:q_end - x][::-1]])
            else:
                run["q"].append(Q[q_start + x:q_start + x + l])
            if on_t:
                run["t_bases"] += l
                y += l
            if on_q:
                run["q_bases"] += l
                x += l
            if on_t and on_q:
                run["aligned"] += l
    close(len(ops))

    # ---- the properties
    # 5: every base of the entry lies in a block or under a breaker -- or in a gap-only candidate, which the count gap_only tells of
    assert sum(b["t_bases"] for b in blocks) + sums["skipped_t"] + sums["lost_t"] == y
    assert sum(b["q_bases"] for b in blocks) + sums["skipped_q"] + sums["lost_q"] == x == q_end - q_start
    for b in blocks:
        n = b["columns"]
        rows = np.frombuffer(b["rows"], dtype=np.uint8)
        t_row, q_row = rows[:n], rows[n:]
        assert len(rows) == 2 * n and n >= 1 and b["aligned"] >= 1                                              # 1
        t_src = T[b["t_start"]:b["t_start"] + b["t_bases"]]
        q_src = Q[b["q_start"]:b["q_start"] + b["q_bases"]]
        if (t_src == DASH).any() or (q_src == DASH).any():
            continue      # a sequence that holds '-' itself: the rows cannot be told from their gaps
        t_gap, q_gap = t_row == DASH, q_row == DASH
        assert not (t_gap & q_gap).any()                                                                        # 1
        assert np.array_equal(t_row[~t_gap], t_src)                                                             # 2
        assert np.array_equal(q_row[~q_gap], COMP_RAW[q_src[::-1]] if minus else q_src)                         # 3
        assert (int((~t_gap).sum()), int((~q_gap).sum()), int((~t_gap & ~q_gap).sum())) == (b["t_bases"], b["q_bases"], b["aligned"])      # 6
    if g == 0:                                                                                                  # 4
        assert len(blocks) <= 1 and sums["breakers"] == 0
        if blocks:
            assert (blocks[0]["t_bases"], blocks[0]["q_bases"], blocks[0]["op_first"], blocks[0]["op_end"]) == (y, x, 0, len(ops))
    return blocks, sums


def maf_records(cols, strand, cigars, seqs, kept=None, set_=0, g=0):
    """cigars: {record: text}; seqs: one bytes per sequence (empty: absent).  -> dict: blocks (tuples in the order of BLOCK_FIELDS),
    text (bytes) and the request's counts."""
    c = {k: np.asarray(cols[k]).astype(np.int64) for k in lm.COLS}
    n = dict.fromkeys(FIELDS, 0)
    rows, texts, at = [], [], 0
    for j, i in enumerate(sorted(cigars)):
        text = xm.as_text(cigars[i])
        q_start, q_end, t_start, t_end = (int(c[k][i]) for k in ("q_start", "q_end", "t_start", "t_end"))
        state = em.entry_state(text, q_end - q_start, t_end - t_start)
        n["ops"] += sum(ch not in "0123456789" for ch in text)
        why = None
        if state & 15:
            why = "cigar_bad"
        elif state:
            why = "empty"
        elif not (set_ == 0 or bool(kept[i])):
            why = "outside"
        else:
            q, t = int(c["q_id"][i]), int(c["t_id"][i])
            if not (len(seqs[q]) and len(seqs[t])):
                why = "no_sequence"
            elif not (t_end <= len(seqs[t]) and q_end <= len(seqs[q])):
                why = "out_of_sequence"
        if why is not None:
            if why != "outside":
                n[why] += 1
            continue
        minus = int(strand[i]) != 0
        blocks, sums = entry_blocks(text, minus, q_start, q_end, t_start, seqs[t], seqs[q], g)
        n["usable"] += 1
        for k in ("gap_only", "breakers", "skipped_t", "skipped_q"):
            n[k] += sums[k]
        for b in blocks:
            rows.append((i, j, b["op_first"], b["op_end"], b["t_start"], b["t_bases"], b["q_start"], b["q_bases"], b["aligned"], b["columns"],
                         MINUS if minus else 0, b["walk_x"], at, 0))
            texts.append(b["rows"])
            at += len(b["rows"])
            n["n_blocks"] += 1
            n["columns"] += b["columns"]
            n["aligned"] += b["aligned"]
        assert sum(b["t_bases"] for b in blocks) + sums["skipped_t"] + sums["lost_t"] == t_end - t_start                # 5
        assert sum(b["q_bases"] for b in blocks) + sums["skipped_q"] + sums["lost_q"] == q_end - q_start
    n["text_bytes"] = at
    assert at == 2 * n["columns"]
    return dict(n, blocks=rows, text=b"".join(texts))


def blocks_array(blocks):
    from sweepga_amd.maf import MAF_BLOCK_DTYPE
    out = np.zeros(len(blocks), dtype=MAF_BLOCK_DTYPE)
    for k, row in enumerate(blocks):
        out[k] = row
    return out


# ---- the text of swg_paf_maf_text ----------------------------------------------------------------------------------------------------
def block_text(t_name, t_len, q_name, q_len, block, rows):
    """One MAF block.  block: a tuple in the order of BLOCK_FIELDS or a dict; rows: the target row, then the query row"""
    b = dict(zip(BLOCK_FIELDS, block)) if not isinstance(block, dict) else block
    n = b["columns"]
    rows = rows.decode("latin-1") if isinstance(rows, bytes) else rows
    minus = bool(b["flags"] & MINUS)
    qs = q_len - b["q_start"] - b["q_bases"] if minus else b["q_start"]
    return ("a score=%d\ns %s %d %d + %d %s\ns %s %d %d %s %d %s\n\n"
            % (b["aligned"], t_name, b["t_start"], b["t_bases"], t_len, rows[:n], q_name, qs, b["q_bases"], "-" if minus else "+", q_len, rows[n:2 * n]))


def paf_text(paf_text_, kept, fasta, set_=1, g=0):
    """(the MAF, counts without `batches`) as swg_paf_maf_text gives them; kept None = no status; fasta: (name, bytes) records in file
    order (of two with one name the first counts)."""
    from tests import ucsc_chain_model as um
    cols, strand, names = lm.parse_paf(paf_text_)
    lines = um.paf_lines(paf_text_)
    sel = [i for i in range(len(strand)) if set_ == 0 or kept[i]]
    counts = dict.fromkeys(COUNTS[:-1], 0)
    counts["records"] = len(sel)
    counts["file_bytes"] = len(HEADER)
    if not sel:
        return HEADER, counts
    size = {}
    for ln in lines:
        f = ln.split("\t")
        size[f[0]] = int(f[1])
        size[f[5]] = int(f[6])
    have = {}
    for nm, seq in fasta:
        have.setdefault(nm, seq)
    named = {int(cols[c][i]) for i in sel for c in ("q_id", "t_id")}
    seqs = []
    for s, nm in enumerate(names):
        seq = have.get(nm, b"") if s in named else b""
        if s in named and nm in have and len(seq) != size[nm]:
            counts["length_mismatch"] += 1
            seq = b""
        seqs.append(seq)
    tags = {i: em.last_cigar_tag(lines[i]) for i in sel}
    got = maf_records(cols, strand, {i: tags[i] or "" for i in sel}, seqs, None, 0, g)
    out = [HEADER]
    for row in got["blocks"]:
        b = dict(zip(BLOCK_FIELDS, row))
        f = lines[b["record"]].split("\t")
        at = b["text_first"]
        out.append(block_text(f[5], int(f[6]), f[0], int(f[1]), b, got["text"][at:at + 2 * b["columns"]]))
    text = "".join(out)
    counts.update(usable=got["usable"], bad=got["cigar_bad"], untagged=sum(tags[i] is None for i in sel), no_sequence=got["no_sequence"],
                  out_of_sequence=got["out_of_sequence"], blocks=got["n_blocks"], file_bytes=len(text.encode("latin-1")))
    for k in ("gap_only", "breakers", "skipped_t", "skipped_q", "columns", "aligned"):
        counts[k] = got[k]
    return text, counts


def batch_costs(paf_text_, kept, set_):
    """the planner's cost per record of the set: text length + (q_end - q_start) + (t_end - t_start)"""
    from tests import ucsc_chain_model as um
    cols, strand, _ = lm.parse_paf(paf_text_)
    lines = um.paf_lines(paf_text_)
    return [len(em.last_cigar_tag(lines[i]) or "") + int(cols["q_end"][i]) - int(cols["q_start"][i]) + int(cols["t_end"][i]) - int(cols["t_start"][i])
            for i in range(len(strand)) if set_ == 0 or kept[i]]
