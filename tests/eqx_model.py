"""Literal model of the resolved CIGARs, written from the definitions in include/sweepga_gpu.h: per usable
entry the text is cut into its ops as they stand, every column run is walked column by column over Python byte strings, and the
output is put together as a string -- no prefix sums, no searches, no flags.  Inputs come from tests/variants_model.py's generator
(derive, plant, random_bases, random_case).  Below the model: the texts of the PAF seam."""
import re

import numpy as np

from tests import lift_exact_model as em
from tests import lift_model as lm
from tests import variants_model as vm

USABLE, CHANGED = 1, 2
ENTRY_FIELDS = ("record", "flags", "text_len", "out_ops", "matches", "mismatches", "n_columns", "eq_wrong", "x_wrong", "m_columns", "inserted", "deleted",
                "block", "text_first")
SUMS = ("matches", "mismatches", "n_columns", "eq_wrong", "x_wrong", "m_columns")
FIELDS = ("ops", "cigar_bad", "empty", "usable", "no_sequence", "out_of_sequence", "columns", "out_ops", "text_bytes", "changed") + SUMS
COUNTS = ("records", "usable", "bad", "untagged", "no_sequence", "out_of_sequence", "length_mismatch", "changed", "lines", "columns", "matches", "mismatches",
          "eq_wrong", "x_wrong", "m_columns", "batches")
_OP = re.compile(r"([0-9]+)([MIDNSHP=X])")


def raw_ops(text):
    """The ops of a text of state 0 as (digits as they stand, letter)"""
    if isinstance(text, bytes):
        text = text.decode("latin-1")
    ops = _OP.findall(text)
    assert "".join(d + ch for d, ch in ops) == text, text
    return ops


def entry_eqx(text, minus, q_start, q_end, t_start, T, Q):
    """One usable entry -> (output text, out_ops, sums as a dict with inserted and deleted).  T, Q: the target's and the query's bytes."""
    out, n_out = [], 0
    s = dict.fromkeys(SUMS + ("inserted", "deleted"), 0)
    x = y = 0
    run = []  # the eq of the current run's columns

    def close():
        nonlocal n_out
        at = 0
        while at < len(run):
            end = at
            while end < len(run) and run[end] == run[at]:
                end += 1
            out.append("%d%s" % (end - at, "=" if run[at] else "X"))
            n_out += 1
            at = end
        run.clear()

    for digits, ch in raw_ops(text):
        l = int(digits)
        if ch in "M=X":
            for b in range(l):
                r = vm.norm(T[t_start + y + b])
                a = vm._COMP[vm.norm(Q[q_end - 1 - (x + b)])] if minus else vm.norm(Q[q_start + x + b])
                eq = r == a and r != "N"
                s["matches" if eq else "mismatches"] += 1
                s["n_columns"] += r == "N" or a == "N"
                s["eq_wrong"] += ch == "=" and not eq
                s["x_wrong"] += ch == "X" and eq
                s["m_columns"] += ch == "M"
                run.append(eq)
            x += l
            y += l
            continue
        close()
        out.append(digits + ch)
        n_out += 1
        if ch == "I":
            s["inserted"] += l
            x += l
        elif ch == "D":
            s["deleted"] += l
            y += l
        elif ch == "N":
            y += l
    close()
    return "".join(out), n_out, s


def as_text(t):
    return t.decode("latin-1") if isinstance(t, bytes) else t


def eqx_records(cols, strand, cigars, seqs, kept=None, set_=0):
    """cigars: {record: text}; seqs: one bytes per sequence (empty: absent).  -> dict: entries (tuples in the order of ENTRY_FIELDS,
    one per entry in record order), text (str) and the request's counts."""
    c = {k: np.asarray(cols[k]).astype(np.int64) for k in lm.COLS}
    n = dict.fromkeys(FIELDS, 0)
    entries, texts, at = [], [], 0
    for i in sorted(cigars):
        text = as_text(cigars[i])
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
            entries.append((i,) + (0,) * 13)
            continue
        new, n_out, s = entry_eqx(text, int(strand[i]) != 0, q_start, q_end, t_start, seqs[t], seqs[q])
        changed = new != text
        block = s["matches"] + s["mismatches"] + s["inserted"] + s["deleted"]
        entries.append((i, USABLE | (CHANGED if changed else 0), len(new), n_out) + tuple(s[k] for k in SUMS) + (s["inserted"], s["deleted"], block, at))
        texts.append(new)
        at += len(new)
        n["usable"] += 1
        n["changed"] += changed
        n["out_ops"] += n_out
        n["columns"] += s["matches"] + s["mismatches"]
        for k in SUMS:
            n[k] += s[k]
    n["text_bytes"] = at
    return dict(n, entries=entries, text="".join(texts))


def entries_array(entries):
    from sweepga_amd.eqx import EQX_ENTRY_DTYPE
    out = np.zeros(len(entries), dtype=EQX_ENTRY_DTYPE)
    for k, row in enumerate(entries):
        out[k] = row
    return out


# ---- the text of swg_paf_eqx_text ----------------------------------------------------------------------------------------------------
def rewrite_line(line, matches, block, new):
    """line (without its end) with column 10, column 11 and the value of its last cg:Z: tag replaced"""
    f = line.split("\t")
    last = max(k for k in range(12, len(f)) if f[k].startswith("cg:Z:"))
    tail = "\r" if f[last].endswith("\r") and last == len(f) - 1 else ""   # (a '\r' at the end of a last line without '\n' is no part of the value)
    f[9], f[10], f[last] = str(matches), str(block), "cg:Z:" + new + tail
    return "\t".join(f)


def paf_text(paf_text_, kept, fasta, set_=1, unresolved="keep"):
    """(the resolved PAF, counts without `batches`) as swg_paf_eqx_text gives them; kept None = no status; fasta: (name, bytes) records
    in file order (of two with one name the first counts)."""
    from tests import ucsc_chain_model as um
    cols, strand, names = lm.parse_paf(paf_text_)
    lines = um.paf_lines(paf_text_)
    sel = [i for i in range(len(strand)) if set_ == 0 or kept[i]]
    counts = dict.fromkeys(COUNTS[:-1], 0)
    counts["records"] = len(sel)
    if not sel:
        return "", counts
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
    got = eqx_records(cols, strand, {i: tags[i] or "" for i in sel}, seqs, None, 0)
    out = []
    for row in got["entries"]:
        e = dict(zip(ENTRY_FIELDS, row))
        i = e["record"]
        if e["flags"] & USABLE:
            out.append(rewrite_line(lines[i], e["matches"], e["block"], got["text"][e["text_first"]:e["text_first"] + e["text_len"]]) + "\n")
        elif unresolved == "keep":
            out.append(lines[i] + "\n")
    counts.update(usable=got["usable"], bad=got["cigar_bad"], untagged=sum(tags[i] is None for i in sel), no_sequence=got["no_sequence"],
                  out_of_sequence=got["out_of_sequence"], changed=got["changed"], lines=len(out), columns=got["columns"])
    for k in ("matches", "mismatches", "eq_wrong", "x_wrong", "m_columns"):
        counts[k] = got[k]
    return "".join(out), counts


def batch_costs(paf_text_, kept, set_):
    """the planner's cost per record of the set: text length + min(q_end - q_start, t_end - t_start)"""
    from tests import ucsc_chain_model as um
    cols, strand, _ = lm.parse_paf(paf_text_)
    lines = um.paf_lines(paf_text_)
    return [len(em.last_cigar_tag(lines[i]) or "") + min(int(cols["q_end"][i]) - int(cols["q_start"][i]), int(cols["t_end"][i]) - int(cols["t_start"][i]))
            for i in range(len(strand)) if set_ == 0 or kept[i]]
