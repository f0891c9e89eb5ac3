"""Gaps seen from Python: what lies between the mappings of one kept chain.  Inside a chain the records that take part (status
SCAFFOLD, chain != 0) are ordered by (q_start, record index); every core record and the nearest core record before it make a
link with dq unaligned query bases and dt unaligned target bases, size = dq - dt an insertion or deletion candidate; every '-'
record of a '+' chain is an inversion candidate -- computed on the device (csrc/swg_gaps.hip).  gaps_records /
gaps_records_device are the two record seams, Gaps.from_paf the two texts of an open PafFile."""
import ctypes as C

import numpy as np

from ._lib import SwgGapPair, SwgGapRow, SwgGapsRequest, load
from ._marshal import host_column, raise_alnstats, records_from_numpy, records_from_tensors, take_texts

# swg_gap_row and swg_gap_pair as numpy records
ROW_DTYPE = np.dtype([(k, "<u4") for k in ("chain", "left", "right", "q_lo", "q_hi", "t_lo", "t_hi")] +
                     [("kind", "u1"), ("flags", "u1"), ("reserved", "<u2")])
PAIR_DTYPE = np.dtype([("q_genome", "<u4"), ("t_genome", "<u4")] +
                      [(k, "<u8") for k in ("links", "n_ins", "ins_bases", "n_del", "del_bases", "n_inv", "inv_bases")])
assert ROW_DTYPE.itemsize == C.sizeof(SwgGapRow) == 32 and PAIR_DTYPE.itemsize == C.sizeof(SwgGapPair) == 64
COLUMNS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")
EVEN, INS, DEL, INV = 0, 1, 2, 3
ROWS, SUMMARY = 1, 2
BINS = 33


class GapsResult:
    """rows: ROW_DTYPE rows ordered by (chain, q_start of the right record, right record); pairs: PAIR_DTYPE entries in ascending
    (q_genome, t_genome); spectrum: uint64 [2, 33], INS and DEL by the bit length of |size|.  rows is None unless ROWS was asked
    for, pairs and spectrum unless SUMMARY was."""

    def __init__(self):
        self.rows = self.pairs = self.spectrum = None


def _call(ctx, fn, rec, status_addr, chain_addr, genome_addr, n_genome, min_size, want):
    """One call, repeated with larger arrays when one of them was too small (the capacity protocol of the C seam)."""
    want = int(want)
    cap = max(1, min(int(rec.n), 1 << 16))
    pair_cap = max(1, min(int(rec.n), int(n_genome) ** 2, 1 << 16))
    while True:
        req = SwgGapsRequest()
        req.want, req.min_size = want, int(min_size)
        out = GapsResult()
        rows = np.zeros(cap, dtype=ROW_DTYPE)
        pairs = np.zeros(pair_cap, dtype=PAIR_DTYPE)
        spectrum = np.zeros((2, BINS), dtype=np.uint64)
        req.capacity, req.rows = cap, C.cast(rows.ctypes.data, C.POINTER(SwgGapRow))
        req.pair_capacity, req.pairs = pair_cap, C.cast(pairs.ctypes.data, C.POINTER(SwgGapPair))
        req.spectrum = C.cast(spectrum.ctypes.data, C.POINTER(C.c_uint64))
        ctx.check(fn(ctx.handle, C.byref(rec), status_addr, chain_addr, genome_addr, C.c_uint32(int(n_genome)), C.byref(req)))
        n_rows, n_pairs = int(req.n_rows) if want & ROWS else 0, int(req.n_pairs) if want & SUMMARY else 0
        if n_rows <= cap and n_pairs <= pair_cap:
            if want & ROWS:
                out.rows = rows[:n_rows].copy()
            if want & SUMMARY:
                out.pairs, out.spectrum = pairs[:n_pairs].copy(), spectrum
            return out
        cap, pair_cap = max(cap, n_rows), max(pair_cap, n_pairs)


def gaps_records(ctx, records, status, chain, seq_genome, min_size=50, n_genome=None, want=ROWS | SUMMARY):
    """swg_gaps_records.  `records`: an SwgRecords with host pointers, or a dict of numpy columns (q_id, t_id, q_start, q_end,
    t_start, t_end, strand; n_seq = len(seq_genome)).  status: uint8 [n], chain: uint32 [n] as a filter call wrote them;
    seq_genome: uint32 [n_seq] (n_genome = its largest value + 1 unless given).  Returns a GapsResult."""
    seq_genome = np.ascontiguousarray(seq_genome, dtype=np.uint32)
    rec, keep = records_from_numpy(records, COLUMNS + ("strand",), len(seq_genome))   # (keep: alive until the call is over)
    if n_genome is None:
        n_genome = int(seq_genome.max()) + 1 if seq_genome.size else 1
    st = host_column(status, np.uint8, int(rec.n), "status")
    ch = host_column(chain, np.uint32, int(rec.n), "chain")
    return _call(ctx, ctx.lib.swg_gaps_records, rec, st.ctypes.data, ch.ctypes.data, seq_genome.ctypes.data if seq_genome.size else None,
                 n_genome, min_size, want)


def gaps_records_device(ctx, columns, status, chain, seq_genome, n_genome, min_size=50, want=ROWS | SUMMARY):
    """swg_gaps_records_device over torch tensors on ctx's GPU: `columns` maps q_id, t_id, q_start, q_end, t_start, t_end to
    contiguous int32 / uint32 tensors of one length and strand to a uint8 one; status is a uint8 tensor and chain a 4-byte one, as
    swg_filter_device left them; seq_genome a 4-byte tensor of n_seq entries.  (Anything with .data_ptr() and .numel() works; the
    caller keeps the tensors alive and their work finished.)"""
    rec = records_from_tensors(columns, {**{k: 4 for k in COLUMNS}, "strand": 1}, seq_genome.numel())
    if status.element_size() != 1 or chain.element_size() != 4 or min(int(status.numel()), int(chain.numel())) < int(rec.n):
        raise ValueError("status must be 1-byte and chain 4-byte, with an entry per record")
    if seq_genome.element_size() != 4:
        raise ValueError("seq_genome must be 4-byte")
    return _call(ctx, ctx.lib.swg_gaps_records_device, rec, int(status.data_ptr()), int(chain.data_ptr()), int(seq_genome.data_ptr()),
                 n_genome, min_size, want)


class Gaps:
    """The gaps of an open PafFile under a filter call's status and chain: `rows` and `summary` (bytes, tab-separated, a header
    line each; None where not asked for) and `table` (the GapsResult of the same input, or None)."""

    def __init__(self, rows, summary, table):
        self.rows, self.summary, self.table = rows, summary, table

    @classmethod
    def from_paf(cls, ctx_or_filter, paf, status, chain, min_size=50, rows=True, summary=True, table=True):
        """swg_paf_gaps for the texts (both from one device call), swg_gaps_records over the handle's columns and its last-'#'
        genome map for the arrays (table=False leaves that second call out).  ctx_or_filter: a Context, or anything with a `.ctx`
        (PafFilter); may be None when no record takes part."""
        ctx = getattr(ctx_or_filter, "ctx", ctx_or_filter)
        lib = load()
        st = host_column(status, np.uint8, paf.n, "status")
        ch = host_column(chain, np.uint32, paf.n, "chain")
        p, n = [C.c_void_p(), C.c_void_p()], [C.c_uint64(), C.c_uint64()]
        args = []
        for k, wanted in enumerate((rows, summary)):
            args += [C.byref(p[k]), C.byref(n[k])] if wanted else [None, None]
        rc = lib.swg_paf_gaps(ctx.handle if ctx is not None else None, paf.handle, st.ctypes.data, ch.ctypes.data, C.c_uint32(int(min_size)), *args)
        raise_alnstats(lib, rc)
        text = take_texts(lib, p, n, (rows, summary))
        result = None
        if table and ctx is not None and paf.n:
            r = paf.records
            result = gaps_records(ctx, r, st, ch, paf.seq_genome_last[:int(r.n_seq)], min_size=min_size, n_genome=int(r.n_genome_last))
        return cls(text[0], text[1], result)
