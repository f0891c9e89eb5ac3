"""Windows seen from Python: per fixed window of W bases along every sequence that carries an inter-genome record, the number of
records that touch it, the summed depth, the bases covered at all and the matches that fall into it -- for all records and for the
records a filter call kept, side by side -- and per sequence their sums.  Integers only: mean depth is depth / (end - start),
identity matches / depth, breadth covered / (end - start).  Computed on the device (csrc/swg_windows.hip; include/sweepga_gpu.h has
the definitions).  windows_records / windows_records_device are the two record seams, Windows.from_paf the two texts of an open
PafFile."""
import ctypes as C

import numpy as np

from ._lib import SwgWindowRow, SwgWindowSeq, SwgWindowsRequest, load
from ._marshal import addr, host_column, raise_alnstats, records_from_numpy, records_from_tensors, take_texts, text_slots

# swg_window_row and swg_window_seq as numpy records ([0] = all, [1] = kept)
ROW_DTYPE = np.dtype([(k, "<u4") for k in ("seq", "index", "start", "end")] + [("n", "<u4", (2,)), ("covered", "<u4", (2,)), ("depth", "<u8", (2,)),
                                                                                ("matches", "<u8", (2,))])
SEQ_DTYPE = np.dtype([("seq", "<u4"), ("windows", "<u4"), ("empty", "<u4", (2,))] + [(k, "<u8", (2,)) for k in ("covered", "depth", "matches", "records")])
assert ROW_DTYPE.itemsize == C.sizeof(SwgWindowRow) == 64 and SEQ_DTYPE.itemsize == C.sizeof(SwgWindowSeq) == 80
AXES = {"query": 0, "target": 1, 0: 0, 1: 1}
ANY = 0xffffffff
ROWS, SUMMARY = 1, 2


class WindowsResult:
    """rows: ROW_DTYPE rows in (seq, index) order; seqs: SEQ_DTYPE entries, one per listed sequence, ascending.  Each is None unless
    its bit was asked for."""

    def __init__(self):
        self.rows = self.seqs = None


def _columns(axis):
    return ("q_id", "t_id") + (("t_start", "t_end") if AXES[axis] else ("q_start", "q_end"))


def _call(ctx, fn, rec, len_addr, genome_addr, n_genome, status_addr, axis, window, other_genome, weight_addr, want):
    """One call for the counts, one more with arrays of exactly that size (the capacity protocol of the C seam, per array)."""
    want = int(want)
    if not 0 <= int(window) <= ANY:
        raise ValueError("the window size is 1 .. 2^32 - 1")
    cap = seq_cap = 0
    while True:
        req = SwgWindowsRequest()
        req.want, req.axis, req.window = want, AXES[axis], int(window)
        req.other_genome = ANY if other_genome is None else int(other_genome)
        req.weight = weight_addr
        out = WindowsResult()
        rows = np.zeros(max(cap, 1), dtype=ROW_DTYPE)
        seqs = np.zeros(max(seq_cap, 1), dtype=SEQ_DTYPE)
        req.capacity, req.rows = cap, C.cast(rows.ctypes.data, C.POINTER(SwgWindowRow))
        req.seq_capacity, req.seqs = seq_cap, C.cast(seqs.ctypes.data, C.POINTER(SwgWindowSeq))
        ctx.check(fn(ctx.handle, C.byref(rec), len_addr, genome_addr, C.c_uint32(int(n_genome)), status_addr, C.byref(req)))
        n_rows, n_seqs = int(req.n_rows) if want & ROWS else 0, int(req.n_seqs) if want & SUMMARY else 0
        if n_rows <= cap and n_seqs <= seq_cap:
            if want & ROWS:
                out.rows = rows[:n_rows].copy()
            if want & SUMMARY:
                out.seqs = seqs[:n_seqs].copy()
            return out
        cap, seq_cap = max(cap, n_rows), max(seq_cap, n_seqs)


def windows_records(ctx, records, seq_len, seq_genome, status=None, axis="query", window=10_000, other_genome=None, weight=None, n_genome=None,
                    want=ROWS | SUMMARY):
    """swg_windows_records.  `records`: an SwgRecords with host pointers, or a dict of numpy columns (q_id, t_id, the start and end of
    the axis, and matches unless `weight` is given; n_seq = len(seq_genome)).  seq_len, seq_genome: uint32 [n_seq] (n_genome = the
    largest genome + 1 unless given); status: uint8 [n] as a filter call wrote it, or None (no kept set); other_genome: a genome id,
    or None for any; weight: uint32 [n] in place of the matches column.  Returns a WindowsResult."""
    seq_genome = np.ascontiguousarray(seq_genome, dtype=np.uint32)
    seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
    if seq_len.size < seq_genome.size:
        raise ValueError("seq_len has fewer entries than seq_genome")
    rec, keep = records_from_numpy(records, _columns(axis), len(seq_genome), optional=("matches",))   # (keep: alive until the call is over)
    if n_genome is None:
        n_genome = int(seq_genome.max()) + 1 if seq_genome.size else 1
    st = host_column(status, np.uint8, int(rec.n), "status", optional=True)
    wt = host_column(weight, np.uint32, int(rec.n), "weight", optional=True)
    return _call(ctx, ctx.lib.swg_windows_records, rec, seq_len.ctypes.data if seq_len.size else None,
                 seq_genome.ctypes.data if seq_genome.size else None, n_genome, addr(st), axis, window, other_genome, addr(wt), want)


def windows_records_device(ctx, columns, seq_len, seq_genome, n_genome, status=None, axis="query", window=10_000, other_genome=None, weight=None,
                           want=ROWS | SUMMARY):
    """swg_windows_records_device over torch tensors on ctx's GPU: `columns` maps q_id, t_id, the start and end of the axis and (unless
    `weight` is given) matches to contiguous int32 / uint32 tensors of one length; seq_len and seq_genome are 4-byte tensors of n_seq
    entries, status a uint8 tensor as swg_filter_device left it, or None; weight a 4-byte tensor with an entry per record.  (Anything
    with .data_ptr() and .numel() works; the caller keeps the tensors alive and their work finished.)"""
    names = _columns(axis) + (() if weight is not None else ("matches",))
    rec = records_from_tensors(columns, {k: 4 for k in names}, seq_genome.numel())
    if seq_genome.element_size() != 4 or seq_len.element_size() != 4 or int(seq_len.numel()) < int(seq_genome.numel()):
        raise ValueError("seq_len and seq_genome must be 4-byte, with an entry per sequence")
    if status is not None and (status.element_size() != 1 or int(status.numel()) < int(rec.n)):
        raise ValueError("status must be 1-byte with an entry per record")
    if weight is not None and (weight.element_size() != 4 or int(weight.numel()) < int(rec.n)):
        raise ValueError("weight must be 4-byte with an entry per record")
    return _call(ctx, ctx.lib.swg_windows_records_device, rec, int(seq_len.data_ptr()), int(seq_genome.data_ptr()), n_genome,
                 int(status.data_ptr()) if status is not None else None, axis, window, other_genome,
                 int(weight.data_ptr()) if weight is not None else None, want)


class Windows:
    """The window texts of an open PafFile: `rows` (a BED-like table, one line per window) and `summary` (one line per listed
    sequence) as bytes, tab-separated with a header line each; None where not asked for."""

    def __init__(self, rows, summary):
        self.rows, self.summary = rows, summary

    @classmethod
    def from_paf(cls, ctx_or_filter, paf, status, axis="query", window=10_000, other_genome=None, rows=True, summary=True):
        """swg_paf_windows: both texts from one device call, under the handle's last-'#' genome map and last-seen lengths.
        other_genome: a genome name (with or without its trailing '#'), or None for any.  ctx_or_filter: a Context, or anything with
        a `.ctx` (PafFilter); may be None for a PAF without records."""
        ctx = getattr(ctx_or_filter, "ctx", ctx_or_filter)
        if not 0 <= int(window) <= ANY:
            raise ValueError("the window size is 1 .. 2^32 - 1")
        lib = load()
        st = host_column(status, np.uint8, paf.n, "status", optional=True)
        p, n = text_slots((rows, summary))
        name = None if other_genome is None else (other_genome if isinstance(other_genome, bytes) else str(other_genome).encode())
        rc = lib.swg_paf_windows(ctx.handle if ctx is not None else None, paf.handle, addr(st), AXES[axis], C.c_uint32(int(window)), name, p, n)
        raise_alnstats(lib, rc)
        text = take_texts(lib, p, n, (rows, summary))
        return cls(text[0], text[1])
