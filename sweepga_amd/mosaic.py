"""The mosaic seen from Python: the best mapping at every base.  On one axis (0 = query, 1 = target) the inter-genome records of
a set (all records, or the records a filter call kept) compete by P = weight << 32 | (0xffffffff - record): the heavier record
wins, among equal weights the earlier one.  The rows are the maximal stretches of a sequence with one winner, ordered by (seq,
start); share[g, h] the bases of genome g's sequences won by records whose other sequence is of genome h -- computed on the
device (csrc/swg_mosaic.hip).  mosaic_records / mosaic_records_device are the two record seams, Mosaic.from_paf the two texts of
an open PafFile."""
import ctypes as C

import numpy as np

from ._lib import SwgError, SwgMosaicRequest, SwgMosaicRow, load
from ._marshal import addr, host_column, raise_alnstats, records_from_numpy, records_from_tensors, take_texts, text_slots

# swg_mosaic_row as a numpy record
ROW_DTYPE = np.dtype([("seq", "<u4"), ("start", "<u4"), ("end", "<u4"), ("record", "<u4")])
COLUMNS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")
AXES = {"query": 0, "target": 1, 0: 0, 1: 1}
SETS = {"all": 0, "kept": 1, 0: 0, 1: 1}
ROWS, SHARE = 1, 2


class MosaicResult:
    """rows: ROW_DTYPE rows ordered by (seq, start); bases: the library's sum(end - start); share: uint64 [n_genome, n_genome].
    Each is None unless its bit was asked for."""

    def __init__(self):
        self.rows = self.bases = self.share = None


def _call(ctx, fn, rec, genome_addr, n_genome, status_addr, weight_addr, axis, set_, want):
    """The capacity protocol of the C seam: the first call (capacity 0) learns n and brings the share, a second one brings the
    rows -- and no share again."""
    want, n_genome = int(want), int(n_genome)
    req = SwgMosaicRequest()
    req.want, req.axis, req.set = want, AXES[axis], SETS[set_]
    req.weight = weight_addr
    out = MosaicResult()
    if want & SHARE:
        out.share = np.zeros((n_genome, n_genome), dtype=np.uint64)
        req.share = C.cast(out.share.ctypes.data, C.POINTER(C.c_uint64))
    args = (ctx.handle, C.byref(rec), genome_addr, C.c_uint32(n_genome), status_addr, C.byref(req))
    ctx.check(fn(*args))
    if want & ROWS:
        n, bases = int(req.n), int(req.bases)
        rows = np.zeros(max(n, 1), dtype=ROW_DTYPE)
        if n:
            req.want = ROWS
            req.capacity = n
            req.rows = C.cast(rows.ctypes.data, C.POINTER(SwgMosaicRow))
            ctx.check(fn(*args))
            if int(req.n) != n or int(req.bases) != bases:
                raise SwgError(-3, "mosaic: two calls on one input disagree")
        out.rows, out.bases = rows[:n], bases
    return out


def mosaic_records(ctx, records, seq_genome, status=None, weight=None, axis="query", set=None, n_genome=None, want=ROWS | SHARE):
    """swg_mosaic_records.  `records`: an SwgRecords with host pointers, or a dict of numpy columns (q_id, t_id, q_start, q_end,
    t_start, t_end and, when weight is None, matches; n_seq = len(seq_genome)).  seq_genome: uint32 [n_seq]; weight: uint32 [n] or
    None = the matches column; set: "all" / "kept" (default: kept when a status is given).  Returns a MosaicResult."""
    seq_genome = np.ascontiguousarray(seq_genome, dtype=np.uint32)
    rec, keep = records_from_numpy(records, COLUMNS, len(seq_genome), optional=("matches",))   # (keep: alive until the call is over)
    if n_genome is None:
        n_genome = int(seq_genome.max()) + 1 if seq_genome.size else 1
    st = host_column(status, np.uint8, int(rec.n), "status", optional=True)
    if set is None:
        set = "kept" if st is not None else "all"
    w = None
    if weight is not None:
        w = np.ascontiguousarray(weight, dtype=np.uint32)
        if w.size < int(rec.n):
            raise ValueError("weight has fewer entries than records")
    return _call(ctx, ctx.lib.swg_mosaic_records, rec, seq_genome.ctypes.data, n_genome, addr(st),
                 w.ctypes.data if w is not None and w.size else None, axis, set, want)


def mosaic_records_device(ctx, columns, seq_genome, n_genome, status=None, weight=None, axis="query", set=None, want=ROWS | SHARE):
    """swg_mosaic_records_device over torch tensors on ctx's GPU: `columns` maps q_id, t_id, q_start, q_end, t_start, t_end (and
    matches, read when weight is None) to contiguous int32 / uint32 tensors of one length, seq_genome is such a tensor of n_seq
    entries, status a uint8 tensor or None, weight a 4-byte tensor or None.  (Anything with .data_ptr() and .numel() works; the
    caller keeps the tensors alive and their work finished.)"""
    rec = records_from_tensors(columns, {k: 4 for k in COLUMNS + (("matches",) if "matches" in columns else ())}, seq_genome.numel())
    if seq_genome.element_size() != 4 or (status is not None and (status.element_size() != 1 or int(status.numel()) < int(rec.n))):
        raise ValueError("seq_genome must be 4-byte, status 1-byte with an entry per record")
    if weight is not None and (weight.element_size() != 4 or int(weight.numel()) < int(rec.n)):
        raise ValueError("weight must be 4-byte with an entry per record")
    if set is None:
        set = "kept" if status is not None else "all"
    return _call(ctx, ctx.lib.swg_mosaic_records_device, rec, int(seq_genome.data_ptr()), n_genome,
                 int(status.data_ptr()) if status is not None else None,
                 int(weight.data_ptr()) if weight is not None and int(weight.numel()) else None, axis, set, want)


class Mosaic:
    """The mosaic texts of an open PafFile: `rows` (bytes: sequence, start, end, other_sequence, strand, record, weight,
    other_start, other_end) and `share` (bytes: genome, other_genome, bases and a #total line); None where not asked for."""

    def __init__(self, rows, share):
        self.rows, self.share = rows, share

    @classmethod
    def from_paf(cls, ctx_or_filter, paf, status, axis="query", set="kept", by="matches", rows=True, share=True):
        """swg_paf_mosaic: both texts from one device call.  ctx_or_filter: a Context, or anything with a `.ctx` (PafFilter); may
        be None for a PAF without records.  by: "matches" or "length"."""
        if by not in ("matches", "length"):
            raise ValueError("by: matches or length")
        ctx = getattr(ctx_or_filter, "ctx", ctx_or_filter)
        lib = load()
        st = host_column(status, np.uint8, paf.n, "status", optional=True)
        p, n = text_slots((rows, share))
        rc = lib.swg_paf_mosaic(ctx.handle if ctx is not None else None, paf.handle, addr(st), AXES[axis], SETS[set],
                                1 if by == "length" else 0, p, n)
        raise_alnstats(lib, rc)
        text = take_texts(lib, p, n, (rows, share))
        return cls(text[0], text[1])
