"""Placement seen from Python: every sequence ordered and oriented along its best partner of each other genome.  On one axis (0 =
query, 1 = target) the inter-genome records of a set (all records, or the records a filter call kept) vote with their length on
that axis for a partner sequence and a strand; the winner of each (sequence, partner genome) gives the row, the weighted median of
its records' anchors the offset, and the rows come in layout order (genome, partner genome, partner, start, sequence) with a rank
along each partner -- computed on the device (csrc/swg_place.hip; include/sweepga_gpu.h has the definitions).  place_records /
place_records_device are the two record seams, Place.from_paf the two texts of an open PafFile."""
import ctypes as C

import numpy as np

from ._lib import SwgPlacePair, SwgPlacement, SwgPlaceRequest, load
from ._marshal import addr, host_column, raise_alnstats, records_from_numpy, records_from_tensors, take_texts, text_slots

# swg_placement and swg_place_pair as numpy records
ROW_DTYPE = np.dtype([(k, "<u4") for k in ("seq", "partner", "genome", "partner_genome")] + [("offset", "<i8"), ("start", "<i8")] +
                     [(k, "<u8") for k in ("bases", "fwd", "rev", "total_bases", "runner_bases", "n_records")] +
                     [(k, "<u4") for k in ("q_lo", "q_hi", "t_lo", "t_hi", "rank")] + [("orient", "u1"), ("reserved", "u1", (3,))])
PAIR_DTYPE = np.dtype([("genome", "<u4"), ("partner_genome", "<u4")] + [(k, "<u8") for k in ("rows", "reversed", "length", "bases", "total_bases")])
assert ROW_DTYPE.itemsize == C.sizeof(SwgPlacement) == 104 and PAIR_DTYPE.itemsize == C.sizeof(SwgPlacePair) == 48
COLUMNS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")
AXES = {"query": 0, "target": 1, 0: 0, 1: 1}
SETS = {"all": 0, "kept": 1, 0: 0, 1: 1}
ROWS, SUMMARY = 1, 2
# the columns of text 0, for Place.table
TABLE_DTYPE = np.dtype([("sequence", object), ("length", "<u8"), ("partner", object), ("partner_length", "<u8"), ("orient", "U1"), ("start", "<i8"),
                        ("end", "<i8")] + [(k, "<u8") for k in ("rank", "bases", "fwd", "rev", "total", "runner", "records", "q_lo", "q_hi", "t_lo", "t_hi")])


class PlaceResult:
    """rows: ROW_DTYPE rows in layout order; pairs: PAIR_DTYPE entries in ascending (genome, partner_genome).  Each is None unless
    its bit was asked for."""

    def __init__(self):
        self.rows = self.pairs = None


def _call(ctx, fn, rec, len_addr, genome_addr, n_genome, status_addr, axis, set_, min_bases, want):
    """One call, repeated with larger arrays when one of them was too small (the capacity protocol of the C seam, per array)."""
    want = int(want)
    cap = max(1, min(int(rec.n), 1 << 16))
    pair_cap = max(1, min(int(rec.n), int(n_genome) ** 2, 1 << 16))
    while True:
        req = SwgPlaceRequest()
        req.want, req.axis, req.set, req.min_bases = want, AXES[axis], SETS[set_], int(min_bases)
        out = PlaceResult()
        rows = np.zeros(cap, dtype=ROW_DTYPE)
        pairs = np.zeros(pair_cap, dtype=PAIR_DTYPE)
        req.capacity, req.rows = cap, C.cast(rows.ctypes.data, C.POINTER(SwgPlacement))
        req.pair_capacity, req.pairs = pair_cap, C.cast(pairs.ctypes.data, C.POINTER(SwgPlacePair))
        ctx.check(fn(ctx.handle, C.byref(rec), len_addr, genome_addr, C.c_uint32(int(n_genome)), status_addr, C.byref(req)))
        n_rows, n_pairs = int(req.n_rows) if want & ROWS else 0, int(req.n_pairs) if want & SUMMARY else 0
        if n_rows <= cap and n_pairs <= pair_cap:
            if want & ROWS:
                out.rows = rows[:n_rows].copy()
            if want & SUMMARY:
                out.pairs = pairs[:n_pairs].copy()
            return out
        cap, pair_cap = max(cap, n_rows), max(pair_cap, n_pairs)


def place_records(ctx, records, seq_len, seq_genome, status=None, axis="query", set=None, min_bases=0, n_genome=None, want=ROWS | SUMMARY):
    """swg_place_records.  `records`: an SwgRecords with host pointers, or a dict of numpy columns (q_id, t_id, q_start, q_end,
    t_start, t_end, strand; n_seq = len(seq_genome)).  seq_len, seq_genome: uint32 [n_seq] (n_genome = the largest genome + 1 unless
    given); status: uint8 [n] as a filter call wrote it, or None; set: "all" / "kept" (default: kept when a status is given).
    Returns a PlaceResult."""
    seq_genome = np.ascontiguousarray(seq_genome, dtype=np.uint32)
    seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
    if seq_len.size < seq_genome.size:
        raise ValueError("seq_len has fewer entries than seq_genome")
    rec, keep = records_from_numpy(records, COLUMNS + ("strand",), len(seq_genome))   # (keep: alive until the call is over)
    if n_genome is None:
        n_genome = int(seq_genome.max()) + 1 if seq_genome.size else 1
    st = host_column(status, np.uint8, int(rec.n), "status", optional=True)
    if set is None:
        set = "kept" if status is not None else "all"
    return _call(ctx, ctx.lib.swg_place_records, rec, seq_len.ctypes.data if seq_len.size else None,
                 seq_genome.ctypes.data if seq_genome.size else None, n_genome, addr(st), axis, set, min_bases, want)


def place_records_device(ctx, columns, seq_len, seq_genome, n_genome, status=None, axis="query", set=None, min_bases=0, want=ROWS | SUMMARY):
    """swg_place_records_device over torch tensors on ctx's GPU: `columns` maps q_id, t_id, q_start, q_end, t_start, t_end to
    contiguous int32 / uint32 tensors of one length and strand to a uint8 one; seq_len and seq_genome are 4-byte tensors of n_seq
    entries, status a uint8 tensor as swg_filter_device left it, or None.  (Anything with .data_ptr() and .numel() works; the caller
    keeps the tensors alive and their work finished.)"""
    rec = records_from_tensors(columns, {**{k: 4 for k in COLUMNS}, "strand": 1}, seq_genome.numel())
    if seq_genome.element_size() != 4 or seq_len.element_size() != 4 or int(seq_len.numel()) < int(seq_genome.numel()):
        raise ValueError("seq_len and seq_genome must be 4-byte, with an entry per sequence")
    if status is not None and (status.element_size() != 1 or int(status.numel()) < int(rec.n)):
        raise ValueError("status must be 1-byte with an entry per record")
    if set is None:
        set = "kept" if status is not None else "all"
    return _call(ctx, ctx.lib.swg_place_records_device, rec, int(seq_len.data_ptr()), int(seq_genome.data_ptr()), n_genome,
                 int(status.data_ptr()) if status is not None else None, axis, set, min_bases, want)


class Place:
    """The placement texts of an open PafFile: `rows` and `summary` (bytes, tab-separated, a header line each; None where not
    asked for) and `table` (the lines of `rows` as a TABLE_DTYPE array, or None)."""

    def __init__(self, rows, summary):
        self.rows, self.summary = rows, summary

    @property
    def table(self):
        if self.rows is None:
            return None
        lines = [l.split("\t") for l in self.rows.decode().splitlines()[1:]]
        out = np.zeros(len(lines), dtype=TABLE_DTYPE)
        for i, f in enumerate(lines):
            out[i] = (f[0], int(f[1]), f[2], int(f[3]), f[4]) + tuple(int(x) for x in f[5:])
        return out

    @classmethod
    def from_paf(cls, ctx_or_filter, paf, status, axis="query", set="kept", min_bases=0, rows=True, summary=True):
        """swg_paf_place: both texts from one device call, under the handle's last-'#' genome map and last-seen lengths.
        ctx_or_filter: a Context, or anything with a `.ctx` (PafFilter); may be None for a PAF without records."""
        ctx = getattr(ctx_or_filter, "ctx", ctx_or_filter)
        lib = load()
        st = host_column(status, np.uint8, paf.n, "status", optional=True)
        p, n = text_slots((rows, summary))
        rc = lib.swg_paf_place(ctx.handle if ctx is not None else None, paf.handle, addr(st), AXES[axis], SETS[set], C.c_uint64(int(min_bases)), p, n)
        raise_alnstats(lib, rc)
        text = take_texts(lib, p, n, (rows, summary))
        return cls(text[0], text[1])
