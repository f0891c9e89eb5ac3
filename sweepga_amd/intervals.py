"""Intervals seen from Python: where the coverage of breadth lies.  Per unit (one sequence against one genome of the other side,
inter-genome records only) and per axis the maximal merged intervals of ALL records, of the records a filter call KEPT, and LOST
= ALL minus KEPT -- computed on the device (csrc/swg_intervals.hip).  intervals_records / intervals_records_device are the two
record seams, Intervals.from_paf the BED-like text of an open PafFile."""
import ctypes as C

import numpy as np

from ._lib import SwgError, SwgInterval, SwgIntervalRequest, load
from ._marshal import addr, host_column, raise_alnstats, records_from_numpy, records_from_tensors, take_texts

# swg_interval as a numpy record
INTERVAL_DTYPE = np.dtype([("seq", "<u4"), ("other_genome", "<u4"), ("start", "<u4"), ("end", "<u4")])
COLUMNS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")
ALL, KEPT, LOST = 0, 1, 2
SETS = ("all", "kept", "lost")
AXES = ("q", "t")
WANT_EVERYTHING = 0x3f


def want_bits(names):
    """("lost", "q") pairs -> the request's bit mask."""
    return sum(1 << (SETS.index(s) * 2 + AXES.index(a)) for s, a in names)


class IntervalLists(dict):
    """{(set, axis): rows} for the wanted lists, set in ("all", "kept", "lost"), axis in ("q", "t"); rows are INTERVAL_DTYPE
    arrays ordered by (seq, other_genome, start).  `bases[(set, axis)]` is the library's sum(end - start) of the list."""

    def __init__(self):
        super().__init__()
        self.bases = {}


def _call(ctx, fn, rec, genome_addr, n_genome, status_addr, want):
    """Two calls, the capacity protocol of the C seam: the first with capacity 0 learns every n, the second brings the rows."""
    want = int(want)
    req = SwgIntervalRequest()
    req.want = want
    ctx.check(fn(ctx.handle, C.byref(rec), genome_addr, C.c_uint32(int(n_genome)), status_addr, C.byref(req)))
    out, bufs = IntervalLists(), {}
    for s in range(3):
        for a in range(2):
            if want >> (s * 2 + a) & 1:
                lst = req.list[s][a]
                bufs[s, a] = (np.zeros(max(int(lst.n), 1), dtype=INTERVAL_DTYPE), int(lst.n), int(lst.bases))
                lst.capacity = int(lst.n)
                lst.rows = C.cast(bufs[s, a][0].ctypes.data, C.POINTER(SwgInterval))
    if any(n for _, n, _ in bufs.values()):
        ctx.check(fn(ctx.handle, C.byref(rec), genome_addr, C.c_uint32(int(n_genome)), status_addr, C.byref(req)))
    for (s, a), (rows, n, bases) in bufs.items():
        lst = req.list[s][a]
        if int(lst.n) != n or int(lst.bases) != bases:
            raise SwgError(-3, "intervals: two calls on one input disagree")
        out[SETS[s], AXES[a]] = rows[:n]
        out.bases[SETS[s], AXES[a]] = bases
    return out


def intervals_records(ctx, records, seq_genome, status=None, n_genome=None, want=None):
    """swg_intervals_records.  `records`: an SwgRecords with host pointers, or a dict of numpy columns (q_id, t_id, q_start, q_end,
    t_start, t_end; n_seq = len(seq_genome)).  seq_genome: uint32 [n_seq].  want: the bit mask (set * 2 + axis) or None = every list
    the status allows.  Returns an IntervalLists."""
    seq_genome = np.ascontiguousarray(seq_genome, dtype=np.uint32)
    rec, keep = records_from_numpy(records, COLUMNS, len(seq_genome))   # (keep: alive until the call is over)
    if n_genome is None:
        n_genome = int(seq_genome.max()) + 1 if seq_genome.size else 1
    st = host_column(status, np.uint8, int(rec.n), "status", optional=True)
    if want is None:
        want = WANT_EVERYTHING if st is not None else 0x3
    return _call(ctx, ctx.lib.swg_intervals_records, rec, seq_genome.ctypes.data, n_genome, addr(st), want)


def intervals_records_device(ctx, columns, seq_genome, n_genome, status=None, want=None):
    """swg_intervals_records_device over torch tensors on ctx's GPU: `columns` maps q_id, t_id, q_start, q_end, t_start, t_end to
    contiguous int32 / uint32 tensors of one length, seq_genome is such a tensor of n_seq entries, status a uint8 tensor or None.
    (Anything with .data_ptr() and .numel() works; the caller keeps the tensors alive and their work finished.)"""
    rec = records_from_tensors(columns, {k: 4 for k in COLUMNS}, seq_genome.numel())
    if seq_genome.element_size() != 4 or (status is not None and (status.element_size() != 1 or int(status.numel()) < int(rec.n))):
        raise ValueError("seq_genome must be 4-byte, status 1-byte with an entry per record")
    if want is None:
        want = WANT_EVERYTHING if status is not None else 0x3
    return _call(ctx, ctx.lib.swg_intervals_records_device, rec, int(seq_genome.data_ptr()), n_genome,
                 int(status.data_ptr()) if status is not None else None, want)


class Intervals:
    """The interval texts of an open PafFile: `text[set]` (bytes, BED-like: name, start, end, other genome, q|t) for the sets asked
    for, `genomes` (names by genome id, trailing '#' kept)."""

    def __init__(self, text, genomes):
        self.text, self.genomes = text, genomes

    @classmethod
    def from_paf(cls, ctx_or_filter, paf, status=None, sets=None):
        """swg_paf_interval_texts: every set of `sets` (names of SETS; None = all three with a status, "all" without) from one
        device call.  ctx_or_filter: a Context, or anything with a `.ctx` (PafFilter); may be None for a PAF without records."""
        from .alnstats import genome_last
        ctx = getattr(ctx_or_filter, "ctx", ctx_or_filter)
        lib = load()
        st = host_column(status, np.uint8, paf.n, "status", optional=True)
        if sets is None:
            sets = SETS if st is not None else ("all",)
        mask = sum(1 << SETS.index(s) for s in sets)
        p, n = (C.c_void_p * 3)(), (C.c_uint64 * 3)()
        rc = lib.swg_paf_interval_texts(ctx.handle if ctx is not None else None, paf.handle, addr(st), mask, p, n)
        raise_alnstats(lib, rc)
        texts = take_texts(lib, p, n, [mask >> k & 1 for k in range(3)])
        text = {s: texts[SETS.index(s)] for s in sets}
        genomes = {}
        for i, nm in enumerate(paf.names):
            genomes.setdefault(int(paf.seq_genome_last[i]), genome_last(nm))
        return cls(text, [genomes[g] for g in range(len(genomes))])
