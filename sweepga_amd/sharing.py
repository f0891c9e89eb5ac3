"""Sharing seen from Python: how many genomes cover each base.  cover(s, g) is the union, over both axes, of the inter-genome
records between sequence s and genome g; depth(s, x) the number of genomes whose cover holds x.  Per set (all records, the records
a filter call kept): the runs of constant depth >= 1 ordered by (seq, start), and the spectrum -- bases of every genome's sequences
at every depth -- computed on the device (csrc/swg_sharing.hip).  sharing_records / sharing_records_device are the two record
seams, Sharing.from_paf the table and the BED of an open PafFile."""
import ctypes as C

import numpy as np

from ._lib import SwgDepthRun, SwgError, SwgSharingRequest, load
from ._marshal import addr, host_column, raise_alnstats, records_from_numpy, records_from_tensors, take_texts, text_slots

# swg_depth_run as a numpy record
RUN_DTYPE = np.dtype([("seq", "<u4"), ("start", "<u4"), ("end", "<u4"), ("depth", "<u4")])
COLUMNS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")
SETS = ("all", "kept")
RUNS_ALL, RUNS_KEPT, SPECTRUM_ALL, SPECTRUM_KEPT = 1, 2, 4, 8
WANT_EVERYTHING = 0xf


class SharingResult:
    """runs[set]: RUN_DTYPE rows ordered by (seq, start); bases[set]: the library's sum(end - start); spectrum[set]: uint64
    [n_genome, n_genome], entry [g, d] = bases of genome g's sequences at depth d.  Each holds the sets whose bit was asked for."""

    def __init__(self):
        self.runs, self.bases, self.spectrum = {}, {}, {}


def _call(ctx, fn, rec, genome_addr, n_genome, len_addr, status_addr, want):
    """The capacity protocol of the C seam: the first call (capacity 0) learns every n and brings the spectra, a second one brings
    the rows -- and no spectrum again."""
    want, n_genome = int(want), int(n_genome)
    req = SwgSharingRequest()
    req.want = want
    out, spec = SharingResult(), {}
    for s in range(2):
        if want >> (2 + s) & 1:
            spec[s] = np.zeros((n_genome, n_genome), dtype=np.uint64)
            req.set[s].spectrum = C.cast(spec[s].ctypes.data, C.POINTER(C.c_uint64))
    args = (ctx.handle, C.byref(rec), genome_addr, C.c_uint32(n_genome), len_addr, status_addr, C.byref(req))
    ctx.check(fn(*args))
    bufs = {}
    for s in range(2):
        if want >> s & 1:
            lst = req.set[s]
            bufs[s] = (np.zeros(max(int(lst.n), 1), dtype=RUN_DTYPE), int(lst.n), int(lst.bases))
            lst.capacity = int(lst.n)
            lst.rows = C.cast(bufs[s][0].ctypes.data, C.POINTER(SwgDepthRun))
    if any(n for _, n, _ in bufs.values()):
        req.want = want & 0x3
        ctx.check(fn(*args))
    for s, (rows, n, bases) in bufs.items():
        if int(req.set[s].n) != n or int(req.set[s].bases) != bases:
            raise SwgError(-3, "sharing: two calls on one input disagree")
        out.runs[SETS[s]] = rows[:n]
        out.bases[SETS[s]] = bases
    for s, a in spec.items():
        out.spectrum[SETS[s]] = a
    return out


def sharing_records(ctx, records, seq_genome, seq_len=None, status=None, n_genome=None, want=None):
    """swg_sharing_records.  `records`: an SwgRecords with host pointers, or a dict of numpy columns (q_id, t_id, q_start, q_end,
    t_start, t_end; n_seq = len(seq_genome)).  seq_genome: uint32 [n_seq]; seq_len: uint32 [n_seq] or None (column 0 of a spectrum
    then stays 0).  want: the bit mask (RUNS_ALL | RUNS_KEPT | SPECTRUM_ALL | SPECTRUM_KEPT) or None = everything the status
    allows.  Returns a SharingResult."""
    seq_genome = np.ascontiguousarray(seq_genome, dtype=np.uint32)
    rec, keep = records_from_numpy(records, COLUMNS, len(seq_genome))   # (keep: alive until the call is over)
    if n_genome is None:
        n_genome = int(seq_genome.max()) + 1 if seq_genome.size else 1
    if seq_len is not None:
        seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
        if seq_len.size != seq_genome.size:
            raise ValueError("seq_len and seq_genome differ in length")
    st = host_column(status, np.uint8, int(rec.n), "status", optional=True)
    if want is None:
        want = WANT_EVERYTHING if st is not None else RUNS_ALL | SPECTRUM_ALL
    return _call(ctx, ctx.lib.swg_sharing_records, rec, seq_genome.ctypes.data, n_genome,
                 seq_len.ctypes.data if seq_len is not None and seq_len.size else None, addr(st), want)


def sharing_records_device(ctx, columns, seq_genome, n_genome, seq_len=None, status=None, want=None):
    """swg_sharing_records_device over torch tensors on ctx's GPU: `columns` maps q_id, t_id, q_start, q_end, t_start, t_end to
    contiguous int32 / uint32 tensors of one length, seq_genome and seq_len (or None) are such tensors of n_seq entries, status a
    uint8 tensor or None.  (Anything with .data_ptr() and .numel() works; the caller keeps the tensors alive and their work
    finished.)"""
    rec = records_from_tensors(columns, {k: 4 for k in COLUMNS}, seq_genome.numel())
    if seq_genome.element_size() != 4 or (status is not None and (status.element_size() != 1 or int(status.numel()) < int(rec.n))):
        raise ValueError("seq_genome must be 4-byte, status 1-byte with an entry per record")
    if seq_len is not None and (seq_len.element_size() != 4 or int(seq_len.numel()) != int(rec.n_seq)):
        raise ValueError("seq_len must be 4-byte with an entry per sequence")
    if want is None:
        want = WANT_EVERYTHING if status is not None else RUNS_ALL | SPECTRUM_ALL
    return _call(ctx, ctx.lib.swg_sharing_records_device, rec, int(seq_genome.data_ptr()), n_genome,
                 int(seq_len.data_ptr()) if seq_len is not None else None, int(status.data_ptr()) if status is not None else None, want)


class Sharing:
    """The sharing texts of an open PafFile: `table` (bytes: genome, length, private / shared / core of all and of kept records,
    a #total row, with detailed=True the spectrum) and `bed` (bytes: sequence, start, end, n_all, n_kept); None where not asked for."""

    def __init__(self, table, bed):
        self.table, self.bed = table, bed

    @classmethod
    def from_paf(cls, ctx_or_filter, paf, status, detailed=False, table=True, bed=True):
        """swg_paf_sharing: both texts from one device call.  ctx_or_filter: a Context, or anything with a `.ctx` (PafFilter); may
        be None for a PAF without records."""
        ctx = getattr(ctx_or_filter, "ctx", ctx_or_filter)
        lib = load()
        st = host_column(status, np.uint8, paf.n, "status", optional=True)
        p, n = text_slots((table, bed))
        rc = lib.swg_paf_sharing(ctx.handle if ctx is not None else None, paf.handle, addr(st), 1 if detailed else 0, p, n)
        raise_alnstats(lib, rc)
        text = take_texts(lib, p, n, (table, bed))
        return cls(text[0], text[1])
