"""Sharing seen from Python: how many genomes cover each base.  cover(s, g) is the union, over both axes, of the inter-genome
records between sequence s and genome g; depth(s, x) the number of genomes whose cover holds x.  Per set (all records, the records
a filter call kept): the runs of constant depth >= 1 ordered by (seq, start), and the spectrum -- bases of every genome's sequences
at every depth -- computed on the device (csrc/swg_sharing.hip).  sharing_records / sharing_records_device are the two record
seams, Sharing.from_paf the table and the BED of an open PafFile."""
import ctypes as C

import numpy as np

from ._lib import SWG_OK, SwgDepthRun, SwgError, SwgRecords, SwgSharingRequest, load

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


def _status(status, n):
    if status is None:
        return None
    st = np.ascontiguousarray(status, dtype=np.uint8)
    if st.size < n:
        raise ValueError("status has fewer entries than records")
    return st if st.size else np.zeros(1, dtype=np.uint8)


def sharing_records(ctx, records, seq_genome, seq_len=None, status=None, n_genome=None, want=None):
    """swg_sharing_records.  `records`: an SwgRecords with host pointers, or a dict of numpy columns (q_id, t_id, q_start, q_end,
    t_start, t_end; n_seq = len(seq_genome)).  seq_genome: uint32 [n_seq]; seq_len: uint32 [n_seq] or None (column 0 of a spectrum
    then stays 0).  want: the bit mask (RUNS_ALL | RUNS_KEPT | SPECTRUM_ALL | SPECTRUM_KEPT) or None = everything the status
    allows.  Returns a SharingResult."""
    keep = []
    seq_genome = np.ascontiguousarray(seq_genome, dtype=np.uint32)
    if isinstance(records, dict):
        rec = SwgRecords()
        rec.n = len(records["q_id"])
        for k in COLUMNS:
            a = np.ascontiguousarray(records[k], dtype=np.uint32)
            keep.append(a)
            setattr(rec, k, a.ctypes.data)
        rec.n_seq = len(seq_genome)
    else:
        rec = records
    if n_genome is None:
        n_genome = int(seq_genome.max()) + 1 if seq_genome.size else 1
    if seq_len is not None:
        seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
        if seq_len.size != seq_genome.size:
            raise ValueError("seq_len and seq_genome differ in length")
    st = _status(status, int(rec.n))
    if want is None:
        want = WANT_EVERYTHING if st is not None else RUNS_ALL | SPECTRUM_ALL
    return _call(ctx, ctx.lib.swg_sharing_records, rec, seq_genome.ctypes.data, n_genome,
                 seq_len.ctypes.data if seq_len is not None and seq_len.size else None, st.ctypes.data if st is not None else None, want)


def sharing_records_device(ctx, columns, seq_genome, n_genome, seq_len=None, status=None, want=None):
    """swg_sharing_records_device over torch tensors on ctx's GPU: `columns` maps q_id, t_id, q_start, q_end, t_start, t_end to
    contiguous int32 / uint32 tensors of one length, seq_genome and seq_len (or None) are such tensors of n_seq entries, status a
    uint8 tensor or None.  (Anything with .data_ptr() and .numel() works; the caller keeps the tensors alive and their work
    finished.)"""
    rec = SwgRecords()
    rec.n = int(columns["q_id"].numel())
    for k in COLUMNS:
        t = columns[k]
        if int(t.numel()) != int(rec.n) or t.element_size() != 4 or not t.is_contiguous():
            raise ValueError(f"column {k}: a contiguous 4-byte tensor of {int(rec.n)} entries is needed")
        setattr(rec, k, int(t.data_ptr()))
    rec.n_seq = int(seq_genome.numel())
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
        st = _status(status, paf.n)
        marker = C.create_string_buffer(1)   # a text is asked for by a non-NULL entry
        p, n = (C.c_void_p * 2)(), (C.c_uint64 * 2)()
        for k, wanted in enumerate((table, bed)):
            p[k] = C.addressof(marker) if wanted else None
        rc = lib.swg_paf_sharing(ctx.handle if ctx is not None else None, paf.handle, st.ctypes.data if st is not None else None,
                                 1 if detailed else 0, p, n)
        if rc != SWG_OK:
            raise SwgError(rc, (lib.swg_alnstats_last_error() or b"").decode(errors="replace"))
        text = [None, None]
        for k, wanted in enumerate((table, bed)):
            if wanted:
                text[k] = C.string_at(p[k], n[k])
                lib.swg_free(C.c_void_p(p[k]))
        return cls(text[0], text[1])
