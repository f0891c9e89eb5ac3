"""Divergence from the CIGARs, on the device (csrc/swg_divergence.hip; include/sweepga_gpu.h states the
definitions): per fixed window of W bases along every sequence that carries an inter-genome record of the set, the exact aligned
columns, matches, mismatches, M columns, unaligned and inserted bases, mismatch runs and indels.  Integers only: column identity is
matches / aligned, gap-compressed identity matches / (aligned + indels), BLAST identity matches / (aligned + unaligned + inserted).
divergence_records / divergence_records_device are the record seams, Divergence.from_paf is swg_paf_divergence: the two texts of an
open PafFile."""
import ctypes as C

import numpy as np

from ._lib import DIVERGENCE_SUMS, SwgCigarSet, SwgDivergenceCounts, SwgDivergenceRequest, SwgDivergenceRow, SwgDivergenceSeq, default_context, load
from ._marshal import addr, host_column, raise_alnstats, records_from_numpy, records_from_tensors, take_texts, text_slots
from .lift import COLUMNS, SETS, cigar_set

ROW_DTYPE = np.dtype([(k, "<u4") for k in ("seq", "start", "end", "n")] + [(k, "<u8") for k in DIVERGENCE_SUMS])
SEQ_DTYPE = np.dtype([("seq", "<u4"), ("windows", "<u4"), ("records", "<u8"), ("entries", "<u8")] + [(k, "<u8") for k in DIVERGENCE_SUMS])
assert ROW_DTYPE.itemsize == C.sizeof(SwgDivergenceRow) == 80 and SEQ_DTYPE.itemsize == C.sizeof(SwgDivergenceSeq) == 88
assert C.sizeof(SwgDivergenceRequest) == 104 and C.sizeof(SwgDivergenceCounts) == 56
AXES = {"query": 0, "target": 1, 0: 0, 1: 1}
ANY = 0xffffffff
ROWS, SUMMARY = 1, 2
COUNTS = ("records", "usable", "bad", "untagged", "windows", "seqs", "batches")


def _axis(axis):
    """A name as its number; a number as it is (the library refuses one beyond 1)."""
    if isinstance(axis, str) and axis not in AXES:
        raise ValueError(f"unknown axis {axis!r}: query or target")
    return int(AXES.get(axis, axis))


class DivergenceResult:
    """rows: ROW_DTYPE rows in (seq, start) order; seqs: SEQ_DTYPE entries, one per listed sequence, ascending -- each None unless its
    bit was asked for; state: a uint8 per entry; the counts as the request returns them."""

    def __init__(self, rows, seqs, state, req):
        self.rows, self.seqs, self.state = rows, seqs, state
        for k in ("n_rows", "n_seqs", "ops", "cigar_bad", "usable"):
            setattr(self, k, int(getattr(req, k)))


def _call(ctx, fn, rec, len_addr, genome_addr, n_genome, status_addr, cigars, k, set_, axis, window, other_genome, want):
    """cigars: (record address, offset address, text address) or None.  One call for the counts, one more with arrays of exactly that
    size (the capacity protocol of the C seam, per array)."""
    want = int(want)
    if not 0 <= int(window) <= ANY:
        raise ValueError("the window size is 1 .. 2^32 - 1")
    cs = None
    if cigars is not None:
        cs = SwgCigarSet()
        cs.record, cs.offset, cs.text, cs.k = cigars[0], cigars[1], cigars[2], int(k)
    state = np.zeros(int(k), dtype=np.uint8)
    cap = seq_cap = 0
    while True:
        req = SwgDivergenceRequest()
        req.set, req.axis, req.window, req.want = int(set_), _axis(axis), int(window), want
        req.other_genome = ANY if other_genome is None else int(other_genome)
        req.state = state.ctypes.data if k else None
        rows = np.zeros(max(cap, 1), dtype=ROW_DTYPE)
        seqs = np.zeros(max(seq_cap, 1), dtype=SEQ_DTYPE)
        req.capacity, req.rows = cap, rows.ctypes.data
        req.seq_capacity, req.seqs = seq_cap, seqs.ctypes.data
        ctx.check(fn(ctx.handle, C.byref(rec), len_addr, genome_addr, C.c_uint32(int(n_genome)), status_addr, C.byref(cs) if cs is not None else None,
                     C.byref(req)))
        n_rows, n_seqs = int(req.n_rows) if want & ROWS else 0, int(req.n_seqs) if want & SUMMARY else 0
        if n_rows <= cap and n_seqs <= seq_cap:
            return DivergenceResult(rows[:n_rows].copy() if want & ROWS else None, seqs[:n_seqs].copy() if want & SUMMARY else None, state, req)
        cap, seq_cap = max(cap, n_rows), max(seq_cap, n_seqs)


def divergence_records(ctx, records, strand, seq_len, seq_genome, n_genome, cigar_records, cigars, status=None, set="all", axis="query", window=10_000,
                       other_genome=None, want=ROWS | SUMMARY):
    """swg_divergence_records.  `records`: a dict of numpy columns (q_id, t_id, q_start, q_end, t_start, t_end); strand: uint8 per
    record (0 = '+'); seq_len, seq_genome: uint32 per sequence, genome ids below n_genome; the CIGAR set as ascending record indices
    and one CIGAR text per record, or the (record, offset, text) arrays of lift.cigar_set() as `cigars` with cigar_records None;
    status: uint8 per record as a filter call wrote it (needed by set "kept"); other_genome: a genome id, or None for any.  Returns a
    DivergenceResult."""
    seq_genome = np.ascontiguousarray(seq_genome, dtype=np.uint32)
    seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
    if seq_len.size < seq_genome.size:
        raise ValueError("seq_len has fewer entries than seq_genome")
    rec, keep = records_from_numpy(records, COLUMNS, len(seq_genome), strand=strand)
    if any(a.size != int(rec.n) for a in keep):
        raise ValueError("the columns and strand differ in length")
    st = host_column(status, np.uint8, int(rec.n), "status", optional=True)
    record, offset, text = cigars if cigar_records is None else cigar_set(cigar_records, cigars)
    k = int(record.size)
    return _call(ctx, ctx.lib.swg_divergence_records, rec, seq_len.ctypes.data if seq_len.size else None, seq_genome.ctypes.data if seq_genome.size else None,
                 n_genome, addr(st), (record.ctypes.data, offset.ctypes.data, text.ctypes.data) if k else None, k, SETS.get(set, set), axis, window,
                 other_genome, want)


def divergence_records_device(ctx, columns, strand, seq_len, seq_genome, n_genome, cigar_record, cigar_offset, cigar_text, k, status=None, set="all",
                              axis="query", window=10_000, other_genome=None, want=ROWS | SUMMARY):
    """swg_divergence_records_device over tensors on ctx's GPU (anything with data_ptr / numel / element_size / is_contiguous): the six
    4-byte columns, strand and status (1 byte per record), seq_len and seq_genome (4 bytes per sequence) and the three arrays of the
    set (uint32 [k], uint64 [k + 1], bytes).  Rows, summary and state come back on the host."""
    rec = records_from_tensors(columns, {c: 4 for c in COLUMNS}, seq_genome.numel())
    if seq_genome.element_size() != 4 or seq_len.element_size() != 4 or int(seq_len.numel()) < int(seq_genome.numel()):
        raise ValueError("seq_len and seq_genome must be 4-byte, with an entry per sequence")
    for name, t in (("strand", strand), ("status", status)):
        if t is not None and (t.element_size() != 1 or int(t.numel()) < int(rec.n)):
            raise ValueError(f"{name} must be 1-byte with an entry per record")
    rec.strand = int(strand.data_ptr())
    k = int(k)
    if k and (int(cigar_record.numel()) * cigar_record.element_size() < 4 * k or int(cigar_offset.numel()) * cigar_offset.element_size() < 8 * (k + 1)):
        raise ValueError("the CIGAR set's record or offset tensor is shorter than k asks for")
    cig = (int(cigar_record.data_ptr()), int(cigar_offset.data_ptr()), int(cigar_text.data_ptr())) if k else None
    return _call(ctx, ctx.lib.swg_divergence_records_device, rec, int(seq_len.data_ptr()), int(seq_genome.data_ptr()), n_genome,
                 int(status.data_ptr()) if status is not None else None, cig, k, SETS.get(set, set), axis, window, other_genome, want)


def parse_rows(text):
    """The rows text -> a list of (sequence, start, end, n, then the eight sums)."""
    return [tuple(v if k == 0 else int(v) for k, v in enumerate(ln.split("\t"))) for ln in text.split("\n") if ln and not ln.startswith("#")]


class Divergence:
    """The divergence track of an open PafFile: `text` (one line per window, a BED source) and `summary_text` (one line per listed
    sequence), tab-separated with a header line each; `counts` (a dict: records usable bad untagged windows seqs batches); `rows` and
    `summary` parsed from the texts."""

    def __init__(self, text, summary_text, counts):
        self.text, self.summary_text, self.counts = text, summary_text, counts

    @property
    def rows(self):
        return parse_rows(self.text)

    @property
    def summary(self):
        return parse_rows(self.summary_text)

    @classmethod
    def from_paf(cls, paf, status, set="kept", axis="query", window=10_000, genome=None, batch_bytes=0, ctx=None):
        """swg_paf_divergence.  status None: set must be "all".  genome: only the mappings whose other side belongs to this genome (a
        name with or without its trailing '#'), None = any.  ctx: a Context, anything with a `.ctx`, or None = the default context,
        which is only opened when the set has records.  batch_bytes: CIGAR text per device call, 0 = the library's default."""
        ctx = getattr(ctx, "ctx", ctx)
        lib = load()
        if not 0 <= int(window) <= ANY:
            raise ValueError("the window size is 1 .. 2^32 - 1")
        st = host_column(status, np.uint8, paf.n, "status", optional=True)
        set_ = SETS.get(set, set)
        rebased = bool(lib.swg_paf_seq_offsets(paf.handle)) or bool(lib.swg_paf_record_offsets(paf.handle, 0))   # (refused by the library)
        in_set = paf.n if set_ == 0 else (int(np.count_nonzero(st[:paf.n])) if st is not None else 0)
        if ctx is None and in_set and not rebased and set_ in (0, 1) and _axis(axis) in (0, 1) and int(window) > 0:
            ctx = default_context()
        counts = SwgDivergenceCounts()
        p, n = text_slots((True, True))
        name = None if genome is None else (genome if isinstance(genome, bytes) else str(genome).encode())
        raise_alnstats(lib, lib.swg_paf_divergence(ctx.handle if ctx is not None else None, paf.handle, addr(st), set_, _axis(axis),
                                                   C.c_uint32(int(window)), name, int(batch_bytes), p, n, C.byref(counts)))
        text = [t.decode("utf-8", errors="surrogateescape") for t in take_texts(lib, p, n, (True, True))]
        return cls(text[0], text[1], {k: int(getattr(counts, k)) for k in COUNTS})
