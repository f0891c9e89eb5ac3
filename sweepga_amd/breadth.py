"""Breadth seen from Python: per ordered genome pair, the bases of each side under at least one inter-genome mapping (merged
intervals), for all records and for the records a filter call kept -- computed on the device (csrc/swg_breadth.hip).
breadth_records / breadth_records_device are the two record seams, Breadth.from_paf the report of an open PafFile."""
import ctypes as C

import numpy as np

from ._lib import SwgBreadthCounts, SwgBreadthPair, load
from ._marshal import addr, host_column, raise_alnstats, records_from_numpy, records_from_tensors, take_texts

# swg_breadth_pair as a numpy record
BREADTH_PAIR_DTYPE = np.dtype([("q_genome", "<u4"), ("t_genome", "<u4"), ("q_bases", "<u8"), ("t_bases", "<u8"), ("q_union", "<u8"),
                               ("t_union", "<u8"), ("first_record", "<u8")])
COLUMNS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")


def _call(ctx, fn, rec, genome_addr, n_genome, status_addr):
    """One call, repeated with a larger pair array when the first was too small (the capacity protocol of the C seam)."""
    cap = max(1, min(int(rec.n), int(n_genome) ** 2, 1 << 16))
    while True:
        sets = []
        for _ in range(2 if status_addr else 1):
            c = SwgBreadthCounts()
            pairs = np.zeros(cap, dtype=BREADTH_PAIR_DTYPE)
            c.pair_capacity = cap
            c.pairs = C.cast(pairs.ctypes.data, C.POINTER(SwgBreadthPair))
            sets.append((c, pairs))
        ctx.check(fn(ctx.handle, C.byref(rec), genome_addr, C.c_uint32(int(n_genome)), status_addr, C.byref(sets[0][0]),
                     C.byref(sets[1][0]) if status_addr else None))
        need = max(int(c.n_pairs) for c, _ in sets)
        if need <= cap:
            out = [pairs[:int(c.n_pairs)].copy() for c, pairs in sets]
            return out[0], (out[1] if status_addr else None)
        cap = need


def breadth_records(ctx, records, seq_genome, status=None, n_genome=None):
    """swg_breadth_records.  `records`: an SwgRecords with host pointers, or a dict of numpy columns (q_id, t_id, q_start, q_end,
    t_start, t_end; n_seq = len(seq_genome)).  seq_genome: uint32 [n_seq].  Returns (all, kept) structured arrays of
    BREADTH_PAIR_DTYPE in order of first record; kept is None without status."""
    seq_genome = np.ascontiguousarray(seq_genome, dtype=np.uint32)
    rec, keep = records_from_numpy(records, COLUMNS, len(seq_genome))   # (keep: alive until the call is over)
    if n_genome is None:
        n_genome = int(seq_genome.max()) + 1 if seq_genome.size else 1
    st = host_column(status, np.uint8, int(rec.n), "status", optional=True)
    return _call(ctx, ctx.lib.swg_breadth_records, rec, seq_genome.ctypes.data, n_genome, addr(st))


def breadth_records_device(ctx, columns, seq_genome, n_genome, status=None):
    """swg_breadth_records_device over torch tensors on ctx's GPU: `columns` maps q_id, t_id, q_start, q_end, t_start, t_end to
    contiguous int32 / uint32 tensors of one length, seq_genome is such a tensor of n_seq entries, status a uint8 tensor or None.
    (Anything with .data_ptr() and .numel() works; the caller keeps the tensors alive and their work finished.)"""
    rec = records_from_tensors(columns, {k: 4 for k in COLUMNS}, seq_genome.numel())
    if seq_genome.element_size() != 4 or (status is not None and (status.element_size() != 1 or int(status.numel()) < int(rec.n))):
        raise ValueError("seq_genome must be 4-byte, status 1-byte with an entry per record")
    return _call(ctx, ctx.lib.swg_breadth_records_device, rec, int(seq_genome.data_ptr()), n_genome,
                 int(status.data_ptr()) if status is not None else None)


class Breadth:
    """The breadth of an open PafFile: `text` (the report, bytes), `all` and `kept` (structured arrays; kept None without status)
    and `genomes` (names by genome id, trailing '#' kept)."""

    def __init__(self, text, all_, kept, genomes):
        self.text, self.all, self.kept, self.genomes = text, all_, kept, genomes

    @classmethod
    def from_paf(cls, ctx_or_filter, paf, status=None, detailed=True):
        """swg_paf_breadth for the text, swg_breadth_records over the handle's columns for the arrays.  ctx_or_filter: a Context,
        or anything with a `.ctx` (PafFilter); may be None for a PAF without records.  The device work is done twice, once
        inside swg_paf_breadth (which hands out text only) and once for the arrays: a convenience for tests and notebooks.  At
        10^8 records call the one you need -- the C function for the report, breadth_records for the integers."""
        from .alnstats import genome_last
        ctx = getattr(ctx_or_filter, "ctx", ctx_or_filter)
        lib = load()
        st = host_column(status, np.uint8, paf.n, "status", optional=True)
        p, n = C.c_void_p(), C.c_uint64()
        rc = lib.swg_paf_breadth(ctx.handle if ctx is not None else None, paf.handle, addr(st), int(bool(detailed)), C.byref(p), C.byref(n))
        raise_alnstats(lib, rc)
        text, = take_texts(lib, [p], [n], [True])
        genomes = {}
        for i, nm in enumerate(paf.names):
            genomes.setdefault(int(paf.seq_genome_last[i]), genome_last(nm))
        names = [genomes[g] for g in range(len(genomes))]
        if paf.n == 0:
            empty = np.zeros(0, dtype=BREADTH_PAIR_DTYPE)
            return cls(text, empty, empty.copy() if st is not None else None, names)
        a, k = breadth_records(ctx, paf.records, paf.seq_genome_last, st, n_genome=int(paf.records.n_genome_last))
        return cls(text, a, k, names)
