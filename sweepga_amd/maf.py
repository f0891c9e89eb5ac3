"""Alignment blocks with their gapped bases, on the device (csrc/swg_maf.hip; include/sweepga_gpu.h states the
definitions): every usable entry cut at its breakers (I, D and N ops of split_gap bases or more) into blocks, and for each block the
target row and the query row -- bases as read, '-' in the gaps, the query reverse-complemented on '-'.  maf_records /
maf_records_device are the record seams: a CIGAR set and a sequence set in, MAF_BLOCK_DTYPE blocks and their rows end to end out.
Maf.from_paf is swg_paf_maf_text: the blocks of an open PafFile as MAF text."""
import ctypes as C

import numpy as np

from ._lib import MAF_COUNTS, MAF_FIELDS, SwgCigarSet, SwgMafCounts, SwgMafOptions, SwgMafRequest, SwgSeqSet, default_context, load
from ._marshal import addr, host_column, raise_alnstats, records_from_numpy, records_from_tensors
from .lift import COLUMNS, SETS, cigar_set
from .variants import _FastaHandle, sequence_set

MINUS = 1
MAF_BLOCK_DTYPE = np.dtype([(k, "<u4") for k in ("record", "entry", "op_first", "op_end", "t_start", "t_bases", "q_start", "q_bases", "aligned", "columns",
                                                 "flags", "walk_x")] + [("text_first", "<u8"), ("reserved", "<u8")])
FIELDS = MAF_FIELDS


class MafResult:
    """blocks: a MAF_BLOCK_DTYPE array or None when the capacity did not hold; text: the rows' bytes (uint8) or None; the counts as
    the request returns them."""

    def __init__(self, blocks, text, req):
        self.blocks, self.text = blocks, text
        for k in FIELDS:
            setattr(self, k, int(getattr(req, k)))

    def rows(self, b):
        """(target row, query row) of block b as bytes"""
        e = self.blocks[b]
        at, n = int(e["text_first"]), int(e["columns"])
        return self.text[at:at + n].tobytes(), self.text[at + n:at + 2 * n].tobytes()


def _call(ctx, fn, rec, status_addr, cigars, k, seqs, set_, split_gap, capacity):
    """cigars: (record, offset, text) addresses or None; seqs: (offset address, bases address, n_seq) or None.  capacity: None = two
    calls, the second with arrays of the sizes the first one reported; or (blocks, text bytes), each an int or None for a NULL
    array."""
    req = SwgMafRequest()
    req.set, req.split_gap = int(set_), int(split_gap)
    cs = ss = None
    if cigars is not None:
        cs = SwgCigarSet()
        cs.record, cs.offset, cs.text, cs.k = cigars[0], cigars[1], cigars[2], int(k)
    if seqs is not None:
        ss = SwgSeqSet()
        ss.offset, ss.bases, ss.n_seq = seqs[0], seqs[1], int(seqs[2])
    call = lambda: ctx.check(fn(ctx.handle, C.byref(rec), status_addr, C.byref(cs) if cs is not None else None,   # noqa: E731
                                C.byref(ss) if ss is not None else None, C.byref(req)))
    if capacity is None:
        call()
        capacity = (int(req.n_blocks), int(req.text_bytes))
    arrays = [None if c is None else np.zeros(max(int(c), 1), dtype=dt) for c, dt in zip(capacity, (MAF_BLOCK_DTYPE, np.uint8))]
    req.block_capacity, req.text_capacity = (0 if c is None else int(c) for c in capacity)
    req.blocks, req.text = (addr(a) for a in arrays)
    call()
    counts = (int(req.n_blocks), int(req.text_bytes))
    out = [a[:n] if a is not None and n <= int(c) else None for a, c, n in zip(arrays, capacity, counts)]
    res = MafResult(out[0], out[1], req)
    res.arrays = arrays   # what the call was given, whole (the tests look at what it left untouched)
    return res


def maf_records(ctx, records, strand, n_seq, cigar_records, cigars, seqs, status=None, set="all", split_gap=0, capacity=None):
    """swg_maf_records.  `records`, strand and the CIGAR set as in diffs.diff_records; seqs: one bytes-like per sequence (empty or
    None = absent) or the (offset, bases) arrays of variants.sequence_set().  Returns a MafResult."""
    rec, keep = records_from_numpy(records, COLUMNS, n_seq, strand=strand)
    if any(a.size != int(rec.n) for a in keep):
        raise ValueError("the columns and strand differ in length")
    st = host_column(status, np.uint8, int(rec.n), "status", optional=True)
    record, offset, text = cigars if cigar_records is None else cigar_set(cigar_records, cigars)
    k = int(record.size)
    sset = None
    if seqs is not None:
        s_off, s_bases = seqs if isinstance(seqs, tuple) else sequence_set(seqs)
        s_off, s_bases = np.ascontiguousarray(s_off, dtype=np.uint64), np.ascontiguousarray(s_bases, dtype=np.uint8)
        keep += [s_off, s_bases]
        sset = (s_off.ctypes.data, s_bases.ctypes.data, s_off.size - 1)
    return _call(ctx, ctx.lib.swg_maf_records, rec, addr(st), (record.ctypes.data, offset.ctypes.data, text.ctypes.data) if k else None, k, sset,
                 SETS.get(set, set), split_gap, capacity)


def maf_records_device(ctx, columns, strand, n_seq, cigar_record, cigar_offset, cigar_text, k, seq_offset, seq_bases, status=None, set="all", split_gap=0,
                       capacity=None):
    """swg_maf_records_device over tensors on ctx's GPU (anything with data_ptr / numel / element_size / is_contiguous): as
    eqx.eqx_records_device.  Blocks and text come back on the host."""
    rec = records_from_tensors(columns, {c: 4 for c in COLUMNS}, n_seq)
    for name, t in (("strand", strand), ("status", status)):
        if t is not None and (t.element_size() != 1 or int(t.numel()) < int(rec.n)):
            raise ValueError(f"{name} must be 1-byte with an entry per record")
    if seq_offset is not None and int(seq_offset.numel()) * seq_offset.element_size() < 8 * (int(n_seq) + 1):
        raise ValueError("seq_offset holds fewer than 8 bytes per sequence and one more")
    rec.strand = int(strand.data_ptr())
    k = int(k)
    if k and (int(cigar_record.numel()) * cigar_record.element_size() < 4 * k or int(cigar_offset.numel()) * cigar_offset.element_size() < 8 * (k + 1)):
        raise ValueError("the CIGAR set's record or offset tensor is shorter than k asks for")
    cig = (int(cigar_record.data_ptr()), int(cigar_offset.data_ptr()), int(cigar_text.data_ptr())) if k else None
    sset = (int(seq_offset.data_ptr()), int(seq_bases.data_ptr()), int(n_seq)) if seq_offset is not None and seq_bases is not None else None
    return _call(ctx, ctx.lib.swg_maf_records_device, rec, int(status.data_ptr()) if status is not None else None, cig, k, sset, SETS.get(set, set),
                 split_gap, capacity)


class Maf:
    """The MAF of an open PafFile: `text`, and `counts` (a dict: records usable bad untagged no_sequence out_of_sequence length_mismatch
    blocks gap_only breakers skipped_t skipped_q columns aligned file_bytes batches).  `a score=` is the block's aligned columns: no
    bases are compared."""

    def __init__(self, text, counts):
        self.text, self.counts = text, counts

    @staticmethod
    def _args(paf, status, set, split_gap, batch_bytes, ctx):
        ctx = getattr(ctx, "ctx", ctx)
        lib = load()
        st = host_column(status, np.uint8, paf.n, "status", optional=True)
        set_ = SETS.get(set, set)
        opts = SwgMafOptions()
        opts.set, opts.split_gap, opts.batch_bytes = int(set_), int(split_gap), int(batch_bytes)
        rebased = bool(lib.swg_paf_seq_offsets(paf.handle)) or bool(lib.swg_paf_record_offsets(paf.handle, 0))   # (refused by the library)
        in_set = paf.n if set_ == 0 else (int(np.count_nonzero(st[:paf.n])) if st is not None else 0)
        if ctx is None and in_set and not rebased and set_ in (0, 1):
            ctx = default_context()
        return lib, ctx.handle if ctx is not None else None, st, opts

    @classmethod
    def from_paf(cls, paf, status, fasta=(), set="kept", split_gap=0, batch_bytes=0, ctx=None):
        """swg_paf_maf_text.  fasta: the paths of the FASTA files (plain / .gz / .bgz).  status None: set must be "all".  split_gap:
        an I, D or N op of that many bases or more ends a block; 0 = one block per record.  ctx: a Context, anything with a `.ctx`,
        or None = the default context, which is only opened when the set has records."""
        lib, handle, st, opts = cls._args(paf, status, set, split_gap, batch_bytes, ctx)
        counts = SwgMafCounts()
        p, n = C.c_void_p(), C.c_uint64()
        with _FastaHandle(lib, fasta) as fa:
            raise_alnstats(lib, lib.swg_paf_maf_text(handle, paf.handle, addr(st), fa, C.byref(opts), C.byref(counts), C.byref(p), C.byref(n)))
        text = C.string_at(p.value, n.value).decode("utf-8", errors="surrogateescape") if p.value else ""
        lib.swg_free(p)
        return cls(text, {k: int(getattr(counts, k)) for k in MAF_COUNTS})

    @classmethod
    def write_paf(cls, paf, status, path, fasta=(), set="kept", split_gap=0, batch_bytes=0, ctx=None):
        """swg_paf_maf_write: the same into a file -> the counts."""
        lib, handle, st, opts = cls._args(paf, status, set, split_gap, batch_bytes, ctx)
        counts = SwgMafCounts()
        with _FastaHandle(lib, fasta) as fa:
            raise_alnstats(lib, lib.swg_paf_maf_write(handle, paf.handle, addr(st), fa, C.byref(opts), str(path).encode(), C.byref(counts)))
        return {k: int(getattr(counts, k)) for k in MAF_COUNTS}
