"""UCSC chain files from the CIGARs, on the device (csrc/swg_ucsc.hip; include/sweepga_gpu.h states the
definitions).  ucsc_chain_records / ucsc_chain_records_device are the record seams: a CIGAR set in, one CHAIN_DTYPE row per entry, the
BLOCK_DTYPE blocks and the text of the block lines out.  UcscChain.from_paf is swg_paf_ucsc_chain_text: the chain file of an open
PafFile as one text."""
import ctypes as C

import numpy as np

from ._lib import SwgCigarSet, SwgUcscCounts, SwgUcscRequest, default_context, load
from ._marshal import addr, host_column, raise_alnstats, records_from_numpy, records_from_tensors
from .lift import COLUMNS, SETS, cigar_set

FROM_TARGET, FROM_QUERY = 0, 1
FROMS = {"target": FROM_TARGET, "query": FROM_QUERY}
MINUS = 1
CIGAR_BEYOND = 32
BLOCK_DTYPE = np.dtype([(k, np.uint32) for k in ("size", "dt", "dq")])
CHAIN_DTYPE = np.dtype([(k, np.uint32) for k in ("record", "flags", "ref_start", "ref_end", "oth_start", "oth_end", "score", "n_blocks")]
                       + [("first_block", np.uint64), ("text_first", np.uint64)])
COUNTS = ("records", "chains", "bad", "beyond", "untagged", "empty", "blocks", "batches")


class UcscResult:
    """chains: a CHAIN_DTYPE array, one row per entry of the set (n_blocks == 0: no chain); blocks: a BLOCK_DTYPE array; text: the
    block lines as bytes -- each None when the capacity given did not hold it; state: a uint8 per entry; the counts as the request
    returns them."""

    def __init__(self, chains, blocks, text, state, req):
        self.chains, self.blocks, self.text, self.state = chains, blocks, text, state
        for k in ("n_chains", "n_blocks", "text_bytes", "ops", "cigar_bad", "beyond", "empty_chains"):
            setattr(self, k, int(getattr(req, k)))


def _call(ctx, fn, rec, seq_len_addr, status_addr, cigars, k, set_, from_, capacity):
    """cigars: (record address, offset address, text address) or None.  capacity: None = two calls, the second with arrays of
    the sizes the first one reported; or (chains, blocks, text bytes), each an int or None for a NULL array."""
    req = SwgUcscRequest()
    req.set, req.from_ = int(set_), int(from_)
    state = np.zeros(int(k), dtype=np.uint8)
    req.state = state.ctypes.data if k else None
    cs = None
    if cigars is not None:
        cs = SwgCigarSet()
        cs.record, cs.offset, cs.text, cs.k = cigars[0], cigars[1], cigars[2], int(k)
    call = lambda: ctx.check(fn(ctx.handle, C.byref(rec), seq_len_addr, status_addr, C.byref(cs) if cs is not None else None, C.byref(req)))   # noqa: E731
    if capacity is None:
        call()
        capacity = (int(k), int(req.n_blocks), int(req.text_bytes))
    arrays = [None if c is None else np.zeros(max(int(c), 1), dtype=dt) for c, dt in zip(capacity, (CHAIN_DTYPE, BLOCK_DTYPE, np.uint8))]
    for name, c, a in zip(("chain", "block", "text"), capacity, arrays):
        setattr(req, name + "_capacity", 0 if c is None else int(c))
    req.chains, req.blocks, req.text = (addr(a) for a in arrays)
    call()
    counts = (int(k), int(req.n_blocks), int(req.text_bytes))
    out = [a[:n] if a is not None and n <= int(c) else None for a, c, n in zip(arrays, capacity, counts)]
    return UcscResult(out[0], out[1], out[2].tobytes() if out[2] is not None else None, state, req)


def ucsc_chain_records(ctx, records, strand, n_seq, seq_len, cigar_records, cigars, status=None, set="all", from_="target", capacity=None):
    """swg_ucsc_chain_records.  `records`: a dict of numpy columns (q_id, t_id, q_start, q_end, t_start, t_end); strand: uint8 per
    record (0 = '+'); seq_len: uint32 per sequence; the CIGAR set as ascending record indices and one CIGAR text per record, or the
    (record, offset, text) arrays of lift.cigar_set() as `cigars` with cigar_records None.  Returns a UcscResult."""
    rec, keep = records_from_numpy(records, COLUMNS, n_seq, strand=strand)
    if any(a.size != int(rec.n) for a in keep):
        raise ValueError("the columns and strand differ in length")
    st = host_column(status, np.uint8, int(rec.n), "status", optional=True)
    sl = host_column(seq_len, np.uint32, int(rec.n_seq), "seq_len", optional=True)
    record, offset, text = cigars if cigar_records is None else cigar_set(cigar_records, cigars)
    k = int(record.size)
    return _call(ctx, ctx.lib.swg_ucsc_chain_records, rec, addr(sl), addr(st), (record.ctypes.data, offset.ctypes.data, text.ctypes.data) if k else None, k,
                 SETS.get(set, set), FROMS.get(from_, from_), capacity)


def ucsc_chain_records_device(ctx, columns, strand, n_seq, seq_len, cigar_record, cigar_offset, cigar_text, k, status=None, set="all", from_="target",
                              capacity=None):
    """swg_ucsc_chain_records_device over tensors on ctx's GPU (anything with data_ptr / numel / element_size / is_contiguous): the six
    4-byte columns, strand and status (1 byte per record), seq_len (4 bytes per sequence) and the three arrays of the set (uint32 [k],
    uint64 [k + 1], bytes).  Rows, blocks, text and state come back on the host."""
    rec = records_from_tensors(columns, {c: 4 for c in COLUMNS}, n_seq)
    for name, t in (("strand", strand), ("status", status)):
        if t is not None and (t.element_size() != 1 or int(t.numel()) < int(rec.n)):
            raise ValueError(f"{name} must be 1-byte with an entry per record")
    if seq_len is not None and int(seq_len.numel()) * seq_len.element_size() < 4 * int(n_seq):
        raise ValueError("seq_len holds fewer than 4 bytes per sequence")
    rec.strand = int(strand.data_ptr())
    k = int(k)
    if k and (int(cigar_record.numel()) * cigar_record.element_size() < 4 * k or int(cigar_offset.numel()) * cigar_offset.element_size() < 8 * (k + 1)):
        raise ValueError("the CIGAR set's record or offset tensor is shorter than k asks for")
    cig = (int(cigar_record.data_ptr()), int(cigar_offset.data_ptr()), int(cigar_text.data_ptr())) if k else None
    return _call(ctx, ctx.lib.swg_ucsc_chain_records_device, rec, int(seq_len.data_ptr()) if seq_len is not None else None,
                 int(status.data_ptr()) if status is not None else None, cig, k, SETS.get(set, set), FROMS.get(from_, from_), capacity)


def parse_chains(text):
    """A chain file's text -> (chains, blocks): per chain the header's twelve fields behind `chain` (numbers as int), and per chain a
    list of (size, dt, dq) with (size, 0, 0) for the last block."""
    chains, blocks = [], []
    for part in text.split("\n\n"):
        lines = [ln for ln in part.split("\n") if ln]
        if not lines:
            continue
        f = lines[0].split(" ")
        chains.append(tuple(int(v) if k in (0, 2, 4, 5, 7, 9, 10, 11) else v for k, v in enumerate(f[1:])))
        blocks.append([tuple(int(v) for v in ln.split("\t")) + (0, 0) * (ln.count("\t") == 0) for ln in lines[1:]])
    return chains, blocks


class UcscChain:
    """The chain file of an open PafFile: `text`, `counts` (a dict: records chains bad beyond untagged empty blocks batches), and
    `chains` / `blocks` parsed from the text (parse_chains)."""

    def __init__(self, text, counts):
        self.text, self.counts = text, counts

    @property
    def chains(self):
        return parse_chains(self.text)[0]

    @property
    def blocks(self):
        return parse_chains(self.text)[1]

    @staticmethod
    def _args(paf, status, from_, set, ctx):
        ctx = getattr(ctx, "ctx", ctx)
        lib = load()
        st = host_column(status, np.uint8, paf.n, "status", optional=True)
        set_, from_ = SETS.get(set, set), FROMS.get(from_, from_)
        rebased = bool(lib.swg_paf_seq_offsets(paf.handle)) or bool(lib.swg_paf_record_offsets(paf.handle, 0))   # (refused by the library)
        in_set = paf.n if set_ == 0 else (int(np.count_nonzero(st[:paf.n])) if st is not None else 0)
        if ctx is None and in_set and not rebased and set_ in (0, 1) and from_ in (0, 1):
            ctx = default_context()
        return lib, ctx.handle if ctx is not None else None, st, set_, from_

    @classmethod
    def from_paf(cls, paf, status, from_="target", set="kept", batch_bytes=0, ctx=None):
        """swg_paf_ucsc_chain_text.  status None: set must be "all".  ctx: a Context, anything with a `.ctx`, or None = the default
        context, which is only opened when the set has records.  batch_bytes: CIGAR text per device call, 0 = the library's default."""
        lib, handle, st, set_, from_ = cls._args(paf, status, from_, set, ctx)
        counts, p, n = SwgUcscCounts(), C.c_void_p(), C.c_uint64()
        raise_alnstats(lib, lib.swg_paf_ucsc_chain_text(handle, paf.handle, addr(st), set_, from_, int(batch_bytes), C.byref(counts), C.byref(p), C.byref(n)))
        text = C.string_at(p.value, n.value).decode("utf-8", errors="surrogateescape")
        lib.swg_free(p)
        return cls(text, {k: int(getattr(counts, k)) for k in COUNTS})

    @classmethod
    def write_paf(cls, paf, status, path, from_="target", set="kept", batch_bytes=0, ctx=None):
        """swg_paf_ucsc_chain_write: the same into a file -> the counts."""
        lib, handle, st, set_, from_ = cls._args(paf, status, from_, set, ctx)
        counts = SwgUcscCounts()
        raise_alnstats(lib, lib.swg_paf_ucsc_chain_write(handle, paf.handle, addr(st), set_, from_, str(path).encode(), int(batch_bytes), C.byref(counts)))
        return {k: int(getattr(counts, k)) for k in COUNTS}
