"""Blocks seen from Python: one row per scaffold chain that a filter call kept -- span on both sequences, member counts, sums and
merged-interval covers -- computed on the device (csrc/swg_blocks.hip) from the record columns plus the filter's status and
chain.  blocks_records / blocks_records_device are the two record seams, Blocks.from_paf the PAF text of an open PafFile."""
import ctypes as C

import numpy as np

from ._lib import SwgBlock, SwgBlockTable, load
from ._marshal import host_column, raise_alnstats, records_from_numpy, records_from_tensors, take_texts

# swg_block as a numpy record
BLOCK_DTYPE = np.dtype([(k, "<u4") for k in ("chain", "q_id", "t_id", "strand", "q_start", "q_end", "t_start", "t_end", "n_core",
                                               "n_inverted", "n_rescued", "reserved")] +
                       [(k, "<u8") for k in ("matches", "block_len", "q_bases", "t_bases", "q_cover", "t_cover", "first_record")])
assert BLOCK_DTYPE.itemsize == C.sizeof(SwgBlock)
COLUMNS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end", "matches", "block_len")


def _call(ctx, fn, rec, status_addr, chain_addr):
    """One call, repeated with a larger array when the first was too small (the capacity protocol of the C seam)."""
    cap = max(1, min(int(rec.n), 1 << 16))
    while True:
        t = SwgBlockTable()
        blocks = np.zeros(cap, dtype=BLOCK_DTYPE)
        t.block_capacity = cap
        t.blocks = C.cast(blocks.ctypes.data, C.POINTER(SwgBlock))
        ctx.check(fn(ctx.handle, C.byref(rec), status_addr, chain_addr, C.byref(t)))
        if int(t.n_blocks) <= cap:
            return blocks[:int(t.n_blocks)].copy()
        cap = int(t.n_blocks)


def blocks_records(ctx, records, status, chain, n_seq=None):
    """swg_blocks_records.  `records`: an SwgRecords with host pointers, or a dict of numpy columns (q_id, t_id, q_start, q_end,
    t_start, t_end, matches, block_len, strand; n_seq = the largest id + 1 unless given).  status: uint8 [n], chain: uint32 [n]
    as a filter call wrote them.  Returns a structured array of BLOCK_DTYPE in ascending chain number."""
    rec, keep = records_from_numpy(records, COLUMNS + ("strand",), n_seq)   # (keep: alive until the call is over)
    st = host_column(status, np.uint8, int(rec.n), "status")
    ch = host_column(chain, np.uint32, int(rec.n), "chain")
    return _call(ctx, ctx.lib.swg_blocks_records, rec, st.ctypes.data, ch.ctypes.data)


def blocks_records_device(ctx, columns, status, chain, n_seq):
    """swg_blocks_records_device over torch tensors on ctx's GPU: `columns` maps q_id, t_id, q_start, q_end, t_start, t_end,
    matches, block_len to contiguous int32 / uint32 tensors of one length and strand to a uint8 one; status is a uint8 tensor and
    chain a 4-byte one, as swg_filter_device left them.  (Anything with .data_ptr() and .numel() works; the caller keeps the
    tensors alive and their work finished.)"""
    rec = records_from_tensors(columns, {**{k: 4 for k in COLUMNS}, "strand": 1}, n_seq)
    if status.element_size() != 1 or chain.element_size() != 4 or min(int(status.numel()), int(chain.numel())) < int(rec.n):
        raise ValueError("status must be 1-byte and chain 4-byte, with an entry per record")
    return _call(ctx, ctx.lib.swg_blocks_records_device, rec, int(status.data_ptr()), int(chain.data_ptr()))


class Blocks:
    """The blocks of an open PafFile under a filter call's status and chain: `text` (PAF, one line per block, bytes) and `table`
    (structured array of BLOCK_DTYPE, ascending chain number)."""

    def __init__(self, text, table):
        self.text, self.table = text, table

    @classmethod
    def from_paf(cls, ctx_or_filter, paf, status, chain):
        """swg_paf_blocks for the text, swg_blocks_records over the handle's columns for the array.  ctx_or_filter: a Context, or
        anything with a `.ctx` (PafFilter); may be None when there is no chain.  The device work is done twice, once for the text
        and once for the array: a convenience for tests and notebooks."""
        ctx = getattr(ctx_or_filter, "ctx", ctx_or_filter)
        lib = load()
        st = host_column(status, np.uint8, paf.n, "status")
        ch = host_column(chain, np.uint32, paf.n, "chain")
        p, n = C.c_void_p(), C.c_uint64()
        rc = lib.swg_paf_blocks(ctx.handle if ctx is not None else None, paf.handle, st.ctypes.data, ch.ctypes.data, C.byref(p), C.byref(n))
        raise_alnstats(lib, rc)
        text, = take_texts(lib, [p], [n], [True])
        if not text:
            return cls(text, np.zeros(0, dtype=BLOCK_DTYPE))
        return cls(text, blocks_records(ctx, paf.records, st, ch))
