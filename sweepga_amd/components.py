"""Components seen from Python: which sequences belong together under the mappings a filter call kept -- the links between
sequence pairs with their summed bases, the connected components over the links heavy enough to join, and each sequence's
component -- computed on the device (csrc/swg_components.hip).  components_records / components_records_device are the two
record seams, Components.from_paf the report of an open PafFile."""
import ctypes as C

import numpy as np

from ._lib import SwgComponent, SwgComponentParams, SwgComponentTable, SwgLink, load
from ._marshal import addr, host_column, raise_alnstats, records_from_numpy, records_from_tensors, take_texts

# swg_link and swg_component as numpy records
LINK_DTYPE = np.dtype([(k, "<u4") for k in ("a", "b", "n_records", "joined")] + [(k, "<u8") for k in ("a_bases", "b_bases", "first_record")])
COMPONENT_DTYPE = np.dtype([(k, "<u4") for k in ("id", "first_seq", "n_seq", "n_links")] + [(k, "<u8") for k in ("length", "n_records", "bases")])
assert LINK_DTYPE.itemsize == C.sizeof(SwgLink) and COMPONENT_DTYPE.itemsize == C.sizeof(SwgComponent)
COLUMNS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")


def params(min_bases=0, min_share=0.0):
    """swg_component_params from a number of bases and a share in [0, 1] (parts per million, rounded half away from zero as the
    command line does)."""
    if not 0.0 <= min_share <= 1.0:
        raise ValueError("min_share must lie in [0, 1]")
    return SwgComponentParams(int(min_bases), int(np.floor(min_share * 1e6 + 0.5)), 0)


class Components:
    """One call's result: `components` (COMPONENT_DTYPE, ascending id), `links` (LINK_DTYPE, ascending (a, b)), `seq_component`
    (uint32 [n_seq]), `cross` (links, records, bases between components) and, from from_paf, `text` (the report, bytes)."""

    def __init__(self, components, links, seq_component, cross, text=None):
        self.components, self.links, self.seq_component, self.cross, self.text = components, links, seq_component, cross, text

    @classmethod
    def from_paf(cls, ctx_or_filter, paf, status=None, min_bases=0, min_share=0.0, detailed=False):
        """swg_paf_components for the text, swg_components_records over the handle's columns for the arrays (seq_len: the lengths
        of the text's `length` column).  ctx_or_filter: a Context, or anything with a `.ctx` (PafFilter); may be None for a PAF
        without records.  The device work is done twice, once for the text and once for the arrays: a convenience for tests and
        notebooks."""
        ctx = getattr(ctx_or_filter, "ctx", ctx_or_filter)
        lib = load()
        st = host_column(status, np.uint8, paf.n, "status", optional=True)
        par = params(min_bases, min_share)
        p, n = C.c_void_p(), C.c_uint64()
        rc = lib.swg_paf_components(ctx.handle if ctx is not None else None, paf.handle, addr(st), C.byref(par), 1 if detailed else 0,
                                    C.byref(p), C.byref(n))
        raise_alnstats(lib, rc)
        text, = take_texts(lib, [p], [n], [True])
        if paf.n == 0:
            return cls(np.zeros(0, dtype=COMPONENT_DTYPE), np.zeros(0, dtype=LINK_DTYPE), np.zeros(0, dtype=np.uint32), (0, 0, 0), text)
        rows = text.split(b"\n")[1:1 + int(paf.records.n_seq)]
        seq_len = np.array([int(r.split(b"\t")[1]) for r in rows], dtype=np.uint32)
        r = components_records(ctx, paf.records, seq_len, st, par)
        r.text = text
        return r


def _call(ctx, fn, rec, seq_len_addr, status_addr, par):
    """One call, repeated with larger arrays when the first were too small (the capacity protocol of the C seam)."""
    n_seq = int(rec.n_seq)
    cap_c, cap_l = max(1, n_seq), max(1, min(int(rec.n), 1 << 16))
    par = par if par is not None else SwgComponentParams(0, 0, 0)
    while True:
        t = SwgComponentTable()
        comps, links = np.zeros(cap_c, dtype=COMPONENT_DTYPE), np.zeros(cap_l, dtype=LINK_DTYPE)
        seq = np.zeros(max(1, n_seq), dtype=np.uint32)
        t.component_capacity, t.components = cap_c, C.cast(comps.ctypes.data, C.POINTER(SwgComponent))
        t.link_capacity, t.links = cap_l, C.cast(links.ctypes.data, C.POINTER(SwgLink))
        t.seq_component = C.cast(seq.ctypes.data, C.POINTER(C.c_uint32))
        ctx.check(fn(ctx.handle, C.byref(rec), seq_len_addr, status_addr, C.byref(par), C.byref(t)))
        if int(t.n_components) <= cap_c and int(t.n_links) <= cap_l:
            return Components(comps[:int(t.n_components)].copy(), links[:int(t.n_links)].copy(), seq[:n_seq].copy(),
                              (int(t.cross_links), int(t.cross_records), int(t.cross_bases)))
        cap_c, cap_l = max(cap_c, int(t.n_components)), max(cap_l, int(t.n_links))


def components_records(ctx, records, seq_len, status=None, par=None):
    """swg_components_records.  `records`: an SwgRecords with host pointers, or a dict of numpy columns (q_id, t_id, q_start,
    q_end, t_start, t_end).  seq_len: uint32 [n_seq], which also gives n_seq for a dict; status: uint8 [n] as a filter call
    wrote it, or None (every record takes part); par: SwgComponentParams (see params()) or None for 0, 0."""
    seq_len = np.ascontiguousarray(seq_len, dtype=np.uint32)
    rec, keep = records_from_numpy(records, COLUMNS, seq_len.size)   # (keep: alive until the call is over)
    if seq_len.size < int(rec.n_seq):
        raise ValueError("seq_len has fewer entries than sequences")
    st = host_column(status, np.uint8, int(rec.n), "status", optional=True)
    sl = seq_len if seq_len.size else np.zeros(1, dtype=np.uint32)
    return _call(ctx, ctx.lib.swg_components_records, rec, sl.ctypes.data, addr(st), par)


def components_records_device(ctx, columns, seq_len, status=None, par=None):
    """swg_components_records_device over torch tensors on ctx's GPU: `columns` maps q_id, t_id, q_start, q_end, t_start, t_end
    to contiguous int32 / uint32 tensors of one length, seq_len is a 4-byte tensor of n_seq entries, status a uint8 tensor or
    None.  (Anything with .data_ptr() and .numel() works; the caller keeps the tensors alive and their work finished.)"""
    rec = records_from_tensors(columns, {k: 4 for k in COLUMNS}, seq_len.numel())
    if seq_len.element_size() != 4 or not seq_len.is_contiguous():
        raise ValueError("seq_len must be a contiguous 4-byte tensor")
    if status is not None and (status.element_size() != 1 or int(status.numel()) < int(rec.n)):
        raise ValueError("status must be 1-byte with an entry per record")
    return _call(ctx, ctx.lib.swg_components_records_device, rec, int(seq_len.data_ptr()), int(status.data_ptr()) if status is not None else None, par)
