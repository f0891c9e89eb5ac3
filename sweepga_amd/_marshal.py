"""What every report module does on its way into and out of the C seams, once: host columns checked and made contiguous,
SwgRecords filled from numpy columns or from device tensors, the texts of a swg_paf_* call fetched and released, and its error
raised from swg_alnstats_last_error()."""
import ctypes as C

import numpy as np

from ._lib import SWG_OK, SwgError, SwgRecords

_MARKER = C.create_string_buffer(1)   # a text is asked for by a non-NULL entry; the library never reads through it


def host_column(a, dtype, n, what, optional=False):
    """`a` as a contiguous array of dtype with an entry per record (a 1-element placeholder for an empty one, so that its address
    is a real one); None stays None when optional."""
    if a is None and optional:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.size < n:
        raise ValueError(f"{what} has fewer entries than records")
    return a if a.size else np.zeros(1, dtype=dtype)


def addr(a):
    """The address of a host array for the C call, None for None."""
    return a.ctypes.data if a is not None else None


def records_from_numpy(records, columns, n_seq, strand=None, optional=()):
    """(SwgRecords, keep).  An SwgRecords passes through with an empty keep.  A dict of numpy columns is converted: every name of
    `columns` -- and of `optional`, where the dict has it -- as contiguous uint32 ("strand" as uint8); `strand` is a uint8
    array given apart from the dict.  An empty column becomes NULL.  n_seq None = the largest id + 1 (1 without records).  `keep`
    holds the converted arrays the struct points into: the caller holds it until after the C call."""
    if not isinstance(records, dict):
        return records, []
    rec, keep = SwgRecords(), []
    rec.n = len(records["q_id"])
    for k in tuple(columns) + tuple(k for k in optional if k in records):
        a = np.ascontiguousarray(records[k], dtype=np.uint8 if k == "strand" else np.uint32)
        keep.append(a)
        setattr(rec, k, a.ctypes.data if a.size else None)
    if strand is not None:
        s = np.ascontiguousarray(strand, dtype=np.uint8)
        keep.append(s)
        rec.strand = s.ctypes.data if s.size else None
    if n_seq is None:
        n_seq = int(max(keep[0].max(), keep[1].max())) + 1 if rec.n else 1
    rec.n_seq = int(n_seq)
    return rec, keep


def records_from_tensors(columns, sizes, n_seq):
    """SwgRecords over device tensors (anything with data_ptr / numel / element_size / is_contiguous): every name of `sizes`, which
    maps it to its element size, must be a contiguous tensor of that size with as many entries as q_id."""
    rec = SwgRecords()
    rec.n = int(columns["q_id"].numel())
    for k, size in sizes.items():
        t = columns[k]
        if int(t.numel()) != int(rec.n) or t.element_size() != size or not t.is_contiguous():
            raise ValueError(f"column {k}: a contiguous {size}-byte tensor of {int(rec.n)} entries is needed")
        setattr(rec, k, int(t.data_ptr()))
    rec.n_seq = int(n_seq)
    return rec


def text_slots(wanted):
    """(text pointers, lengths) for a swg_paf_* call that hands out len(wanted) texts: a non-NULL entry asks for the text."""
    p, n = (C.c_void_p * len(wanted))(), (C.c_uint64 * len(wanted))()
    for k, w in enumerate(wanted):
        p[k] = C.addressof(_MARKER) if w else None
    return p, n


def take_texts(lib, ptrs, lens, wanted):
    """The wanted texts of a swg_paf_* call as bytes (None for the others), each released with swg_free."""
    out = []
    for p, n, w in zip(ptrs, lens, wanted):
        if not w:
            out.append(None)
            continue
        p, n = getattr(p, "value", p), getattr(n, "value", n)
        out.append(C.string_at(p, n))
        lib.swg_free(C.c_void_p(p))
    return out


def raise_alnstats(lib, rc):
    """SwgError with the text of swg_alnstats_last_error() unless rc is SWG_OK."""
    if rc != SWG_OK:
        raise SwgError(rc, (lib.swg_alnstats_last_error() or b"").decode(errors="replace"))
