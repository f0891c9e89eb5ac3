"""alnstats (src/bin/alnstats.rs) seen from Python: AlignmentStats of a PAF, print_stats / compare_stats text.
AlnStats(path / text) is host code of libsweepga_gpu.so (no GPU needed); AlnStats.from_paf and alnstats_counts compute the
same statistics on the device from record columns, before and after a filter call at once."""
import ctypes as C
import os

import numpy as np

from ._lib import SwgAlnstatsCounts, SwgAlnstatsPairCounts, load
from ._marshal import addr, host_column, raise_alnstats, take_texts


# swg_alnstats_pair_counts as a numpy record
PAIR_DTYPE = np.dtype([("q_genome", "<u4"), ("t_genome", "<u4"), ("bases", "<u8"), ("matches", "<u8"), ("first_record", "<u8")])


def genome_last(name):
    """alnstats' genome of a sequence name (:94-100): up to and including the last '#', the whole name without one."""
    p = name.rfind("#")
    return name if p < 0 else name[:p + 1]


def genome_map(names):
    """(seq_genome uint32 [len(names)], genome names in order of first appearance) under genome_last."""
    ids, out = {}, np.zeros(max(len(names), 1), dtype=np.uint32)
    for i, nm in enumerate(names):
        out[i] = ids.setdefault(genome_last(nm), len(ids))
    return out, list(ids)


def alnstats_counts(ctx, records, seq_genome, n_genome, status=None, device=False, pair_capacity=None):
    """swg_alnstats_records / swg_alnstats_records_device: the integer statistics of `records` (an SwgRecords whose q_id,
    t_id, q_start, q_end and matches columns are set; host pointers, or device pointers with device=True) under the map
    seq_genome (numpy array on the host, or a device address with device=True).  Returns (all, kept) dictionaries -- kept is
    None without status -- with the scalar counts, `pairs` (numpy records of PAIR_DTYPE in order of first appearance; None when
    pair_capacity was too small, `n_pairs` then says how many there are) and `seq_last` (uint64 [n_seq], 2 * record + side,
    2^64 - 1 = absent)."""
    lib = ctx.lib
    n, n_seq = int(records.n), int(records.n_seq)
    cap = int(pair_capacity) if pair_capacity is not None else max(1, min(n, int(n_genome) ** 2))
    fn = lib.swg_alnstats_records_device if device else lib.swg_alnstats_records
    keep = []

    def addr(a, dtype):
        if a is None:
            return None
        if device:
            return int(a)
        a = np.ascontiguousarray(a, dtype=dtype)
        keep.append(a)
        return a.ctypes.data

    sets = []
    for _ in range(2 if status is not None else 1):
        c = SwgAlnstatsCounts()
        pairs = np.zeros(cap, dtype=PAIR_DTYPE)
        last = np.zeros(max(n_seq, 1), dtype=np.uint64)
        c.pair_capacity = cap
        c.pairs = C.cast(pairs.ctypes.data, C.POINTER(SwgAlnstatsPairCounts))
        c.seq_last = last.ctypes.data_as(C.POINTER(C.c_uint64))
        sets.append((c, pairs, last))
    ctx.check(fn(ctx.handle, C.byref(records), addr(seq_genome, np.uint32), C.c_uint32(int(n_genome)), addr(status, np.uint8),
                 C.byref(sets[0][0]), C.byref(sets[1][0]) if status is not None else None))
    out = []
    for c, pairs, last in sets:
        d = {k: int(getattr(c, k)) for k in ("total_mappings", "total_bases", "total_matches", "self_mappings", "inter_chromosomal",
                                             "inter_genome", "chr_pair_count", "n_pairs")}
        d["pairs"] = pairs[:d["n_pairs"]] if d["n_pairs"] <= cap else None
        d["seq_last"] = last[:n_seq]
        out.append(d)
    return out[0], (out[1] if status is not None else None)


class SwgAlnstatsSummary(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("total_mappings", "total_bases", "total_matches", "self_mappings", "inter_chromosomal",
                                           "inter_genome", "chr_pair_count", "genome_pairs", "above_95_pct")] + \
               [("avg_identity", C.c_double), ("avg_coverage", C.c_double)]


class AlnStats:
    """parse_paf (:103-164) over a file (plain / .gz / .bgz) or over text in memory."""

    def __init__(self, path=None, text=None, threads=0, _handle=None):
        self.lib = lib = load()
        lib.swg_alnstats_open.restype = C.c_int
        lib.swg_alnstats_open.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        lib.swg_alnstats_open_buffer.restype = C.c_int
        lib.swg_alnstats_open_buffer.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]
        lib.swg_alnstats_close.restype = None
        lib.swg_alnstats_close.argtypes = [C.c_void_p]
        lib.swg_alnstats_get.restype = C.POINTER(SwgAlnstatsSummary)
        lib.swg_alnstats_get.argtypes = [C.c_void_p]
        lib.swg_alnstats_pair.restype = C.c_int
        lib.swg_alnstats_pair.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_double),
                                          C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        lib.swg_alnstats_report.restype = C.c_int
        lib.swg_alnstats_report.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        lib.swg_alnstats_compare.restype = C.c_int
        lib.swg_alnstats_compare.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        lib.swg_alnstats_last_error.restype = C.c_char_p
        lib.swg_free.restype = None
        lib.swg_free.argtypes = [C.c_void_p]
        if _handle is not None:  # a handle the library made (from_paf)
            self.handle = _handle
            self.summary = lib.swg_alnstats_get(_handle).contents
            return
        h = C.c_void_p()
        if text is not None:
            data = text if isinstance(text, bytes) else text.encode("utf-8", errors="surrogateescape")
            rc = lib.swg_alnstats_open_buffer(data, len(data), threads, C.byref(h))
        else:
            rc = lib.swg_alnstats_open(os.fsencode(path), threads, C.byref(h))
        raise_alnstats(lib, rc)
        self.handle = h
        self.summary = lib.swg_alnstats_get(h).contents

    @classmethod
    def from_paf(cls, ctx_or_filter, paf, status=None):
        """swg_paf_alnstats: the statistics of an open PafFile computed on the device -> (all, kept).  `all` is what
        AlnStats(path) gives for the file; with `status` (the filter's per-record result) `kept` is what it gives for the
        file PafFile.write(..., status) writes, else None.  ctx_or_filter: a Context, or anything with a `.ctx` (PafFilter)."""
        ctx = getattr(ctx_or_filter, "ctx", ctx_or_filter)
        lib = load()
        st = host_column(status, np.uint8, paf.n, "status", optional=True)
        a, k = C.c_void_p(), C.c_void_p()
        rc = lib.swg_paf_alnstats(ctx.handle if ctx is not None else None, paf.handle, addr(st), C.byref(a), C.byref(k) if st is not None else None)
        raise_alnstats(lib, rc)
        return cls(_handle=a), (cls(_handle=k) if st is not None else None)

    @property
    def pairs(self):
        """[(query genome, target genome, coverage %, bases, matches)] in order of first appearance."""
        out = []
        for i in range(int(self.summary.genome_pairs)):
            q, t, c, b, m = C.c_char_p(), C.c_char_p(), C.c_double(), C.c_uint64(), C.c_uint64()
            self.lib.swg_alnstats_pair(self.handle, i, C.byref(q), C.byref(t), C.byref(c), C.byref(b), C.byref(m))
            out.append((q.value.decode(errors="surrogateescape"), t.value.decode(errors="surrogateescape"), c.value, b.value, m.value))
        return out

    def _text(self, rc, p, n):
        raise_alnstats(self.lib, rc)
        return take_texts(self.lib, [p], [n], [True])[0]

    def report(self, label, detailed=False):
        """print_stats (:166-228) as bytes."""
        p, n = C.c_void_p(), C.c_uint64()
        return self._text(self.lib.swg_alnstats_report(self.handle, os.fsencode(label), int(detailed), C.byref(p), C.byref(n)), p, n)

    def compare(self, other, file1, file2):
        """compare_stats (:230-284) as bytes."""
        p, n = C.c_void_p(), C.c_uint64()
        return self._text(self.lib.swg_alnstats_compare(self.handle, other.handle, os.fsencode(file1), os.fsencode(file2), C.byref(p),
                                                        C.byref(n)), p, n)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.swg_alnstats_close(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
