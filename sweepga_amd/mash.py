"""`--joblist` seen from Python: FASTA records, MinHash sketches (src/mash.rs), Mash distances, haplotype pair selection
(src/knn_graph.rs) and the wfmash job list (src/joblist.rs).  Sketches, distances and random pairs run on the GPU;
the FASTA reader, the haplotype merge and the kNN ranking are host code of libsweepga_gpu.so."""
import ctypes as C
import os

import numpy as np

from ._lib import SWG_OK, SwgError, load

_P = C.c_void_p
_U64 = C.c_uint64


def _bind():
    lib = load()
    if getattr(lib, "_mash_bound", False):
        return lib
    sig = {
        "swg_fasta_open": (C.c_int, [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.POINTER(_P)]),
        "swg_fasta_close": (None, [_P]),
        "swg_fasta_num_records": (_U64, [_P]),
        "swg_fasta_name": (C.c_char_p, [_P, _U64]),
        "swg_fasta_file_index": (C.c_int, [_P, _U64]),
        "swg_fasta_offsets": (_P, [_P]),
        "swg_fasta_bases": (_P, [_P]),
        "swg_fasta_last_error": (C.c_char_p, []),
        "swg_mash_sketch": (C.c_int, [_P, _P, _P, _U64, C.c_int, _U64, _P, _P, _P]),
        "swg_mash_merge": (C.c_int, [_P, _P, _U64, _P, _U64, _U64, _P, C.POINTER(_U64)]),
        "swg_mash_distances": (C.c_int, [_P, _P, _P, _U64, _U64, C.c_int, _P, _P, _P]),
        "swg_mash_random_pairs": (C.c_int, [_P, _U64, C.c_double, _U64, _U64, _P]),
        "swg_select_pairs": (C.c_int, [_P, C.c_char_p, _P, _U64, C.POINTER(_P), C.POINTER(_U64)]),
        "swg_joblist": (C.c_int, [_P, C.POINTER(C.c_char_p), C.c_int, C.c_char_p, C.c_int, _U64, _U64, _U64, C.c_char_p, C.c_int,
                                  C.POINTER(_P), C.POINTER(_U64), _P]),
        "swg_free": (None, [_P]),
        "swg_last_error": (C.c_char_p, [_P]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    lib._mash_bound = True
    return lib


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _ctx_handle(ctx):
    return ctx.handle if ctx is not None else None


def _raise(lib, rc, ctx):
    if rc != SWG_OK:
        raise SwgError(rc, (lib.swg_last_error(_ctx_handle(ctx)) or b"").decode(errors="replace"))


def _paths(paths):
    if isinstance(paths, (str, bytes, os.PathLike)):
        paths = [paths]
    enc = [os.fsencode(p) for p in paths]
    return (C.c_char_p * len(enc))(*enc), len(enc)


class Fasta:
    """Records of one or more FASTA files (plain / .gz / .bgz), read as src/main.rs:791-830 and :963-990 read them."""

    def __init__(self, paths, threads=0):
        lib = _bind()
        arr, n = _paths(paths)
        h = _P()
        rc = lib.swg_fasta_open(arr, n, threads, C.byref(h))
        if rc != SWG_OK:
            raise SwgError(rc, (lib.swg_fasta_last_error() or b"").decode(errors="replace"))
        try:
            n_rec = int(lib.swg_fasta_num_records(h))
            self.names = [lib.swg_fasta_name(h, i).decode(errors="surrogateescape") for i in range(n_rec)]
            self.file_index = np.array([lib.swg_fasta_file_index(h, i) for i in range(n_rec)], dtype=np.int32)
            self.offsets = np.ctypeslib.as_array(C.cast(lib.swg_fasta_offsets(h), C.POINTER(C.c_uint64)), shape=(n_rec + 1,)).copy()
            total = int(self.offsets[-1])
            bp = lib.swg_fasta_bases(h)
            self.bases = (np.ctypeslib.as_array(C.cast(bp, C.POINTER(C.c_uint8)), shape=(total,)).copy() if total
                          else np.zeros(0, dtype=np.uint8))
        finally:
            lib.swg_fasta_close(h)

    def __len__(self):
        return len(self.names)

    def sequence(self, i):
        return self.bases[self.offsets[i]:self.offsets[i + 1]].tobytes()


def _concat(seqs):
    seqs = [s if isinstance(s, bytes) else bytes(s) for s in seqs]
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64) if seqs else []
    bases = np.frombuffer(b"".join(seqs), dtype=np.uint8) if seqs else np.zeros(0, dtype=np.uint8)
    return np.ascontiguousarray(bases), offsets


def sketch(ctx, seqs=None, k=15, s=1000, bases=None, offsets=None, timing=False):
    """KmerSketch::from_sequence for every sequence (list of bytes, or bases + offsets as Fasta holds them): a list of
    ascending uint64 arrays, duplicates kept.  timing=True also returns {wall, h2d, hash, select (ms), kmers}."""
    lib = _bind()
    if bases is None:
        bases, offsets = _concat(seqs)
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    counts = np.zeros(max(n, 1), dtype=np.uint64)
    mins = np.zeros(max(n * s, 1), dtype=np.uint64) if 1 <= s <= 65536 else np.zeros(1, dtype=np.uint64)
    tm = np.zeros(5, dtype=np.float64)
    rc = lib.swg_mash_sketch(_ctx_handle(ctx), _ptr(bases) if len(bases) else None, _ptr(offsets), n, int(k), int(s), _ptr(counts),
                             _ptr(mins), _ptr(tm) if timing else None)
    _raise(lib, rc, ctx)
    out = [mins[i * s:i * s + int(counts[i])].copy() for i in range(n)]
    if timing:
        return out, dict(wall_ms=tm[0], h2d_ms=tm[1], hash_ms=tm[2], select_ms=tm[3], kmers=int(tm[4]))
    return out


def _table(sketches):
    stride = max([len(x) for x in sketches] + [1])
    flat = np.zeros(len(sketches) * stride, dtype=np.uint64)
    counts = np.zeros(max(len(sketches), 1), dtype=np.uint64)
    for i, x in enumerate(sketches):
        flat[i * stride:i * stride + len(x)] = x
        counts[i] = len(x)
    return flat, counts, stride


def merge(sketches, s):
    """merge_sketches (knn_graph.rs:568-582): concatenated, sorted, deduplicated, truncated to s."""
    lib = _bind()
    flat, counts, stride = _table(sketches)
    members = np.arange(len(sketches), dtype=np.uint64)
    out = np.zeros(max(s, 1), dtype=np.uint64)
    n_out = _U64()
    rc = lib.swg_mash_merge(_ptr(flat), _ptr(counts), stride, _ptr(members) if len(members) else None, len(sketches), s, _ptr(out),
                            C.byref(n_out))
    if rc != SWG_OK:
        raise SwgError(rc, "swg_mash_merge")
    return out[:n_out.value].copy()


def distances(ctx, sketches, k, counts_too=False):
    """All-vs-all Mash distance (mash.rs:39-73) over sketches taken as sets: n x n float64 (plus intersection / union)."""
    lib = _bind()
    n = len(sketches)
    flat, counts, stride = _table(sketches)
    dist = np.zeros((n, n), dtype=np.float64)
    inter = np.zeros((n, n), dtype=np.uint32) if counts_too else None
    union = np.zeros((n, n), dtype=np.uint32) if counts_too else None
    rc = lib.swg_mash_distances(_ctx_handle(ctx), _ptr(flat), _ptr(counts), stride, n, int(k),
                                _ptr(dist), _ptr(inter), _ptr(union))
    _raise(lib, rc, ctx)
    return (dist, inter, union) if counts_too else dist


def random_pairs_mask(ctx, n, fraction, row_begin=0, row_end=None):
    """generate_random_pairs (knn_graph.rs:362-386) as bits: [rows, ceil(n / 64)] uint64, bit j of row i set when selected."""
    lib = _bind()
    row_end = n if row_end is None else row_end
    wpr = (n + 63) // 64
    mask = np.zeros((max(row_end - row_begin, 0), wpr), dtype=np.uint64)
    rc = lib.swg_mash_random_pairs(_ctx_handle(ctx), n, float(fraction), row_begin, row_end, _ptr(mask) if mask.size else None)
    _raise(lib, rc, ctx)
    return mask


def select_pairs(ctx, strategy, dist=None, n=None):
    """Selected (i, j) pairs (i < j, sorted) for a --sparsify string over a distance matrix (or n items without one)."""
    lib = _bind()
    if dist is not None:
        dist = np.ascontiguousarray(dist, dtype=np.float64)
        n = dist.shape[0]
    p = _P()
    cnt = _U64()
    rc = lib.swg_select_pairs(_ctx_handle(ctx), strategy.encode(), _ptr(dist), int(n), C.byref(p), C.byref(cnt))
    _raise(lib, rc, ctx)
    try:
        m = int(cnt.value)
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(2 * m,)).copy() if m else np.zeros(0, dtype=np.uint64)
    finally:
        lib.swg_free(p)
    return [(int(arr[2 * i]), int(arr[2 * i + 1])) for i in range(m)]


def joblist(ctx, paths, strategy="none", k=15, s=1000, threads=8, min_aln_length=0, output_dir=".", io_threads=0, timing=False):
    """`sweepga --joblist` text (one wfmash command per line).  timing=True also returns {read, sketch, merge, distances,
    select, total} in ms."""
    lib = _bind()
    arr, n = _paths(paths)
    p = _P()
    ln = _U64()
    tm = np.zeros(6, dtype=np.float64)
    rc = lib.swg_joblist(_ctx_handle(ctx), arr, n, strategy.encode(), int(k), int(s), int(threads), int(min_aln_length),
                         os.fsencode(output_dir) if output_dir is not None else None, io_threads, C.byref(p), C.byref(ln),
                         _ptr(tm) if timing else None)
    _raise(lib, rc, ctx)
    try:
        text = C.string_at(p, ln.value).decode(errors="surrogateescape")
    finally:
        lib.swg_free(p)
    if timing:
        return text, dict(zip(("read_ms", "sketch_ms", "merge_ms", "distances_ms", "select_ms", "total_ms"), tm.tolist()))
    return text
