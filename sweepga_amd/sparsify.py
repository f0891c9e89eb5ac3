"""Tree sparsification (--sparsify tree:/knn:, src/tree_filter.rs) on records: thin ctypes mirror of the swg_tree_select_* and
swg_filter_subset* entries of include/sweepga_gpu.h.  The per-pair sums and the mask are device work, the selection of the
pairs is host code shared with the text tool (swg_paf_tree_filter)."""
import ctypes as C

import numpy as np

from ._lib import SWG_OK, SwgError, SwgStats, load

ROUTE_DEVICE, ROUTE_TEXT = 0, 1


def genome_two(name):
    """extract_genome_prefix (src/tree_filter.rs:15-24): the first two '#' parts + '#', the whole name without a '#'."""
    parts = name.split("#")
    return f"{parts[0]}#{parts[1]}#" if len(parts) >= 2 else name


def genome_map(names):
    """(seq_genome uint32 [len(names)], prefixes in order of first appearance) under genome_two."""
    ids, out = {}, np.zeros(max(len(names), 1), dtype=np.uint32)
    for i, nm in enumerate(names):
        out[i] = ids.setdefault(genome_two(nm), len(ids))
    return out, list(ids)


def _strings(prefixes):
    raw = [p if isinstance(p, bytes) else p.encode("utf-8", errors="surrogateescape") for p in prefixes]
    return (C.c_char_p * max(len(raw), 1))(*raw)


def select_pairs(prefixes, pair_a, pair_b, sum_matches, sum_block_len, k_nearest, k_farthest=0, random_fraction=0.0):
    """swg_tree_select_pairs (host code): uint8 [n_pairs], 1 = the pair survives."""
    lib = load()
    a = np.ascontiguousarray(pair_a, dtype=np.uint32)
    b = np.ascontiguousarray(pair_b, dtype=np.uint32)
    m = np.ascontiguousarray(sum_matches, dtype=np.uint64)
    l = np.ascontiguousarray(sum_block_len, dtype=np.uint64)
    sel = np.zeros(max(len(a), 1), dtype=np.uint8)
    rc = lib.swg_tree_select_pairs(len(prefixes), _strings(prefixes), len(a), a.ctypes.data, b.ctypes.data, m.ctypes.data, l.ctypes.data,
                                   int(k_nearest), int(k_farthest), float(random_fraction), sel.ctypes.data)
    if rc != SWG_OK:
        raise SwgError(rc, "swg_tree_select_pairs")
    return sel[:len(a)]


def tree_select(ctx, records, seq_genome, prefixes, k_nearest, k_farthest=0, random_fraction=0.0, device=False, keep=None):
    """swg_tree_select_records / _device: the keep flag of every record of `records` (an SwgRecords with q_id, t_id, matches and
    block_len set) under the map seq_genome -> genome id, whose prefixes are `prefixes`.  Host: seq_genome is a numpy array and
    the mask comes back as one.  device=True: seq_genome and `keep` are device addresses, the mask is written there.  Returns
    (keep, n_kept)."""
    n = int(records.n)
    fn = ctx.lib.swg_tree_select_records_device if device else ctx.lib.swg_tree_select_records
    if device:
        g_addr, k_addr, out = int(seq_genome), int(keep), keep
    else:
        g = np.ascontiguousarray(seq_genome, dtype=np.uint32)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        g_addr, k_addr = g.ctypes.data, out.ctypes.data
    n_kept = C.c_uint64()
    ctx.check(fn(ctx.handle, C.byref(records), g_addr, len(prefixes), _strings(prefixes), int(k_nearest), int(k_farthest),
                 float(random_fraction), k_addr, C.byref(n_kept)))
    return (out if device else out[:n]), n_kept.value


def paf_tree_select(ctx, paf_handle, k_nearest, k_farthest=0, random_fraction=0.0, threads=0):
    """swg_paf_tree_select on an open swg_paf handle (a c_void_p): (keep uint8 [n], n_kept, route)."""
    lib = load()
    n = int(lib.swg_paf_records(paf_handle).contents.n)
    keep = np.zeros(max(n, 1), dtype=np.uint8)
    n_kept, route = C.c_uint64(), C.c_int()
    rc = lib.swg_paf_tree_select(ctx.handle if ctx is not None else None, paf_handle, int(k_nearest), int(k_farthest),
                                 float(random_fraction), int(threads), keep.ctypes.data, C.byref(n_kept), C.byref(route))
    if rc != SWG_OK:
        raise SwgError(rc, (lib.swg_last_error(ctx.handle) or b"").decode() if ctx is not None else "swg_paf_tree_select")
    return keep[:n], n_kept.value, route.value


def aln_tree_select(ctx, aln_handle, k_nearest, k_farthest=0, random_fraction=0.0):
    """swg_aln_tree_select on a .1aln record handle (swg_aln_open): (keep uint8 [n], n_kept)."""
    lib = load()
    n = int(lib.swg_aln_records(aln_handle).contents.n)
    keep = np.zeros(max(n, 1), dtype=np.uint8)
    n_kept = C.c_uint64()
    ctx.check(lib.swg_aln_tree_select(ctx.handle, aln_handle, int(k_nearest), int(k_farthest), float(random_fraction), keep.ctypes.data,
                                      C.byref(n_kept)))
    return keep[:n], n_kept.value


def handle_prefixes(handle, aln=False):
    """The two-part-prefix genome table of a swg_paf (or, aln=True, swg_aln) handle: prefixes by genome id."""
    lib = load()
    count, get = (lib.swg_aln_num_genomes_two, lib.swg_aln_genome_two_prefix) if aln else (lib.swg_paf_num_genomes_two, lib.swg_paf_genome_two_prefix)
    return [get(handle, g).decode("utf-8", errors="surrogateescape") for g in range(count(handle))]


def filter_subset(ctx, records, keep, cfg, device=False, status=None, chain=None):
    """swg_filter_subset / swg_filter_subset_device: the filter on the records with keep != 0, answered for every record (dropped
    ones: 0 / 0).  Host: keep is a numpy array (or None = every record); returns (status uint8 [n], chain uint32 [n], SwgStats).
    device=True: keep, status and chain are device addresses."""
    n = int(records.n)
    st = SwgStats()
    if device:
        ctx.check(ctx.lib.swg_filter_subset_device(ctx.handle, C.byref(records), None if keep is None else int(keep), C.byref(cfg),
                                                   int(status), int(chain), C.byref(st)))
        return status, chain, st
    k = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    s = np.full(max(n, 1), 0xff, dtype=np.uint8)
    c = np.full(max(n, 1), 0xffffffff, dtype=np.uint32)
    ctx.check(ctx.lib.swg_filter_subset(ctx.handle, C.byref(records), None if k is None else k.ctypes.data, C.byref(cfg), s.ctypes.data,
                                        c.ctypes.data, C.byref(st)))
    return s[:n], c[:n], st
