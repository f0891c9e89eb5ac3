"""Differences from the CIGARs, on the device (csrc/swg_diffs.hip; include/sweepga_gpu.h states the
definitions): every mismatch run, insertion and deletion inside the mappings.  diff_records / diff_records_device are the record
seams: a CIGAR set in, ROW_DTYPE rows, PAIR_DTYPE sums per genome pair and a [4][33] length spectrum out.  Diffs.from_paf is
swg_paf_diffs_text: the two texts of an open PafFile."""
import ctypes as C

import numpy as np

from ._lib import DIFF_SUMS, SwgCigarSet, SwgDiffCounts, SwgDiffRequest, default_context, load
from ._marshal import addr, host_column, raise_alnstats, records_from_numpy, records_from_tensors
from .lift import COLUMNS, SETS, cigar_set

SNP, INS, DEL, SKIP = 1, 2, 4, 8
MINUS = 256
BINS = 33
KINDS = {"snp": SNP, "ins": INS, "del": DEL, "skip": SKIP}
KIND_NAMES = {SNP: "SNP", INS: "INS", DEL: "DEL", SKIP: "SKIP"}
ROW_DTYPE = np.dtype([(k, "<u4") for k in ("record", "kind_flags", "t_start", "t_end", "q_start", "q_end", "left", "right")])
PAIR_DTYPE = np.dtype([("q_genome", "<u4"), ("t_genome", "<u4")] + [(k, "<u8") for k in DIFF_SUMS])
COUNTS = ("records", "usable", "bad", "untagged", "rows", "snp_runs", "snp_bases", "n_ins", "ins_bases", "n_del", "del_bases", "n_skip", "skip_bases",
          "m_columns", "batches")


def kinds_mask(kinds):
    """An int as it is; a name or an iterable of names (snp ins del skip) as the OR of their bits."""
    if isinstance(kinds, (int, np.integer)):
        return int(kinds)
    if isinstance(kinds, str):
        kinds = [k for k in kinds.split(",") if k]
    mask = 0
    for k in kinds:
        if k not in KINDS:
            raise ValueError(f"unknown kind {k!r}: snp, ins, del or skip")
        mask |= KINDS[k]
    return mask


class DiffsResult:
    """rows: a ROW_DTYPE array, pairs: a PAIR_DTYPE array -- each None when the capacity given did not hold it; spectrum: uint64
    [4][33] (SNP, INS, DEL, SKIP by the bit length of the op); state: a uint8 per entry; the counts as the request returns them."""

    def __init__(self, rows, pairs, spectrum, state, req):
        self.rows, self.pairs, self.spectrum, self.state = rows, pairs, spectrum, state
        for k in ("n_rows", "n_pairs", "ops", "cigar_bad", "usable"):
            setattr(self, k, int(getattr(req, k)))


def _call(ctx, fn, rec, genome_addr, n_genome, status_addr, cigars, k, set_, kinds, min_indel, capacity):
    """cigars: (record address, offset address, text address) or None.  capacity: None = two calls, the second with arrays of the
    sizes the first one reported; or (rows, pairs), each an int or None for a NULL array."""
    req = SwgDiffRequest()
    req.set, req.kinds, req.min_indel = int(set_), int(kinds), int(min_indel)
    state = np.zeros(int(k), dtype=np.uint8)
    spectrum = np.zeros((4, BINS), dtype=np.uint64)
    req.state = state.ctypes.data if k else None
    req.spectrum = spectrum.ctypes.data
    cs = None
    if cigars is not None:
        cs = SwgCigarSet()
        cs.record, cs.offset, cs.text, cs.k = cigars[0], cigars[1], cigars[2], int(k)
    call = lambda: ctx.check(fn(ctx.handle, C.byref(rec), genome_addr, int(n_genome), status_addr, C.byref(cs) if cs is not None else None, C.byref(req)))   # noqa: E731
    if capacity is None:
        call()
        capacity = (int(req.n_rows), int(req.n_pairs))
    arrays = [None if c is None else np.zeros(max(int(c), 1), dtype=dt) for c, dt in zip(capacity, (ROW_DTYPE, PAIR_DTYPE))]
    req.row_capacity, req.pair_capacity = (0 if c is None else int(c) for c in capacity)
    req.rows, req.pairs = (addr(a) for a in arrays)
    call()
    counts = (int(req.n_rows), int(req.n_pairs))
    out = [a[:n] if a is not None and n <= int(c) else None for a, c, n in zip(arrays, capacity, counts)]
    return DiffsResult(out[0], out[1], spectrum, state, req)


def diff_records(ctx, records, strand, n_seq, seq_genome, n_genome, cigar_records, cigars, status=None, set="all", kinds=("snp", "ins", "del"),
                 min_indel=1, capacity=None):
    """swg_diff_records.  `records`: a dict of numpy columns (q_id, t_id, q_start, q_end, t_start, t_end); strand: uint8 per record
    (0 = '+'); seq_genome: uint32 per sequence, ids below n_genome; the CIGAR set as ascending record indices and one CIGAR text per
    record, or the (record, offset, text) arrays of lift.cigar_set() as `cigars` with cigar_records None.  Returns a DiffsResult."""
    rec, keep = records_from_numpy(records, COLUMNS, n_seq, strand=strand)
    if any(a.size != int(rec.n) for a in keep):
        raise ValueError("the columns and strand differ in length")
    st = host_column(status, np.uint8, int(rec.n), "status", optional=True)
    sg = host_column(seq_genome, np.uint32, int(rec.n_seq), "seq_genome", optional=True)
    record, offset, text = cigars if cigar_records is None else cigar_set(cigar_records, cigars)
    k = int(record.size)
    return _call(ctx, ctx.lib.swg_diff_records, rec, addr(sg), n_genome, addr(st), (record.ctypes.data, offset.ctypes.data, text.ctypes.data) if k else None,
                 k, SETS.get(set, set), kinds_mask(kinds), min_indel, capacity)


def diff_records_device(ctx, columns, strand, n_seq, seq_genome, n_genome, cigar_record, cigar_offset, cigar_text, k, status=None, set="all",
                        kinds=("snp", "ins", "del"), min_indel=1, capacity=None):
    """swg_diff_records_device over tensors on ctx's GPU (anything with data_ptr / numel / element_size / is_contiguous): the six 4-byte
    columns, strand and status (1 byte per record), seq_genome (4 bytes per sequence) and the three arrays of the set (uint32 [k],
    uint64 [k + 1], bytes).  Rows, pairs, spectrum and state come back on the host."""
    rec = records_from_tensors(columns, {c: 4 for c in COLUMNS}, n_seq)
    for name, t in (("strand", strand), ("status", status)):
        if t is not None and (t.element_size() != 1 or int(t.numel()) < int(rec.n)):
            raise ValueError(f"{name} must be 1-byte with an entry per record")
    if seq_genome is not None and int(seq_genome.numel()) * seq_genome.element_size() < 4 * int(n_seq):
        raise ValueError("seq_genome holds fewer than 4 bytes per sequence")
    rec.strand = int(strand.data_ptr())
    k = int(k)
    if k and (int(cigar_record.numel()) * cigar_record.element_size() < 4 * k or int(cigar_offset.numel()) * cigar_offset.element_size() < 8 * (k + 1)):
        raise ValueError("the CIGAR set's record or offset tensor is shorter than k asks for")
    cig = (int(cigar_record.data_ptr()), int(cigar_offset.data_ptr()), int(cigar_text.data_ptr())) if k else None
    return _call(ctx, ctx.lib.swg_diff_records_device, rec, int(seq_genome.data_ptr()) if seq_genome is not None else None, n_genome,
                 int(status.data_ptr()) if status is not None else None, cig, k, SETS.get(set, set), kinds_mask(kinds), min_indel, capacity)


def parse_rows(text):
    """The rows text -> a list of (t_name, t_start, t_end, q_name, q_start, q_end, strand, kind, len, left, right, record)."""
    rows = []
    for ln in text.split("\n"):
        if not ln or ln.startswith("#"):
            continue
        f = ln.split("\t")
        rows.append(tuple(v if k in (0, 3, 6, 7) else int(v) for k, v in enumerate(f)))
    return rows


def parse_summary(text):
    """The summary text -> (pairs, spectrum): per genome pair (q_genome, t_genome, then the twelve sums), and a dict
    (KIND, lo, hi) -> count."""
    pairs, spectrum = [], {}
    for ln in text.split("\n"):
        f = ln.split("\t")
        if f[0] == "#spectrum":
            spectrum[(f[1], int(f[2]), int(f[3]))] = int(f[4])
        elif ln and not ln.startswith("#"):
            pairs.append((f[0], f[1]) + tuple(int(v) for v in f[2:]))
    return pairs, spectrum


class Diffs:
    """The differences of an open PafFile: `text` (the rows) and `summary_text`, `counts` (a dict: records usable bad untagged rows,
    the runs and bases of each kind, m_columns, batches), and `rows`, `pairs`, `spectrum` parsed from the texts."""

    def __init__(self, text, summary_text, counts):
        self.text, self.summary_text, self.counts = text, summary_text, counts

    @property
    def rows(self):
        return parse_rows(self.text)

    @property
    def pairs(self):
        return parse_summary(self.summary_text)[0]

    @property
    def spectrum(self):
        return parse_summary(self.summary_text)[1]

    @staticmethod
    def _args(paf, status, set, kinds, ctx):
        ctx = getattr(ctx, "ctx", ctx)
        lib = load()
        st = host_column(status, np.uint8, paf.n, "status", optional=True)
        set_, mask = SETS.get(set, set), kinds_mask(kinds)
        rebased = bool(lib.swg_paf_seq_offsets(paf.handle)) or bool(lib.swg_paf_record_offsets(paf.handle, 0))   # (refused by the library)
        in_set = paf.n if set_ == 0 else (int(np.count_nonzero(st[:paf.n])) if st is not None else 0)
        if ctx is None and in_set and not rebased and set_ in (0, 1) and 0 < mask < 16:
            ctx = default_context()
        return lib, ctx.handle if ctx is not None else None, st, set_, mask

    @classmethod
    def from_paf(cls, paf, status, set="kept", kinds=("snp", "ins", "del"), min_indel=1, batch_bytes=0, ctx=None):
        """swg_paf_diffs_text.  status None: set must be "all".  ctx: a Context, anything with a `.ctx`, or None = the default context,
        which is only opened when the set has records.  batch_bytes: CIGAR text per device call, 0 = the library's default."""
        lib, handle, st, set_, mask = cls._args(paf, status, set, kinds, ctx)
        counts = SwgDiffCounts()
        p, n = (C.c_void_p(), C.c_void_p()), (C.c_uint64(), C.c_uint64())
        raise_alnstats(lib, lib.swg_paf_diffs_text(handle, paf.handle, addr(st), set_, mask, int(min_indel), int(batch_bytes), C.byref(counts),
                                                   C.byref(p[0]), C.byref(n[0]), C.byref(p[1]), C.byref(n[1])))
        texts = []
        for q, m in zip(p, n):
            texts.append(C.string_at(q.value, m.value).decode("utf-8", errors="surrogateescape") if q.value else "")
            lib.swg_free(q)
        return cls(texts[0], texts[1], {k: int(getattr(counts, k)) for k in COUNTS})

    @classmethod
    def write_paf(cls, paf, status, path, summary_path=None, set="kept", kinds=("snp", "ins", "del"), min_indel=1, batch_bytes=0, ctx=None):
        """swg_paf_diffs_write: the same into files (either path may be None, not both) -> the counts."""
        lib, handle, st, set_, mask = cls._args(paf, status, set, kinds, ctx)
        counts = SwgDiffCounts()
        enc = lambda v: None if v is None else str(v).encode()   # noqa: E731
        raise_alnstats(lib, lib.swg_paf_diffs_write(handle, paf.handle, addr(st), set_, mask, int(min_indel), int(batch_bytes), enc(path), enc(summary_path),
                                                    C.byref(counts)))
        return {k: int(getattr(counts, k)) for k in COUNTS}
