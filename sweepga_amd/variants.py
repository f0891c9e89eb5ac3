"""Variant calls from the CIGARs and the sequences, on the device (csrc/swg_variants.hip, DESIGN.md section 34;
include/sweepga_gpu.h states the definitions): every SNV, insertion and deletion inside the mappings with its bases.
variant_records / variant_records_device are the record seams: a CIGAR set and a sequence set in, VARIANT_DTYPE variants, their
allele pool and PAIR_DTYPE sums per genome pair out.  Variants.from_paf is swg_paf_vcf_text: the VCF and the summary of an open PafFile
against FASTA files."""
import ctypes as C
import os

import numpy as np

from ._lib import SWG_OK, VARIANT_SUMS, VCF_COUNTS, SwgCigarSet, SwgError, SwgSeqSet, SwgVariantRequest, SwgVcfCounts, SwgVcfOptions, default_context, load
from ._marshal import addr, host_column, raise_alnstats, records_from_numpy, records_from_tensors
from .lift import COLUMNS, SETS, cigar_set

SNP, INS, DEL = 1, 2, 4
MINUS = 256
ANY = 0xFFFFFFFF
VARIANT_DTYPE = np.dtype([(k, "<u4") for k in ("record", "kind_flags", "pos", "ref_len", "alt_len", "q_pos")] + [("allele_offset", "<u8")])
PAIR_DTYPE = np.dtype([("q_genome", "<u4"), ("t_genome", "<u4")] + [(k, "<u8") for k in VARIANT_SUMS])
FIELDS = ("n_variants", "pool_bytes", "n_pairs", "ops", "cigar_bad", "usable", "no_sequence", "out_of_sequence", "columns")


def sequence_set(seqs):
    """One bytes-like per sequence (empty or None: absent) -> (offset uint64 [n + 1], bases uint8)."""
    parts = [np.frombuffer(bytes(s or b""), dtype=np.uint8) for s in seqs]
    offset = np.zeros(len(parts) + 1, dtype=np.uint64)
    offset[1:] = np.cumsum([p.size for p in parts], dtype=np.uint64)
    bases = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return offset, bases if bases.size else np.zeros(1, dtype=np.uint8)


class VariantsResult:
    """variants: a VARIANT_DTYPE array and pool: its allele bytes (uint8) -- both None when either capacity did not hold; pairs: a
    PAIR_DTYPE array or None; the counts as the request returns them."""

    def __init__(self, variants, pool, pairs, req):
        self.variants, self.pool, self.pairs = variants, pool, pairs
        for k in FIELDS:
            setattr(self, k, int(getattr(req, k)))

    def alleles(self, i):
        """(REF, ALT) of variant i as bytes"""
        v = self.variants[i]
        at, r, a = int(v["allele_offset"]), int(v["ref_len"]), int(v["alt_len"])
        return self.pool[at:at + r].tobytes(), self.pool[at + r:at + r + a].tobytes()


def _genome(g):
    return ANY if g is None else int(g)


def _call(ctx, fn, rec, genome_addr, n_genome, status_addr, cigars, k, seqs, set_, t_genome, q_genome, max_indel, capacity):
    """cigars: (record, offset, text) addresses or None; seqs: (offset address, bases address, n_seq) or None.  capacity: None = two
    calls, the second with arrays of the sizes the first one reported; or (variants, pool bytes, pairs), each an int or None for a
    NULL array."""
    req = SwgVariantRequest()
    req.set, req.t_genome, req.q_genome, req.max_indel = int(set_), _genome(t_genome), _genome(q_genome), int(max_indel)
    cs = ss = None
    if cigars is not None:
        cs = SwgCigarSet()
        cs.record, cs.offset, cs.text, cs.k = cigars[0], cigars[1], cigars[2], int(k)
    if seqs is not None:
        ss = SwgSeqSet()
        ss.offset, ss.bases, ss.n_seq = seqs[0], seqs[1], int(seqs[2])
    call = lambda: ctx.check(fn(ctx.handle, C.byref(rec), genome_addr, int(n_genome), status_addr, C.byref(cs) if cs is not None else None,   # noqa: E731
                                C.byref(ss) if ss is not None else None, C.byref(req)))
    if capacity is None:
        call()
        capacity = (int(req.n_variants), int(req.pool_bytes), int(req.n_pairs))
    arrays = [None if c is None else np.zeros(max(int(c), 1), dtype=dt) for c, dt in zip(capacity, (VARIANT_DTYPE, np.uint8, PAIR_DTYPE))]
    req.variant_capacity, req.pool_capacity, req.pair_capacity = (0 if c is None else int(c) for c in capacity)
    req.variants, req.pool, req.pairs = (addr(a) for a in arrays)
    call()
    counts = (int(req.n_variants), int(req.pool_bytes), int(req.n_pairs))
    fit = [a is not None and n <= int(c) for a, c, n in zip(arrays, capacity, counts)]
    fit[0] = fit[1] = fit[0] and fit[1]
    out = [a[:n] if f else None for a, n, f in zip(arrays, counts, fit)]
    res = VariantsResult(out[0], out[1], out[2], req)
    res.arrays = arrays   # what the call was given, whole (the tests look at what it left untouched)
    return res


def variant_records(ctx, records, strand, n_seq, seq_genome, n_genome, cigar_records, cigars, seqs, status=None, set="all", ref=None, query=None,
                    max_indel=0, capacity=None):
    """swg_variant_records.  `records`, strand, seq_genome and the CIGAR set as in diffs.diff_records; seqs: one bytes-like per
    sequence (empty or None = absent) or the (offset, bases) arrays of sequence_set(); ref / query: a target / query genome id or
    None = any.  Returns a VariantsResult."""
    rec, keep = records_from_numpy(records, COLUMNS, n_seq, strand=strand)
    if any(a.size != int(rec.n) for a in keep):
        raise ValueError("the columns and strand differ in length")
    st = host_column(status, np.uint8, int(rec.n), "status", optional=True)
    sg = host_column(seq_genome, np.uint32, int(rec.n_seq), "seq_genome", optional=True)
    record, offset, text = cigars if cigar_records is None else cigar_set(cigar_records, cigars)
    k = int(record.size)
    sset = None
    if seqs is not None:
        s_off, s_bases = seqs if isinstance(seqs, tuple) else sequence_set(seqs)
        s_off, s_bases = np.ascontiguousarray(s_off, dtype=np.uint64), np.ascontiguousarray(s_bases, dtype=np.uint8)
        keep += [s_off, s_bases]
        sset = (s_off.ctypes.data, s_bases.ctypes.data, s_off.size - 1)
    return _call(ctx, ctx.lib.swg_variant_records, rec, addr(sg), n_genome, addr(st), (record.ctypes.data, offset.ctypes.data, text.ctypes.data) if k else None,
                 k, sset, SETS.get(set, set), ref, query, max_indel, capacity)


def variant_records_device(ctx, columns, strand, n_seq, seq_genome, n_genome, cigar_record, cigar_offset, cigar_text, k, seq_offset, seq_bases, status=None,
                           set="all", ref=None, query=None, max_indel=0, capacity=None):
    """swg_variant_records_device over tensors on ctx's GPU (anything with data_ptr / numel / element_size / is_contiguous): as
    diffs.diff_records_device, plus seq_offset (uint64 [n_seq + 1]) and seq_bases (bytes).  Variants, pool and pairs come back on
    the host."""
    rec = records_from_tensors(columns, {c: 4 for c in COLUMNS}, n_seq)
    for name, t in (("strand", strand), ("status", status)):
        if t is not None and (t.element_size() != 1 or int(t.numel()) < int(rec.n)):
            raise ValueError(f"{name} must be 1-byte with an entry per record")
    if seq_genome is not None and int(seq_genome.numel()) * seq_genome.element_size() < 4 * int(n_seq):
        raise ValueError("seq_genome holds fewer than 4 bytes per sequence")
    if seq_offset is not None and int(seq_offset.numel()) * seq_offset.element_size() < 8 * (int(n_seq) + 1):
        raise ValueError("seq_offset holds fewer than 8 bytes per sequence and one more")
    rec.strand = int(strand.data_ptr())
    k = int(k)
    if k and (int(cigar_record.numel()) * cigar_record.element_size() < 4 * k or int(cigar_offset.numel()) * cigar_offset.element_size() < 8 * (k + 1)):
        raise ValueError("the CIGAR set's record or offset tensor is shorter than k asks for")
    cig = (int(cigar_record.data_ptr()), int(cigar_offset.data_ptr()), int(cigar_text.data_ptr())) if k else None
    sset = (int(seq_offset.data_ptr()), int(seq_bases.data_ptr()), int(n_seq)) if seq_offset is not None and seq_bases is not None else None
    return _call(ctx, ctx.lib.swg_variant_records_device, rec, int(seq_genome.data_ptr()) if seq_genome is not None else None, n_genome,
                 int(status.data_ptr()) if status is not None else None, cig, k, sset, SETS.get(set, set), ref, query, max_indel, capacity)


def parse_vcf(text):
    """The VCF text -> a list of (chrom, pos (1-based), ref, alt, info as a dict of str)"""
    out = []
    for ln in text.split("\n"):
        if not ln or ln.startswith("#"):
            continue
        f = ln.split("\t")
        out.append((f[0], int(f[1]), f[3], f[4], dict(kv.split("=", 1) for kv in f[7].split(";"))))
    return out


def parse_summary(text):
    """The summary text -> per genome pair (q_genome, t_genome, then the sums, ts and tv as ints)"""
    return [tuple(f[:2]) + tuple(int(v) for v in f[2:]) for f in (ln.split("\t") for ln in text.split("\n") if ln and not ln.startswith("#"))]


class _FastaHandle:
    """swg_fasta_open over paths, closed on exit"""

    def __init__(self, lib, paths, threads=0):
        if isinstance(paths, (str, bytes, os.PathLike)):
            paths = [paths]
        enc = [os.fsencode(p) for p in paths]
        self.lib, self.handle = lib, C.c_void_p()
        rc = lib.swg_fasta_open((C.c_char_p * len(enc))(*enc), len(enc), threads, C.byref(self.handle)) if enc else SWG_OK
        if rc != SWG_OK:
            raise SwgError(rc, (lib.swg_fasta_last_error() or b"").decode(errors="replace"))

    def __enter__(self):
        return self.handle if self.handle.value else None

    def __exit__(self, *exc):
        if self.handle.value:
            self.lib.swg_fasta_close(self.handle)


class Variants:
    """The variant calls of an open PafFile: `text` (the VCF) and `summary_text`, `counts` (a dict: records usable bad untagged variants
    snvs n_ins n_del same n_columns m_equal long_indels unanchored no_sequence out_of_sequence length_mismatch batches), and `variants`,
    `pairs` parsed from the texts."""

    def __init__(self, text, summary_text, counts):
        self.text, self.summary_text, self.counts = text, summary_text, counts
        self._variants = self._pairs = None

    @property
    def variants(self):
        """the lines of the VCF, parsed once: (chrom, pos, ref, alt, info)"""
        if self._variants is None:
            self._variants = parse_vcf(self.text)
        return self._variants

    @property
    def pool(self):
        """The allele bytes of the VCF's lines in the file's order, REF before ALT.  (Not the device's pool, which lies in (record, op,
        column) order and stays with the record seams: the file is sorted per contig.)"""
        return "".join(v[2] + v[3] for v in self.variants).encode()

    @property
    def pairs(self):
        if self._pairs is None:
            self._pairs = parse_summary(self.summary_text)
        return self._pairs

    @staticmethod
    def _args(paf, status, set, ref, query, max_indel, batch_bytes, ctx):
        ctx = getattr(ctx, "ctx", ctx)
        lib = load()
        st = host_column(status, np.uint8, paf.n, "status", optional=True)
        set_ = SETS.get(set, set)
        opts = SwgVcfOptions()
        opts.set, opts.max_indel, opts.batch_bytes = int(set_), int(max_indel), int(batch_bytes)
        opts.ref_genome = None if ref is None else str(ref).encode()
        opts.query_genome = None if query is None else str(query).encode()
        rebased = bool(lib.swg_paf_seq_offsets(paf.handle)) or bool(lib.swg_paf_record_offsets(paf.handle, 0))   # (refused by the library)
        in_set = paf.n if set_ == 0 else (int(np.count_nonzero(st[:paf.n])) if st is not None else 0)
        if ctx is None and in_set and not rebased and set_ in (0, 1):
            ctx = default_context()
        return lib, ctx.handle if ctx is not None else None, st, opts

    @classmethod
    def from_paf(cls, paf, status, fasta=(), set="kept", ref=None, query=None, max_indel=10000, batch_bytes=0, ctx=None):
        """swg_paf_vcf_text.  fasta: the paths of the FASTA files (plain / .gz / .bgz).  status None: set must be "all".  ref / query: a
        genome name (the two-part prefix) or None = any; a query names the sample column.  ctx: a Context, anything with a `.ctx`, or
        None = the default context, which is only opened when the set has records."""
        lib, handle, st, opts = cls._args(paf, status, set, ref, query, max_indel, batch_bytes, ctx)
        counts = SwgVcfCounts()
        p, n = (C.c_void_p(), C.c_void_p()), (C.c_uint64(), C.c_uint64())
        with _FastaHandle(lib, fasta) as fa:
            raise_alnstats(lib, lib.swg_paf_vcf_text(handle, paf.handle, addr(st), fa, C.byref(opts), C.byref(counts), C.byref(p[0]), C.byref(n[0]),
                                                     C.byref(p[1]), C.byref(n[1])))
        texts = []
        for q, m in zip(p, n):
            texts.append(C.string_at(q.value, m.value).decode("utf-8", errors="surrogateescape") if q.value else "")
            lib.swg_free(q)
        return cls(texts[0], texts[1], {k: int(getattr(counts, k)) for k in VCF_COUNTS})

    @classmethod
    def write_paf(cls, paf, status, path, summary_path=None, fasta=(), set="kept", ref=None, query=None, max_indel=10000, batch_bytes=0, ctx=None):
        """swg_paf_vcf_write: the same into files (either path may be None, not both) -> the counts."""
        lib, handle, st, opts = cls._args(paf, status, set, ref, query, max_indel, batch_bytes, ctx)
        counts = SwgVcfCounts()
        enc = lambda v: None if v is None else str(v).encode()   # noqa: E731
        with _FastaHandle(lib, fasta) as fa:
            raise_alnstats(lib, lib.swg_paf_vcf_write(handle, paf.handle, addr(st), fa, C.byref(opts), enc(path), enc(summary_path), C.byref(counts)))
        return {k: int(getattr(counts, k)) for k in VCF_COUNTS}
