"""The lift seen from Python: caller-given regions projected through the mappings of a filter call on the device
(csrc/swg_lift.hip).  lift_records / lift_records_device are the two record seams, Lift.from_paf BED text through an open PafFile.
lift_closure_records / lift_closure_records_device / LiftClosure.from_paf are the same three for the transitive lift
(csrc/swg_lift_closure.hip): what each region reaches in up to max_hops hops, as disjoint pieces with the hop that found them.
lift_exact_records / lift_exact_records_device / lift_hit_records / lift_hit_records_device / Lift.from_paf(exact=True) are the
base-exact lift (csrc/swg_cigar.hip): the rows refined through the CIGARs of the records that are hit."""
import ctypes as C

import numpy as np

from ._lib import (SwgCigarSet, SwgClosureRequest, SwgLiftExactRequest, SwgLiftPafCounts, SwgLiftRequest, SwgLiftSliceRequest, default_context,
                   load)
from ._marshal import addr, host_column, raise_alnstats, records_from_numpy, records_from_tensors, take_texts, text_slots

COLUMNS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")
REGION_DTYPE = np.dtype([("seq", np.uint32), ("start", np.uint32), ("end", np.uint32), ("reserved", np.uint32)])
ROW_DTYPE = np.dtype([(k, np.uint32) for k in ("region", "record", "src_start", "src_end", "dst_seq", "dst_start", "dst_end", "flags")])
EXACT_ROW_DTYPE = np.dtype(ROW_DTYPE.descr + [("aligned", np.uint32), ("matches", np.uint32)])
UNKNOWN = 2**32 - 1
SET_ALL, SET_KEPT = 0, 1
AXIS_QUERY, AXIS_TARGET, AXIS_BOTH = 1, 2, 3
MINUS, ON_TARGET, EXACT = 1, 2, 4
CIGAR_SYNTAX, CIGAR_VALUE, CIGAR_QUERY_SUM, CIGAR_TARGET_SUM, CIGAR_EMPTY = 1, 2, 4, 8, 16
CLOSURE_ROW_DTYPE = np.dtype([(k, np.uint32) for k in ("region", "seq", "start", "end", "hop", "reserved")])
CLOSURE_SUMMARY_DTYPE = np.dtype([("bases", np.uint64), ("pieces", np.uint32), ("sequences", np.uint32), ("hops", np.uint32), ("flags", np.uint32)])
CLOSURE_CUT = 1
SETS = {"all": SET_ALL, "kept": SET_KEPT}
AXES = {"query": AXIS_QUERY, "target": AXIS_TARGET, "both": AXIS_BOTH}


class LiftResult:
    """rows: a ROW_DTYPE array in (region, axis, start on the axis, record) order, or None when the capacity given did not hold
    them; n: their number; summary: an (m, 2, 2) uint32 array, hits[region][set][axis]; candidates: (query axis, target axis)."""

    def __init__(self, rows, n, summary, candidates):
        self.rows, self.n, self.summary, self.candidates = rows, n, summary, candidates


def regions_array(regions):
    """A REGION_DTYPE array from one, or from an iterable of (seq, start, end)."""
    if isinstance(regions, np.ndarray) and regions.dtype == REGION_DTYPE:
        return np.ascontiguousarray(regions)
    out = np.zeros(len(regions), dtype=REGION_DTYPE)
    for k, (seq, start, end) in enumerate(regions):
        out[k] = (seq, start, end, 0)
    return out


def _call(ctx, fn, rec, status_addr, regions_addr, m, set_, axes, capacity):
    """capacity None: the two-call protocol (count, then fetch); a number: one call with an array of that size."""
    req = SwgLiftRequest()
    req.set, req.axes = int(set_), int(axes)
    summary = np.zeros((m, 2, 2), dtype=np.uint32)
    req.summary = summary.ctypes.data if m else None
    rows = None
    if capacity is not None:
        rows = np.zeros(int(capacity), dtype=ROW_DTYPE)
        req.capacity, req.rows = int(capacity), rows.ctypes.data if capacity else None
    ctx.check(fn(ctx.handle, C.byref(rec), status_addr, regions_addr, m, C.byref(req)))
    if capacity is None:
        rows = np.zeros(int(req.n), dtype=ROW_DTYPE)
        if req.n:
            req.capacity, req.rows = int(req.n), rows.ctypes.data
            ctx.check(fn(ctx.handle, C.byref(rec), status_addr, regions_addr, m, C.byref(req)))
    elif req.n > capacity:
        rows = None
    else:
        rows = rows[:int(req.n)]
    return LiftResult(rows, int(req.n), summary, (int(req.candidates[0]), int(req.candidates[1])))


def _host_records(records, strand, n_seq):
    """(SwgRecords over the caller's numpy columns, the arrays that must stay alive)"""
    rec, keep = records_from_numpy(records, COLUMNS, n_seq, strand=strand)
    if any(a.size != int(rec.n) for a in keep):
        raise ValueError("the columns and strand differ in length")
    return rec, keep


def _device_records(columns, strand, n_seq, regions, n_regions, status):
    rec = records_from_tensors(columns, {k: 4 for k in COLUMNS}, n_seq)
    for name, t in (("strand", strand), ("status", status)):
        if t is not None and (t.element_size() != 1 or int(t.numel()) < int(rec.n)):
            raise ValueError(f"{name} must be 1-byte with an entry per record")
    if int(regions.numel()) * regions.element_size() < 16 * int(n_regions):
        raise ValueError("regions holds fewer than 16 bytes per region")
    rec.strand = int(strand.data_ptr())
    return rec


def lift_records(ctx, records, strand, n_seq, regions, status=None, set="all", axes="both", capacity=None):
    """swg_lift_records.  `records`: a dict of numpy columns (q_id, t_id, q_start, q_end, t_start, t_end); strand: uint8 per record
    (0 = '+'); regions: a REGION_DTYPE array or (seq, start, end) triples, seq = UNKNOWN for a name the input does not have;
    set: "all" / "kept" (or 0 / 1), axes: "query" / "target" / "both" (or the bit mask).  Returns a LiftResult."""
    regs = regions_array(regions)
    rec, keep = _host_records(records, strand, n_seq)
    st = host_column(status, np.uint8, int(rec.n), "status", optional=True)
    return _call(ctx, ctx.lib.swg_lift_records, rec, addr(st), regs.ctypes.data if regs.size else None,
                 regs.size, SETS.get(set, set), AXES.get(axes, axes), capacity)


def lift_records_device(ctx, columns, strand, n_seq, regions, n_regions, status=None, set="all", axes="both", capacity=None):
    """swg_lift_records_device over torch tensors on ctx's GPU: `columns` maps q_id, t_id, q_start, q_end, t_start, t_end to
    contiguous 4-byte tensors of one length, strand and status (or None) are 1-byte tensors with an entry per record, regions a
    tensor of 16 * n_regions bytes laid out as REGION_DTYPE.  (Anything with .data_ptr(), .numel() and .element_size() works; the
    caller keeps the tensors alive and their work finished.)  Rows and summary come back as numpy arrays on the host."""
    rec = _device_records(columns, strand, n_seq, regions, n_regions, status)
    return _call(ctx, ctx.lib.swg_lift_records_device, rec, int(status.data_ptr()) if status is not None else None, int(regions.data_ptr()),
                 int(n_regions), SETS.get(set, set), AXES.get(axes, axes), capacity)


class LiftExactResult(LiftResult):
    """A LiftResult whose rows are an EXACT_ROW_DTYPE array; state: a uint8 per entry of the CIGAR set (0 = usable); ops, cigar_bad
    and exact_rows as the request returns them."""

    def __init__(self, rows, n, summary, candidates, state, ops, cigar_bad, exact_rows):
        super().__init__(rows, n, summary, candidates)
        self.state, self.ops, self.cigar_bad, self.exact_rows = state, ops, cigar_bad, exact_rows


def cigar_set(records, cigars):
    """(record, offset, text) as the numpy arrays of a swg_cigar_set from ascending record indices and one CIGAR (str or bytes)
    per record."""
    texts = [t.encode("latin-1") if isinstance(t, str) else bytes(t) for t in cigars]
    record = np.ascontiguousarray(records, dtype=np.uint32)
    if len(texts) != record.size:
        raise ValueError("one CIGAR per record is needed")
    offset = np.zeros(record.size + 1, dtype=np.uint64)
    np.cumsum([len(t) for t in texts], out=offset[1:])
    text = np.frombuffer(b"".join(texts) or b"\0", dtype=np.uint8)
    return record, offset, text


def _exact_call(ctx, fn, rec, status_addr, regions_addr, m, cigars, k, set_, axes, capacity):
    """cigars: (record address, offset address, text address) or None; capacity as in _call."""
    req = SwgLiftExactRequest()
    req.set, req.axes = int(set_), int(axes)
    summary = np.zeros((m, 2, 2), dtype=np.uint32)
    req.summary = summary.ctypes.data if m else None
    state = np.zeros(int(k), dtype=np.uint8)
    req.state = state.ctypes.data if k else None
    cs = None
    if cigars is not None:
        cs = SwgCigarSet()
        cs.record, cs.offset, cs.text, cs.k = cigars[0], cigars[1], cigars[2], int(k)
    call = lambda: ctx.check(fn(ctx.handle, C.byref(rec), status_addr, regions_addr, m, C.byref(cs) if cs is not None else None, C.byref(req)))   # noqa: E731
    rows = None
    if capacity is not None:
        rows = np.zeros(int(capacity), dtype=EXACT_ROW_DTYPE)
        req.capacity, req.rows = int(capacity), rows.ctypes.data if capacity else None
    call()
    if capacity is None:
        rows = np.zeros(int(req.n), dtype=EXACT_ROW_DTYPE)
        if req.n:
            req.capacity, req.rows = int(req.n), rows.ctypes.data
            call()
    elif req.n > capacity:
        rows = None
    else:
        rows = rows[:int(req.n)]
    return LiftExactResult(rows, int(req.n), summary, (int(req.candidates[0]), int(req.candidates[1])), state, int(req.ops), int(req.cigar_bad),
                           int(req.exact_rows))


def lift_exact_records(ctx, records, strand, n_seq, regions, cigar_records, cigars, status=None, set="all", axes="both", capacity=None):
    """swg_lift_exact_records: the arguments of lift_records, plus the CIGAR set -- ascending record indices and one CIGAR text per
    record (empty: the record has none), or the (record, offset, text) arrays of cigar_set() as `cigars` with cigar_records None.
    Returns a LiftExactResult."""
    regs = regions_array(regions)
    rec, keep = _host_records(records, strand, n_seq)
    st = host_column(status, np.uint8, int(rec.n), "status", optional=True)
    record, offset, text = cigars if cigar_records is None else cigar_set(cigar_records, cigars)
    k = int(record.size)
    return _exact_call(ctx, ctx.lib.swg_lift_exact_records, rec, addr(st), regs.ctypes.data if regs.size else None, regs.size,
                       (record.ctypes.data, offset.ctypes.data, text.ctypes.data) if k else None, k, SETS.get(set, set), AXES.get(axes, axes), capacity)


def lift_exact_records_device(ctx, columns, strand, n_seq, regions, n_regions, cigar_record, cigar_offset, cigar_text, k, status=None, set="all",
                              axes="both", capacity=None):
    """swg_lift_exact_records_device: the arguments of lift_records_device, plus the three arrays of the set as device tensors
    (uint32 [k], uint64 [k + 1], bytes) and k.  Rows, summary and state come back as numpy arrays on the host."""
    rec = _device_records(columns, strand, n_seq, regions, n_regions, status)
    k = int(k)
    if k and (int(cigar_record.numel()) * cigar_record.element_size() < 4 * k or int(cigar_offset.numel()) * cigar_offset.element_size() < 8 * (k + 1)):
        raise ValueError("the CIGAR set's record or offset tensor is shorter than k asks for")
    cig = (int(cigar_record.data_ptr()), int(cigar_offset.data_ptr()), int(cigar_text.data_ptr())) if k else None
    return _exact_call(ctx, ctx.lib.swg_lift_exact_records_device, rec, int(status.data_ptr()) if status is not None else None,
                       int(regions.data_ptr()), int(n_regions), cig, k, SETS.get(set, set), AXES.get(axes, axes), capacity)


def _hit_call(ctx, fn, rec, status_addr, regions_addr, m, set_, axes, capacity):
    k = C.c_uint64(0)
    out = np.zeros(int(capacity) if capacity is not None else 0, dtype=np.uint32)
    call = lambda: ctx.check(fn(ctx.handle, C.byref(rec), status_addr, regions_addr, m, int(set_), int(axes), out.ctypes.data if out.size else None,   # noqa: E731
                                out.size, C.byref(k)))
    call()
    if capacity is None and k.value:
        out = np.zeros(int(k.value), dtype=np.uint32)
        call()
    return (out[:int(k.value)] if k.value <= out.size else None), int(k.value)


def lift_hit_records(ctx, records, strand, n_seq, regions, status=None, set="all", axes="both", capacity=None):
    """swg_lift_hit_records: the distinct records with a hit, ascending -> (uint32 array, or None when `capacity` did not hold them; k)."""
    regs = regions_array(regions)
    rec, keep = _host_records(records, strand, n_seq)
    st = host_column(status, np.uint8, int(rec.n), "status", optional=True)
    return _hit_call(ctx, ctx.lib.swg_lift_hit_records, rec, addr(st), regs.ctypes.data if regs.size else None, regs.size, SETS.get(set, set),
                     AXES.get(axes, axes), capacity)


def lift_hit_records_device(ctx, columns, strand, n_seq, regions, n_regions, status=None, set="all", axes="both", capacity=None):
    """swg_lift_hit_records_device over the tensors of lift_records_device; the list comes back as a numpy array on the host."""
    rec = _device_records(columns, strand, n_seq, regions, n_regions, status)
    return _hit_call(ctx, ctx.lib.swg_lift_hit_records_device, rec, int(status.data_ptr()) if status is not None else None, int(regions.data_ptr()),
                     int(n_regions), SETS.get(set, set), AXES.get(axes, axes), capacity)


class LiftClosureResult:
    """rows: a CLOSURE_ROW_DTYPE array in (region, seq, start) order, or None when the capacity given did not hold them; n: their
    number; summary: a CLOSURE_SUMMARY_DTYPE array per region; hops_run, projections (summed over the hops) and candidates (query
    axis, target axis; summed over the hops) as the request returns them."""

    def __init__(self, rows, n, summary, hops_run, projections, candidates):
        self.rows, self.n, self.summary, self.hops_run, self.projections, self.candidates = rows, n, summary, hops_run, projections, candidates


def _closure_call(ctx, fn, rec, status_addr, regions_addr, m, set_, axes, max_hops, min_len, capacity):
    req = SwgClosureRequest()
    req.set, req.axes, req.max_hops, req.min_len = int(set_), int(axes), int(max_hops), int(min_len)
    summary = np.zeros(m, dtype=CLOSURE_SUMMARY_DTYPE)
    req.summary = summary.ctypes.data if m else None
    rows = None
    if capacity is not None:
        rows = np.zeros(int(capacity), dtype=CLOSURE_ROW_DTYPE)
        req.capacity, req.rows = int(capacity), rows.ctypes.data if capacity else None
    ctx.check(fn(ctx.handle, C.byref(rec), status_addr, regions_addr, m, C.byref(req)))
    if capacity is None:
        rows = np.zeros(int(req.n), dtype=CLOSURE_ROW_DTYPE)
        if req.n:
            req.capacity, req.rows = int(req.n), rows.ctypes.data
            ctx.check(fn(ctx.handle, C.byref(rec), status_addr, regions_addr, m, C.byref(req)))
    elif req.n > capacity:
        rows = None
    else:
        rows = rows[:int(req.n)]
    return LiftClosureResult(rows, int(req.n), summary, int(req.hops_run), int(req.projections), (int(req.candidates[0]), int(req.candidates[1])))


def lift_closure_records(ctx, records, strand, n_seq, regions, max_hops, min_len=100, status=None, set="all", axes="both", capacity=None):
    """swg_lift_closure_records: the arguments of lift_records, plus the largest number of hops (1 .. 65,535) and the length below
    which a piece is reported but not walked on.  Returns a LiftClosureResult."""
    regs = regions_array(regions)
    rec, keep = _host_records(records, strand, n_seq)
    st = host_column(status, np.uint8, int(rec.n), "status", optional=True)
    return _closure_call(ctx, ctx.lib.swg_lift_closure_records, rec, addr(st),
                         regs.ctypes.data if regs.size else None, regs.size, SETS.get(set, set), AXES.get(axes, axes), max_hops, min_len, capacity)


def lift_closure_records_device(ctx, columns, strand, n_seq, regions, n_regions, max_hops, min_len=100, status=None, set="all", axes="both",
                                capacity=None):
    """swg_lift_closure_records_device: the arguments of lift_records_device, plus max_hops and min_len."""
    rec = _device_records(columns, strand, n_seq, regions, n_regions, status)
    return _closure_call(ctx, ctx.lib.swg_lift_closure_records_device, rec, int(status.data_ptr()) if status is not None else None,
                         int(regions.data_ptr()), int(n_regions), SETS.get(set, set), AXES.get(axes, axes), max_hops, min_len, capacity)


def parse_rows(text):
    """The rows text as a ROW_DTYPE-like structured array with names: (dst_name, dst_start, dst_end, label, src_name, src_start,
    src_end, strand, axis, record) per line."""
    dt = np.dtype([("dst_name", object), ("dst_start", np.uint32), ("dst_end", np.uint32), ("label", object), ("src_name", object),
                   ("src_start", np.uint32), ("src_end", np.uint32), ("strand", "U1"), ("axis", "U1"), ("record", np.uint32)])
    lines = [ln.split("\t") for ln in text.split("\n") if ln]
    out = np.zeros(len(lines), dtype=dt)
    for k, f in enumerate(lines):
        out[k] = (f[0], int(f[1]), int(f[2]), f[3], f[4], int(f[5]), int(f[6]), f[7], f[8], int(f[9]))
    return out


def parse_exact_rows(text):
    """The rows text of an exact lift: parse_rows' fields, then aligned, matches and mode ("exact" / "interp")."""
    dt = np.dtype([("dst_name", object), ("dst_start", np.uint32), ("dst_end", np.uint32), ("label", object), ("src_name", object),
                   ("src_start", np.uint32), ("src_end", np.uint32), ("strand", "U1"), ("axis", "U1"), ("record", np.uint32),
                   ("aligned", np.uint32), ("matches", np.uint32), ("mode", "U6")])
    lines = [ln.split("\t") for ln in text.split("\n") if ln]
    out = np.zeros(len(lines), dtype=dt)
    for k, f in enumerate(lines):
        out[k] = (f[0], int(f[1]), int(f[2]), f[3], f[4], int(f[5]), int(f[6]), f[7], f[8], int(f[9]), int(f[10]), int(f[11]), f[12])
    return out


class Lift:
    """BED regions lifted through an open PafFile: `text` (one line per row: dst_name dst_start dst_end label src_name src_start
    src_end strand axis record) and `summary_text` (label sequence start end all_q all_t kept_q kept_t state per region); `rows` and
    `summary` are the same parsed into structured numpy arrays.  None where not asked for.  An exact lift (from_paf(exact=True)) has
    three more columns per row -- aligned matches mode -- and `exact_counts`: (records hit, entries of state 0, bad entries, records
    without a cg:Z: tag)."""

    def __init__(self, text, summary_text, exact_counts=None):
        self.text, self.summary_text, self.exact_counts = text, summary_text, exact_counts

    @property
    def rows(self):
        if self.text is None:
            return None
        return parse_exact_rows(self.text) if self.exact_counts is not None else parse_rows(self.text)

    @property
    def summary(self):
        if self.summary_text is None:
            return None
        dt = np.dtype([("label", object), ("sequence", object), ("start", np.uint32), ("end", np.uint32), ("all_q", np.uint32),
                       ("all_t", np.uint32), ("kept_q", np.int64), ("kept_t", np.int64), ("state", object)])
        lines = [ln.split("\t") for ln in self.summary_text.split("\n")[1:] if ln]
        out = np.zeros(len(lines), dtype=dt)
        for k, f in enumerate(lines):
            out[k] = (f[0], f[1], int(f[2]), int(f[3]), int(f[4]), int(f[5]), -1 if f[6] == "-" else int(f[6]), -1 if f[7] == "-" else int(f[7]), f[8])
        return out

    @classmethod
    def from_paf(cls, paf, status, bed_text, set="kept", axes="both", ctx=None, rows=True, summary=True, exact=False):
        """swg_paf_lift: both texts from one device call.  status None: set must be "all".  ctx: a Context, anything with a `.ctx`
        (PafFilter), or None = the default context, which is only opened when there are records and regions.  exact: swg_paf_lift_exact,
        the rows through the cg:Z: tags of the lines that are hit."""
        ctx = getattr(ctx, "ctx", ctx)
        lib = load()
        bed = bed_text.encode("utf-8", errors="surrogateescape") if isinstance(bed_text, str) else bytes(bed_text)
        rebased = bool(lib.swg_paf_seq_offsets(paf.handle)) or bool(lib.swg_paf_record_offsets(paf.handle, 0))   # (refused by the library)
        if ctx is None and paf.n and bed.strip() and not rebased:
            ctx = default_context()
        st = host_column(status, np.uint8, paf.n, "status", optional=True)
        p, n = text_slots((rows, summary))
        fn = lib.swg_paf_lift_exact if exact else lib.swg_paf_lift
        rc = fn(ctx.handle if ctx is not None else None, paf.handle, addr(st), bed, len(bed), SETS.get(set, set), AXES.get(axes, axes), p, n)
        raise_alnstats(lib, rc)
        text = [t.decode("utf-8", errors="surrogateescape") if t is not None else None for t in take_texts(lib, p, n, (rows, summary))]
        counts = None
        if exact:
            c4 = (C.c_uint64 * 4)()
            lib.swg_paf_lift_exact_counts(c4)
            counts = tuple(int(x) for x in c4)
        return cls(text[0], text[1], counts)


class LiftClosure:
    """BED regions walked through an open PafFile hop by hop: `text` (one line per piece: name start end label hop; no strand -- a
    merged piece can come from both orientations) and `summary_text` (label sequence start end pieces sequences genomes bases hops
    state per region); `rows` and `summary` are the same parsed into structured numpy arrays.  None where not asked for."""

    def __init__(self, text, summary_text):
        self.text, self.summary_text = text, summary_text

    @property
    def rows(self):
        if self.text is None:
            return None
        dt = np.dtype([("name", object), ("start", np.uint32), ("end", np.uint32), ("label", object), ("hop", np.uint32)])
        lines = [ln.split("\t") for ln in self.text.split("\n") if ln]
        out = np.zeros(len(lines), dtype=dt)
        for k, f in enumerate(lines):
            out[k] = (f[0], int(f[1]), int(f[2]), f[3], int(f[4]))
        return out

    @property
    def summary(self):
        if self.summary_text is None:
            return None
        dt = np.dtype([("label", object), ("sequence", object), ("start", np.uint32), ("end", np.uint32), ("pieces", np.uint32),
                       ("sequences", np.uint32), ("genomes", np.uint32), ("bases", np.uint64), ("hops", np.uint32), ("state", object)])
        lines = [ln.split("\t") for ln in self.summary_text.split("\n")[1:] if ln]
        out = np.zeros(len(lines), dtype=dt)
        for k, f in enumerate(lines):
            out[k] = (f[0], f[1], int(f[2]), int(f[3]), int(f[4]), int(f[5]), int(f[6]), int(f[7]), int(f[8]), f[9])
        return out

    @classmethod
    def from_paf(cls, paf, status, bed_text, max_hops, min_len=100, set="kept", axes="both", ctx=None, rows=True, summary=True):
        """swg_paf_lift_closure: both texts from one walk.  status None: set must be "all".  ctx as in Lift.from_paf."""
        ctx = getattr(ctx, "ctx", ctx)
        lib = load()
        bed = bed_text.encode("utf-8", errors="surrogateescape") if isinstance(bed_text, str) else bytes(bed_text)
        rebased = bool(lib.swg_paf_seq_offsets(paf.handle)) or bool(lib.swg_paf_record_offsets(paf.handle, 0))   # (refused by the library)
        if ctx is None and paf.n and bed.strip() and not rebased and 0 < int(max_hops) <= 65535:
            ctx = default_context()
        st = host_column(status, np.uint8, paf.n, "status", optional=True)
        p, n = text_slots((rows, summary))
        rc = lib.swg_paf_lift_closure(ctx.handle if ctx is not None else None, paf.handle, addr(st), bed, len(bed), SETS.get(set, set),
                                      AXES.get(axes, axes), int(max_hops), int(min_len), p, n)
        raise_alnstats(lib, rc)
        text = [t.decode("utf-8", errors="surrogateescape") if t is not None else None for t in take_texts(lib, p, n, (rows, summary))]
        return cls(text[0], text[1])


# ---- lift slices (csrc/swg_slice.hip): every exact row as an alignment of its own, with its sliced CIGAR --------------------------
SLICE_DTYPE = np.dtype([(k, np.uint32) for k in ("region", "record", "q_start", "q_end", "t_start", "t_end", "flags", "aligned", "matches", "text_len")]
                       + [("block", np.uint64), ("text_first", np.uint64)])
SLICE_HAS_EQ = 8
SLICE_COUNTS = ("n_rows", "n_slices", "n_interp", "n_empty", "n_short", "text_bytes", "ops", "cigar_bad")
PAF_COUNTS = ("rows", "slices", "interp", "empty", "too_short", "hits", "bad", "batches")


def slice_text_tile():
    """The output bytes one work-group of the text kernel writes (SWG_SLICE_TEXT_TILE as the library was built with it)."""
    return int(load().swg_lift_slice_text_tile())


class LiftSliceResult:
    """slices: a SLICE_DTYPE array in the lift's row order, or None when slice_capacity did not hold them; text: the slices' CIGARs end
    to end as bytes (slice s is text[text_first : text_first + text_len]), or None when text_capacity did not hold it; state: a uint8
    per entry of the CIGAR set; counts: a dict of SLICE_COUNTS."""

    def __init__(self, slices, text, state, counts):
        self.slices, self.text, self.state, self.counts = slices, text, state, counts

    def cigar(self, s):
        w = self.slices[s]
        return self.text[int(w["text_first"]):int(w["text_first"]) + int(w["text_len"])].decode("latin-1")


def _slice_call(ctx, fn, rec, status_addr, regions_addr, m, cigars, k, set_, axes, min_aligned, slice_capacity, text_capacity, want_slices=True,
                want_text=True):
    """slice_capacity / text_capacity None: the two-call protocol (count, then fetch); a number: one call with arrays of that size.
    want_slices / want_text False: that pointer is NULL."""
    req = SwgLiftSliceRequest()
    req.set, req.axes, req.min_aligned = int(set_), int(axes), int(min_aligned)
    state = np.zeros(int(k), dtype=np.uint8)
    req.state = state.ctypes.data if k else None
    cs = None
    if cigars is not None:
        cs = SwgCigarSet()
        cs.record, cs.offset, cs.text, cs.k = cigars[0], cigars[1], cigars[2], int(k)
    call = lambda: ctx.check(fn(ctx.handle, C.byref(rec), status_addr, regions_addr, m, C.byref(cs) if cs is not None else None, C.byref(req)))   # noqa: E731
    two_calls = slice_capacity is None or text_capacity is None
    if two_calls:
        call()
        slice_capacity = int(req.n_slices) if slice_capacity is None else slice_capacity
        text_capacity = int(req.text_bytes) if text_capacity is None else text_capacity
    slices = np.zeros(int(slice_capacity), dtype=SLICE_DTYPE)
    text = np.zeros(max(int(text_capacity), 1), dtype=np.uint8)
    req.slice_capacity, req.slices = int(slice_capacity), slices.ctypes.data if want_slices else None
    req.text_capacity, req.text = int(text_capacity), text.ctypes.data if want_text else None
    call()
    counts = {key: int(getattr(req, key)) for key in SLICE_COUNTS}
    got_slices = want_slices and counts["n_slices"] <= slice_capacity
    got_text = want_text and counts["text_bytes"] <= text_capacity
    return LiftSliceResult(slices[:counts["n_slices"]] if got_slices else None, text[:counts["text_bytes"]].tobytes() if got_text else None, state, counts)


def lift_slice_records(ctx, records, strand, n_seq, regions, cigar_records, cigars, status=None, set="all", axes="both", min_aligned=1,
                       slice_capacity=None, text_capacity=None, want_slices=True, want_text=True):
    """swg_lift_slice_records: the arguments of lift_exact_records, plus min_aligned and the two capacities.  Returns a LiftSliceResult."""
    regs = regions_array(regions)
    rec, keep = _host_records(records, strand, n_seq)
    st = host_column(status, np.uint8, int(rec.n), "status", optional=True)
    record, offset, text = cigars if cigar_records is None else cigar_set(cigar_records, cigars)
    k = int(record.size)
    return _slice_call(ctx, ctx.lib.swg_lift_slice_records, rec, addr(st), regs.ctypes.data if regs.size else None, regs.size,
                       (record.ctypes.data, offset.ctypes.data, text.ctypes.data) if k else None, k, SETS.get(set, set), AXES.get(axes, axes), min_aligned,
                       slice_capacity, text_capacity, want_slices, want_text)


def lift_slice_records_device(ctx, columns, strand, n_seq, regions, n_regions, cigar_record, cigar_offset, cigar_text, k, status=None, set="all",
                              axes="both", min_aligned=1, slice_capacity=None, text_capacity=None, want_slices=True, want_text=True):
    """swg_lift_slice_records_device: the arguments of lift_exact_records_device, plus min_aligned and the two capacities.  Slices, text
    and state come back on the host."""
    rec = _device_records(columns, strand, n_seq, regions, n_regions, status)
    k = int(k)
    if k and (int(cigar_record.numel()) * cigar_record.element_size() < 4 * k or int(cigar_offset.numel()) * cigar_offset.element_size() < 8 * (k + 1)):
        raise ValueError("the CIGAR set's record or offset tensor is shorter than k asks for")
    cig = (int(cigar_record.data_ptr()), int(cigar_offset.data_ptr()), int(cigar_text.data_ptr())) if k else None
    return _slice_call(ctx, ctx.lib.swg_lift_slice_records_device, rec, int(status.data_ptr()) if status is not None else None,
                       int(regions.data_ptr()), int(n_regions), cig, k, SETS.get(set, set), AXES.get(axes, axes), min_aligned, slice_capacity,
                       text_capacity, want_slices, want_text)


class LiftPaf:
    """BED regions lifted through an open PafFile, every slice as one PAF line with its own coordinates and its sliced cg:Z: (`text`);
    `counts`: a dict of PAF_COUNTS; rows(): the lines split into fields, the numeric PAF columns as int."""

    def __init__(self, text, counts):
        self.text, self.counts = text, counts

    def rows(self):
        out = []
        for ln in self.text.split("\n"):
            if ln:
                f = ln.split("\t")
                out.append(tuple(int(v) if k in (1, 2, 3, 6, 7, 8, 9, 10, 11) else v for k, v in enumerate(f)))
        return out

    @staticmethod
    def _args(paf, status, bed_text, set, axes, ctx):
        ctx = getattr(ctx, "ctx", ctx)
        lib = load()
        bed = bed_text.encode("utf-8", errors="surrogateescape") if isinstance(bed_text, str) else bytes(bed_text)
        rebased = bool(lib.swg_paf_seq_offsets(paf.handle)) or bool(lib.swg_paf_record_offsets(paf.handle, 0))   # (refused by the library)
        if ctx is None and paf.n and bed.strip() and not rebased:
            ctx = default_context()
        st = host_column(status, np.uint8, paf.n, "status", optional=True)
        return lib, ctx.handle if ctx is not None else None, st, bed, SETS.get(set, set), AXES.get(axes, axes)

    @classmethod
    def from_paf(cls, paf, status, bed_text, set="kept", axes="both", min_aligned=1, batch_bytes=0, ctx=None):
        """swg_paf_lift_paf_text.  status None: set must be "all".  ctx as in Lift.from_paf.  batch_bytes: the cost of the regions per
        device call (the CIGAR text of their hits), 0 = the library's default."""
        lib, handle, st, bed, set_, axes_ = cls._args(paf, status, bed_text, set, axes, ctx)
        counts, p, n = SwgLiftPafCounts(), C.c_void_p(), C.c_uint64()
        raise_alnstats(lib, lib.swg_paf_lift_paf_text(handle, paf.handle, addr(st), bed, len(bed), set_, axes_, int(min_aligned), int(batch_bytes),
                                                      C.byref(counts), C.byref(p), C.byref(n)))
        text = C.string_at(p.value, n.value).decode("utf-8", errors="surrogateescape")
        lib.swg_free(p)
        return cls(text, {k: int(getattr(counts, k)) for k in PAF_COUNTS})

    @classmethod
    def write_paf(cls, paf, status, bed_text, path, set="kept", axes="both", min_aligned=1, batch_bytes=0, ctx=None):
        """swg_paf_lift_paf_write: the same into a file -> the counts."""
        lib, handle, st, bed, set_, axes_ = cls._args(paf, status, bed_text, set, axes, ctx)
        counts = SwgLiftPafCounts()
        raise_alnstats(lib, lib.swg_paf_lift_paf_write(handle, paf.handle, addr(st), bed, len(bed), set_, axes_, int(min_aligned), int(batch_bytes),
                                                       str(path).encode(), C.byref(counts)))
        return {k: int(getattr(counts, k)) for k in PAF_COUNTS}
