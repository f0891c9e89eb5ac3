"""The dot plot seen from Python: the records of a filter call rasterised on the device (csrc/swg_dotplot.hip) into four uint32
count planes -- all '+', all '-', kept '+', kept '-' -- over two concatenated axes (x = targets, y = queries).  dotplot_records /
dotplot_records_device are the two record seams, Dotplot.from_paf the image and the layout table of an open PafFile."""
import ctypes as C

import numpy as np

from ._lib import SwgDotAxes, SwgDotRequest, SwgDotView, default_context, load
from ._marshal import addr, host_column, raise_alnstats, records_from_numpy, records_from_tensors, take_texts, text_slots

COLUMNS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")
ABSENT = 2**64 - 1
ALL_PLUS, ALL_MINUS, KEPT_PLUS, KEPT_MINUS = 1, 2, 4, 8
MAX_SIDE = 16384


class DotplotResult:
    """planes: a list of four (height, width) uint32 arrays, row y = 0 at the axis origin, None where the plane's bit was not asked
    for ([all+, all-, kept+, kept-]); hits: their sums (None likewise); drawn: (drawn records, drawn kept records)."""

    def __init__(self, planes, hits, drawn):
        self.planes, self.hits, self.drawn = planes, hits, drawn


def _call(ctx, fn, rec, width, height, x_total, y_total, x_addr, y_addr, status_addr, want):
    width, height, want = int(width), int(height), int(want)
    axes = SwgDotAxes(width, height, int(x_total), int(y_total), x_addr, y_addr)
    req = SwgDotRequest()
    req.want = want
    planes = [None] * 4
    if 1 <= width <= MAX_SIDE and 1 <= height <= MAX_SIDE:      # (anything else is the library's to refuse)
        for j in range(4):
            if want >> j & 1:
                planes[j] = np.empty((height, width), dtype=np.uint32)
                req.plane[j] = planes[j].ctypes.data
    ctx.check(fn(ctx.handle, C.byref(rec), C.byref(axes), status_addr, C.byref(req)))
    hits = [int(req.hits[j]) if planes[j] is not None else None for j in range(4)]
    return DotplotResult(planes, hits, (int(req.drawn[0]), int(req.drawn[1])))


def dotplot_records(ctx, records, strand, x_off, y_off, x_total, y_total, width, height, status=None, want=None):
    """swg_dotplot_records.  `records`: a dict of numpy columns (q_id, t_id, q_start, q_end, t_start, t_end); strand: uint8 per
    record (0 = '+'); x_off / y_off: uint64 per sequence id (ABSENT = not on the axis).  want: the bit mask (ALL_PLUS | ALL_MINUS |
    KEPT_PLUS | KEPT_MINUS) or None = everything the status allows.  Returns a DotplotResult."""
    x_off = np.ascontiguousarray(x_off, dtype=np.uint64)
    y_off = np.ascontiguousarray(y_off, dtype=np.uint64)
    if x_off.size != y_off.size:
        raise ValueError("x_off and y_off differ in length")
    rec, keep = records_from_numpy(records, COLUMNS, x_off.size, strand=strand)   # (keep: alive until the call is over)
    if any(a.size != int(rec.n) for a in keep):
        raise ValueError("the columns and strand differ in length")
    st = host_column(status, np.uint8, int(rec.n), "status", optional=True)
    if want is None:
        want = 0xf if st is not None else ALL_PLUS | ALL_MINUS
    return _call(ctx, ctx.lib.swg_dotplot_records, rec, width, height, x_total, y_total, x_off.ctypes.data if x_off.size else None,
                 y_off.ctypes.data if y_off.size else None, addr(st), want)


def dotplot_records_device(ctx, columns, strand, x_off, y_off, x_total, y_total, width, height, status=None, want=None):
    """swg_dotplot_records_device over torch tensors on ctx's GPU: `columns` maps q_id, t_id, q_start, q_end, t_start, t_end to
    contiguous 4-byte tensors of one length, strand and status (or None) are 1-byte tensors with an entry per record, x_off and
    y_off 8-byte tensors of n_seq entries.  (Anything with .data_ptr(), .numel() and .element_size() works; the caller keeps the
    tensors alive and their work finished.)  The planes come back as numpy arrays on the host."""
    rec = records_from_tensors(columns, {k: 4 for k in COLUMNS}, x_off.numel())
    for name, t in (("strand", strand), ("status", status)):
        if t is not None and (t.element_size() != 1 or int(t.numel()) < int(rec.n)):
            raise ValueError(f"{name} must be 1-byte with an entry per record")
    if x_off.element_size() != 8 or y_off.element_size() != 8 or int(x_off.numel()) != int(y_off.numel()):
        raise ValueError("x_off and y_off must be 8-byte tensors of one length")
    rec.strand = int(strand.data_ptr())
    if want is None:
        want = 0xf if status is not None else ALL_PLUS | ALL_MINUS
    return _call(ctx, ctx.lib.swg_dotplot_records_device, rec, width, height, x_total, y_total, int(x_off.data_ptr()), int(y_off.data_ptr()),
                 int(status.data_ptr()) if status is not None else None, want)


class Dotplot:
    """The dot plot of an open PafFile: `ppm` (bytes: a binary PPM, origin bottom-left; kept mappings black, kept inversions red,
    dropped ones grey and pink, genome borders pale blue) and `layout` (str: axis, sequence, genome, offset, length, first_pixel,
    last_pixel per sequence of either axis); None where not asked for."""

    def __init__(self, ppm, layout, width, height):
        self.ppm, self.layout, self.width, self.height = ppm, layout, width, height

    def image(self):
        """The pixels as an (H, W, 3) uint8 array, row 0 = the top of the image."""
        head = b"P6\n%d %d\n255\n" % (self.width, self.height)
        if self.ppm is None or not self.ppm.startswith(head):
            raise ValueError("no image")
        return np.frombuffer(self.ppm, dtype=np.uint8, offset=len(head)).reshape(self.height, self.width, 3)

    @classmethod
    def from_paf(cls, paf, status, width, height=None, query_prefix=None, target_prefix=None, ctx=None, image=True, layout=True):
        """swg_paf_dotplot: both texts from one device call.  ctx: a Context, anything with a `.ctx` (PafFilter), or None = the
        default context, which is only opened when the image of a PAF with records is asked for."""
        ctx = getattr(ctx, "ctx", ctx)
        lib = load()
        height = width if height is None else height
        if ctx is None and image and paf.n:
            ctx = default_context()
        st = host_column(status, np.uint8, paf.n, "status", optional=True)
        view = SwgDotView(int(width), int(height), query_prefix.encode() if query_prefix else None, target_prefix.encode() if target_prefix else None)
        p, n = text_slots((image, layout))
        rc = lib.swg_paf_dotplot(ctx.handle if ctx is not None else None, paf.handle, addr(st), C.byref(view), p, n)
        raise_alnstats(lib, rc)
        text = take_texts(lib, p, n, (image, layout))
        return cls(text[0], text[1].decode("utf-8", errors="surrogateescape") if text[1] is not None else None, int(width), int(height))
