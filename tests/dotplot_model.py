"""The dot plot of DESIGN.md section 22 as a plain loop per record and per step, straight from the definitions: Python integers,
one `+= 1` per pixel.  No staging table, no lane runs, no list of long records; the image and the layout table are built here too,
from the PAF text alone.  Shares no code with the product."""
import numpy as np

ABSENT = 2**64 - 1
COLS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")
HEADER = "axis\tsequence\tgenome\toffset\tlength\tfirst_pixel\tlast_pixel\n"
KEPT_MINUS, KEPT_PLUS, ALL_MINUS, ALL_PLUS, BORDER, WHITE = (200, 30, 30), (0, 0, 0), (245, 190, 190), (190, 190, 190), (225, 232, 245), (255, 255, 255)


def record_pixels(x0, x1, ya, yb, minus):
    """The pixel list of one record from its four endpoint pixels."""
    y0, y1 = (yb, ya) if minus else (ya, yb)
    dx, dy = x1 - x0, abs(y1 - y0)
    L = max(dx, dy)
    if L == 0:
        return [(x0, y0)]
    sign = -1 if minus else 1
    return [(x0 + (2 * k * dx + L) // (2 * L), y0 + sign * ((2 * k * dy + L) // (2 * L))) for k in range(L + 1)]


def dotplot(cols, strand, status, x_off, y_off, x_total, y_total, width, height):
    """-> (planes uint32 [4, height, width], hits [4], drawn [2]); status None: the KEPT planes stay empty."""
    planes = np.zeros((4, height, width), dtype=np.uint32)
    drawn = [0, 0]
    c = {k: [int(v) for v in cols[k]] for k in COLS}
    for i in range(len(c["q_id"])):
        q, t, qs, qe, ts, te = (c[k][i] for k in COLS)
        xo, yo = int(x_off[t]), int(y_off[q])
        if qe <= qs or te <= ts or xo == ABSENT or yo == ABSENT:
            continue
        assert xo + te <= x_total and yo + qe <= y_total, "record %d ends beyond its axis" % i
        minus = 1 if int(strand[i]) else 0
        kept = status is not None and int(status[i]) != 0
        px = record_pixels((xo + ts) * width // x_total, (xo + te - 1) * width // x_total, (yo + qs) * height // y_total,
                           (yo + qe - 1) * height // y_total, minus)
        assert len(set(px)) == len(px)      # a record touches a pixel at most once
        drawn[0] += 1
        drawn[1] += kept
        for x, y in px:
            planes[minus, y, x] += 1
            if kept:
                planes[2 + minus, y, x] += 1
    return planes, [int(planes[p].astype(np.uint64).sum()) for p in range(4)], drawn


# ---- the texts ------------------------------------------------------------------------------------------------------------------
def parse(text):
    """PAF text -> (cols, strand, names, seq_genome, genome names, last-seen lengths): lines with at least 11 fields; sequence ids
    in order of first appearance (a line's query before its target), genome = the name up to and including its last '#', genome ids
    in sequence-id order."""
    ids, lengths, rows, strand = {}, {}, [], []
    for ln in text.split("\n"):
        f = ln.rstrip("\r").split("\t")
        if len(f) < 11:
            continue
        for nm in (f[0], f[5]):
            ids.setdefault(nm, len(ids))
        lengths[f[0]] = int(f[1])
        lengths[f[5]] = int(f[6])       # (the target column has the last word)
        rows.append((ids[f[0]], ids[f[5]], int(f[2]), int(f[3]), int(f[7]), int(f[8])))
        strand.append(0 if f[4] == "+" else 1)
    names, gids, seq_genome = list(ids), {}, []
    for nm in names:
        p = nm.rfind("#")
        seq_genome.append(gids.setdefault(nm if p < 0 else nm[:p + 1], len(gids)))
    arr = np.array(rows, dtype=np.int64).reshape(-1, 6)
    return {k: arr[:, j] for j, k in enumerate(COLS)}, strand, names, seq_genome, list(gids), [lengths[nm] for nm in names]


def axis_of(ids_on_axis, names, seq_genome, lengths, prefix):
    """[(seq, offset, length)] in axis order, and the total."""
    chosen = sorted((seq_genome[s], s) for s in set(int(v) for v in ids_on_axis) if not prefix or names[s].startswith(prefix))
    out, total = [], 0
    for _, s in chosen:
        out.append((s, total, lengths[s]))
        total += lengths[s]
    return out, total


def paf_texts(text, kept, width, height, query_prefix=None, target_prefix=None):
    """(ppm bytes, layout str) of a PAF text; kept: a boolean mask over its records."""
    cols, strand, names, seq_genome, genomes, lengths = parse(text)
    head = b"P6\n%d %d\n255\n" % (width, height)
    white = head + b"\xff" * (3 * width * height)
    if len(strand) == 0:
        return white, HEADER
    ax, x_total = axis_of(cols["t_id"], names, seq_genome, lengths, target_prefix)
    ay, y_total = axis_of(cols["q_id"], names, seq_genome, lengths, query_prefix)
    if x_total == 0 or y_total == 0:
        return white, HEADER
    layout = [HEADER]
    for tag, axis, total, side in (("x", ax, x_total, width), ("y", ay, y_total, height)):
        for s, off, ln in axis:
            first = min(off, total - 1) * side // total
            last = (off + ln - 1) * side // total if ln else first
            layout.append("%s\t%s\t%s\t%d\t%d\t%d\t%d\n" % (tag, names[s], genomes[seq_genome[s]], off, ln, first, last))
    x_off, y_off = [ABSENT] * len(names), [ABSENT] * len(names)
    for s, off, _ in ax:
        x_off[s] = off
    for s, off, _ in ay:
        y_off[s] = off
    planes, _, _ = dotplot(cols, strand, np.asarray(kept).astype(np.uint8), x_off, y_off, x_total, y_total, width, height)
    p = planes.astype(np.int64)
    img = np.empty((height, width, 3), dtype=np.uint8)
    img[:] = WHITE
    for tag, axis, total, side in (("x", ax, x_total, width), ("y", ay, y_total, height)):
        for k in range(1, len(axis)):
            if seq_genome[axis[k][0]] != seq_genome[axis[k - 1][0]] and axis[k][1] < total:
                at = axis[k][1] * side // total
                if tag == "x":
                    img[:, at] = BORDER
                else:
                    img[at, :] = BORDER
    any_all, any_kept = (p[0] + p[1]) > 0, (p[2] + p[3]) > 0
    img[any_all] = ALL_PLUS
    img[any_all & (p[1] > p[0])] = ALL_MINUS
    img[any_kept] = KEPT_PLUS
    img[any_kept & (p[3] > p[2])] = KEPT_MINUS
    return head + img[::-1].tobytes(), "".join(layout)      # (image row r is y = H - 1 - r)
