"""The dot plot on the device (sweepga_amd/csrc/swg_dotplot.hip) against tests/dotplot_model.py: the two record seams against the
model and each other on the hand case of tests/test_dotplot_cpu.py, sub-pixel records around the wavefront and the work-group,
lines around 64 steps and at the largest size, the arithmetic's corners, breadth's shapes under a real 1:1 status, the want bits,
the refusals, a memory limit, and the texts of swg_paf_dotplot / Dotplot.from_paf / --dotplot byte for byte.  Every comparison is
exact: integers and bytes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import dotplot_model as dm
from tests.test_dotplot_cpu import HAND_LAYOUT, REBASED, hand_case, hand_paf, hand_ppm, planes_of
from tests.test_gpu_alnstats import filter_cfgs, gen_text, records_of, run_filter
from tests.test_gpu_breadth import SHAPE_NAMES, shape_texts
from tests.test_gpu_intervals import kept_mask
from tests.test_gpu_wide import Hip

pytestmark = pytest.mark.gpu
ABSENT = dm.ABSENT
COLS = dm.COLS


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


class Dev:
    """A numpy array in device memory with what dotplot_records_device asks of a tensor."""

    def __init__(self, hip, a, dtype):
        self.a = np.ascontiguousarray(a, dtype=dtype)
        self.ptr = hip.up(self.a)

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.a.size

    def element_size(self):
        return self.a.itemsize

    def is_contiguous(self):
        return True


def same_results(a, b):
    return (all((x is None) == (y is None) and (x is None or np.array_equal(x, y)) for x, y in zip(a.planes, b.planes))
            and a.hits == b.hits and a.drawn == b.drawn)


def both_seams(sw, cols, strand, status, x_off, y_off, x_total, y_total, width, height, want=None, ctx=None):
    """The result of the host seam, after checking that the device seam gives the same."""
    from sweepga_amd.dotplot import dotplot_records, dotplot_records_device
    ctx = ctx or sw.default_context()
    got = dotplot_records(ctx, cols, strand, x_off, y_off, x_total, y_total, width, height, status=status, want=want)
    hip = Hip()
    try:
        dcols = {k: Dev(hip, cols[k], np.uint32) for k in COLS}
        dev = dotplot_records_device(ctx, dcols, Dev(hip, strand, np.uint8), Dev(hip, x_off, np.uint64), Dev(hip, y_off, np.uint64), x_total, y_total,
                                     width, height, status=Dev(hip, status, np.uint8) if status is not None else None, want=want)
    finally:
        hip.free()
    assert same_results(dev, got)
    return got


def check(sw, cols, strand, status, x_off, y_off, x_total, y_total, width, height, what="", ctx=None, model=None):
    """Both seams against the model (`model`: its result computed before)."""
    cols = {k: np.asarray(cols[k]).astype(np.uint32) for k in COLS}
    strand = np.asarray(strand).astype(np.uint8)
    got = both_seams(sw, cols, strand, status, x_off, y_off, x_total, y_total, width, height, ctx=ctx)
    planes, hits, drawn = model or dm.dotplot(cols, strand, status, x_off, y_off, x_total, y_total, width, height)
    n_planes = 4 if status is not None else 2
    for p in range(n_planes):
        assert got.planes[p].shape == (height, width) and got.planes[p].dtype == np.uint32
        assert np.array_equal(got.planes[p], planes[p]), (what, p, int((got.planes[p] != planes[p]).sum()))
    assert got.planes[n_planes:] == [None] * (4 - n_planes) and got.hits == hits[:n_planes] + [None] * (4 - n_planes), what
    assert list(got.drawn) == drawn, what
    if status is not None:      # kept <= all, pixel by pixel
        assert (got.planes[2] <= got.planes[0]).all() and (got.planes[3] <= got.planes[1]).all(), what
    return got


def one_axis(total):
    """Sequence 0 alone on both axes."""
    return np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64), total, total


def columns(rows):
    """rows of (q, t, qs, qe, ts, te, strand, status) -> (cols, strand, status)"""
    arr = np.array(rows, dtype=np.int64).reshape(-1, 8)
    return {k: arr[:, i].astype(np.uint32) for i, k in enumerate(COLS)}, arr[:, 6].astype(np.uint8), arr[:, 7].astype(np.uint8)


def axes_for(cols, n_seq, slack=17):
    """Every sequence on both axes in id order, each as long as its records need: (x_off, y_off, x_total, y_total)."""
    ln = np.zeros(n_seq, dtype=np.int64)
    np.maximum.at(ln, cols["q_id"].astype(np.int64), cols["q_end"].astype(np.int64))
    np.maximum.at(ln, cols["t_id"].astype(np.int64), cols["t_end"].astype(np.int64))
    ln += slack
    off = (np.cumsum(ln) - ln).astype(np.uint64)
    return off, off.copy(), int(ln.sum()), int(ln.sum())


def test_hand_case(sw):
    cols, strand, status, x_off, y_off, want, hits, drawn = hand_case()
    got = check(sw, cols, strand, status, x_off, y_off, 80, 50, 8, 6, "hand")
    assert np.array_equal(np.stack(got.planes), planes_of(want)) and got.hits == hits and list(got.drawn) == drawn
    check(sw, cols, strand, None, x_off, y_off, 80, 50, 8, 6, "hand, no status")


# ---- records smaller than a pixel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_records_on_one_pixel(sw, n):
    cols, strand, status = columns([(0, 0, 50, 52, 30, 33, 0, 1)] * n)
    got = check(sw, cols, strand, status, *one_axis(100), 10, 10, "%d on one pixel" % n)
    assert got.planes[0][5, 3] == n == got.planes[2][5, 3] and got.hits == [n, 0, n, 0]


def test_two_pixels_in_turn_and_one_wave_with_all_four_planes(sw):
    rows = [(0, 0, 50, 52, 30, 33, 0, 1) if i % 2 == 0 else (0, 0, 70, 71, 90, 91, 0, 1) for i in range(600)]      # runs of one lane
    got = check(sw, *columns(rows), *one_axis(100), 10, 10, "alternating")
    assert got.planes[0][5, 3] == 300 == got.planes[0][7, 9]
    rows = [(0, 0, 50, 52, 30, 33, i & 1, i >> 1 & 1) for i in range(64)]      # one run of 64 lanes, every plane in it
    got = check(sw, *columns(rows), *one_axis(100), 10, 10, "four planes")
    assert [int(p[5, 3]) for p in got.planes] == [32, 32, 16, 16]
    rows = [(0, 0, 50, 52, 30, 33, (i // 5) & 1, (i // 3) & 1) for i in range(1_000)]      # runs that change plane, four work-groups
    check(sw, *columns(rows), *one_axis(100), 10, 10, "four planes, 1000 records")


def test_a_pixel_shared_across_the_work_group_border_and_more_pixels_than_the_table_holds(sw):
    """512 records, two work-groups of 256: every record on a pixel of its own (more than the staging table takes: the heads that
    find no slot go to the planes directly), but for records 255 and 256, which share one."""
    x = np.arange(512)
    x[256] = 255
    rows = [(0, 0, 7, 8, int(v), int(v) + 1, i % 3 == 0, i % 2) for i, v in enumerate(x)]
    got = check(sw, *columns(rows), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64), 2048, 16, 2048, 16, "border")
    assert int(got.planes[0][7, 255]) + int(got.planes[1][7, 255]) == 2 and sum(got.hits[:2]) == 512
    # 5000 pixels met again and again in a scrambled order: table, overflow and flush together
    rng = np.random.default_rng(5)
    at = rng.integers(0, 5_000, 40_000)
    rows = [(0, 0, int(v) // 100, int(v) // 100 + 1, int(v) % 100, int(v) % 100 + 1, int(s), int(k)) for v, s, k in
            zip(at, rng.integers(0, 2, at.size), rng.integers(0, 2, at.size))]
    check(sw, *columns(rows), *one_axis(100), 100, 100, "scrambled pixels")


# ---- lines ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 63, 64, 65])
def test_lines_around_the_wavefront(sw, L):
    """px(a) = a on 128 x 128 over 128 bases: a diagonal of L + 1 pixels, a falling one that reaches y = 0, a shallow and a steep one."""
    rows = [(0, 0, 3, 3 + L + 1, 5, 5 + L + 1, 0, 1),          # rising: (5, 3) .. (5 + L, 3 + L)
            (0, 0, 0, L + 1, 10, 10 + L + 1, 1, 1),            # falling from y = L down to y = 0
            (0, 0, 20, 20 + L // 3 + 1, 0, L + 1, 0, 0),       # shallow
            (0, 0, 0, L + 1, 40, 40 + L // 2 + 1, 1, 0)]       # steep, falling
    got = check(sw, *columns(rows), *one_axis(128), 128, 128, "L = %d" % L)
    assert got.planes[3][0, 10 + L] == 1 and got.planes[3][L, 10] == 1 and got.planes[2][3 + L, 5 + L] == 1
    assert got.hits == [2 * (L + 1), 2 * (L + 1), L + 1, L + 1]


@pytest.mark.parametrize("shape", [(16384, 2), (2, 16384)])
def test_the_longest_line(sw, shape):
    width, height = shape
    rows = [(0, 0, 0, height, 0, width, 0, 1), (0, 0, 0, height, 0, width, 1, 0)]
    x_off, y_off = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    got = check(sw, *columns(rows), x_off, y_off, width, height, width, height, "L = 16383")
    assert got.hits == [16384, 16384, 16384, 0] and got.planes[0][0, 0] == 1 and got.planes[2][height - 1, width - 1] == 1 and got.planes[1][height - 1, 0] == 1 and got.planes[1][0, width - 1] == 1


def test_300_long_records_crossing_in_one_pixel(sw):
    rows = [(0, 0, 0, 101, 0, 101, i & 1, i % 3 == 0) for i in range(300)]
    got = check(sw, *columns(rows), *one_axis(101), 101, 101, "crossing")
    assert [int(p[50, 50]) for p in got.planes] == [150, 150, 50, 50] and got.planes[0][0, 0] == 150 and got.planes[1][100, 0] == 150


# ---- arithmetic ----------------------------------------------------------------------------------------------------------------
def test_totals_that_do_not_divide_and_fewer_bases_than_pixels(sw):
    rng = np.random.default_rng(11)
    n = 400
    qs, ts = rng.integers(0, 990, n), rng.integers(0, 40, n)
    cols = {"q_id": np.zeros(n), "t_id": np.ones(n), "q_start": qs, "q_end": qs + rng.integers(0, 11, n), "t_start": ts, "t_end": ts + rng.integers(0, 4, n)}
    strand, status = rng.integers(0, 2, n), rng.integers(0, 2, n).astype(np.uint8)
    # y: 1003 bases on 7 rows; x: 43 bases on 64 columns -- several pixels per base, a one-base record is a pixel, two bases a line
    x_off, y_off = np.array([ABSENT, 0], dtype=np.uint64), np.array([0, ABSENT], dtype=np.uint64)
    check(sw, cols, strand, status, x_off, y_off, 43, 1003, 64, 7, "43 on 64, 1003 on 7")
    check(sw, cols, strand, status, x_off, y_off, 43, 1003, 1, 1, "one pixel")
    check(sw, cols, strand, status, x_off, y_off, 4_300, 1_000_003, 33, 129, "wide totals")


def test_offsets_up_to_2_to_the_48_and_the_largest_coordinate(sw):
    top, big = 2**32 - 1, 2**48 - 1
    rows = [(0, 0, top - 6, top, 0, top, 0, 1),            # a coordinate of 2^32 - 1 on both axes
            (1, 1, 0, 1_000, 0, 1_000, 1, 1),              # offset + end = 2^48 - 1: the last pixel
            (1, 1, 999, 1_000, 999, 1_000, 0, 0),
            (1, 0, 0, 1_000, top // 2, top, 0, 1)]
    off = np.array([0, big - 1_000], dtype=np.uint64)
    got = check(sw, *columns(rows), off, off.copy(), big, big, 16384, 3, "2^48 - 1")
    assert got.planes[0][2, 16383] == 1 and got.planes[3][2, 16383] == 1 and got.planes[0][0, 0] == 1
    got = check(sw, *columns(rows), off, off.copy(), big, big, 5, 16384, "2^48 - 1, upright")
    assert got.planes[0][16383, 4] == 1


# ---- shapes --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shapes():
    return shape_texts()


@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_breadths_shapes_under_a_real_filter_status(sw, shapes, shape):
    rng = np.random.default_rng(len(shape))
    with sw.PafFile(text=shapes[shape]) as paf:
        status, _ = run_filter(sw, paf, filter_cfgs(sw)["one_to_one"])
        cols = {c: paf.column(c).copy() for c in COLS}
        strand = paf.column("strand").copy()
        n_seq = int(paf.records.n_seq)
    assert int((status != 0).sum()) > 0
    axes = axes_for(cols, n_seq)
    got = check(sw, cols, strand, status, *axes, 64, 48, shape)
    assert got.drawn[0] > 0 and got.hits[2] + got.hits[3] > 0
    perm = rng.permutation(len(status))
    assert same_results(both_seams(sw, {c: cols[c][perm] for c in COLS}, strand[perm], status[perm], *axes, 64, 48), got)


def test_100000_random_records(sw):
    rng = np.random.default_rng(29)
    n, n_seq = 100_000, 40
    qs, ts = rng.integers(0, 4_000_000, n), rng.integers(0, 4_000_000, n)
    ln = np.where(rng.random(n) < 0.05, rng.integers(0, 3_000_000, n), rng.integers(0, 30_000, n))      # a twentieth crosses several pixels
    cols = {"q_id": rng.integers(0, n_seq, n), "t_id": rng.integers(0, n_seq, n), "q_start": qs, "q_end": qs + ln, "t_start": ts,
            "t_end": ts + (ln * rng.uniform(0.5, 1.5, n)).astype(np.int64)}
    cols = {k: np.asarray(v).astype(np.uint32) for k, v in cols.items()}
    strand, status = (rng.random(n) < 0.3).astype(np.uint8), (rng.random(n) < 0.5).astype(np.uint8)
    x_off, y_off, x_total, y_total = axes_for(cols, n_seq)
    order = np.argsort(np.arange(n_seq) % 5, kind="stable")      # (genome, id) order on y, and a sequence missing from x
    ln_seq = np.diff(np.append(y_off, y_total).astype(np.int64))
    y_off[order] = (np.cumsum(ln_seq[order]) - ln_seq[order]).astype(np.uint64)
    x_off[7] = ABSENT
    got = check(sw, cols, strand, status, x_off, y_off, x_total, y_total, 256, 256, "random")
    assert 0 < got.drawn[1] < got.drawn[0] < n and got.hits[0] + got.hits[1] > got.drawn[0] + 5_000


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def raw_call(sw, ctx, cols, strand, status, x_off, y_off, x_total, y_total, width, height, want, planes):
    from sweepga_amd._lib import SwgDotAxes, SwgDotRequest
    rec = records_of({**cols, "strand": strand}, len(x_off))
    axes = SwgDotAxes(width, height, x_total, y_total, x_off.ctypes.data, y_off.ctypes.data)
    req = SwgDotRequest()
    req.want = want
    for j in range(4):
        req.plane[j] = planes[j].ctypes.data if planes[j] is not None else None
        req.hits[j] = 12345
    req.drawn[0] = req.drawn[1] = 12345
    rc = ctx.lib.swg_dotplot_records(ctx.handle, C.byref(rec), C.byref(axes), status.ctypes.data if status is not None else None, C.byref(req))
    return rc, req


def test_each_want_bit_alone_leaves_the_other_planes_untouched(sw):
    ctx = sw.default_context()
    cols, strand, status, x_off, y_off, want, hits, drawn = hand_case()
    expected = planes_of(want)
    for bits in (1, 2, 4, 8, 5, 0xa, 0xf):
        planes = [np.full((6, 8), 0xabababab, dtype=np.uint32) for _ in range(4)]
        rc, req = raw_call(sw, ctx, cols, strand, status, x_off, y_off, 80, 50, 8, 6, bits, planes)
        assert rc == 0, (bits, ctx.lib.swg_last_error(ctx.handle))
        for j in range(4):
            if bits >> j & 1:
                assert np.array_equal(planes[j], expected[j]) and int(req.hits[j]) == hits[j], (bits, j)
            else:
                assert (planes[j] == 0xabababab).all() and int(req.hits[j]) == 12345, (bits, j)
        assert list(req.drawn) == drawn
    # an unwanted plane may be NULL; the ALL planes need no status
    rc, req = raw_call(sw, ctx, cols, strand, None, x_off, y_off, 80, 50, 8, 6, 3, [np.zeros((6, 8), dtype=np.uint32), np.zeros((6, 8), dtype=np.uint32), None, None])
    assert rc == 0 and list(req.hits) == [10, 4, 12345, 12345] and list(req.drawn) == [5, 0]


def test_refusals_on_the_device(sw):
    ctx = sw.default_context()
    cols, strand, status, x_off, y_off, _, _, _ = hand_case()
    fresh = lambda: [np.full((6, 8), 7, dtype=np.uint32) for _ in range(4)]      # noqa: E731
    args = (cols, strand, status, x_off, y_off, 80, 50, 8, 6, 0xf)
    cases = {"a KEPT bit without status": (cols, strand, None, x_off, y_off, 80, 50, 8, 6, 0x4),
             "want == 0": args[:9] + (0,), "a fifth bit": args[:9] + (0x10,),
             "a total of 0": args[:5] + (0, 50, 8, 6, 0xf), "a total of 2^48": args[:5] + (80, 2**48, 8, 6, 0xf),
             "a width of 0": args[:7] + (0, 6, 0xf), "a height of 16385": args[:7] + (8, 16385, 0xf),
             "a record beyond the x total": args[:5] + (79, 50, 8, 6, 0xf), "a record beyond the y total": args[:5] + (80, 49, 8, 6, 0xf)}
    bad = {c: v.copy() for c, v in cols.items()}
    bad["q_id"][5] = 5      # (a record that is not drawn: the id is refused all the same)
    cases["an id out of range"] = (bad,) + args[1:]
    for what, a in cases.items():
        planes = fresh()
        rc, _ = raw_call(sw, ctx, *a, planes)
        assert rc == -1, what
    rc, _ = raw_call(sw, ctx, *args[:9], 0x3, [np.zeros((6, 8), dtype=np.uint32), None, None, None])
    assert rc == -1      # a wanted plane with a NULL array
    from sweepga_amd._lib import SwgDotRequest
    rc, req = raw_call(sw, ctx, *args, fresh())
    assert rc == 0
    req2 = SwgDotRequest()
    req2.want, req2.reserved = 1, 1
    assert ctx.lib.swg_dotplot_records(ctx.handle, None, None, None, C.byref(req2)) == -1


def test_a_memory_limit_too_small_is_a_clean_oom(sw):
    from sweepga_amd.dotplot import dotplot_records
    ctx = sw.Context(0)
    try:
        cols, strand, status, x_off, y_off, want, hits, drawn = hand_case()
        ctx.set_memory_limit(1 << 20)       # one plane of 1024 x 1024 is 4 MB
        with pytest.raises(sw.SwgError) as e:
            dotplot_records(ctx, cols, strand, x_off, y_off, 80, 50, 1024, 1024, status=status)
        assert e.value.code == -4
        got = dotplot_records(ctx, cols, strand, x_off, y_off, 80, 50, 8, 6, status=status)      # the same context, a call that fits
        assert np.array_equal(np.stack(got.planes), planes_of(want)) and got.hits == hits
        ctx.set_memory_limit(0)
        big = dotplot_records(ctx, cols, strand, x_off, y_off, 80, 50, 1024, 1024, status=status)
        model = dm.dotplot(cols, strand, status, x_off, y_off, 80, 50, 1024, 1024)
        assert np.array_equal(np.stack(big.planes), model[0]) and big.hits == model[1]
    finally:
        ctx.close()


# ---- the texts -----------------------------------------------------------------------------------------------------------------
def test_texts_of_an_open_paf_equal_the_model_rendering(sw):
    text, status = hand_paf()
    with sw.PafFile(text=text) as paf:
        d = sw.Dotplot.from_paf(paf, status, 8, 6)
        assert d.ppm == hand_ppm() and d.layout == HAND_LAYOUT and (d.ppm, d.layout) == dm.paf_texts(text, status != 0, 8, 6)
        assert d.image().shape == (6, 8, 3) and tuple(d.image()[5, 0]) == dm.KEPT_PLUS and tuple(d.image()[0, 7]) == dm.ALL_PLUS
        d = sw.Dotplot.from_paf(paf, status, 8, 6, query_prefix="B#", ctx=sw.default_context())
        assert (d.ppm, d.layout) == dm.paf_texts(text, status != 0, 8, 6, "B#", None)
    text = gen_text(61, 12_000, n_genomes=4, chrs_per_genome=3, span=300_000)
    with sw.PafFile(text=text) as paf:
        status, _ = run_filter(sw, paf, filter_cfgs(sw)["one_to_one"])
        assert 0 < int((status != 0).sum()) < len(status)
        for w, h, qp, tp in ((96, 80, None, None), (50, 77, "g1#", None), (64, 64, "g2#1#chr0", "g0"), (33, 20, None, "g3#1#")):
            d = sw.Dotplot.from_paf(paf, status, w, h, query_prefix=qp, target_prefix=tp)
            ppm, layout = dm.paf_texts(text, status != 0, w, h, qp, tp)
            assert d.layout == layout and d.ppm == ppm and layout.count("\n") > 2, (w, h, qp, tp)
        colours = {tuple(c) for c in d.image().reshape(-1, 3)[::7]} | {tuple(c) for c in sw.Dotplot.from_paf(paf, status, 96, 80).image().reshape(-1, 3)}
        assert {dm.KEPT_PLUS, dm.ALL_PLUS, dm.BORDER, dm.WHITE} <= colours
        only = sw.Dotplot.from_paf(paf, status, 96, 80, layout=False)
        assert only.layout is None and only.ppm == dm.paf_texts(text, status != 0, 96, 80)[0]
    with sw.PafFile(text=REBASED) as paf:
        with pytest.raises(sw.SwgError) as e:
            sw.Dotplot.from_paf(paf, np.ones(1, dtype=np.uint8), 8, 6)
        assert e.value.code == -6 and "2^32" in str(e.value)
    # a record beyond the last-seen length of its sequence
    ln = "\t".join(["a#1#x", "100", "0", "50", "+", "b#1#y", "40", "10", "60", "50", "50", "60"]) + "\n"
    with sw.PafFile(text=ln) as paf:
        with pytest.raises(sw.SwgError) as e:
            sw.Dotplot.from_paf(paf, np.ones(1, dtype=np.uint8), 8, 6)
        assert e.value.code == -1 and "beyond" in str(e.value)


def test_cli_dotplot(sw, tmp_path):
    from sweepga_amd import build
    text = gen_text(71, 15_000, n_genomes=4, chrs_per_genome=3, span=400_000)
    inp = tmp_path / "in.paf"
    inp.write_text(text, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-jump", "10k", "--scaffold-mass", "2k", "--quiet"]
    plain, out, img, lay = (tmp_path / x for x in ("plain.paf", "out.paf", "dot.ppm", "dot.tsv"))
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), *flags], capture_output=True)
    assert r0.returncode == 0 and plain.stat().st_size > 0, r0.stderr
    kept = kept_mask(text, plain.read_bytes().decode())
    for size, w, h, qp, tp in (("96", 96, 96, None, None), ("120x50", 120, 50, "g1#", "g2#1#chr")):
        want = dm.paf_texts(text, kept, w, h, qp, tp)
        prefixes = (["--dotplot-query", qp] if qp else []) + (["--dotplot-target=" + tp] if tp else [])
        for given in ((("image", "layout"),) if qp is None else (("image",), ("layout",), ("image", "layout"))):
            for p in (out, img, lay):
                p.unlink(missing_ok=True)
            extra = (["--dotplot", str(img)] if "image" in given else []) + (["--dotplot-layout", str(lay)] if "layout" in given else [])
            r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), *extra, "--dotplot-size", size, *prefixes, *flags], capture_output=True)
            assert r.returncode == 0 and r.stdout == b"" and out.read_bytes() == plain.read_bytes(), r.stderr     # the PAF does not change
            assert img.exists() == ("image" in given) and lay.exists() == ("layout" in given)
            assert "image" not in given or img.read_bytes() == want[0]
            assert "layout" not in given or lay.read_text() == want[1]
    # the default size, and the layout on standard error
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--dotplot", str(img), "--dotplot-layout", "-", *flags], capture_output=True)
    big = dm.paf_texts(text, kept, 2048, 2048)
    assert r.returncode == 0 and r.stderr.decode() == big[1] and img.read_bytes() == big[0] and out.read_bytes() == plain.read_bytes()
    # --no-filter: every line to standard output, the device is opened, kept = all
    r = subprocess.run([build.CLI, str(inp), "--no-filter", "--dotplot", str(img), "--dotplot-layout", str(lay), "--dotplot-size", "64x40"], capture_output=True)
    every = dm.paf_texts(text, np.ones(len(kept), dtype=bool), 64, 40)
    assert r.returncode == 0 and r.stdout == text.encode() and img.read_bytes() == every[0] and lay.read_text() == every[1]
    # rebased columns: refused right after the parse
    wide = tmp_path / "wide.paf"
    wide.write_text(REBASED)
    img.unlink()
    r = subprocess.run([build.CLI, str(wide), "--output-file", str(out), "--dotplot", str(img)], capture_output=True, text=True)
    assert r.returncode == 3 and "2^32" in r.stderr and not img.exists()


def test_smallest_shapes_on_a_fresh_context(sw):
    """The seams around the kernels at the smallest shapes -- one record; three records of one sequence pair in one chain -- on a
    context of its own: its first call sizes the arena from the input, the later ones find it sized.  Each shape twice, host seam
    against device seam byte for byte and both against the model."""
    rows = [(0, 1, 10, 110, 20, 125, 0, 1), (0, 1, 200, 300, 210, 310, 1, 1), (0, 1, 400, 450, 420, 470, 0, 1)]
    x_off, y_off = np.array([0, 1000], dtype=np.uint64), np.array([0, 1000], dtype=np.uint64)
    ctx = sw.Context(0)
    try:
        for n in (1, 3, 1, 3):
            cols, strand, kept = columns(rows[:n])
            for status in (None, kept):   # (None: the optional column stays NULL on its way to the device)
                got = check(sw, cols, strand, status, x_off, y_off, 2000, 2000, 8, 6, f"n = {n}", ctx=ctx)
                assert list(got.drawn) == [n, n if status is not None else 0]
    finally:
        ctx.close()
