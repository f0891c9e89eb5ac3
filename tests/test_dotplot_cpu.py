"""The dot plot without a GPU: the model of tests/dotplot_model.py against pixels worked out by hand, and the host side of the
feature -- header, ctypes mirrors, exported symbols, the refusals that need no device, a record-free PAF, an empty axis, prefix
selection through the layout table, the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import dotplot_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABSENT = dm.ABSENT
T0, T1, Q0, Q1, Z = 0, 1, 2, 3, 4
HAND_NAMES = {T0: "A#1#t0", T1: "B#1#t1", Q0: "A#1#q0", Q1: "B#1#q1", Z: "C#1#z"}
HAND_LEN = {T0: 50, T1: 30, Q0: 30, Q1: 20, Z: 40}


def hand_case():
    """An 8 x 6 image over totals 80 (x: t0 of 50 bases, then t1 of 30) and 50 (y: q0 of 30, then q1 of 20): px(a) = a // 10,
    py(a) = 6 a // 50, so the rows begin at a = 0, 9, 17, 25, 34, 42.  Sequence z is on neither axis.
    -> (cols, strand, status, x_off, y_off, expected {plane: set of (x, y)}, hits, drawn), all worked out by hand."""
    rows = [
        # (q, t, qs, qe, ts, te, strand, status)
        (Q0, T0, 0, 30, 0, 50, 0, 1),     # 0 rising, shallow: x 0 .. 4, y 0 .. 3, L = 4; y = (6 k + 4) // 8 = 0 1 2 2 3 -- at k = 2 the
                                          #   numerator 16 divides exactly: 1.5 rounds up to 2
        (Q1, T1, 0, 20, 0, 30, 1, 0),     # 1 falling, dropped: x 5 .. 7, y from 5 down to 3, L = 2
        (Q0, T1, 0, 30, 0, 12, 0, 1),     # 2 steep: x 5 .. 6, y 0 .. 3, L = 3; x = 5 + (2 k + 3) // 6 = 5 5 6 6
        (Q0, T0, 10, 12, 20, 25, 1, 1),   # 3 smaller than a pixel, '-', kept: (2, 1)
        (Q1, T1, 15, 20, 25, 30, 0, 0),   # 4 ends on the last base of both axes: (7, 5)
        (Q0, T0, 5, 5, 5, 9, 0, 1),       # 5 zero length on the query: not drawn
        (Z, T0, 0, 10, 0, 10, 0, 1),      # 6 its query is on no axis: not drawn
        (Q0, Q1, 0, 10, 0, 10, 0, 1),     # 7 its target is a sequence of the y axis only: not drawn
    ]
    arr = np.array(rows, dtype=np.int64)
    cols = {k: arr[:, i].astype(np.uint32) for i, k in enumerate(dm.COLS)}
    x_off = np.array([0, 50, ABSENT, ABSENT, ABSENT], dtype=np.uint64)
    y_off = np.array([ABSENT, ABSENT, 0, 30, ABSENT], dtype=np.uint64)
    r0, r2 = {(0, 0), (1, 1), (2, 2), (3, 2), (4, 3)}, {(5, 0), (5, 1), (6, 2), (6, 3)}
    want = {0: r0 | r2 | {(7, 5)}, 1: {(5, 5), (6, 4), (7, 3), (2, 1)}, 2: r0 | r2, 3: {(2, 1)}}
    return cols, arr[:, 6].astype(np.uint8), arr[:, 7].astype(np.uint8), x_off, y_off, want, [10, 4, 9, 1], [5, 3]


def planes_of(want, width=8, height=6):
    out = np.zeros((4, height, width), dtype=np.uint32)
    for p, pixels in want.items():
        for x, y in pixels:
            out[p, y, x] += 1
    return out


def hand_paf():
    """The drawn records of the hand case and its zero-length one as PAF text: q0, t0, q1, t1 intern as 0 .. 3, genomes A and B, so
    the axes come out as in hand_case.  -> (text, status)"""
    cols, strand, status, _, _, _, _, _ = hand_case()
    lines = []
    for k in range(6):
        q, t = int(cols["q_id"][k]), int(cols["t_id"][k])
        lines.append("\t".join([HAND_NAMES[q], str(HAND_LEN[q]), str(cols["q_start"][k]), str(cols["q_end"][k]), "-" if strand[k] else "+",
                                HAND_NAMES[t], str(HAND_LEN[t]), str(cols["t_start"][k]), str(cols["t_end"][k]), "10", "20", "60"]))
    return "\n".join(lines) + "\n", status[:6]


# the image of hand_paf(), top row (y = 5) first: K kept '+', R kept '-', g dropped '+', p dropped '-', b a genome border (column
# px(50) = 5, row py(30) = 3), . white
HAND_IMAGE = (".....p.g",
              ".....bp.",
              "bbbbKbKp",
              "..KK.bK.",
              ".KR..K..",
              "K....K..")
COLOUR = {"K": dm.KEPT_PLUS, "R": dm.KEPT_MINUS, "g": dm.ALL_PLUS, "p": dm.ALL_MINUS, "b": dm.BORDER, ".": dm.WHITE}
HAND_LAYOUT = (dm.HEADER + "x\tA#1#t0\tA#1#\t0\t50\t0\t4\n" + "x\tB#1#t1\tB#1#\t50\t30\t5\t7\n" +
               "y\tA#1#q0\tA#1#\t0\t30\t0\t3\n" + "y\tB#1#q1\tB#1#\t30\t20\t3\t5\n")


def hand_ppm():
    return b"P6\n8 6\n255\n" + bytes(v for row in HAND_IMAGE for ch in row for v in COLOUR[ch])


def test_model_against_pixels_worked_out_by_hand():
    cols, strand, status, x_off, y_off, want, hits, drawn = hand_case()
    planes, got_hits, got_drawn = dm.dotplot(cols, strand, status, x_off, y_off, 80, 50, 8, 6)
    assert np.array_equal(planes, planes_of(want)) and got_hits == hits and got_drawn == drawn
    assert (planes[2:] <= planes[:2]).all()
    none, h, d = dm.dotplot(cols, strand, None, x_off, y_off, 80, 50, 8, 6)
    assert np.array_equal(none[:2], planes[:2]) and not none[2:].any() and h == [10, 4, 0, 0] and d == [5, 0]
    # the steps: the rounding tie, a single pixel, a falling line
    assert dm.record_pixels(0, 4, 0, 3, 0) == [(0, 0), (1, 1), (2, 2), (3, 2), (4, 3)]
    assert dm.record_pixels(5, 7, 3, 5, 1) == [(5, 5), (6, 4), (7, 3)] and dm.record_pixels(2, 2, 1, 1, 1) == [(2, 1)]


def test_model_texts_against_an_image_written_out():
    text, status = hand_paf()
    ppm, layout = dm.paf_texts(text, status != 0, 8, 6)
    assert layout == HAND_LAYOUT and ppm == hand_ppm()
    ppm, layout = dm.paf_texts(text, status != 0, 8, 6, query_prefix="B#")      # q1 alone on y: total 20, py(a) = 6 a // 20
    assert layout == dm.HEADER + HAND_LAYOUT.split("\n", 3)[1] + "\n" + HAND_LAYOUT.split("\n", 3)[2] + "\n" + "y\tB#1#q1\tB#1#\t0\t20\t0\t5\n"
    img = np.frombuffer(ppm, dtype=np.uint8, offset=11).reshape(6, 8, 3)[::-1]
    assert tuple(img[5, 5]) == dm.ALL_MINUS and tuple(img[0, 7]) == dm.ALL_MINUS and tuple(img[4, 7]) == dm.ALL_PLUS and tuple(img[0, 0]) == dm.WHITE
    assert dm.paf_texts(text, status != 0, 3, 2, query_prefix="nothing") == (b"P6\n3 2\n255\n" + b"\xff" * 18, dm.HEADER)


@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib, dotplot
    structs = (("swg_dot_axes", _lib.SwgDotAxes), ("swg_dot_request", _lib.SwgDotRequest), ("swg_dot_view", _lib.SwgDotView))
    prints = ['printf("%%zu\\n", sizeof(%s));' % name for name, _ in structs]
    prints += ['printf("%%zu\\n", offsetof(%s, %s));' % (name, f) for name, cls in structs for f, _ in cls._fields_]
    prints += ['printf("%u %u %u %u\\n", SWG_DOT_ALL_PLUS, SWG_DOT_ALL_MINUS, SWG_DOT_KEPT_PLUS, SWG_DOT_KEPT_MINUS);',
               'printf("%d\\n", SWG_DOT_ABSENT == 0xffffffffffffffffull);']
    prints += ['printf("%%zu\\n", sizeof(%s));' % s for s in ("swg_records", "swg_sharing_request")]
    prints.append('printf("%d\\n", SWG_ABI_VERSION);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(cls) for _, cls in structs] + [getattr(cls, f).offset for _, cls in structs for f, _ in cls._fields_]
    want += [1, 2, 4, 8, 1, 128, 88, 1]      # the structures that existed before keep their sizes
    assert got == want
    assert got[:3] == [40, 88, 24]
    # no implicit padding: the fields fill each structure
    for _, cls in structs:
        assert sum(C.sizeof(t) for _, t in cls._fields_) == C.sizeof(cls)
    assert (dotplot.ALL_PLUS, dotplot.ALL_MINUS, dotplot.KEPT_PLUS, dotplot.KEPT_MINUS, dotplot.ABSENT) == (1, 2, 4, 8, 2**64 - 1)


def test_symbols_are_exported_and_declared(lib):
    import sweepga_amd
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_dotplot_records", "swg_dotplot_records_device", "swg_paf_dotplot"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    assert lib.swg_abi_version() == 1
    for name in ("Dotplot", "DotplotResult", "dotplot_records", "dotplot_records_device"):
        assert hasattr(sweepga_amd, name)


def slots(image=True, layout=True):
    marker = C.create_string_buffer(1)
    p = (C.c_void_p * 2)()
    p[0], p[1] = (C.addressof(marker) if image else None), (C.addressof(marker) if layout else None)
    return p, (C.c_uint64 * 2)(7, 7), marker


REBASED = "\t".join(["a#1#x", str(2**33), str(2**32), str(2**32 + 50), "+", "b#1#y", "900", "10", "60", "50", "50", "60"]) + "\n"


def test_refusals_that_need_no_device(lib):
    from sweepga_amd import Dotplot, PafFile, SwgError, _lib
    cols, strand, status, x_off, y_off, _, _, _ = hand_case()
    rec = _lib.SwgRecords()
    rec.n = len(status)
    for k, a in cols.items():
        setattr(rec, k, a.ctypes.data)
    rec.strand = strand.ctypes.data
    rec.n_seq = len(x_off)
    axes = _lib.SwgDotAxes(8, 6, 80, 50, x_off.ctypes.data, y_off.ctypes.data)
    poison = np.full(48, 0xabababab, dtype=np.uint32)
    for fn in (lib.swg_dotplot_records, lib.swg_dotplot_records_device):     # a NULL context: there is no CPU path
        req = _lib.SwgDotRequest()
        req.want = 0xf
        for j in range(4):
            req.plane[j] = poison.ctypes.data
            req.hits[j] = 12345
        assert fn(None, C.byref(rec), C.byref(axes), status.ctypes.data, C.byref(req)) == -1
        assert (poison == 0xabababab).all() and list(req.hits) == [12345] * 4
    text, st = hand_paf()
    st = np.ascontiguousarray(st)
    with PafFile(text=text) as paf:
        view = _lib.SwgDotView(8, 6, None, None)
        p, n, _m = slots()
        assert lib.swg_paf_dotplot(None, paf.handle, st.ctypes.data, C.byref(view), p, n) == -1 and not p[0] and not p[1] and list(n) == [0, 0]
        assert b"NULL context" in lib.swg_alnstats_last_error()
        p, n, _m = slots()
        assert lib.swg_paf_dotplot(None, paf.handle, None, C.byref(view), p, n) == -1 and b"status" in lib.swg_alnstats_last_error()
        p, n, _m = slots(False, False)
        assert lib.swg_paf_dotplot(None, paf.handle, st.ctypes.data, C.byref(view), p, n) == -1
        p, n, _m = slots()
        assert lib.swg_paf_dotplot(None, paf.handle, st.ctypes.data, None, p, n) == -1
        assert lib.swg_paf_dotplot(None, paf.handle, st.ctypes.data, C.byref(view), None, n) == -1
        assert lib.swg_paf_dotplot(None, None, st.ctypes.data, C.byref(view), p, n) == -1
        for w, h in ((0, 6), (8, 0), (16385, 6), (8, 16385)):
            p, n, _m = slots(False, True)
            assert lib.swg_paf_dotplot(None, paf.handle, st.ctypes.data, C.byref(_lib.SwgDotView(w, h, None, None)), p, n) == -1
            assert b"16384" in lib.swg_alnstats_last_error() and not p[1]
    with PafFile(text=REBASED) as paf:       # rebased columns: refused before a context is looked at
        with pytest.raises(SwgError) as e:
            Dotplot.from_paf(paf, np.ones(1, dtype=np.uint8), 8, 6, image=False)
        assert e.value.code == -6 and "2^32" in str(e.value)


def test_record_free_paf_empty_axis_and_prefixes_without_a_device(lib):
    from sweepga_amd import Dotplot, PafFile
    white = b"P6\n5 3\n255\n" + b"\xff" * 45
    for text in ("", "# nothing\nfew\tfields\n"):
        with PafFile(text=text) as paf:
            assert paf.n == 0
            d = Dotplot.from_paf(paf, np.zeros(0, dtype=np.uint8), 5, 3)
            assert (d.ppm, d.layout) == (white, dm.HEADER) == dm.paf_texts(text, np.zeros(0, dtype=bool), 5, 3)
            assert d.image().shape == (3, 5, 3) and (d.image() == 255).all()
            only = Dotplot.from_paf(paf, np.zeros(0, dtype=np.uint8), 5, 3, layout=False)
            assert only.layout is None and only.ppm == white
    text, status = hand_paf()
    lib_ = lib
    with PafFile(text=text) as paf:
        st = np.ascontiguousarray(status)
        # an axis that a prefix leaves empty: all white, the header alone, and no context is asked for
        from sweepga_amd import _lib
        for qp, tp in ((b"nothing", None), (None, b"C#"), (b"zz", b"zz")):
            p, n, _m = slots()
            assert lib_.swg_paf_dotplot(None, paf.handle, st.ctypes.data, C.byref(_lib.SwgDotView(5, 3, qp, tp)), p, n) == 0
            got = (C.string_at(p[0], n[0]), C.string_at(p[1], n[1]).decode())
            lib_.swg_free(C.c_void_p(p[0]))
            lib_.swg_free(C.c_void_p(p[1]))
            assert got == (white, dm.HEADER) == dm.paf_texts(text, status != 0, 5, 3, qp.decode() if qp else None, tp.decode() if tp else None)
        # the layout alone needs no device: prefix selection against the model and against the table written out
        assert Dotplot.from_paf(paf, status, 8, 6, image=False).layout == HAND_LAYOUT
        for qp, tp, w, h in ((None, None, 8, 6), ("B#", None, 8, 6), (None, "A#1#t", 7, 5), ("A", "B", 16384, 1), ("", "", 2048, 2048)):
            d = Dotplot.from_paf(paf, status, w, h, query_prefix=qp, target_prefix=tp, image=False)
            assert d.ppm is None and d.layout == dm.paf_texts(text, status != 0, w, h, qp, tp)[1], (qp, tp)
        assert Dotplot.from_paf(paf, status, 8, 6, query_prefix="B#", image=False).layout.endswith("y\tB#1#q1\tB#1#\t0\t20\t0\t5\n")
    # sequences ordered by (genome, id), lengths by the last-seen rule, a sequence of length 0
    lines = [("b#2", 70, "a#1", 100), ("a#2", 30, "b#1", 60), ("b#2", 75, "a#3", 0), ("a#2", 30, "b#1", 64)]
    text = "".join("\t".join([q, str(ql), "0", "0", "+", t, str(tl), "0", "0", "1", "1", "60"]) + "\n" for q, ql, t, tl in lines)
    with PafFile(text=text) as paf:
        got = Dotplot.from_paf(paf, np.ones(4, dtype=np.uint8), 10, 10, image=False).layout
    assert got == dm.paf_texts(text, np.ones(4, dtype=bool), 10, 10)[1]
    # (genome b# is met first: id 0; x holds 164 bases, y 105)
    assert got == (dm.HEADER + "x\tb#1\tb#\t0\t64\t0\t3\n" + "x\ta#1\ta#\t64\t100\t3\t9\n" + "x\ta#3\ta#\t164\t0\t9\t9\n" +
                   "y\tb#2\tb#\t0\t75\t0\t7\n" + "y\ta#2\ta#\t75\t30\t7\t9\n")


def test_command_line_lists_the_flags_and_wants_values(lib):
    from sweepga_amd import build
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--dotplot FILE", "--dotplot-size N|WxH", "--dotplot-layout FILE", "--dotplot-query PREFIX", "--dotplot-target PREFIX"):
        assert flag in r.stdout, flag
    for flag in ("--dotplot", "--dotplot-size", "--dotplot-layout", "--dotplot-query", "--dotplot-target"):
        r = subprocess.run([build.CLI, "in.paf", "--dotplot", "x.ppm", flag + "="], capture_output=True, text=True)
        assert r.returncode == 2 and "empty value for " + flag in r.stderr, (flag, r.stderr)
        r = subprocess.run([build.CLI, "in.paf", flag], capture_output=True, text=True)
        assert r.returncode == 2 and flag in r.stderr
    for bad in ("0", "16385", "abc", "10x", "x10", "10x0", "8x6x4", "-5", "1e3", "20 48"):
        r = subprocess.run([build.CLI, "in.paf", "--dotplot", "x.ppm", "--dotplot-size=" + bad], capture_output=True, text=True)
        assert r.returncode == 2 and "invalid value for --dotplot-size" in r.stderr, (bad, r.stderr)
    for flag, v in (("--dotplot-size", "64"), ("--dotplot-query", "a"), ("--dotplot-target", "a")):
        r = subprocess.run([build.CLI, "in.paf", flag, v], capture_output=True, text=True)
        assert r.returncode == 2 and "need --dotplot" in r.stderr
    r = subprocess.run([build.CLI, "in.paf", "--dotplot", "-"], capture_output=True, text=True)
    assert r.returncode == 2 and "binary image" in r.stderr


def test_command_line_refuses_64_bit_columns_before_it_filters(lib, tmp_path):
    """A value >= 2^32 rebases the columns; the dot plot flags say so right after the parse -- exit 3 -- and nothing is begun."""
    from sweepga_amd import build
    inp, out, rep = tmp_path / "in.paf", tmp_path / "out.paf", tmp_path / "dot.out"
    inp.write_text(REBASED)
    for flag in ("--dotplot", "--dotplot-layout"):
        for extra in ([], ["--no-filter"]):
            r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), flag, str(rep), *extra], capture_output=True, text=True)
            assert r.returncode == 3 and "--dotplot" in r.stderr and "2^32" in r.stderr, r.stderr
            assert r.stdout == "" and not out.exists() and not rep.exists()
