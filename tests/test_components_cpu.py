"""Components without a GPU: tests/components_model.py against answers derived by hand from the definition in
include/sweepga_gpu.h, and the host side of the library -- symbols, structure layouts, the refusals that need no device, the
command line's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import components_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def columns(rec):
    a = np.asarray(rec, dtype=np.uint32).reshape(-1, 6)
    return {k: np.ascontiguousarray(a[:, j]) for j, k in enumerate(cm.COLUMNS)}


def hand_case():
    """Six sequences, seven records (q, t, q_start, q_end, t_start, t_end):
         link (0, 1): r0 gives 100 to 0 and 90 to 1, r1 (the other orientation) 60 to 0 and 50 to 1 -> 160, 140, 2 records, first 0
         r2 is a self mapping, r3 has status 0: no link
         link (2, 3): r4, query 3: 20 on 2, 10 on 3, first 4
         link (1, 4): r5, query 4: 150 on 1, 150 on 4, first 5
         link (0, 4): r6: 5 and 5, first 6
         sequence 5 has no record."""
    rec = [(0, 1, 0, 100, 0, 90), (1, 0, 10, 60, 20, 80), (0, 0, 0, 500, 0, 500), (2, 3, 0, 400, 0, 400), (3, 2, 0, 10, 0, 20),
           (4, 1, 0, 150, 100, 250), (0, 4, 0, 5, 0, 5)]
    status = np.array([1, 2, 1, 0, 3, 1, 1], dtype=np.uint8)
    seq_len = np.array([1000, 1000, 500, 2000, 300, 0], dtype=np.uint32)
    return columns(rec), status, seq_len


def links_of(res):
    return {(l[0], l[1]): l[2:] for l in res["links"]}


def test_links_both_orientations_self_and_dropped_records():
    cols, status, seq_len = hand_case()
    res = cm.components(cols, status, seq_len)
    # (n_records, joined, a_bases, b_bases, first_record)
    assert links_of(res) == {(0, 1): (2, 1, 160, 140, 0), (0, 4): (1, 1, 5, 5, 6), (1, 4): (1, 1, 150, 150, 5), (2, 3): (1, 1, 20, 10, 4)}
    assert [l[:2] for l in res["links"]] == [(0, 1), (0, 4), (1, 4), (2, 3)]
    # status == NULL: r3 takes part too, the self mapping still does not
    assert links_of(cm.components(cols, None, seq_len))[(2, 3)] == (2, 1, 420, 410, 3)


def test_plain_connected_components_numbered_by_smallest_member():
    cols, status, seq_len = hand_case()
    res = cm.components(cols, status, seq_len)
    assert res["seq_component"] == [1, 1, 2, 2, 1, 3]            # sequence 5: a singleton
    # (id, first_seq, n_seq, n_links, length, n_records, bases)
    assert res["components"] == [(1, 0, 3, 3, 2300, 4, 610), (2, 2, 2, 1, 2500, 1, 30), (3, 5, 1, 0, 0, 0, 0)]
    assert res["cross"] == (0, 0, 0)


def test_share_threshold_at_and_below_need():
    cols, status, seq_len = hand_case()
    # 160000 ppm of 1000 bases: need(0) = need(1) = 160; a_bases = 160 joins, b_bases = 140 alone would not
    assert links_of(cm.components(cols, status, seq_len, 0, 160_000))[(0, 1)][1] == 1
    # one ppm more: need = ceil(160.001) = 161
    assert cm.need(160_001, 1000) == 161 and links_of(cm.components(cols, status, seq_len, 0, 160_001))[(0, 1)][1] == 0
    # a link that joins from the b side only: (1, 4) at 500000 ppm, need(1) = 500 > 150, need(4) = 150 = b_bases
    res = cm.components(cols, status, seq_len, 0, 500_000)
    assert {k: v[1] for k, v in links_of(res).items()} == {(0, 1): 0, (0, 4): 0, (1, 4): 1, (2, 3): 0}
    assert res["seq_component"] == [1, 2, 3, 4, 2, 5]            # {1, 4} is numbered by its smallest member, 1
    assert res["components"][1] == (2, 1, 2, 1, 1300, 1, 300)
    assert res["cross"] == (3, 4, 340)                           # (0, 1): 300, (0, 4): 10, (2, 3): 30
    assert links_of(cm.components(cols, status, seq_len, 0, 500_001))[(1, 4)][1] == 0   # need(4) = ceil(150.0003) = 151
    # a zero seq_len needs nothing
    assert cm.need(1_000_000, 0) == 0


def test_min_bases_alone_and_an_unjoined_link_inside_a_component():
    cols, status, seq_len = hand_case()
    res = cm.components(cols, status, seq_len, 150, 0)
    assert {k: v[1] for k, v in links_of(res).items()} == {(0, 1): 1, (0, 4): 0, (1, 4): 1, (2, 3): 0}
    assert res["seq_component"] == [1, 1, 2, 3, 1, 4]
    assert res["components"][0] == (1, 0, 3, 3, 2300, 4, 610)    # (0, 4) is not joined, but both its ends lie inside
    assert res["cross"] == (1, 1, 30)
    assert links_of(cm.components(cols, status, seq_len, 151, 0))[(1, 4)][1] == 0


def test_report_text_by_hand():
    cols, status, seq_len = hand_case()
    names = ["s%d" % i for i in range(6)]
    res = cm.components(cols, status, seq_len, 0, 500_000)
    text = cm.report(names, seq_len, res, True).decode().split("\n")
    assert text[0] == "sequence\tlength\tcomponent\tcomponent_sequences\tcomponent_length\tlinks\trecords\tbases"
    assert text[2] == "s1\t1000\t2\t2\t1300\t2\t3\t600" and text[6] == "s5\t0\t5\t1\t0\t0\t0\t0"
    assert text[7] == "#links" and text[8] == "s0\ts1\t2\t160\t140\t0" and text[10] == "s1\ts4\t1\t150\t150\t1"
    assert text[12:] == ["#cross\t3\t4\t340", ""]
    assert cm.report(names, seq_len, res, False).decode().split("\n")[7:] == ["#cross\t3\t4\t340", ""]
    paf = "a\t10\t0\t5\t+\tb\t20\t0\t5\t5\t5\t60\nb\t21\t0\t5\t+\tb\t22\t0\t5\t5\t5\t60\nshort\tline\n"
    assert cm.last_lengths(paf, ["a", "b"]) == [10, 22]


# ---- the host side of the library ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_symbols_are_exported_and_declared(lib):
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_components_records", "swg_components_records_device", "swg_paf_components"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    assert lib.swg_abi_version() == 1 and "#define SWG_ABI_VERSION 1\n" in hdr
    import sweepga_amd
    assert sweepga_amd.Components is not None and sweepga_amd.components_records is not None and sweepga_amd.components_records_device is not None


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib
    from sweepga_amd.components import COMPONENT_DTYPE, LINK_DTYPE
    structs = [("swg_link", _lib.SwgLink, 40), ("swg_component", _lib.SwgComponent, 40), ("swg_component_params", _lib.SwgComponentParams, 16),
               ("swg_component_table", _lib.SwgComponentTable, 80)]
    prints, want = [], []
    for name, cls, size in structs:
        prints.append('printf("%%zu\\n", sizeof(%s));' % name)
        want.append(size)
        assert C.sizeof(cls) == size
        for f, _ in cls._fields_:
            prints.append('printf("%%zu\\n", offsetof(%s, %s));' % (name, f))
            want.append(getattr(cls, f).offset)
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want
    # no implicit padding: the fields fill the structures
    for _, cls, size in structs[:3]:
        assert sum(C.sizeof(t) for _, t in cls._fields_) == size
    assert LINK_DTYPE.itemsize == COMPONENT_DTYPE.itemsize == 40
    assert [LINK_DTYPE.fields[f][1] for f, _ in _lib.SwgLink._fields_] == [getattr(_lib.SwgLink, f).offset for f, _ in _lib.SwgLink._fields_]
    assert [COMPONENT_DTYPE.fields[f][1] for f, _ in _lib.SwgComponent._fields_] == [getattr(_lib.SwgComponent, f).offset for f, _ in _lib.SwgComponent._fields_]


LINE = "a#1#x\t100\t0\t50\t+\tb#1#y\t200\t10\t60\t50\t50\t60\n"


def test_a_null_context_is_refused(lib):
    from sweepga_amd import PafFile, _lib
    cols, status, seq_len = hand_case()
    rec = _lib.SwgRecords()
    rec.n = len(status)
    for k, a in cols.items():
        setattr(rec, k, a.ctypes.data)
    rec.n_seq = 6
    table, par = _lib.SwgComponentTable(), _lib.SwgComponentParams(0, 0, 0)
    for fn in (lib.swg_components_records, lib.swg_components_records_device):   # (refused before any pointer is looked at)
        assert fn(None, C.byref(rec), seq_len.ctypes.data, status.ctypes.data, C.byref(par), C.byref(table)) == -1
    with PafFile(text=LINE) as paf:
        p, n = C.c_void_p(), C.c_uint64()
        assert lib.swg_paf_components(None, paf.handle, None, None, 0, C.byref(p), C.byref(n)) == -1 and not p.value
        assert b"NULL context" in lib.swg_alnstats_last_error()


def test_no_records_needs_no_device(lib):
    from sweepga_amd import Components, PafFile
    for text in ("", "# nothing\nfew\tfields\n"):
        with PafFile(text=text) as paf:
            assert paf.n == 0
            for detailed in (False, True):
                c = Components.from_paf(None, paf, detailed=detailed)
                assert c.text == (cm.HEADER + ("#links\n" if detailed else "") + "#cross\t0\t0\t0\n").encode() and len(c.components) == 0


def test_64_bit_columns_are_refused_without_a_device(lib, tmp_path):
    from sweepga_amd import build, PafFile
    ln = "\t".join(["a#1#x", str(2**33), str(2**32), str(2**32 + 50), "+", "b#1#y", "900", "10", "60", "50", "50", "60"]) + "\n"
    with PafFile(text=ln) as paf:
        assert paf.is_rebased
        p, n = C.c_void_p(), C.c_uint64()
        assert lib.swg_paf_components(None, paf.handle, None, None, 0, C.byref(p), C.byref(n)) == -6
        assert b"2^32" in lib.swg_alnstats_last_error()
    inp, out, rep = tmp_path / "in.paf", tmp_path / "out.paf", tmp_path / "c.tsv"
    inp.write_text(ln)
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--components", str(rep)], capture_output=True, text=True)
    assert r.returncode == 3 and "--components" in r.stderr and "2^32" in r.stderr, r.stderr
    assert r.stdout == "" and not out.exists() and not rep.exists()


def test_command_line_usage(lib):
    from sweepga_amd import build
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--components REPORT", "--components-detailed", "--component-min-bases N", "--component-min-share F"):
        assert flag in r.stdout
    r = subprocess.run([build.CLI, "in.paf", "--components"], capture_output=True, text=True)
    assert r.returncode == 2 and "--components" in r.stderr
    for share in ("1.5", "-0.1", "nan", "x"):
        r = subprocess.run([build.CLI, "in.paf", "--components", "c.tsv", "--component-min-share", share], capture_output=True, text=True)
        assert r.returncode == 2 and "--component-min-share" in r.stderr, share
    for sub in (["--components-detailed"], ["--component-min-bases", "10k"], ["--component-min-share", "0.5"]):
        r = subprocess.run([build.CLI, "in.paf", *sub], capture_output=True, text=True)
        assert r.returncode == 2 and "need --components" in r.stderr, sub
    r = subprocess.run([build.CLI, "in.paf", "--components", "c.tsv", "--component-min-bases", "ten"], capture_output=True, text=True)
    assert r.returncode == 2 and "--component-min-bases" in r.stderr
