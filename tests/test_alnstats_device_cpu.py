"""The host side of the on-device alnstats: the new structures of include/sweepga_gpu.h against their ctypes mirrors (sizes and
offsets compiled from the header), the new exports, the command line's two flags, and alnstats' genome rule (the name up to
and including the LAST '#', src/bin/alnstats.rs:94-100).  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


COUNTS_FIELDS = ["total_mappings", "total_bases", "total_matches", "self_mappings", "inter_chromosomal", "inter_genome",
                 "chr_pair_count", "n_pairs", "pair_capacity", "pairs", "seq_last"]
PAIR_FIELDS = ["q_genome", "t_genome", "bases", "matches", "first_record"]


def test_counts_structs_match_header(lib, tmp_path):
    from sweepga_amd import _lib
    prints = ['printf("%zu %zu\\n", sizeof(swg_alnstats_counts), sizeof(swg_alnstats_pair_counts));']
    prints += ['printf("%%zu\\n", offsetof(swg_alnstats_counts, %s));' % f for f in COUNTS_FIELDS]
    prints += ['printf("%%zu\\n", offsetof(swg_alnstats_pair_counts, %s));' % f for f in PAIR_FIELDS]
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){%s return 0;}\n' % "".join(prints))
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    cs, ps = _lib.SwgAlnstatsCounts, _lib.SwgAlnstatsPairCounts
    assert [f for f, _ in cs._fields_] == COUNTS_FIELDS and [f for f, _ in ps._fields_] == PAIR_FIELDS
    want = [C.sizeof(cs), C.sizeof(ps)] + [getattr(cs, f).offset for f in COUNTS_FIELDS] + [getattr(ps, f).offset for f in PAIR_FIELDS]
    assert got == want
    assert C.sizeof(ps) == 32 and C.sizeof(cs) == 88


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    from sweepga_amd import _lib
    for s in ("swg_alnstats_records", "swg_alnstats_records_device", "swg_paf_alnstats"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None
    assert lib.swg_abi_version() == 1
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    assert "#define SWG_ABI_VERSION 1" in hdr


def test_existing_struct_sizes_unchanged(lib):
    """Additions only: the structures callers already compile against keep their sizes."""
    from sweepga_amd import _lib
    from sweepga_amd.alnstats import SwgAlnstatsSummary
    assert (C.sizeof(_lib.SwgConfig), C.sizeof(_lib.SwgRecords), C.sizeof(_lib.SwgStats), C.sizeof(SwgAlnstatsSummary)) == (128, 128, 72, 88)


def test_without_a_device_the_seams_refuse(lib):
    """No CPU fallback: a NULL context is an error for records; a PAF without records needs no device."""
    from sweepga_amd import PafFile
    from sweepga_amd._lib import SwgAlnstatsCounts, SwgRecords
    from sweepga_amd.alnstats import AlnStats
    r = SwgRecords()
    c = SwgAlnstatsCounts()
    assert lib.swg_alnstats_records(None, C.byref(r), None, 0, None, C.byref(c), None) == -1
    assert lib.swg_alnstats_records_device(None, C.byref(r), None, 0, None, C.byref(c), None) == -1
    with PafFile(text="q\t1\t0\t1\t+\tt\t1\t0\t1\t1\t1\t60\n") as paf:
        a, k = C.c_void_p(), C.c_void_p()
        assert lib.swg_paf_alnstats(None, paf.handle, None, C.byref(a), C.byref(k)) == -1 and not a.value and not k.value
    text = "too\tfew\tfields\n\n# comment\n"
    with PafFile(text=text) as paf:
        assert paf.n == 0
        all_, kept = AlnStats.from_paf(None, paf, status=np.zeros(0, dtype=np.uint8))
        host = AlnStats(text=text)
        assert all_.report("x", True) == kept.report("x", True) == host.report("x", True)
        assert all_.compare(kept, "a", "b") == host.compare(host, "a", "b")


def test_cli_help_lists_the_flags_and_stats_needs_a_value(lib):
    from sweepga_amd import build
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--stats REPORT" in r.stdout and "--stats-detailed" in r.stdout
    r = subprocess.run([build.CLI, "in.paf", "--stats"], capture_output=True, text=True)
    assert r.returncode == 2 and "--stats" in r.stderr and r.stdout == ""


def test_cli_stats_without_a_filter_is_the_host_report(lib, tmp_path):
    """--no-filter opens no device: the report is the host tool's for the input against itself; standard output (the PAF)
    is what it is without --stats."""
    from sweepga_amd import build
    text = ("a#1#c1\t100\t0\t50\t+\tb#1#c1\t200\t0\t50\t40\t50\t60\n"
            "a#1#c1\t100\t50\t90\t-\ta#1#c2\t300\t0\t40\t30\t40\t60\n"
            "short\tline\n"
            "b#1#c1\t200\t0\t10\t+\tb#1#c1\t200\t0\t10\t10\t10\t60\r\n")
    inp, rep = tmp_path / "in.paf", tmp_path / "rep.txt"
    inp.write_text(text, newline="")
    plain = subprocess.run([build.CLI, str(inp), "--no-filter"], capture_output=True)
    r = subprocess.run([build.CLI, str(inp), "--no-filter", "--stats", str(rep), "--stats-detailed"], capture_output=True)
    assert r.returncode == plain.returncode == 0 and r.stdout == plain.stdout
    host = subprocess.run([build.STATS, str(inp), "-"], input=plain.stdout, capture_output=True)
    one = subprocess.run([build.STATS, str(inp), "-d"], capture_output=True)
    dash = subprocess.run([build.STATS, "-", "-d"], input=plain.stdout, capture_output=True)
    assert host.returncode == one.returncode == dash.returncode == 0
    assert rep.read_bytes() == host.stdout + one.stdout + dash.stdout
    r = subprocess.run([build.CLI, str(inp), "--no-filter", "--stats", "-"], capture_output=True)
    assert r.returncode == 0 and r.stdout == plain.stdout and r.stderr == host.stdout


def test_last_hash_genome_map():
    from sweepga_amd.alnstats import genome_last, genome_map
    assert genome_last("SGDref#1#chrI") == "SGDref#1#"
    assert genome_last("x#y#z#w") == "x#y#z#"          # NOT the filter's two-part prefix "x#y#"
    assert genome_last("one#chr") == "one#"
    assert genome_last("plain") == "plain"
    assert genome_last("trailing#") == "trailing#"
    assert genome_last("#lead") == "#"
    assert genome_last("") == ""
    ids, names = genome_map(["a#1#c1", "b#1#c1", "a#1#c2", "plain", "a#2#c1", "plain2", "a#1#c1#x"])
    assert list(ids) == [0, 1, 0, 2, 3, 4, 5] and names == ["a#1#", "b#1#", "plain", "a#2#", "plain2", "a#1#c1#"]
    # the library's own table for the same names (the PAF handle's last-'#' map is the one swg_paf_alnstats uses)
    from sweepga_amd import PafFile
    seqs = ["a#1#c1", "b#1#c1", "a#1#c2", "plain", "a#2#c1", "plain2", "a#1#c1#x", "x#y#z#w"]
    text = "".join(f"{s}\t10\t0\t5\t+\t{s}\t10\t0\t5\t5\t5\t60\n" for s in seqs)
    with PafFile(text=text) as paf:
        assert paf.names == seqs
        mine, _ = genome_map(seqs)
        assert list(paf.seq_genome_last) == list(mine)
