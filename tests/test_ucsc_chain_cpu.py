"""The chain files without a GPU: the brute-force model of tests/ucsc_chain_model.py against chains worked out by hand and against
the exact lift's model, and the host side of the feature -- header, ctypes mirrors, exported symbols, the no-device paths and
refusals of swg_paf_ucsc_chain_write / _text, the usage errors of --ucsc-chain, and the header formatter, batch planner and splice
under the host sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import lift_exact_model as em
from tests import ucsc_chain_model as um
from tests.test_lift_cpu import REBASED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = "5=2I6=4D5X2="       # blocks 5 | 2 I | 6 | 4 D | 7 (5X2= merge): x 20, y 22, 13 '=' columns
H = "3I4=2I3D2=1I"       # leading and trailing I, an I directly followed by a D: blocks 4 | dq 2, dt 3 | 2: x 12, y 9
QS, TS = 700, 9000       # the sizes of the two sequences


def test_model_against_chains_worked_out_by_hand():
    T, Q = um.FROM_TARGET, um.FROM_QUERY
    #      (ref_start, ref_end, ref_size, minus, oth_start, oth_end, oth_size, blocks)
    assert um.chain_of(G, 0, 100, 120, 1000, 1022, QS, TS, T) == (0, (1000, 1022, TS, 0, 100, 120, QS, [(5, 0, 2), (6, 4, 0), (7, 0, 0)]), 13)
    assert um.chain_of(G, 0, 100, 120, 1000, 1022, QS, TS, Q) == (0, (100, 120, QS, 0, 1000, 1022, TS, [(5, 2, 0), (6, 0, 4), (7, 0, 0)]), 13)
    # '-': the query side in reverse-complement coordinates, 700 - 220 = 480
    assert um.chain_of(G, 1, 200, 220, 2000, 2022, QS, TS, T) == (0, (2000, 2022, TS, 1, 480, 500, QS, [(5, 0, 2), (6, 4, 0), (7, 0, 0)]), 13)
    # seen from the query: [700 - 500, 700 - 480) forward, the target reverse-complemented [9000 - 2022, 9000 - 2000), blocks reversed
    assert um.chain_of(G, 1, 200, 220, 2000, 2022, QS, TS, Q) == (0, (200, 220, QS, 1, 6978, 7000, TS, [(7, 0, 4), (6, 2, 0), (5, 0, 0)]), 13)
    # leading and trailing I are cut off (x 3 .. 11), I directly followed by D is one gap
    assert um.chain_of(H, 0, 400, 412, 4000, 4009, QS, TS, T) == (0, (4000, 4009, TS, 0, 403, 411, QS, [(4, 3, 2), (2, 0, 0)]), 6)
    assert um.chain_of(H, 1, 500, 512, 5000, 5009, QS, TS, T) == (0, (5000, 5009, TS, 1, 700 - 512 + 3, 700 - 512 + 11, QS, [(4, 3, 2), (2, 0, 0)]), 6)
    assert um.chain_of(H, 1, 500, 512, 5000, 5009, QS, TS, Q) == (0, (501, 509, QS, 1, TS - 5009, TS - 5000, TS, [(2, 2, 3), (4, 0, 0)]), 6)
    # leading and trailing D (y 2 .. 6)
    assert um.chain_of("2D4=1D", 0, 1100, 1104, 1100, 1107, 2000, TS, T) == (0, (1102, 1106, TS, 0, 1100, 1104, 2000, [(4, 0, 0)]), 4)
    # M only: the score is the aligned columns
    assert um.chain_of("10M", 0, 300, 310, 3000, 3010, QS, TS, T) == (0, (3000, 3010, TS, 0, 300, 310, QS, [(10, 0, 0)]), 10)
    assert um.chain_of("3M2=", 0, 0, 5, 0, 5, QS, TS, T)[2] == 2
    # S / H / P at the ends, zero-length ops between two aligned ops: one block
    assert um.chain_of("2S1H3=0I0X0P2=4S", 0, 10, 15, 20, 25, QS, TS, T) == (0, (20, 25, TS, 0, 10, 15, QS, [(5, 0, 0)]), 5)
    # zero-length ops between an aligned op and a gap
    assert um.chain_of("3=0D0M2I0S2=", 0, 10, 17, 20, 25, QS, TS, T) == (0, (20, 25, TS, 0, 10, 17, QS, [(3, 0, 2), (2, 0, 0)]), 5)
    # gaps only, and zero-length aligned ops only: state 0, no chain
    assert um.chain_of("5I3D", 0, 10, 15, 20, 23, QS, TS, T) == (0, None, 0)
    assert um.chain_of("0=0M", 0, 10, 10, 20, 20, QS, TS, T) == (0, None, 0)
    # every state
    assert um.chain_of("5=x5=", 0, 600, 610, 6000, 6010, QS, TS, T) == (1, None, 0)
    assert um.chain_of("4294967296D10=", 0, 620, 630, 6020, 6030, QS, TS, T) == (2, None, 0)
    assert um.chain_of("9=", 0, 640, 650, 6040, 6049, QS, TS, T) == (4, None, 0)
    assert um.chain_of("9=", 0, 660, 669, 6060, 6070, QS, TS, T) == (8, None, 0)
    assert um.chain_of("", 0, 680, 690, 6080, 6090, QS, TS, T) == (16, None, 0)
    assert um.chain_of("10=", 0, 695, 705, 100, 110, QS, TS, T) == (32, None, 0)         # beyond on the query
    assert um.chain_of("10=", 0, 0, 10, 8995, 9005, QS, TS, T) == (32, None, 0)          # ... on the target
    assert um.chain_of("9=", 0, 695, 705, 100, 109, QS, TS, T) == (36, None, 0) and um.chain_of("", 0, 0, 10, 8995, 9005, QS, TS, T) == (48, None, 0)
    assert um.chain_of("10=", 0, 690, 700, 8990, 9000, QS, TS, T)[0] == 0                # ending AT the size is inside
    # the text
    assert um.block_text([(5, 0, 2), (6, 4, 0), (7, 0, 0)]) == "5\t0\t2\n6\t4\t0\n7\n\n" and um.block_text([(4, 0, 0)]) == "4\n\n"
    assert um.header_text(13, "t", "q", (2000, 2022, TS, 1, 480, 500, QS, None), 7) == "chain 13 t 9000 + 2000 2022 q 700 - 480 500 7\n"


def random_cigar(rng, max_ops=12):
    ops = []
    for _ in range(int(rng.integers(1, max_ops + 1))):
        ops.append("%d%s" % (0 if rng.random() < 0.15 else rng.integers(1, 6), "M=XIDNSHP"[int(rng.integers(0, 9))]))
    return "".join(ops)


def test_random_chains_walk_back_and_swap_twice():
    """chain_of asserts on every chain: the blocks walked from the start are the literal expansion's columns, the '-' swap the
    reverse-complemented ones, and swap applied twice is the identity."""
    rng = np.random.default_rng(5)
    chains = 0
    for _ in range(3000):
        text = random_cigar(rng)
        Lq, Lt = em.advances(em.parse(text)[1])
        qs, ts = int(rng.integers(0, 50)), int(rng.integers(0, 50))
        for minus in (0, 1):
            st, a, score = um.chain_of(text, minus, qs, qs + Lq, ts, ts + Lt, qs + Lq + 7, ts + Lt + 3, um.FROM_TARGET)
            st2, b, score2 = um.chain_of(text, minus, qs, qs + Lq, ts, ts + Lt, qs + Lq + 7, ts + Lt + 3, um.FROM_QUERY)
            assert st == st2 == 0 and score == score2 and (a is None) == (b is None)
            if a is not None:
                chains += 1
                assert um.swap(a) == b and um.swap(b) == a and sum(s for s, _, _ in a[7]) == sum(s for s, _, _ in b[7])
    assert chains > 4000


def test_lifting_a_base_through_the_chain_is_the_exact_lift():
    """Every target base of a record: through the model's chain (from = target) and as a 1-base exact row of lift_exact_model."""
    rng = np.random.default_rng(6)
    checked = 0
    for _ in range(300):
        text = random_cigar(rng, 8)
        ops = em.parse(text)[1]
        Lq, Lt = em.advances(ops)
        qs, ts, minus = int(rng.integers(0, 30)), int(rng.integers(0, 30)), int(rng.integers(0, 2))
        q_size = qs + Lq + 5
        _, chain, _ = um.chain_of(text, minus, qs, qs + Lq, ts, ts + Lt, q_size, ts + Lt + 5, um.FROM_TARGET)
        cols3 = em.columns(ops)
        for tpos in range(ts, ts + Lt):
            d0, d1, aligned, _ = em.exact_row(cols3, 1, minus, tpos, tpos + 1, qs, qs + Lq, ts, ts + Lt)
            got = um.lift_base(chain, tpos) if chain is not None else None
            if aligned:
                assert d1 == d0 + 1 and got == (q_size - 1 - d0 if minus else d0), (text, minus, tpos)
                checked += 1
            else:
                assert got is None, (text, minus, tpos)
    assert checked > 1000


@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib, ucsc
    structs = (("swg_ucsc_block", _lib.SwgUcscBlock), ("swg_ucsc_chain", _lib.SwgUcscChain), ("swg_ucsc_request", _lib.SwgUcscRequest),
               ("swg_ucsc_counts", _lib.SwgUcscCounts), ("swg_cigar_set", _lib.SwgCigarSet))
    cname = lambda f: f.rstrip("_")      # noqa: E731  (`from` is a Python keyword)
    prints = ['printf("%%zu\\n", sizeof(%s));' % name for name, _ in structs]
    prints += ['printf("%%zu\\n", offsetof(%s, %s));' % (name, cname(f)) for name, cls in structs for f, _ in cls._fields_]
    prints += ['printf("%u %u %u %u %d\\n", SWG_CIGAR_BEYOND, SWG_UCSC_FROM_TARGET, SWG_UCSC_FROM_QUERY, SWG_UCSC_MINUS, SWG_ABI_VERSION);']
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(cls) for _, cls in structs] + [getattr(cls, f).offset for _, cls in structs for f, _ in cls._fields_]
    want += [32, 0, 1, 1, 1]
    assert got == want
    assert got[:5] == [12, 48, 120, 64, 32]
    for _, cls in structs:      # no implicit padding
        assert sum(C.sizeof(t) for _, t in cls._fields_) == C.sizeof(cls)
    assert ucsc.BLOCK_DTYPE.itemsize == 12 and ucsc.CHAIN_DTYPE.itemsize == 48
    for dt, cls in ((ucsc.BLOCK_DTYPE, _lib.SwgUcscBlock), (ucsc.CHAIN_DTYPE, _lib.SwgUcscChain)):
        assert [dt.fields[f][1] for f, _ in cls._fields_] == [getattr(cls, f).offset for f, _ in cls._fields_]
    assert (ucsc.CIGAR_BEYOND, ucsc.FROM_QUERY, ucsc.MINUS) == (um.BEYOND, um.FROM_QUERY, um.MINUS)
    assert tuple(f for f, _ in _lib.SwgUcscCounts._fields_) == ucsc.COUNTS == um.COUNTS


def test_symbols_are_exported_and_declared(lib):
    import sweepga_amd
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_ucsc_chain_records", "swg_ucsc_chain_records_device", "swg_paf_ucsc_chain_write", "swg_paf_ucsc_chain_text"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    assert lib.swg_abi_version() == 1
    for name in ("UcscChain", "UcscResult", "ucsc_chain_records", "ucsc_chain_records_device"):
        assert hasattr(sweepga_amd, name)


def tagged(fields, *tags):
    return "\t".join([str(f) for f in fields] + ["tp:A:P"] + list(tags))


def mixed_paf():
    """A PAF that mixes what the whole path has to cope with -> (text, kept mask): =/X CIGARs on both strands, M CIGARs, a line
    without a tag, one with two tags (the last counts), an empty and a broken tag, a record that ends beyond its sequence, an
    intra-sequence record, a CIGAR of gaps only, and a sequence whose length differs between lines (the last mention counts)."""
    q, t = "g1#1#q", "g2#1#t"
    lines = [
        tagged([q, QS, 100, 120, "+", t, TS, 1000, 1022, 13, 22, 60], "cg:Z:" + G),
        tagged([q, QS, 200, 220, "-", t, TS, 2000, 2022, 13, 22, 60], "cg:Z:" + G, "nm:i:3"),
        tagged([q, QS, 300, 310, "+", t, TS, 3000, 3010, 10, 10, 60], "cg:Z:10M"),
        tagged([q, QS, 400, 412, "+", t, TS, 4000, 4009, 6, 12, 60], "cg:Z:" + H),
        tagged([q, QS, 500, 512, "-", t, TS, 5000, 5009, 6, 12, 60], "cg:Z:" + H),
        tagged([q, QS, 520, 530, "+", t, TS, 5100, 5110, 10, 10, 60]),
        tagged([q, QS, 600, 650, "+", t, TS, 6000, 6050, 49, 50, 60], "cg:Z:50M", "cg:Z:49=1X"),
        tagged([q, QS, 652, 660, "+", t, TS, 6100, 6108, 8, 8, 60], "cg:Z:"),
        tagged([q, QS, 662, 672, "+", t, TS, 6200, 6210, 10, 10, 60], "cg:Z:5=x5="),
        tagged([q, QS, 690, 705, "-", t, TS, 7000, 7015, 15, 15, 60], "cg:Z:15="),
        tagged([t, TS, 100, 110, "-", t, TS, 200, 212, 10, 12, 60], "cg:Z:4=2D6="),
        tagged([q, QS, 10, 15, "+", t, TS, 20, 23, 0, 8, 60], "cg:Z:5I3D"),
        tagged(["g3#1#s", 90, 0, 9, "+", t, TS, 8000, 8009, 9, 9, 60], "cg:Z:4294967295=", "cg:Z:3=1X5="),
        tagged(["g3#1#s", 95, 5, 95, "-", q, QS, 0, 80, 80, 90, 60], "cg:Z:40=5I40=5I"),
    ]
    kept = np.array([1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 1, 0, 1], dtype=bool)
    return "\n".join(lines) + "\n", kept


def test_the_mixed_paf_of_the_model():
    text, kept = mixed_paf()
    out, counts = um.paf_chain_text(text, None, 0, um.FROM_TARGET)
    assert counts == {"records": 14, "chains": 9, "bad": 1, "beyond": 1, "untagged": 1, "empty": 1, "blocks": 17}
    assert out.startswith("chain 13 g2#1#t 9000 + 1000 1022 g1#1#q 700 + 100 120 1\n5\t0\t2\n6\t4\t0\n7\n\nchain 13 g2#1#t 9000 + 2000 2022 g1#1#q 700 - 480 500 2\n")
    assert "chain 10 g2#1#t 9000 + 200 212 g2#1#t 9000 - 8890 8900 7\n4\t2\t0\n6\n\n" in out         # the intra-sequence record
    assert out.endswith("chain 80 g1#1#q 700 + 0 80 g3#1#s 95 - 0 85 9\n40\t0\t5\n40\n\n")           # the size of the last mention, the trailing I cut off
    swapped, c2 = um.paf_chain_text(text, kept, 1, um.FROM_QUERY)
    assert c2 == {"records": 11, "chains": 7, "bad": 1, "beyond": 1, "untagged": 1, "empty": 1, "blocks": 15}
    assert "chain 13 g1#1#q 700 + 200 220 g2#1#t 9000 - 6978 7000 2\n7\t0\t4\n6\t2\t0\n5\n\n" in swapped
    assert um.paf_chain_text("", None, 0) == ("", {k: 0 for k in um.COUNTS[:-1]})


def chain_text(lib, paf, status, set_=0, from_=0, batch=0, ctx=None):
    """swg_paf_ucsc_chain_text -> (rc, text or None, counts)"""
    from sweepga_amd import _lib
    counts, p, n = _lib.SwgUcscCounts(), C.c_void_p(77), C.c_uint64(77)
    rc = lib.swg_paf_ucsc_chain_text(ctx, paf.handle, status.ctypes.data if status is not None else None, set_, from_, batch, C.byref(counts),
                                     C.byref(p), C.byref(n))
    text = None
    if p.value:
        text = C.string_at(p.value, n.value).decode()
        lib.swg_free(p)
    else:
        assert n.value == 0
    return rc, text, {k: int(getattr(counts, k)) for k in um.COUNTS}


def test_paf_seams_without_a_device(lib, tmp_path):
    """A PAF without records of the set gives an empty file and text and needs no device; the refusals come before a context is
    looked at, and before the file is touched."""
    from sweepga_amd import PafFile, SwgError, UcscChain, _lib
    zero = {k: 0 for k in um.COUNTS}
    out = tmp_path / "x.chain"
    for text in ("", "# nothing\nfew\tfields\n"):
        with PafFile(text=text) as paf:
            for st in (None, np.zeros(1, dtype=np.uint8)):
                assert chain_text(lib, paf, st) == (0, "", zero)
                assert chain_text(lib, paf, st, from_=1, batch=5) == (0, "", zero)
            out.write_text("stale")
            counts = _lib.SwgUcscCounts()
            assert lib.swg_paf_ucsc_chain_write(None, paf.handle, None, 0, 0, str(out).encode(), 0, C.byref(counts)) == 0
            assert out.read_bytes() == b"" and counts.records == 0 and counts.batches == 0
            assert lib.swg_paf_ucsc_chain_write(None, paf.handle, None, 0, 0, str(out).encode(), 0, None) == 0      # counts may be NULL
            got = UcscChain.from_paf(paf, None, set="all")
            assert (got.text, got.counts, got.chains, got.blocks) == ("", zero, [], [])
    text, kept = mixed_paf()
    with PafFile(text=text) as paf:
        none = np.zeros(paf.n, dtype=np.uint8)
        assert chain_text(lib, paf, none, set_=1) == (0, "", zero)                       # a set that is never in status: no device
        assert UcscChain.from_paf(paf, none).text == "" and UcscChain.write_paf(paf, none, out) == zero and out.read_bytes() == b""
        st = kept.astype(np.uint8)
        out.write_text("stale")
        rc, t, _ = chain_text(lib, paf, st, set_=1)
        assert rc == -1 and t is None and b"swg_paf_ucsc_chain_text: NULL context" in lib.swg_alnstats_last_error()
        for set_, from_, word in ((2, 0, b"set"), (0, 2, b"from"), (1, 7, b"from")):
            rc, t, _ = chain_text(lib, paf, st, set_=set_, from_=from_)
            assert rc == -1 and t is None and word in lib.swg_alnstats_last_error()
            assert lib.swg_paf_ucsc_chain_write(None, paf.handle, st.ctypes.data, set_, from_, str(out).encode(), 0, None) == -1
            assert out.read_text() == "stale"
        assert chain_text(lib, paf, None, set_=1)[0] == -1 and b"status" in lib.swg_alnstats_last_error()
        assert lib.swg_paf_ucsc_chain_write(None, paf.handle, None, 1, 0, str(out).encode(), 0, None) == -1 and out.read_text() == "stale"
        assert lib.swg_paf_ucsc_chain_write(None, paf.handle, none.ctypes.data, 1, 0, str(tmp_path / "no" / "dir.chain").encode(), 0, None) == -1
        assert b"cannot open" in lib.swg_alnstats_last_error()
        p, n = C.c_void_p(), C.c_uint64()
        assert lib.swg_paf_ucsc_chain_text(None, None, None, 0, 0, 0, None, C.byref(p), C.byref(n)) == -1
        assert lib.swg_paf_ucsc_chain_text(None, paf.handle, None, 0, 0, 0, None, None, C.byref(n)) == -1
        assert lib.swg_paf_ucsc_chain_write(None, paf.handle, None, 0, 0, None, 0, None) == -1
        with pytest.raises(SwgError):
            UcscChain.from_paf(paf, st, set=2)
    with PafFile(text=REBASED) as paf:
        with pytest.raises(SwgError) as e:
            UcscChain.from_paf(paf, np.ones(1, dtype=np.uint8))
        assert e.value.code == -6 and "2^32" in str(e.value)
        out.write_text("stale")
        with pytest.raises(SwgError):
            UcscChain.write_paf(paf, np.ones(1, dtype=np.uint8), out)
        assert out.read_text() == "stale"


def test_record_seams_refuse_without_a_device(lib):
    """A NULL context: there is no CPU path, and nothing the caller owns is touched."""
    from sweepga_amd import _lib
    from sweepga_amd.lift import cigar_set
    from tests import lift_model as lm
    cols, strand, _ = lm.parse_paf(mixed_paf()[0])
    rec = _lib.SwgRecords()
    rec.n = len(strand)
    for k, a in cols.items():
        setattr(rec, k, a.ctypes.data)
    rec.strand, rec.n_seq = strand.ctypes.data, 3
    seq_len = np.array([QS, TS, 95], dtype=np.uint32)
    record, offset, text = cigar_set([0, 2], [G, "10M"])
    cs = _lib.SwgCigarSet()
    cs.record, cs.offset, cs.text, cs.k = record.ctypes.data, offset.ctypes.data, text.ctypes.data, 2
    poison = np.full(48 * 2, 0xab, dtype=np.uint8)
    for fn in (lib.swg_ucsc_chain_records, lib.swg_ucsc_chain_records_device):
        req = _lib.SwgUcscRequest()
        req.chain_capacity, req.chains, req.n_chains, req.text_bytes = 2, poison.ctypes.data, 12345, 77
        assert fn(None, C.byref(rec), seq_len.ctypes.data, None, C.byref(cs), C.byref(req)) == -1
        assert (poison == 0xab).all() and req.n_chains == 12345 and req.text_bytes == 77


def test_command_line_usage_errors(lib, tmp_path):
    from sweepga_amd import build
    paf = tmp_path / "in.paf"
    paf.write_text(mixed_paf()[0])
    out, chain = tmp_path / "out.paf", tmp_path / "x.chain"
    run = lambda *a: subprocess.run([build.CLI, str(paf), "--output-file", str(out), *a], capture_output=True, text=True)      # noqa: E731
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and all(w in r.stdout for w in ("--ucsc-chain FILE", "--ucsc-chain-from target|query", "--ucsc-chain-set kept|all",
                                                              "--ucsc-chain-batch BYTES"))
    cases = [(["--ucsc-chain-from", "query"], "need --ucsc-chain"), (["--ucsc-chain-set", "all"], "need --ucsc-chain"),
             (["--ucsc-chain-batch", "4k"], "need --ucsc-chain"),
             (["--ucsc-chain", str(chain), "--ucsc-chain-from", "both"], "--ucsc-chain-from: target or query"),
             (["--ucsc-chain", str(chain), "--ucsc-chain-set", "lost"], "--ucsc-chain-set: kept or all"),
             (["--ucsc-chain", str(chain), "--ucsc-chain-batch", "0"], "--ucsc-chain-batch"),
             (["--ucsc-chain", str(chain), "--ucsc-chain-batch", "many"], "--ucsc-chain-batch"),
             (["--ucsc-chain", "-"], "not a standard error report"), (["--ucsc-chain", ""], "empty value for --ucsc-chain")]
    for extra, word in cases:
        r = run(*extra)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)
        assert r.stdout == "" and not out.exists() and not chain.exists(), extra


def test_text_helpers_under_the_host_sanitizers(tmp_path):
    """tests/native/ucsc_text_check.cpp: a stand-alone program over csrc/host/ucsc_text.cpp, built with the address and
    undefined-behaviour sanitizers; its answers must be the model's byte for byte."""
    exe = str(tmp_path / "ucsc_text_check")
    host = os.path.join(ROOT, "sweepga_amd", "csrc", "host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "native", "ucsc_text_check.cpp"), os.path.join(host, "ucsc_text.cpp"),
                           os.path.join(host, "cigar_text.cpp"), "-lpthread"])
    top = 2**32 - 1
    feed, want = [], []
    # headers at every field's extreme: 10-digit values, an id beyond 2^32, empty and very long names
    for score, flags, rs, re, os_, oe, rsize, osize, id_, ref, oth in (
            (13, 0, 1000, 1022, 100, 120, TS, QS, 1, "g2#1#t", "g1#1#q"), (top, 1, top, top, top, top, top, top, 2**32 + 5, "", ""),
            (0, 0x2001, 0, 0, 0, 0, 0, 0, 2**64 - 1, "x" * 5000, "y"), (1, 0, 9, 10, 0, 1, 10, 1, top, "a b", "c\td")):
        feed += ["H", " ".join(str(v) for v in (score, flags, rs, re, os_, oe, rsize, osize, id_)), ref, oth]
        want.append(um.header_text(score, ref, oth, (rs, re, rsize, flags & 1, os_, oe, osize, None), id_))
    assert want[1] == "chain 4294967295  4294967295 + 4294967295 4294967295  4294967295 - 4294967295 4294967295 4294967301\n"

    # the planner: consecutive entries within batch_bytes, a longer entry alone; 0 = one batch below 2^32
    def plan(batch, lens):
        first, held = [0], 0
        for j, n in enumerate(lens):
            if j > first[-1] and held + n > (batch if 0 < batch < top else top):
                first.append(j)
                held = 0
            held += n
        return first + [len(lens)] if lens else first
    lens = [7, 3, 0, 12, 1, 1, 5, 0]
    for batch in (1, 7, 6, 12, 11, 10, 13, 29, 28, 0, top, 2**40):
        feed += ["P", " ".join(str(v) for v in [batch, len(lens)] + lens)]
        want.append(" ".join(str(v) for v in plan(batch, lens)) + "\n")
    assert plan(1, lens) == list(range(9)) and plan(7, lens) == [0, 1, 3, 4, 8] and plan(6, lens) == [0, 1, 3, 4, 6, 8] and plan(0, lens) == [0, 8]
    for batch, ls in ((5, []), (0, []), (1, [0, 0, 0]), (0, [top - 1, 1, 1]), (0, [2**31, 2**31]), (3, [4])):
        feed += ["P", " ".join(str(v) for v in [batch, len(ls)] + ls)]
        want.append(" ".join(str(v) for v in plan(batch, ls)) + "\n")
    # the splice: chains with several blocks, with one, and rows with none, at either end and in a row
    for rows, text in (([(0, 0, ""), (2, 0, "chain a"), (0, 0, ""), (0, 0, ""), (1, 9, "chain b"), (3, 12, "chain c"), (0, 0, "")], "5\t0\t2\n7\n\n4\n\n1\t1\t1\n2\t0\t9\n3\n\n"),
                       ([(1, 0, "chain only")], "4294967295\n\n"), ([(0, 0, ""), (0, 0, "")], ""), ([], "")):
        feed += ["S", "%d %d" % (len(rows), len(text))] + ["%d %d %s" % r for r in rows] + [text.replace("\n", "|")]
        ends = [r[1] for r in rows if r[0]][1:] + [len(text)]
        pieces = [r[2] + "\n" + text[r[1]:e] for r, e in zip([r for r in rows if r[0]], ends)]
        want.append("".join(pieces).replace("\n", "|") + "\n")
    assert want[-4].startswith("chain a|5\t0\t2|7||chain b|4||chain c|1\t1\t1|")
    r = subprocess.run([exe], input=("\n".join(feed) + "\n").encode(), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.decode() == "".join(want)
