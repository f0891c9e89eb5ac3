"""The chain files on the device (sweepga_amd/csrc/swg_ucsc.hip) against tests/ucsc_chain_model.py: in every case the host seam
against the model and the device seam against the host seam -- rows, blocks, the text of the block lines, states and counts, byte for
byte.  The shapes are the smallest at which each part can go wrong: the mark kernel's tile of 1,024 ops and its borders, runs of
zero-length ops longer than two tiles, entry borders on tile borders, entries of one op; the block and format kernels' tile of 256
blocks, reversal across it, numbers of 1 to 10 digits in every field; the capacity protocol; a random case; the texts of
swg_paf_ucsc_chain_write / UcscChain.from_paf / --ucsc-chain for every batch size.  Every comparison is exact: integers and bytes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import lift_exact_model as em
from tests import lift_model as lm
from tests import ucsc_chain_model as um
from tests.test_gpu_alnstats import filter_cfgs, run_filter
from tests.test_gpu_intervals import kept_mask
from tests.test_gpu_lift import Dev
from tests.test_gpu_lift_exact import corrupt, random_case
from tests.test_gpu_wide import Hip
from tests.test_ucsc_chain_cpu import G, H, QS, TS, mixed_paf

pytestmark = pytest.mark.gpu
COLS = lm.COLS
T = 1024         # ops per tile of the mark kernel
TB = 256         # blocks per work-group of the block and format kernels
FIELDS = ("n_chains", "n_blocks", "text_bytes", "ops", "cigar_bad", "beyond", "empty_chains")


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


def same(a, b):
    return (a.chains.tobytes() == b.chains.tobytes() and a.blocks.tobytes() == b.blocks.tobytes() and a.text == b.text
            and a.state.tobytes() == b.state.tobytes() and all(getattr(a, f) == getattr(b, f) for f in FIELDS))


def both_seams(sw, cols, strand, seq_len, cig, status=None, set_=0, from_=0, ctx=None, shift=0):
    """The result of the host seam, after checking that the device seam gives the same.  shift: the device text starts that many
    bytes behind a 16-byte boundary."""
    from sweepga_amd.lift import cigar_set
    from sweepga_amd.ucsc import ucsc_chain_records, ucsc_chain_records_device
    ctx = ctx or sw.default_context()
    recs = sorted(cig)
    n_seq = len(seq_len)
    got = ucsc_chain_records(ctx, cols, strand, n_seq, seq_len, recs, [cig[i] for i in recs], status=status, set=set_, from_=from_)
    record, offset, text = cigar_set(recs, [cig[i] for i in recs])
    hip = Hip()
    try:
        dcols = {k: Dev(hip, cols[k], np.uint32) for k in COLS}
        dtext = Dev(hip, np.concatenate([np.zeros(shift, dtype=np.uint8), text]))
        dtext.ptr += shift
        dev = ucsc_chain_records_device(ctx, dcols, Dev(hip, strand, np.uint8), n_seq, Dev(hip, seq_len, np.uint32), Dev(hip, record), Dev(hip, offset),
                                        dtext, len(recs), status=Dev(hip, status, np.uint8) if status is not None else None, set=set_, from_=from_)
    finally:
        hip.free()
    assert same(dev, got)
    return got


def compare(got, want, what=""):
    assert got.state.tolist() == want["state"], (what, [(k, a, b) for k, (a, b) in enumerate(zip(got.state.tolist(), want["state"])) if a != b][:8])
    assert {f: getattr(got, f) for f in FIELDS} == {f: want[f] for f in FIELDS}, what
    rows = um.rows_array(want["rows"])
    if got.chains.tobytes() != rows.tobytes():
        bad = [k for k in range(len(rows)) if got.chains[k].tobytes() != rows[k].tobytes()]
        raise AssertionError((what, len(bad), [(tuple(got.chains[k]), want["rows"][k]) for k in bad[:5]]))
    blocks = [tuple(int(v) for v in b) for b in got.blocks]
    if blocks != want["blocks"]:
        bad = [k for k in range(len(blocks)) if blocks[k] != want["blocks"][k]]
        raise AssertionError((what, len(bad), [(k, blocks[k], want["blocks"][k]) for k in bad[:8]]))
    assert got.text == want["text"], what


def check(sw, cols, strand, seq_len, cig, status=None, set_=0, what="", ctx=None, shift=0, froms=(0, 1)):
    """Both seams against the model, for both values of `from`."""
    cols = {k: np.asarray(cols[k]).astype(np.uint32) for k in COLS}
    strand = np.asarray(strand).astype(np.uint8)
    seq_len = np.asarray(seq_len).astype(np.uint32)
    out = []
    for from_ in froms:
        got = both_seams(sw, cols, strand, seq_len, cig, status, set_, from_, ctx, shift)
        compare(got, um.chain_records(cols, strand, seq_len, cig, None if status is None else np.asarray(status) != 0, set_, from_), (what, from_))
        out.append(got)
    return out[0]


def records_of(texts, strands=None, gap=3):
    """One record per CIGAR text, query on sequence 0 and target on sequence 1, one behind the other: the sides are what the ops add
    up to (entries that do not parse get sides of their own).  -> (cols, strand, seq_len)"""
    n = len(texts)
    q, t, cols = 5, 7, {k: np.zeros(n, dtype=np.int64) for k in COLS}
    cols["t_id"][:] = 1
    for i, text in enumerate(texts):
        state, ops = em.parse(text)
        Lq, Lt = em.advances(ops) if text and not state else (7, 9)
        cols["q_start"][i], cols["q_end"][i], cols["t_start"][i], cols["t_end"][i] = q, q + Lq, t, t + Lt
        q, t = q + Lq + gap, t + Lt + gap
    assert q < 2**32 and t < 2**32
    strand = np.asarray(strands if strands is not None else np.arange(n) % 2).astype(np.uint8)
    return {k: v.astype(np.uint32) for k, v in cols.items()}, strand, np.array([q + 11, t + 13], dtype=np.uint32)


def check_texts(sw, texts, what="", strands=None, **kw):
    cols, strand, seq_len = records_of(texts, strands)
    return check(sw, cols, strand, seq_len, dict(enumerate(texts)), what=what, **kw)


def pairs(n, a="1=", b="1I"):
    """n ops: a b a b ..."""
    return "".join(a if k % 2 == 0 else b for k in range(n))


# ---- marks and block starts ------------------------------------------------------------------------------------------------------------
def test_hand_cases(sw):
    texts = [G, G, "10M", H, H, "2D4=1D", "2S1H3=0I0X0P2=4S", "3=0D0M2I0S2=", "5I3D", "0=0M", "3M2="]
    got = check_texts(sw, texts, "hand", strands=[0, 1, 0, 0, 1, 0, 1, 1, 0, 1, 0])
    assert [tuple(int(v) for v in b) for b in got.blocks[:6]] == [(5, 0, 2), (6, 4, 0), (7, 0, 0)] * 2
    assert got.chains["n_blocks"].tolist() == [3, 3, 1, 2, 2, 1, 1, 2, 0, 0, 1] and got.chains["score"].tolist() == [13, 13, 10, 6, 6, 4, 5, 5, 0, 0, 2]
    assert (got.n_chains, got.empty_chains, got.n_blocks) == (9, 2, 16) and got.text.startswith(b"5\t0\t2\n6\t4\t0\n7\n\n5\t0\t2\n")


@pytest.mark.parametrize("ops", [T - 1, T, T + 1])
def test_an_entry_of_about_one_tile_of_ops(sw, ops):
    for shift in (0, 5):
        got = check_texts(sw, [pairs(ops), "2=", pairs(ops, "1D", "3X")], "ops %d" % ops, shift=shift)
        assert got.ops == 2 * ops + 1 and got.chains["n_blocks"].tolist() == [(ops + 1) // 2, 1, ops // 2]


def test_a_block_and_a_gap_run_across_a_tile_border(sw):
    """1=1X1=... and 1I1D... each lying across the border between two op tiles: one block, one gap."""
    one = pairs(T - 7) + pairs(15, "1=", "1X") + pairs(T - 15, "2D", "1M") + pairs(13, "1I", "1D") + "3=" + "1I" * 2 + "0=" + "1D" * 3 + "4M"
    assert T - 7 < T < T + 8 and 2 * T - 7 < 2 * T < 2 * T + 6
    got = check_texts(sw, [one, "7=", one], "across", strands=[1, 0, 0])
    blocks = [tuple(int(v) for v in b) for b in got.blocks[:got.chains["n_blocks"][0]]]
    assert (16, 2, 0) in blocks                 # the =/X run of 15 ops, merged with the 1= in front of it
    assert (1, 8, 7) in blocks                  # the gap run of 13 ops, merged with the 2D in front of it
    assert (3, 3, 2) in blocks and blocks[-1] == (4, 0, 0)      # a gap around a zero-length '='


def test_runs_of_zero_length_ops_longer_than_two_tiles(sw):
    between_aligned = "3=" + "0I0S0=0D" * 600 + "2X"                                  # one block of 5
    beside_a_gap = "3=" + "0=0I" * 1100 + "2I" + "0D0P" * 1100 + "4="                 # 3 | dq 2 | 4
    lead = "0M" * 2100 + "1D" + "0I" * 2100 + "6=" + "0D" * 2100
    got = check_texts(sw, [between_aligned, beside_a_gap, lead, between_aligned], "zero runs", strands=[1, 1, 0, 0])
    assert [tuple(int(v) for v in b) for b in got.blocks] == [(5, 0, 0), (3, 0, 2), (4, 0, 0), (6, 0, 0), (5, 0, 0)]
    assert got.chains["n_blocks"].tolist() == [1, 2, 1, 1]


def test_one_cigar_of_100000_zero_length_ops(sw):
    got = check_texts(sw, ["2=", "0=" * 100_000 + "5=", "1I" + "0=" * 3000 + "3="], "10^5")
    assert got.ops == 103_004 and [tuple(int(v) for v in b) for b in got.blocks] == [(2, 0, 0), (5, 0, 0), (3, 0, 0)]


def test_entry_borders_on_tile_borders_entries_of_one_op_and_5000_entries(sw):
    """An entry border exactly on a tile border with aligned ops on both sides: two chains, not one block.  Entries of one op, and
    5,000 of them in 10 kB: every neighbour is aligned, every border is a reset."""
    got = check_texts(sw, [pairs(T - 1) + "1=", "2=" + pairs(T - 1, "1D", "1="), "1X", "9="], "border on a border")
    assert got.ops == 2 * T + 2 and got.chains["n_blocks"].tolist() == [T // 2, 1 + (T - 1) // 2, 1, 1]
    texts = [("1=", "2X", "3M", "4I", "5D", "0=", "7S")[k % 7] for k in range(5_000)]
    for shift in (0, 9):
        got = check_texts(sw, texts, "5000 entries", shift=shift)
        assert got.n_chains == got.n_blocks == sum(k % 7 < 3 for k in range(5_000)) and got.empty_chains == 5_000 - got.n_chains
    check_texts(sw, ["", "1=", "", "", "2I1=", ""], "empty entries between")


# ---- blocks, chains, the format ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, TB - 1, TB, TB + 1])
def test_block_counts_around_the_block_tile_reversed(sw, B):
    """On '-' seen from the query the blocks are reversed: across the border of the block kernel's tile, beside chains that are not."""
    rng = np.random.default_rng(B)
    def chain(b):
        out = []
        for j in range(b):
            out.append("%d=" % rng.integers(1, 2000))
            if j + 1 < b:
                out.append(("%dI" % rng.integers(1, 30), "%dD" % rng.integers(1, 30), "%dI%dD" % (rng.integers(1, 30), rng.integers(1, 30)))[int(rng.integers(0, 3))])
        return "".join(out)
    got = check_texts(sw, ["3=", chain(B), chain(5), chain(B), "4="], "B = %d" % B, strands=[1, 1, 0, 1, 1])
    assert got.chains["n_blocks"].tolist() == [1, B, 5, B, 1]


def built(blocks):
    return "".join("%d=" % s + ("%dD" % dt if dt else "") + ("%dI" % dq if dq else "") for s, dt, dq in blocks)


def test_numbers_of_1_to_10_digits_in_every_field(sw):
    """Built from the blocks, so that the expectation needs no expansion: sizes, dt and dq of 10^0 .. 10^9, each on a record of its
    own sequence pair; 4294967295= on a record that fits.  Both strands and both `from` values against the rules applied by hand."""
    from sweepga_amd.ucsc import ucsc_chain_records
    tens = [10**d for d in range(10)]
    chains = [[(s, 1, 0) for s in tens[:-1]] + [(tens[-1], 0, 0)], [(1, d, 0) for d in tens] + [(2, 0, 0)], [(1, 0, d) for d in tens] + [(2, 0, 0)],
              [(7, d, e) for d, e in zip(tens[::-1][:5], tens[:5])] + [(3, 0, 0)], [(2**32 - 1, 0, 0)]]
    n = len(chains)
    texts, strand = [built(c) for c in chains] * 2, np.array([0] * n + [1] * n, dtype=np.uint8)
    Lq = [sum(s + dq for s, _, dq in c) for c in chains] * 2
    Lt = [sum(s + dt for s, dt, _ in c) for c in chains] * 2
    assert max(Lq + Lt) == 2**32 - 1
    qs = [0 if L > 2**31 else 17 for L in Lq]
    ts = [0 if L > 2**31 else 29 for L in Lt]
    cols = {"q_id": np.arange(2 * n) * 2, "t_id": np.arange(2 * n) * 2 + 1, "q_start": qs, "q_end": [a + L for a, L in zip(qs, Lq)],
            "t_start": ts, "t_end": [a + L for a, L in zip(ts, Lt)]}
    cols = {k: np.asarray(v).astype(np.uint32) for k, v in cols.items()}
    seq_len = np.zeros(4 * n, dtype=np.uint32)
    seq_len[0::2] = [min(e + 3, 2**32 - 1) for e in cols["q_end"].tolist()]
    seq_len[1::2] = [min(e + 5, 2**32 - 1) for e in cols["t_end"].tolist()]
    cig = dict(enumerate(texts))
    for from_ in (0, 1):
        got = both_seams(sw, cols, strand, seq_len, cig, from_=from_)
        want_blocks, want_rows, text = [], [], b""
        for i in range(2 * n):
            c, minus = chains[i % n], int(strand[i])
            qsz, tsz = int(seq_len[2 * i]), int(seq_len[2 * i + 1])
            base = (ts[i], ts[i] + Lt[i], tsz, minus, (qsz - qs[i] - Lq[i]) if minus else qs[i], ((qsz - qs[i] - Lq[i]) if minus else qs[i]) + Lq[i], qsz, c)
            ch = um.swap(base) if from_ else base
            want_rows.append((i, minus, ch[0], ch[1], ch[4], ch[5], sum(s for s, _, _ in c), len(c), len(want_blocks), len(text)))
            want_blocks += ch[7]
            text += um.block_text(ch[7]).encode()
        assert [tuple(int(v) for v in b) for b in got.blocks] == want_blocks, from_
        assert got.chains.tobytes() == um.rows_array(want_rows).tobytes(), from_
        assert got.text == text and got.state.tolist() == [0] * (2 * n) and got.n_chains == 2 * n
    assert b"\n4294967295\n\n" in text and b"1\t1000000000\t0\n" in text and b"\t1000000000\n" in text and b"1000000000\n\n" in text
    # the same numbers through the host seam's capacities: a text one byte short is not written
    ctx = sw.default_context()
    short = ucsc_chain_records(ctx, cols, strand, 4 * n, seq_len, list(range(2 * n)), texts, capacity=(2 * n, len(want_blocks), len(text) - 1))
    assert short.text is None and short.text_bytes == len(text) and short.blocks is not None


def test_every_state_beside_intact_neighbours(sw):
    good = "4=1I3=1D2="
    bad = ["5=x5=", "4294967296D10=", "9=1I", "9=1D", "", "7", "M3=", "3=3", "3=\t2="]
    texts = []
    for b in bad:
        texts += [good, b]
    texts.append(good)
    cols, strand, seq_len = records_of(texts)
    k = len(texts)
    cols["q_end"][5] = cols["q_start"][5] + 11           # "9=1I": x = 10, the record says 11 -> 4
    cols["t_end"][5] = cols["t_start"][5] + 9
    cols["q_end"][7] = cols["q_start"][7] + 9            # "9=1D": y = 10, the record says 11 -> 8
    cols["t_end"][7] = cols["t_start"][7] + 11
    got = check(sw, cols, strand, seq_len, dict(enumerate(texts)), what="states")
    assert got.state.tolist()[1::2] == [1, 2, 4, 8, 16, 1, 1, 1, 1] and set(got.state.tolist()[0::2]) == {0}
    assert got.n_chains == len(bad) + 1 and got.cigar_bad == 8 and got.n_blocks == 3 * got.n_chains and got.empty_chains == 0
    # state 32 on either axis, alone and beside other bits; ending AT the size is inside
    seq_len = np.array([int(cols["q_end"][k - 3]), int(cols["t_end"][k - 5])], dtype=np.uint32)
    got = check(sw, cols, strand, seq_len, dict(enumerate(texts)), what="beyond")
    want = [0, 1, 0, 2, 0, 4, 0, 8, 0, 16, 0, 1, 0, 1, 0, 1 | 32, 32, 1 | 32, 32]
    assert got.state.tolist() == want and got.beyond == 4 and got.n_chains == 8
    assert int(cols["q_end"][k - 3]) == int(seq_len[0]) and got.state[k - 3] == 32     # (its target end is beyond; the query end is not)
    seq_len = np.array([int(cols["q_end"][k - 5]), int(cols["t_end"][k - 1])], dtype=np.uint32)      # ... and on the query alone
    got = check(sw, cols, strand, seq_len, dict(enumerate(texts)), what="beyond on the query")
    assert got.state.tolist()[k - 5:] == [0, 33, 32, 33, 32] and got.beyond == 4


# ---- the protocol ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(7)
    cols, strand, texts = random_case(rng, 600, 4)
    return cols, strand, texts, np.full(4, 300_000, dtype=np.uint32), (rng.random(600) < 0.6).astype(np.uint8)


def raw_call(sw, fn, cols, strand, seq_len, cig, caps, set_=0, from_=0, status=None, ctx=None, null=()):
    """A record seam with caller arrays full of 0xAB -> (rc, request, chains, blocks, text, state bytes)"""
    from sweepga_amd import _lib
    from sweepga_amd.lift import cigar_set
    ctx = ctx or sw.default_context()
    rec = _lib.SwgRecords()
    rec.n = len(strand)
    keep = {k: np.ascontiguousarray(cols[k], dtype=np.uint32) for k in COLS}
    for k, a in keep.items():
        setattr(rec, k, a.ctypes.data)
    rec.strand, rec.n_seq = strand.ctypes.data, len(seq_len) if seq_len is not None else 4
    record, offset, text = cig if isinstance(cig, tuple) else cigar_set(sorted(cig), [cig[i] for i in sorted(cig)])
    cs = _lib.SwgCigarSet()
    cs.record, cs.offset, cs.text, cs.k = record.ctypes.data, offset.ctypes.data, text.ctypes.data, len(record)
    arrays = [np.full(size * max(c, 1), 0xab, dtype=np.uint8) for size, c in zip((48, 12, 1), caps)]
    state = np.full(max(len(record), 1), 0xab, dtype=np.uint8)
    req = _lib.SwgUcscRequest()
    req.set, req.from_, req.state, req.n_blocks = set_, from_, state.ctypes.data, 99
    req.chain_capacity, req.block_capacity, req.text_capacity = caps
    req.chains, req.blocks, req.text = (None if k in null else a.ctypes.data for k, a in enumerate(arrays))
    rc = fn(ctx.handle, C.byref(rec), seq_len.ctypes.data if seq_len is not None else None, status.ctypes.data if status is not None else None,
            C.byref(cs), C.byref(req))
    return (rc, req) + tuple(a.tobytes() for a in arrays) + (state.tobytes(),)


def test_capacities_with_poisoned_arrays(sw, small):
    cols, strand, texts, seq_len, _ = small
    lib = sw.default_context().lib
    cig = dict(enumerate(texts))
    want = um.chain_records(cols, strand, seq_len, cig)
    counts = (600, want["n_blocks"], want["text_bytes"])
    full = (um.rows_array(want["rows"]).tobytes(), np.array(want["blocks"], dtype=np.uint32).tobytes(), want["text"])
    assert counts[1] > 600 and counts[2] > 4 * counts[1]
    for which in range(3):
        for cap in (0, counts[which] - 1, counts[which]):
            caps = tuple(cap if k == which else counts[k] for k in range(3))
            rc, req, *arrays, state = raw_call(sw, lib.swg_ucsc_chain_records, cols, strand, seq_len, cig, caps)
            assert rc == 0 and (req.n_chains, req.n_blocks, req.text_bytes) == (want["n_chains"], counts[1], counts[2]) and list(state) == want["state"]
            for k in range(3):
                if caps[k] < counts[k]:
                    assert set(arrays[k]) == {0xab}, (which, cap, k)      # an array that does not hold its count is left alone
                else:
                    assert arrays[k] == full[k], (which, cap, k)
    rc, req, *arrays, state = raw_call(sw, lib.swg_ucsc_chain_records, cols, strand, seq_len, cig, counts, null=(0, 1, 2))
    assert rc == 0 and req.text_bytes == counts[2] and all(set(a) == {0xab} for a in arrays)


def test_no_entries_a_set_never_in_status_and_a_partial_set(sw, small):
    from sweepga_amd.ucsc import ucsc_chain_records
    cols, strand, texts, seq_len, status = small
    ctx = sw.default_context()
    got = ucsc_chain_records(ctx, cols, strand, 4, seq_len, [], [])
    assert (got.n_chains, got.n_blocks, got.text_bytes, got.ops, len(got.chains), got.text) == (0, 0, 0, 0, 0, b"")
    every = dict(enumerate(texts))
    none = check(sw, cols, strand, seq_len, every, status=np.zeros(600, dtype=np.uint8), set_=1, what="never in status")
    assert (none.n_chains, none.n_blocks, none.text, none.empty_chains) == (0, 0, b"", 0) and set(none.state.tolist()) == {0}
    kept = check(sw, cols, strand, seq_len, every, status=status, set_=1, what="kept")
    assert kept.n_chains == int(status.sum()) - kept.empty_chains and 0 < kept.n_chains < 600
    check(sw, cols, strand, seq_len, {i: texts[i] for i in range(0, 600, 3)}, status=status, set_=1, what="a partial set")


def test_refusals(sw, small):
    from sweepga_amd.lift import cigar_set
    from sweepga_amd.ucsc import ucsc_chain_records, ucsc_chain_records_device
    cols, strand, texts, seq_len, status = small
    ctx = sw.default_context()
    lib = ctx.lib
    good = cigar_set([3, 5, 9], ["1=", "2=", ""])
    bad_sets = [(np.array([3, 3, 9], dtype=np.uint32), good[1], good[2]), (np.array([5, 3, 9], dtype=np.uint32), good[1], good[2]),
                (np.array([3, 5, 600], dtype=np.uint32), good[1], good[2]), (good[0], np.array([0, 4, 2, 4], dtype=np.uint64), good[2]),
                (good[0], np.array([1, 2, 4, 4], dtype=np.uint64), good[2])]
    hip = Hip()
    try:
        dcols = {k: Dev(hip, cols[k], np.uint32) for k in COLS}
        dstrand, dlen = Dev(hip, strand, np.uint8), Dev(hip, seq_len, np.uint32)
        for record, offset, text in bad_sets:
            rc, req, chains, blocks, txt, state = raw_call(sw, lib.swg_ucsc_chain_records, cols, strand, seq_len, (record, offset, text), (4, 4, 64))
            assert rc == -1 and set(chains) == set(state) == {0xab} and req.n_blocks == 99, (record, offset)
            with pytest.raises(sw.SwgError) as e:
                ucsc_chain_records_device(ctx, dcols, dstrand, 4, dlen, Dev(hip, record), Dev(hip, offset), Dev(hip, text), 3)
            assert e.value.code == -1, (record, offset)
        with pytest.raises(sw.SwgError) as e:      # a NULL seq_len: the '-' strand needs the sizes
            ucsc_chain_records_device(ctx, dcols, dstrand, 4, None, Dev(hip, good[0]), Dev(hip, good[1]), Dev(hip, good[2]), 3)
        assert e.value.code == -1 and "seq_len" in str(e.value)
    finally:
        hip.free()
    for fn in (lib.swg_ucsc_chain_records, lib.swg_ucsc_chain_records_device):      # k is looked at before any array
        from sweepga_amd import _lib
        cs = _lib.SwgCigarSet()
        cs.record, cs.offset, cs.text, cs.k = good[0].ctypes.data, good[1].ctypes.data, good[2].ctypes.data, 2**31
        rec = _lib.SwgRecords()
        rec.n, rec.n_seq = 600, 4
        assert fn(ctx.handle, C.byref(rec), seq_len.ctypes.data, None, C.byref(cs), C.byref(_lib.SwgUcscRequest())) == -5
    rc, req, chains, *_ = raw_call(sw, lib.swg_ucsc_chain_records, cols, strand, None, good, (4, 4, 64))
    assert rc == -1 and set(chains) == {0xab} and b"seq_len" in lib.swg_last_error(ctx.handle)
    for kw in ({"set": 2}, {"from_": 2}, {"set": 1}):      # (set 1: KEPT without a status)
        with pytest.raises(sw.SwgError) as e:
            ucsc_chain_records(ctx, cols, strand, 4, seq_len, [3], ["1="], **kw)
        assert e.value.code == -1
    with pytest.raises(sw.SwgError) as e:      # a set for no records
        ucsc_chain_records(ctx, {k: np.zeros(0, dtype=np.uint32) for k in COLS}, np.zeros(0, dtype=np.uint8), 4, seq_len, [0], ["1="])
    assert e.value.code == -1


def test_a_memory_limit_too_small_is_a_clean_oom(sw, small):
    from sweepga_amd.ucsc import ucsc_chain_records
    cols, strand, texts, seq_len, _ = small
    ctx = sw.Context(0)
    try:
        long = "1=1I" * 100_000      # 400 kB of text, 2 * 10^5 ops: 32 bytes of prefix sums each, 6.4 MB
        c1 = {"q_id": [0], "t_id": [1], "q_start": [0], "q_end": [200_000], "t_start": [0], "t_end": [100_000]}
        c1 = {k: np.array(v, dtype=np.uint32) for k, v in c1.items()}
        ctx.set_memory_limit(4 << 20)
        with pytest.raises(sw.SwgError) as e:
            ucsc_chain_records(ctx, c1, np.zeros(1, dtype=np.uint8), 2, [200_000, 100_000], [0], [long])
        assert e.value.code == -4
        got = ucsc_chain_records(ctx, cols, strand, 4, seq_len, list(range(600)), texts)      # the same context, a call that fits
        compare(got, um.chain_records(cols, strand, seq_len, dict(enumerate(texts))), "under the limit")
        ctx.set_memory_limit(0)
        got = ucsc_chain_records(ctx, c1, np.zeros(1, dtype=np.uint8), 2, [200_000, 100_000], [0], [long], from_=1)
        assert got.n_blocks == 100_000 and got.text == b"1\t1\t0\n" * 99_999 + b"1\n\n" and tuple(got.chains[0])[2:8] == (0, 199_999, 0, 100_000, 100_000, 100_000)
    finally:
        ctx.close()


def test_smallest_shapes_on_a_fresh_context(sw):
    """The seams around the kernels at the smallest shapes -- one record; three records -- with and without a status, on a context of
    its own: its first call sizes the arena from the input, the later ones find it sized.  Each shape twice, host seam against device
    seam byte for byte and both against the model."""
    texts = [G, "10M", H]
    cols, strand, seq_len = records_of(texts)
    ctx = sw.Context(0)
    try:
        for n in (1, 3, 1, 3):
            part = {k: v[:n] for k, v in cols.items()}
            for status in (None, np.array([1, 0, 1], dtype=np.uint8)[:n]):
                got = check(sw, part, strand[:n], seq_len, dict(enumerate(texts[:n])), status=status, set_=0 if status is None else 1, what=f"n = {n}", ctx=ctx)
                assert got.n_chains == (n if status is None else (n + 1) // 2) and got.chains["n_blocks"][0] == 3
    finally:
        ctx.close()


# ---- the whole path ------------------------------------------------------------------------------------------------------------------------
def test_write_the_python_class_and_the_command_line_for_every_batch_size(sw, tmp_path):
    from sweepga_amd import build
    text, kept = mixed_paf()
    st = kept.astype(np.uint8)
    out = tmp_path / "x.chain"
    with sw.PafFile(text=text) as paf:
        for set_, status in ((0, None), (1, st), (0, st)):
            n_records = 14 if set_ == 0 else int(kept.sum())
            for from_ in (0, 1):
                want, counts = um.paf_chain_text(text, kept, set_, from_)
                assert want.count("chain ") == counts["chains"] > 5
                for batch in (1, 100, 4096, 0):
                    got = sw.UcscChain.from_paf(paf, status, from_=from_, set=set_, batch_bytes=batch)
                    assert got.text == want, (set_, from_, batch)
                    assert {k: v for k, v in got.counts.items() if k != "batches"} == counts
                    assert sw.UcscChain.write_paf(paf, status, out, from_=from_, set=set_, batch_bytes=batch) == got.counts and out.read_text() == want
                    # every record a batch of its own, or one batch (the whole text is 100-odd bytes: 100, 4096 and 0 cannot differ)
                    assert got.counts["batches"] == (n_records if batch == 1 else 1)
                assert len(got.chains) == counts["chains"] and sum(len(b) for b in got.blocks) == counts["blocks"]
                assert [c[-1] for c in got.chains] == list(range(1, counts["chains"] + 1))
    # the command line: a real 1:1 filter, the chain file of what it keeps; the output PAF does not change
    rng = np.random.default_rng(12)
    cols, strand, texts = random_case(rng, 2_000, 6)
    lines = []
    for i in range(2_000):
        f = ["g%d#1#c" % cols["q_id"][i], "400000", str(cols["q_start"][i]), str(cols["q_end"][i]), "-" if strand[i] else "+",
             "g%d#1#c" % cols["t_id"][i], "400000", str(cols["t_start"][i]), str(cols["t_end"][i]), "50", "60", "60"]
        tags = (["tp:A:P", "cg:Z:" + texts[i]], ["cg:Z:" + texts[i], "nm:i:3"], ["tp:A:P"], ["cg:Z:1M", "cg:Z:" + texts[i]], ["cg:Z:"], ["cg:Z:" + texts[i] + "9"])[i % 6]
        lines.append("\t".join(f + tags))
    big = "\n".join(lines) + "\n"
    inp, plain, outp = tmp_path / "in.paf", tmp_path / "plain.paf", tmp_path / "out.paf"
    inp.write_text(big, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-jump", "10k", "--scaffold-mass", "2k"]
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), *flags, "--quiet"], capture_output=True)
    assert r0.returncode == 0 and plain.stat().st_size > 0, r0.stderr
    kept = kept_mask(big, plain.read_bytes().decode())
    with sw.PafFile(text=big) as paf:      # every batch size gives the same bytes, and the number of batches the planner's rule says
        for set_, from_ in ((1, 0), (0, 1)):
            want, c = um.paf_chain_text(big, kept, set_, from_)
            got = [sw.UcscChain.from_paf(paf, kept.astype(np.uint8), from_=from_, set=set_, batch_bytes=b) for b in (1, 100, 4096, 0)]
            assert all(g.text == want for g in got) and all({k: v for k, v in g.counts.items() if k != "batches"} == c for g in got)
            batches = [g.counts["batches"] for g in got]
            assert batches == [um.paf_batches(big, kept, set_, b) for b in (1, 100, 4096, 0)] and batches[0] > batches[1] > batches[2] >= batches[3] == 1
            assert set_ == 1 or len(set(batches)) == 4      # (the kept set's text is below 4,096 bytes: there 4,096 and 0 cannot differ)
    for extra, set_, from_ in (([], 1, 0), (["--ucsc-chain-from", "query", "--ucsc-chain-set", "all", "--ucsc-chain-batch", "2k"], 0, 1)):
        want, c = um.paf_chain_text(big, kept, set_, from_)
        r = subprocess.run([build.CLI, str(inp), "--output-file", str(outp), "--ucsc-chain", str(out), *extra, *flags], capture_output=True)
        assert r.returncode == 0 and r.stdout == b"" and outp.read_bytes() == plain.read_bytes(), r.stderr
        # the case is not a trivial one: 4 of the 6 kinds of line carry a usable tag and a random CIGAR rarely lacks an aligned op, so
        # more than a third of the set's records give chains (the kept set of the 1:1 filter is well over 100 of the 2,000 records)
        assert out.read_text() == want and c["records"] > 100 and 3 * c["chains"] > c["records"]
        assert ("--ucsc-chain: %d chains of %d records, %d blocks, %d bad, %d beyond, %d without a cg:Z: tag, %d without an aligned column\n"
                % (c["chains"], c["records"], c["blocks"], c["bad"], c["beyond"], c["untagged"], c["empty"])) in r.stderr.decode()
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(outp), "--ucsc-chain", str(out), "--no-filter", "--quiet"], capture_output=True)
    assert r.returncode == 0 and out.read_text() == um.paf_chain_text(big, None, 0, 0)[0], r.stderr


def test_20000_records_built_from_random_cigars(sw):
    """5 % of the entries are corrupted, 5 % of the records are left out of the set, a real 1:1 status picks the kept set."""
    rng = np.random.default_rng(9)
    n, n_seq = 20_000, 12
    cols, strand, texts = random_case(rng, n, n_seq)
    lines = []
    for i in range(n):
        lines.append("\t".join(["g%d#1#c" % cols["q_id"][i], "400000", str(cols["q_start"][i]), str(cols["q_end"][i]), "-" if strand[i] else "+",
                                "g%d#1#c" % cols["t_id"][i], "400000", str(cols["t_start"][i]), str(cols["t_end"][i]), "50", "60", "60"]))
    with sw.PafFile(text="\n".join(lines) + "\n") as paf:
        status, _ = run_filter(sw, paf, filter_cfgs(sw)["one_to_one"])
        pcols = {c: paf.column(c).copy() for c in COLS}      # (the handle's ids: names in order of first appearance)
        pstrand, p_seq = paf.column("strand").copy(), int(paf.records.n_seq)
    assert 0 < int((status != 0).sum()) < n
    roll = rng.random(n)
    cig = {i: (corrupt(texts[i], rng) if roll[i] < 0.05 else texts[i]) for i in range(n) if roll[i] >= 0.10 or roll[i] < 0.05}
    seq_len = np.full(p_seq, 199_000, dtype=np.uint32)      # starts are uniform below 200,000: about 1 record in 200 ends beyond it
    for set_, from_ in ((0, 0), (1, 1)):
        got = check(sw, pcols, pstrand, seq_len, cig, status=status, set_=set_, what="random, set %d" % set_, froms=(from_,))
        assert int((got.state == 0).sum()) >= 0.85 * len(cig) and got.cigar_bad > 0.03 * len(cig) and got.beyond > 0
        assert got.n_chains > (15_000, 0)[set_] and got.n_blocks > got.n_chains
