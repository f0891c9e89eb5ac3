"""The base-exact lift on the device (sweepga_amd/csrc/swg_cigar.hip) against tests/lift_exact_model.py: in every case the host seam
against the model and the device seam against the host seam, row for row, state for state.  The shapes are the smallest at which
each part can go wrong: the parser's tile of 4,096 text bytes and its borders, a number in front of a border, entries of one op, empty
entries, more entries than a tile has bytes, every rejection beside intact neighbours; the scans' tile of 4,096 ops, one CIGAR of 10^5
ops, clips that cut an op at its first and last base; the set and capacity protocol; a random case built from CIGARs; the texts of
swg_paf_lift_exact / Lift.from_paf(exact=True) / --lift-exact byte for byte.  Every comparison is exact: integers and bytes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import lift_exact_model as em
from tests import lift_model as lm
from tests.test_gpu_alnstats import filter_cfgs, run_filter
from tests.test_gpu_intervals import kept_mask
from tests.test_gpu_lift import Dev
from tests.test_gpu_wide import Hip
from tests.test_lift_exact_cpu import hand_case

pytestmark = pytest.mark.gpu
COLS = lm.COLS
TILE = 4096      # text bytes per parser tile, and elements per tile of the library's scans


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context()
    return sweepga_amd


def n_ops(texts):
    return sum(sum(ch not in "0123456789" for ch in t) for t in texts)


def same(a, b):
    return (a.n == b.n and a.candidates == b.candidates and np.array_equal(a.summary, b.summary) and a.rows.tobytes() == b.rows.tobytes()
            and a.state.tobytes() == b.state.tobytes() and (a.ops, a.cigar_bad, a.exact_rows) == (b.ops, b.cigar_bad, b.exact_rows))


def both_seams(sw, cols, strand, n_seq, regions, cig, status=None, set_=0, axes=3, ctx=None, shift=0):
    """The result of the host seam, after checking that the device seam gives the same.  shift: the device text starts that many
    bytes behind a 16-byte boundary."""
    from sweepga_amd.lift import cigar_set, lift_exact_records, lift_exact_records_device, regions_array
    ctx = ctx or sw.default_context()
    recs = sorted(cig)
    got = lift_exact_records(ctx, cols, strand, n_seq, regions, recs, [cig[i] for i in recs], status=status, set=set_, axes=axes)
    regs = regions_array(regions)
    record, offset, text = cigar_set(recs, [cig[i] for i in recs])
    hip = Hip()
    try:
        dcols = {k: Dev(hip, cols[k], np.uint32) for k in COLS}
        dtext = Dev(hip, np.concatenate([np.zeros(shift, dtype=np.uint8), text]))
        dtext.ptr += shift
        dev = lift_exact_records_device(ctx, dcols, Dev(hip, strand, np.uint8), n_seq, Dev(hip, regs.view(np.uint32)), len(regs),
                                        Dev(hip, record), Dev(hip, offset), dtext, len(recs),
                                        status=Dev(hip, status, np.uint8) if status is not None else None, set=set_, axes=axes)
    finally:
        hip.free()
    assert same(dev, got)
    return got


def check(sw, cols, strand, n_seq, regions, cig, status=None, set_=0, axes=3, what="", ctx=None, shift=0):
    """Both seams against the model."""
    cols = {k: np.asarray(cols[k]).astype(np.uint32) for k in COLS}
    strand = np.asarray(strand).astype(np.uint8)
    got = both_seams(sw, cols, strand, n_seq, regions, cig, status, set_, axes, ctx, shift)
    rows, summary, states = em.lift_exact(cols, strand, None if status is None else np.asarray(status) != 0, regions, cig, set_, axes)
    assert got.n == len(rows) == len(got.rows), (what, got.n, len(rows))
    want = em.rows_array(rows)
    if got.rows.tobytes() != want.tobytes():
        bad = [k for k in range(len(rows)) if got.rows[k].tobytes() != want[k].tobytes()]
        raise AssertionError((what, len(bad), [(tuple(got.rows[k]), rows[k]) for k in bad[:5]]))
    assert np.array_equal(got.summary, summary), what
    want_state = [states[i] for i in sorted(cig)]
    assert got.state.tolist() == want_state, (what, [(i, a, b) for i, a, b in zip(sorted(cig), got.state.tolist(), want_state) if a != b][:8])
    assert got.ops == n_ops(cig.values()), (what, got.ops)
    assert got.cigar_bad == sum(0 < s < em.EMPTY for s in want_state), what
    assert got.exact_rows == sum(1 for r in rows if r[7] & em.EXACT), what
    return got


def records_of(texts, rng, strands=None):
    """One record per CIGAR text, query on sequence 0 and target on sequence 1, one behind the other with gaps: the sides are what
    the ops add up to (entries that do not parse get sides of their own); a record whose target side is longer than 2^31 lies alone
    on sequence 2, from 0.  -> (cols, strand)"""
    n = len(texts)
    q, t, cols = 0, 0, {k: np.zeros(n, dtype=np.int64) for k in COLS}
    cols["t_id"][:] = 1
    for i, text in enumerate(texts):
        state, ops = em.parse(text)
        Lq, Lt = em.advances(ops) if text and not state else (7, 9)
        q += int(rng.integers(0, 4))
        t += int(rng.integers(0, 4))
        if Lt > 2**31:
            cols["t_id"][i] = 2
            cols["q_start"][i], cols["q_end"][i], cols["t_start"][i], cols["t_end"][i] = q, q + Lq, 0, Lt
            q += Lq
            continue
        cols["q_start"][i], cols["q_end"][i], cols["t_start"][i], cols["t_end"][i] = q, q + Lq, t, t + Lt
        q, t = q + Lq, t + Lt
    assert q < 2**32 and t < 2**32
    strand = np.asarray(strands if strands is not None else rng.integers(0, 2, n)).astype(np.uint8)
    return {k: v.astype(np.uint32) for k, v in cols.items()}, strand


def regions_over(cols, rng, m, width=40):
    """m regions on both sequences, most of them short, and the two whole sequences"""
    out = [(0, 0, int(cols["q_end"].max())), (1, 0, int(cols["t_end"].max()))]
    for k in range(m):
        seq = k & 1
        top = int((cols["t_end"] if seq else cols["q_end"]).max())
        a = int(rng.integers(0, max(top, 1)))
        out.append((seq, a, min(a + int(rng.integers(1, width)), 2**32 - 1)))
    return out


def filler(nbytes, rng):
    """A CIGAR text of exactly nbytes (>= 2): ops of length 1 to 3, one two-digit op when nbytes is odd"""
    assert nbytes >= 2
    out = []
    if nbytes % 2:
        out.append("1%d%s" % (rng.integers(0, 4), "=XMID"[int(rng.integers(0, 5))]))
        nbytes -= 3
    out += ["%d%s" % (rng.integers(1, 4), "==XMIDSN"[int(rng.integers(0, 8))]) for _ in range(nbytes // 2)]
    order = rng.permutation(len(out))
    return "".join(out[k] for k in order)


def test_hand_case(sw):
    cols, strand, regions, cigars, rows, states = hand_case()
    got = check(sw, cols, strand, 2, regions, cigars, what="hand")
    assert [tuple(int(v) for v in r) for r in got.rows] == rows
    assert got.state.tolist() == [states[i] for i in sorted(cigars)] and got.cigar_bad == 4 and got.exact_rows == 16
    check(sw, cols, strand, 2, regions, cigars, status=(np.arange(len(strand)) % 2).astype(np.uint8), set_=1, what="hand, kept")


# ---- the parser ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbytes", [TILE - 1, TILE, TILE + 1])
def test_text_of_about_one_tile(sw, nbytes):
    rng = np.random.default_rng(nbytes)
    for parts in ((nbytes,), (1000, nbytes - 1000), (nbytes - 2, 2)):
        texts = [filler(p, rng) for p in parts]
        assert sum(len(t) for t in texts) == nbytes
        cols, strand = records_of(texts, rng)
        for shift in (0, 5):      # (the device text on and off a 16-byte boundary)
            check(sw, cols, strand, 2, regions_over(cols, rng, 60), dict(enumerate(texts)), what="%d bytes" % nbytes, shift=shift)


def test_numbers_in_front_of_tile_borders(sw):
    """Border b (of 10) has a number of b digits right in front of it and the number's letter as the tile's first byte; the op
    belongs to an entry that began earlier in the tile, except at the even borders, where the entry begins with the number.  Then an
    entry border exactly on a tile border, with the next entry's first number of one digit."""
    rng = np.random.default_rng(2)
    texts, at = [], 0
    for b in range(1, 11):
        number = str(10**(b - 1) + b)
        room = b * TILE - at - b      # bytes in front of the number
        if b % 2:
            texts.append(filler(room, rng) + number + "D" + filler(20, rng))
        else:
            texts += [filler(room, rng), number + "D" + filler(21, rng)]
        at = sum(len(t) for t in texts)
    texts.append(filler(11 * TILE - at, rng))      # ends on the border
    texts.append("7=" + filler(30, rng))           # begins on it
    offs = np.cumsum([0] + [len(t) for t in texts])
    assert 11 * TILE in offs and all("".join(texts)[b * TILE] == "D" for b in range(1, 11))
    cols, strand = records_of(texts, rng)
    got = check(sw, cols, strand, 2, regions_over(cols, rng, 300, 200), dict(enumerate(texts)), what="borders")
    assert not got.state.any()


def test_entries_of_one_op_empty_entries_and_more_entries_than_a_tile_has_bytes(sw):
    rng = np.random.default_rng(3)
    texts = ["5=", "", "3X", "", "", "2I", "4D", "1M"] + ["1="] * 2000 + [""] * 700 + ["2="] * 2200 + ["", "9="]
    cols, strand = records_of(texts, rng)
    got = check(sw, cols, strand, 2, regions_over(cols, rng, 200, 30), dict(enumerate(texts)), what="small entries")
    assert int((got.state == em.EMPTY).sum()) == 704 and got.cigar_bad == 0 and got.ops == 4206
    # a set of empty entries only: no text at all
    check(sw, cols, strand, 2, regions_over(cols, rng, 20, 30), {i: "" for i in range(0, 50, 3)}, what="no text")


def test_rejections_beside_intact_neighbours(sw):
    rng = np.random.default_rng(4)
    faulty = [("2I4294967295D", 0), ("3=4294967296D", em.VALUE), ("12345678901M", em.SYNTAX), ("00000000001M", em.SYNTAX), ("M3=", em.SYNTAX),
              ("3=I2=", em.SYNTAX), ("3=5", em.SYNTAX), ("3=2m1=", em.SYNTAX), ("3= 2=", em.SYNTAX), ("5", em.SYNTAX),
              ("4294967296D5", em.SYNTAX | em.VALUE), ("0000000003=", 0), ("0M0I0D3=0S0H0P0N0X", 0)]
    texts = []
    for f, _ in faulty:
        texts += [filler(int(rng.integers(2, 40)), rng), f]
    texts.append(filler(24, rng))
    cols, strand = records_of(texts, rng)
    regions = regions_over(cols, rng, 200, 30) + [(2, 0, 2**32 - 1), (2, 0, 1), (2, 2**32 - 2, 2**32 - 1), (2, 5, 5)]
    got = check(sw, cols, strand, 3, regions, dict(enumerate(texts)), what="rejections")
    assert got.state[1::2].tolist() == [s for _, s in faulty] and not got.state[0::2].any()
    # the same entries with a rejected one at each end of the text and across a tile border
    texts = ["3=5"] + [filler(TILE - 5, rng), "12345678901M"] + texts + ["x"]
    cols, strand = records_of(texts, rng)
    check(sw, cols, strand, 3, regions_over(cols, rng, 100, 30) + [(2, 0, 2**32 - 1)], dict(enumerate(texts)), what="rejections at the ends")


# ---- prefix sums and searches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ops", [TILE - 1, TILE, TILE + 1])
def test_a_record_of_about_one_scan_tile_of_ops(sw, ops):
    rng = np.random.default_rng(ops)
    texts = [filler(2 * ops, rng), filler(10, rng)]
    cols, strand = records_of(texts, rng, strands=[ops & 1, 0])
    got = check(sw, cols, strand, 2, regions_over(cols, rng, 150, 60), dict(enumerate(texts)), what="%d ops" % ops)
    assert got.ops == ops + 5


def test_one_cigar_of_100000_ops(sw):
    rng = np.random.default_rng(5)
    kinds = rng.choice(list("=XMID"), 100_000, p=[0.6, 0.1, 0.1, 0.1, 0.1])
    lens = rng.integers(1, 4, 100_000)
    text = "".join("%d%s" % (l, k) for l, k in zip(lens, kinds))
    for minus in (0, 1):
        cols, strand = records_of([text], rng, strands=[minus])
        ops = em.parse(text)[1]
        qs, qe, ts, te = (int(cols[k][0]) for k in ("q_start", "q_end", "t_start", "t_end"))
        regions = [(0, qs, qs + 1), (0, qe - 1, qe), (1, ts, ts + 1), (1, te - 1, te), (0, qs, qe), (1, ts, te)]      # the first op, the last op, the whole
        x = y = 0
        seen = set()
        for l, ch in ops[:400] + ops[-400:]:      # every op kind, cut at its first and at its last base, on the side it advances
            if ch not in seen or rng.random() < 0.02:
                seen.add(ch)
                if ch != "D":
                    regions += [(0, qs + x, qs + x + 1), (0, qs + x + l - 1, qs + x + l + 2), (0, max(qs + x - 1, qs), qs + x + 1)]
                if ch != "I":
                    regions += [(1, ts + y, ts + y + 1), (1, ts + y + l - 1, ts + y + l + 2), (1, max(ts + y - 1, ts), ts + y + 1)]
            x += l if ch != "D" else 0
            y += l if ch != "I" else 0
        regions += [(int(s), int(a), int(a + w)) for s, a, w in zip(rng.integers(0, 2, 40), rng.integers(0, 150_000, 40), rng.integers(1, 5_000, 40))]
        assert seen == set("=XMID")
        got = check(sw, cols, strand, 2, regions, {0: text}, what="10^5 ops, strand %d" % minus)
        assert got.ops == 100_000 and got.exact_rows == got.n > 40


def test_sums_off_by_one(sw):
    rng = np.random.default_rng(6)
    texts = [filler(30, rng) for _ in range(6)]
    cols, strand = records_of(texts, rng)
    for i, (k, d) in enumerate((("q_end", 1), ("t_end", 1), ("q_start", 1), ("t_start", 1), ("q_end", 0))):
        cols[k][i] += d
    cols["t_end"][4] += 1
    got = check(sw, cols, strand, 2, regions_over(cols, rng, 60, 30), dict(enumerate(texts)), what="sums")
    assert got.state.tolist() == [em.Q_SUM, em.T_SUM, em.Q_SUM, em.T_SUM, em.T_SUM, 0]
    # sums beyond 32 bits: 2^32 - 1 D twice against a target side of 2^32 - 2 is a mismatch, not a wrap-around match
    big = str(2**32 - 1) + "D"
    cols = {"q_id": [0], "t_id": [1], "q_start": [5], "q_end": [8], "t_start": [1], "t_end": [2**32 - 1]}
    got = check(sw, cols, [0], 2, [(0, 0, 100), (1, 0, 2**32 - 1)], {0: "3=" + big + big}, what="64-bit sums")
    assert got.state.tolist() == [em.T_SUM]
    got = check(sw, cols, [0], 2, [(0, 0, 100), (1, 0, 2**32 - 1), (1, 3, 9), (1, 2**32 - 3, 2**32 - 2)], {0: "2=" + str(2**32 - 5) + "D1="}, what="a long D")
    assert got.state.tolist() == [0] and got.exact_rows == 4


# ---- the set and the protocol ------------------------------------------------------------------------------------------------------------
def random_case(rng, n, n_seq, max_ops=12):
    """n records built FROM random CIGARs: every entry is consistent by construction."""
    kinds, texts = list("=XMIDNS"), []
    for _ in range(n):
        k = int(rng.integers(1, max_ops))
        texts.append("".join("%d%s" % (l, c) for l, c in zip(rng.integers(1, 30, k), rng.choice(kinds, k, p=[0.5, 0.1, 0.1, 0.1, 0.1, 0.05, 0.05]))))
    adv = np.array([em.advances(em.parse(t)[1]) for t in texts], dtype=np.int64)
    qs, ts = rng.integers(0, 200_000, n), rng.integers(0, 200_000, n)
    cols = {"q_id": rng.integers(0, n_seq, n), "t_id": rng.integers(0, n_seq, n), "q_start": qs, "q_end": qs + adv[:, 0], "t_start": ts, "t_end": ts + adv[:, 1]}
    return {k: np.asarray(v).astype(np.uint32) for k, v in cols.items()}, rng.integers(0, 2, n).astype(np.uint8), texts


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(7)
    cols, strand, texts = random_case(rng, 600, 4)
    regions = [(int(s), int(a), int(a + w)) for s, a, w in zip(rng.integers(0, 4, 80), rng.integers(0, 200_000, 80), rng.integers(0, 3_000, 80))]
    regions[3] = (lm.UNKNOWN, 0, 10)
    return cols, strand, texts, regions, (rng.random(600) < 0.6).astype(np.uint8)


def test_every_axes_and_set_and_a_partial_set(sw, small):
    cols, strand, texts, regions, status = small
    every = dict(enumerate(texts))
    for set_, axes in ((0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3)):
        got = check(sw, cols, strand, 4, regions, every, status=status, set_=set_, axes=axes, what=(set_, axes))
        assert got.exact_rows == got.n > 0
    hit = em.hit_records(lm.lift(cols, strand, None, regions, 0, 3)[0])
    never = [i for i in range(600) if i not in set(hit)]
    part = {i: texts[i] for i in hit[::2] + never[:50]}      # half of the hit records, and 50 that are never hit
    got = check(sw, cols, strand, 4, regions, part, what="a partial set")
    assert 0 < got.exact_rows < got.n
    assert check(sw, cols, strand, 4, regions, {i: texts[i] for i in never}, what="never hit").exact_rows == 0


def test_no_set_is_the_lift(sw, small):
    from sweepga_amd.lift import lift_exact_records, lift_records
    cols, strand, texts, regions, status = small
    ctx = sw.default_context()
    plain = lift_records(ctx, cols, strand, 4, regions, status=status, set=1)
    got = lift_exact_records(ctx, cols, strand, 4, regions, [], [], status=status, set=1)
    assert got.n == plain.n > 0 and (got.ops, got.cigar_bad, got.exact_rows, len(got.state)) == (0, 0, 0, 0)
    raw = got.rows.tobytes()
    assert b"".join(raw[40 * k:40 * k + 32] for k in range(got.n)) == plain.rows.tobytes()
    assert not got.rows["aligned"].any() and not got.rows["matches"].any()
    assert np.array_equal(got.summary, plain.summary) and got.candidates == plain.candidates
    check(sw, cols, strand, 4, regions, {}, status=status, set_=1, what="k = 0, both seams")


def raw_call(sw, fn, cols, strand, n_seq, regions, cig, capacity, ctx=None):
    """swg_lift_exact_records with caller arrays full of 0xAB -> (rc, request, rows bytes, state bytes)"""
    from sweepga_amd import _lib
    from sweepga_amd.lift import REGION_DTYPE, cigar_set
    ctx = ctx or sw.default_context()
    rec = _lib.SwgRecords()
    rec.n = len(strand)
    keep = {k: np.ascontiguousarray(cols[k], dtype=np.uint32) for k in COLS}
    for k, a in keep.items():
        setattr(rec, k, a.ctypes.data)
    rec.strand, rec.n_seq = strand.ctypes.data, n_seq
    regs = np.array([(s, a, b, 0) for s, a, b in regions], dtype=REGION_DTYPE)
    record, offset, text = cig if isinstance(cig, tuple) else cigar_set(sorted(cig), [cig[i] for i in sorted(cig)])
    cs = _lib.SwgCigarSet()
    cs.record, cs.offset, cs.text, cs.k = record.ctypes.data, offset.ctypes.data, text.ctypes.data, len(record)
    rows = np.full(40 * max(capacity, 1), 0xab, dtype=np.uint8)
    state = np.full(max(len(record), 1), 0xab, dtype=np.uint8)
    req = _lib.SwgLiftExactRequest()
    req.set, req.axes, req.capacity, req.rows, req.state, req.exact_rows = 0, 3, capacity, rows.ctypes.data, state.ctypes.data, 99
    rc = fn(ctx.handle, C.byref(rec), None, regs.ctypes.data, len(regs), C.byref(cs), C.byref(req))
    return rc, req, rows.tobytes(), state.tobytes()


def test_capacities_with_poisoned_arrays(sw, small):
    cols, strand, texts, regions, _ = small
    lib = sw.default_context().lib
    cig = dict(enumerate(texts))
    want, _, states = em.lift_exact(cols, strand, None, regions, cig, 0, 3)
    n = len(want)
    for capacity in (0, n - 1):
        rc, req, rows, state = raw_call(sw, lib.swg_lift_exact_records, cols, strand, 4, regions, cig, capacity)
        assert rc == 0 and req.n == n and set(rows) == {0xab} and req.exact_rows == 0      # the rows are not written ...
        assert list(state) == [states[i] for i in range(600)] and req.ops == n_ops(texts) and req.cigar_bad == 0      # ... ops, bad and state are
    rc, req, rows, state = raw_call(sw, lib.swg_lift_exact_records, cols, strand, 4, regions, cig, n)
    assert rc == 0 and req.n == n == req.exact_rows and rows == em.rows_array(want).tobytes()


def test_records_and_regions_permuted(sw, small):
    cols, strand, texts, regions, _ = small
    rng = np.random.default_rng(8)
    got = check(sw, cols, strand, 4, regions, dict(enumerate(texts)), what="in order")
    perm = rng.permutation(600)                        # new position k holds record perm[k]
    again = check(sw, {c: cols[c][perm] for c in COLS}, strand[perm], 4, regions, {k: texts[perm[k]] for k in range(600)}, what="records permuted")
    back = again.rows.copy()
    back["record"] = perm[back["record"]]
    s0 = np.where(back["flags"] & 2, cols["t_start"][back["record"]], cols["q_start"][back["record"]])
    back = back[np.lexsort((back["record"], s0, back["flags"] >> 1 & 1, back["region"]))]
    assert back.tobytes() == got.rows.tobytes()
    rperm = rng.permutation(len(regions))
    again = check(sw, cols, strand, 4, [regions[r] for r in rperm], dict(enumerate(texts)), what="regions permuted")
    back = again.rows.copy()
    back["region"] = rperm[back["region"]]
    assert back[np.argsort(back["region"], kind="stable")].tobytes() == got.rows.tobytes()


def test_refusals(sw, small):
    from sweepga_amd.lift import cigar_set, lift_exact_records, lift_exact_records_device, regions_array
    cols, strand, texts, regions, _ = small
    ctx = sw.default_context()
    lib = ctx.lib
    good = cigar_set([3, 5, 9], ["1=", "2=", ""])
    bad_sets = [(np.array([3, 3, 9], dtype=np.uint32), good[1], good[2]), (np.array([5, 3, 9], dtype=np.uint32), good[1], good[2]),
                (np.array([3, 5, 600], dtype=np.uint32), good[1], good[2]), (good[0], np.array([0, 4, 2, 4], dtype=np.uint64), good[2]),
                (good[0], np.array([1, 2, 4, 4], dtype=np.uint64), good[2])]
    regs = regions_array(regions)
    hip = Hip()
    try:
        dcols = {k: Dev(hip, cols[k], np.uint32) for k in COLS}
        dstrand, dregs = Dev(hip, strand, np.uint8), Dev(hip, regs.view(np.uint32))
        for record, offset, text in bad_sets:
            rc, req, rows, state = raw_call(sw, lib.swg_lift_exact_records, cols, strand, 4, regions, (record, offset, text), 4)
            assert rc == -1 and set(rows) == {0xab} and set(state) == {0xab}, (record, offset)
            with pytest.raises(sw.SwgError) as e:
                lift_exact_records_device(ctx, dcols, dstrand, 4, dregs, len(regs), Dev(hip, record), Dev(hip, offset), Dev(hip, text), 3)
            assert e.value.code == -1, (record, offset)
        for fn in (lib.swg_lift_exact_records, lib.swg_lift_exact_records_device):      # k is looked at before any array
            from sweepga_amd import _lib
            cs = _lib.SwgCigarSet()
            cs.record, cs.offset, cs.text, cs.k = good[0].ctypes.data, good[1].ctypes.data, good[2].ctypes.data, 2**31
            rec = _lib.SwgRecords()
            rec.n, rec.n_seq = 600, 4
            req = _lib.SwgLiftExactRequest()
            req.set, req.axes = 0, 3
            assert fn(ctx.handle, C.byref(rec), None, regs.ctypes.data, len(regs), C.byref(cs), C.byref(req)) == -5
    finally:
        hip.free()
    for kw in ({"set": 2}, {"axes": 0}, {"axes": 4}, {"set": 1}):      # the lift's own refusals (set 1: KEPT without a status)
        with pytest.raises(sw.SwgError) as e:
            lift_exact_records(ctx, cols, strand, 4, regions, [3], ["1="], **kw)
        assert e.value.code == -1
    with pytest.raises(sw.SwgError) as e:      # a set for no records
        lift_exact_records(ctx, {k: np.zeros(0, dtype=np.uint32) for k in COLS}, np.zeros(0, dtype=np.uint8), 4, regions, [0], ["1="])
    assert e.value.code == -1
    # no regions: the set is still parsed
    got = lift_exact_records(ctx, cols, strand, 4, [], [0, 1, 2], [texts[0], "x", ""])
    assert got.n == 0 and got.state.tolist() == [0, em.SYNTAX, em.EMPTY] and got.cigar_bad == 1 and got.ops == n_ops([texts[0], "x"])


def test_a_memory_limit_too_small_is_a_clean_oom(sw, small):
    from sweepga_amd.lift import lift_exact_records
    cols, strand, texts, regions, _ = small
    ctx = sw.Context(0)
    try:
        long = "1=" * 200_000      # 400 kB of text, 2 * 10^5 ops: 32 bytes of prefix sums each, 6.4 MB
        c1 = {"q_id": [0], "t_id": [1], "q_start": [0], "q_end": [200_000], "t_start": [0], "t_end": [200_000]}
        c1 = {k: np.array(v, dtype=np.uint32) for k, v in c1.items()}
        ctx.set_memory_limit(4 << 20)
        with pytest.raises(sw.SwgError) as e:
            lift_exact_records(ctx, c1, np.zeros(1, dtype=np.uint8), 2, [(0, 5, 9)], [0], [long])
        assert e.value.code == -4
        got = lift_exact_records(ctx, cols, strand, 4, regions, list(range(600)), texts)      # the same context, a call that fits
        assert got.rows.tobytes() == em.rows_array(em.lift_exact(cols, strand, None, regions, dict(enumerate(texts)))[0]).tobytes()
        ctx.set_memory_limit(0)
        got = lift_exact_records(ctx, c1, np.zeros(1, dtype=np.uint8), 2, [(0, 5, 9)], [0], [long])
        assert [tuple(int(v) for v in r) for r in got.rows] == [(0, 0, 5, 9, 1, 5, 9, 4, 4, 4)] and got.ops == 200_000
    finally:
        ctx.close()


def test_hit_records(sw, small):
    from sweepga_amd.lift import lift_hit_records, lift_hit_records_device, regions_array
    cols, strand, texts, regions, status = small
    ctx = sw.default_context()
    regs = regions_array(regions)
    hip = Hip()
    try:
        dcols = {k: Dev(hip, cols[k], np.uint32) for k in COLS}
        dstrand, dregs, dstatus = Dev(hip, strand, np.uint8), Dev(hip, regs.view(np.uint32)), Dev(hip, status, np.uint8)
        for set_, axes in ((0, 3), (1, 3), (0, 1), (1, 2)):
            want = em.hit_records(lm.lift(cols, strand, status != 0, regions, set_, axes)[0])
            k = len(want)
            assert k > 2
            for capacity in (None, k, k - 1, 0):
                got = lift_hit_records(ctx, cols, strand, 4, regions, status=status, set=set_, axes=axes, capacity=capacity)
                dev = lift_hit_records_device(ctx, dcols, dstrand, 4, dregs, len(regs), status=dstatus, set=set_, axes=axes, capacity=capacity)
                for out, kk in (got, dev):
                    assert kk == k and (out is None if capacity in (k - 1, 0) else out.tolist() == want), (set_, axes, capacity)
        # a capacity one short: the caller's array is left alone
        out = np.full(k, 0xabababab, dtype=np.uint32)
        kk = C.c_uint64(0)
        from sweepga_amd.lift import _host_records
        rec, keep = _host_records(cols, strand, 4)
        assert ctx.lib.swg_lift_hit_records(ctx.handle, C.byref(rec), status.ctypes.data, regs.ctypes.data, len(regs), 1, 2, out.ctypes.data, k - 1,
                                            C.byref(kk)) == 0
        assert kk.value == k and (out == 0xabababab).all()
    finally:
        hip.free()
    assert lift_hit_records(ctx, cols, strand, 4, [(lm.UNKNOWN, 0, 9), (0, 5, 5)]) [1] == 0       # no hit: no record
    assert lift_hit_records(ctx, cols, strand, 4, [])[1] == 0


# ---- a random case -------------------------------------------------------------------------------------------------------------------------
def corrupt(text, rng):
    kind = int(rng.integers(0, 5))
    if kind == 0:
        return text + "7"
    if kind == 1:
        return "M" + text
    if kind == 2:
        return text.lower() if any(c.isalpha() for c in text) else text + "x"
    if kind == 3:
        return text + "4294967296D"
    return text + "1="      # one base more on both sides: the sums are off


def test_20000_records_built_from_random_cigars(sw):
    """5 % of the entries are corrupted, 5 % of the records are left out of the set, a real 1:1 status picks the kept set.  At least
    85 % of the entries are usable and at least half of the rows exact by construction: the comparison cannot pass on interpolated
    rows alone."""
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
    regions = [(int(s), int(a), int(a + w)) for s, a, w in zip(rng.integers(0, p_seq, 500), rng.integers(0, 200_000, 500), rng.integers(1, 3_000, 500))]
    for set_ in (0, 1):
        got = check(sw, pcols, pstrand, p_seq, regions, cig, status=status, set_=set_, what="random, set %d" % set_)
        assert int((got.state == 0).sum()) >= 0.85 * len(cig) and got.cigar_bad > 0.03 * len(cig)
        assert got.exact_rows >= 0.5 * got.n and got.n > (1_000, 20)[set_] and got.exact_rows < got.n


# ---- the texts -----------------------------------------------------------------------------------------------------------------------------
def tagged_paf(rng, n):
    """A PAF whose lines mix =/X CIGARs, M CIGARs, no tag, two tags (the last one counts), an empty tag and a broken one."""
    cols, strand, texts = random_case(rng, n, 6)
    lines = []
    for i in range(n):
        f = ["g%d#1#c" % cols["q_id"][i], "400000", str(cols["q_start"][i]), str(cols["q_end"][i]), "-" if strand[i] else "+",
             "g%d#1#c" % cols["t_id"][i], "400000", str(cols["t_start"][i]), str(cols["t_end"][i]), "50", "60", "60"]
        kind = i % 8
        as_m = "".join("%d%s" % (l, "M" if ch in "=X" else ch) for l, ch in em.parse(texts[i])[1])
        tags = (["tp:A:P", "cg:Z:" + texts[i]], ["cg:Z:" + texts[i], "nm:i:3"], ["cg:Z:" + as_m], ["tp:A:P"], [], ["cg:Z:" + as_m, "xx:Z:cg:Z:1=", "cg:Z:" + texts[i]],
                ["cg:Z:"], ["cg:Z:" + texts[i] + "9"])[kind]
        lines.append("\t".join(f + tags))
    return "\n".join(lines) + "\n"


def test_texts_of_an_open_paf_the_python_class_and_the_command_line(sw, tmp_path):
    from sweepga_amd import build
    rng = np.random.default_rng(10)
    text = tagged_paf(rng, 3_000)
    names = lm.parse_paf(text)[2]
    bed_text = "# genes\n" + "".join("%s\t%d\t%d%s\n" % (names[k % len(names)] if k % 9 else "absent", a, a + w, "\tgene%d" % k if k % 3 else "")
                                     for k, (a, w) in enumerate(zip(rng.integers(0, 200_000, 150), rng.integers(0, 4_000, 150))))
    inp, bed = tmp_path / "in.paf", tmp_path / "r.bed"
    inp.write_text(text, newline="")
    bed.write_text(bed_text, newline="")
    flags = ["--num-mappings", "1:1", "--scaffold-jump", "10k", "--scaffold-mass", "2k"]
    plain, out, rows, summ = (tmp_path / x for x in ("plain.paf", "out.paf", "lift.tsv", "lift_summary.tsv"))
    r0 = subprocess.run([build.CLI, str(inp), "--output-file", str(plain), *flags, "--quiet"], capture_output=True)
    assert r0.returncode == 0 and plain.stat().st_size > 0, r0.stderr
    kept = kept_mask(text, plain.read_bytes().decode())
    with sw.PafFile(text=text) as paf:
        for set_, axes in ((1, 3), (0, 2), (0, 1)):
            want = em.paf_texts(text, kept, bed_text, set_, axes)
            assert want[0].count("\texact\n") > 20 and want[0].count("\tinterp\n") > 20 and want[2][2] > 0 and want[2][3] > 0
            got = sw.Lift.from_paf(paf, kept.astype(np.uint8), bed_text, set=set_, axes=axes, exact=True)
            assert (got.text, got.summary_text, got.exact_counts) == want, (set_, axes)
            assert len(got.rows) == want[0].count("\n") and set(got.rows["mode"]) == {"exact", "interp"}
            assert sw.Lift.from_paf(paf, kept.astype(np.uint8), bed_text, set=set_, axes=axes).text == lm.paf_texts(text, kept, bed_text, set_, axes)[0]
        only = sw.Lift.from_paf(paf, kept.astype(np.uint8), bed_text, rows=False, exact=True)
        assert only.text is None and only.summary_text == em.paf_texts(text, kept, bed_text, 1, 3)[1]
    want = em.paf_texts(text, kept, bed_text, 1, 3)
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--lift-regions", str(bed), "--lift", str(rows), "--lift-summary", str(summ),
                        "--lift-exact", *flags], capture_output=True)
    assert r.returncode == 0 and r.stdout == b"" and out.read_bytes() == plain.read_bytes(), r.stderr     # the PAF does not change
    assert rows.read_text() == want[0] and summ.read_text() == want[1]
    assert ("--lift-exact: %d records hit, %d exact, %d bad, %d without a cg:Z: tag\n" % want[2]) in r.stderr.decode()
    # without the switch: the interpolated lift's bytes, and no word of the exact one
    r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), "--lift-regions", str(bed), "--lift", str(rows), "--lift-summary", str(summ), *flags],
                       capture_output=True)
    assert r.returncode == 0 and (rows.read_text(), summ.read_text()) == lm.paf_texts(text, kept, bed_text, 1, 3) and b"lift-exact" not in r.stderr
    # more hit records and rows than the first guesses hold: 70,000 one-base records under one region
    many = "".join("a#1#x\t100000\t%d\t%d\t+\tb#1#y\t100000\t%d\t%d\t1\t1\t60\tcg:Z:1=\n" % (k, k + 1, k, k + 1) for k in range(70_000))
    with sw.PafFile(text=many) as paf:
        got = sw.Lift.from_paf(paf, None, "a#1#x\t0\t100000\n", set="all", exact=True)
        assert got.exact_counts == (70_000, 70_000, 0, 0) and got.text.count("\t1\t1\texact\n") == 70_000
        assert got.text.split("\n")[69_999] == "b#1#y\t69999\t70000\ta#1#x:0-100000\ta#1#x\t69999\t70000\t+\tq\t69999\t1\t1\texact"
