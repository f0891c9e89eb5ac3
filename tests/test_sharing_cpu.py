"""Sharing without a GPU: the model of tests/sharing_model.py against answers derived by hand, its two formulations against each
other and against tests/intervals_model.py, the device plan of csrc/swg_sharing.hip walked through in numpy, and the host side of
the feature -- header, ctypes mirrors, exported symbols, the refusals that need no device, a record-free PAF, the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import intervals_model as im
from tests import sharing_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = sm.COLS
SEQ_NAMES = ["A#1#a1", "A#1#a2", "B#1#b1", "C#1#c1", "B#1#b2"]
GENOME_NAMES = ["A#1#", "B#1#", "C#1#"]


def hand_case():
    """Sequences a1 = 0, a2 = 1 (genome A = 0), b1 = 2, b2 = 4 (genome B = 1), c1 = 3 (genome C = 2); three genomes, so depth 2 is
    core.  -> (columns, seq_genome, seq_len, status, expected): expected holds the runs, bases and spectra of both sets and the
    joint runs, all worked out by hand."""
    a1, a2, b1, c1, b2 = 0, 1, 2, 3, 4
    seq_genome = np.array([0, 0, 1, 2, 1], dtype=np.uint32)
    seq_len = np.array([1_000, 500, 2_000, 800, 300], dtype=np.uint32)
    rows = [
        # (q, t, qs, qe, ts, te, status)
        (a1, b1, 0, 100, 1_000, 1_100, 1),     # 0  B covers a1 [0,100) from the query axis ...
        (b1, a1, 1_050, 1_150, 50, 150, 0),    # 1  ... and [50,150) from the target axis: [50,100) twice by ONE genome, depth 1.  Dropped.
        (c1, a1, 0, 100, 150, 250, 1),         # 2  C's cover of a1 begins at 150, exactly where B's ends: ALL has one run [0,250)
        (a1, b1, 400, 500, 0, 100, 1),         # 3
        (a1, b1, 420, 450, 100, 130, 1),       # 4  nested in record 3 on a1; touches it on b1: [0,130)
        (a1, b1, 500, 600, 200, 300, 0),       # 5  touches record 3 on a1: ALL [400,600), KEPT only [400,500) -- kept in part
        (a1, c1, 450, 550, 300, 400, 1),       # 6  a second genome over a1 [450,550): depth 2 = every other genome = core
        (a1, b1, 700, 700, 500, 500, 1),       # 7  zero length where, after a gap, ...
        (a1, b1, 700, 750, 500, 550, 1),       # 8  ... a run begins
        (a1, a2, 0, 1_000, 0, 500, 1),         # 9  intra-genome: ignored; a2 is never covered
        (b2, b1, 0, 300, 0, 300, 1),           # 10 intra-genome: b2 is never covered
    ]
    arr = np.array(rows, dtype=np.int64)
    cols = {k: arr[:, i].astype(np.uint32) for i, k in enumerate(COLS)}
    status = arr[:, 6].astype(np.uint8)
    want = {
        "runs_all": [(a1, 0, 250, 1), (a1, 400, 450, 1), (a1, 450, 550, 2), (a1, 550, 600, 1), (a1, 700, 750, 1),
                     (b1, 0, 130, 1), (b1, 200, 300, 1), (b1, 500, 550, 1), (b1, 1_000, 1_150, 1), (c1, 0, 100, 1), (c1, 300, 400, 1)],
        "runs_kept": [(a1, 0, 100, 1), (a1, 150, 250, 1), (a1, 400, 450, 1), (a1, 450, 500, 2), (a1, 500, 550, 1), (a1, 700, 750, 1),
                      (b1, 0, 130, 1), (b1, 500, 550, 1), (b1, 1_000, 1_100, 1), (c1, 0, 100, 1), (c1, 300, 400, 1)],
        "bases_all": 1_130, "bases_kept": 880,
        # [genome][depth]; column 0 = the genome's length minus the rest: A = 1500, B = 2300, C = 800
        "spectrum_all": [[1_000, 400, 100], [1_870, 430, 0], [600, 200, 0]],
        "spectrum_kept": [[1_100, 350, 50], [2_020, 280, 0], [600, 200, 0]],
        "joint": [(a1, 0, 100, 1, 1), (a1, 100, 150, 1, 0), (a1, 150, 250, 1, 1), (a1, 400, 450, 1, 1), (a1, 450, 500, 2, 2), (a1, 500, 550, 2, 1),
                  (a1, 550, 600, 1, 0), (a1, 700, 750, 1, 1), (b1, 0, 130, 1, 1), (b1, 200, 300, 1, 0), (b1, 500, 550, 1, 1), (b1, 1_000, 1_100, 1, 1),
                  (b1, 1_100, 1_150, 1, 0), (c1, 0, 100, 1, 1), (c1, 300, 400, 1, 1)],
    }
    return cols, seq_genome, seq_len, status, want


HAND_TABLE = ("genome\tlength\tprivate_all\tshared_all\tcore_all\tprivate_kept\tshared_kept\tcore_kept\n"
              "A#1#\t1500\t1000\t400\t100\t1100\t350\t50\n"
              "B#1#\t2300\t1870\t430\t0\t2020\t280\t0\n"
              "C#1#\t800\t600\t200\t0\t600\t200\t0\n"
              "#total\t4600\t3470\t1030\t100\t3720\t830\t50\n")
HAND_SPECTRUM = ("#spectrum\nA#1#\tall\t0\t1000\nA#1#\tall\t1\t400\nA#1#\tall\t2\t100\nA#1#\tkept\t0\t1100\nA#1#\tkept\t1\t350\nA#1#\tkept\t2\t50\n"
                 "B#1#\tall\t0\t1870\nB#1#\tall\t1\t430\nB#1#\tkept\t0\t2020\nB#1#\tkept\t1\t280\n"
                 "C#1#\tall\t0\t600\nC#1#\tall\t1\t200\nC#1#\tkept\t0\t600\nC#1#\tkept\t1\t200\n")


def hand_paf():
    """The hand case as PAF text (its names intern in the order a1, b1, c1, a2, b2: ids differ from hand_case's, names do not)."""
    cols, seq_genome, seq_len, status, _ = hand_case()
    lines = []
    for k in range(len(status)):
        q, t = int(cols["q_id"][k]), int(cols["t_id"][k])
        lines.append("\t".join([SEQ_NAMES[q], str(seq_len[q]), str(cols["q_start"][k]), str(cols["q_end"][k]), "+", SEQ_NAMES[t], str(seq_len[t]),
                                str(cols["t_start"][k]), str(cols["t_end"][k]), "10", "20", "60"]))
    return "\n".join(lines) + "\n", status


def check_hand(runs_all, sp_all, runs_kept, sp_kept, want):
    assert sm.as_tuples(runs_all) == want["runs_all"] and sm.as_tuples(runs_kept) == want["runs_kept"]
    assert np.asarray(sp_all).tolist() == want["spectrum_all"] and np.asarray(sp_kept).tolist() == want["spectrum_kept"]
    assert sum(e - s for _, s, e, _ in want["runs_all"]) == want["bases_all"] and sum(e - s for _, s, e, _ in want["runs_kept"]) == want["bases_kept"]


@pytest.mark.parametrize("per_base", [True, False])
def test_model_against_hand_derived_answers(per_base):
    cols, seq_genome, seq_len, status, want = hand_case()
    a = sm.sharing(cols, seq_genome, seq_len, None, 3, per_base=per_base)
    k = sm.sharing(cols, seq_genome, seq_len, status != 0, 3, per_base=per_base)
    check_hand(a[0], a[1], k[0], k[1], want)
    assert sm.joint_runs(cols, seq_genome, status != 0, 3) == want["joint"]
    perm = np.random.default_rng(1).permutation(len(status))   # no order dependence
    again = sm.sharing({c: v[perm] for c, v in cols.items()}, seq_genome, seq_len, status[perm] != 0, 3, per_base=per_base)
    assert sm.as_tuples(again[0]) == want["runs_kept"] and again[1].tolist() == want["spectrum_kept"]
    no_len = sm.sharing(cols, seq_genome, None, None, 3, per_base=per_base)[1]     # without lengths column 0 stays 0
    assert no_len[:, 0].tolist() == [0, 0, 0] and no_len[:, 1:].tolist() == [r[1:] for r in want["spectrum_all"]]
    # two genomes: nothing between private and core; one genome: nothing counts
    two = sm.sharing(cols, np.array([0, 0, 1, 1, 1]), seq_len, None, 2, per_base=per_base)
    assert two[1].sum() == seq_len.sum() and set(two[0]["depth"].tolist()) == {1}
    one = sm.sharing(cols, np.zeros(5, dtype=np.uint32), seq_len, None, 1, per_base=per_base)
    assert len(one[0]) == 0 and one[1].tolist() == [[int(seq_len.sum())]]


def test_texts_against_text_written_out():
    cols, seq_genome, seq_len, status, want = hand_case()
    sp_all, sp_kept = np.array(want["spectrum_all"]), np.array(want["spectrum_kept"])
    assert sm.table_text(GENOME_NAMES, sp_all, sp_kept).decode() == HAND_TABLE
    assert sm.table_text(GENOME_NAMES, sp_all, sp_kept, detailed=True).decode() == HAND_TABLE + HAND_SPECTRUM
    bed = sm.bed_text(SEQ_NAMES, want["joint"]).decode()
    assert bed.startswith("A#1#a1\t0\t100\t1\t1\nA#1#a1\t100\t150\t1\t0\n") and bed.endswith("C#1#c1\t300\t400\t1\t1\n") and bed.count("\n") == 15
    text, status = hand_paf()
    table, bed2 = sm.paf_texts(text, status != 0, detailed=True)
    assert table.decode() == HAND_TABLE + HAND_SPECTRUM and bed2.decode() == bed      # (ids differ, names and order of a1 < b1 < c1 do not)
    one = sm.table_text(["X#"], np.array([[700]]), np.array([[700]])).decode()
    assert one.endswith("X#\t700\t700\t0\t0\t700\t0\t0\n#total\t700\t700\t0\t0\t700\t0\t0\n")    # one genome: everything private
    two = sm.table_text(["X#", "Y#"], np.array([[5, 7], [0, 3]]), np.array([[12, 0], [3, 0]])).decode()
    assert "X#\t12\t5\t0\t7\t12\t0\t0\n" in two                                                 # two genomes: shared is 0


def random_case(rng, n, n_seq, per_genome, span=3_000, longest=300):
    q, t = rng.integers(0, n_seq, n), rng.integers(0, n_seq, n)
    seq_genome = (np.arange(n_seq) // per_genome).astype(np.uint32)
    qs, ts = rng.integers(0, span, n), rng.integers(0, span, n)
    qe = qs + rng.integers(0, longest, n) * (rng.random(n) < 0.9)     # a tenth of the records: zero length
    te = ts + rng.integers(0, longest, n) * (rng.random(n) < 0.9)
    cols = {k: v.astype(np.uint32) for k, v in zip(COLS, (q, t, qs, qe, ts, te))}
    return cols, seq_genome, rng.random(n) < 0.4


def joint_from_lists(runs_all, runs_kept):
    """The joint runs per base from the two lists (small coordinates)."""
    out = []
    for seq in sorted(set(runs_all["seq"].tolist())):
        top = int(runs_all["end"][runs_all["seq"] == seq].max())
        d = np.zeros((2, top), dtype=np.int64)
        for which, rows in ((0, runs_all), (1, runs_kept)):
            for r in rows[rows["seq"] == seq]:
                d[which, int(r["start"]):int(r["end"])] = int(r["depth"])
        out += [(seq, a, b, int(d[0, a]), int(d[1, a])) for a, b, _ in sm.stretches(d[0] * 100_000 + d[1]) if d[0, a]]
    return out


def test_the_two_formulations_agree_on_random_records():
    rng = np.random.default_rng(7)
    for n, n_seq, per_genome in ((1, 2, 1), (400, 6, 2), (1_500, 24, 3), (1_500, 9, 1)):
        cols, seq_genome, kept = random_case(rng, n, n_seq, per_genome)
        seq_len = np.full(n_seq, 4_000, dtype=np.uint32)
        G = int(seq_genome.max()) + 1
        lists = {}
        for name, k in (("all", None), ("kept", kept)):
            a = sm.sharing(cols, seq_genome, seq_len, k, per_base=True)
            b = sm.sharing(cols, seq_genome, seq_len, k, per_base=False)
            assert sm.same_rows(a[0], b[0]) and np.array_equal(a[1], b[1])
            r = lists[name] = a[0]
            same = r["seq"][1:] == r["seq"][:-1]
            touch = same & (r["start"][1:] == r["end"][:-1])
            assert (r["end"] > r["start"]).all() and (r["depth"] >= 1).all() and (r["depth"] < G).all()
            assert (r["start"][1:][same] >= r["end"][:-1][same]).all() and (r["depth"][1:][touch] != r["depth"][:-1][touch]).all()
            assert (a[1].sum(axis=1) == [int(seq_len[seq_genome == g].sum()) for g in range(G)]).all()   # a row sums to its genome's length
        assert sm.joint_runs(cols, seq_genome, kept) == joint_from_lists(lists["all"], lists["kept"])


def test_consistency_with_the_intervals_model():
    """Where every unit is touched from one axis only -- every sequence is a query in all its records or a target in all of them --
    cover(s, g) is the unit's interval list of that axis: the depth-weighted length of the runs is the bases of both axes' lists."""
    rng = np.random.default_rng(11)
    n, n_seq = 2_000, 20
    cols, seq_genome, kept = random_case(rng, n, n_seq, 2)
    cols["q_id"] = (rng.integers(0, n_seq // 2, n) * 2).astype(np.uint32)          # even ids are queries, odd ids targets
    cols["t_id"] = (rng.integers(0, n_seq // 2, n) * 2 + 1).astype(np.uint32)
    seq_genome = (np.arange(n_seq) % 5).astype(np.uint32)
    for name, k in (("all", None), ("kept", kept)):
        runs, _ = sm.sharing(cols, seq_genome, None, k)
        lists = im.intervals(*[cols[c] for c in COLS], seq_genome, np.ones(n, dtype=bool) if k is None else k)
        weighted = int(((runs["end"].astype(np.int64) - runs["start"]) * runs["depth"]).sum())
        assert weighted == sum(int((lists["kept", a]["end"].astype(np.int64) - lists["kept", a]["start"]).sum()) for a in im.AXES) > 0, name
        if k is None:
            assert weighted == sum(int((lists["all", a]["end"].astype(np.int64) - lists["all", a]["start"]).sum()) for a in im.AXES)


def device_plan(cols, seq_genome, mask, rng):
    """The steps of csrc/swg_sharing.hip one after the other in numpy, every "arbitrary order" made arbitrary: both axes under one
    key, running maximum, heads, +1 / -1 events of the merged intervals, a wrapping prefix sum, the group begins by a running
    maximum, the breakpoints, the openers.  -> runs."""
    g = np.asarray(seq_genome).astype(np.int64)
    G = int(g.max()) + 1
    q, t = cols["q_id"].astype(np.int64), cols["t_id"].astype(np.int64)
    use = g[q] != g[t]
    if mask is not None:
        use = use & mask
    seg = np.concatenate([q * G + g[t], t * G + g[q]])[np.concatenate([use, use])]
    start = np.concatenate([cols["q_start"], cols["t_start"]]).astype(np.int64)[np.concatenate([use, use])]
    end = np.concatenate([cols["q_end"], cols["t_end"]]).astype(np.int64)[np.concatenate([use, use])]
    order = np.lexsort((rng.random(len(seg)), (seg << 32) | start))
    seg, start, end = seg[order], start[order], end[order]
    ev_key, ev_delta, running = [], [], 0
    for k in range(len(seg)):
        if end[k] <= start[k]:
            continue
        P = (int(seg[k]) << 32) | int(end[k])
        if running == 0 or running >> 32 != seg[k] or start[k] > (running & 0xffffffff):
            ev_key.append(((int(seg[k]) // G) << 32) | int(start[k]))
            ev_delta.append(1)
            if running:
                ev_key.append(((running >> 32) // G << 32) | (running & 0xffffffff))
                ev_delta.append(0xffffffff)
        running = max(running, P)
    if running:
        ev_key.append(((running >> 32) // G << 32) | (running & 0xffffffff))
        ev_delta.append(0xffffffff)
    key, delta = np.array(ev_key, dtype=np.uint64), np.array(ev_delta, dtype=np.uint64)
    if len(key) == 0:
        return np.zeros(0, dtype=sm.RUN_DTYPE)
    order = np.lexsort((rng.random(len(key)), key))
    key, delta = key[order], delta[order]
    before = (np.cumsum(delta) - delta) & np.uint64(0xffffffff)                 # exclusive, wrapping
    p = np.arange(len(key))
    first = np.maximum.accumulate(np.where(np.concatenate([[False], key[1:] != key[:-1]]), p, 0))
    last = np.concatenate([key[1:] != key[:-1], [True]])
    behind = np.concatenate([before[1:], [0]])
    breaks = np.flatnonzero(last & (behind != before[first]))
    b_key, b_depth = key[breaks], behind[breaks]
    openers = np.flatnonzero(b_depth != 0)
    runs = np.zeros(len(openers), dtype=sm.RUN_DTYPE)
    runs["seq"], runs["start"] = b_key[openers] >> np.uint64(32), b_key[openers] & np.uint64(0xffffffff)
    runs["end"], runs["depth"] = b_key[openers + 1] & np.uint64(0xffffffff), b_depth[openers]
    return runs


def test_the_device_plan_walked_through_in_numpy():
    rng = np.random.default_rng(3)
    cols, seq_genome, seq_len, status, want = hand_case()
    assert sm.as_tuples(device_plan(cols, seq_genome, None, rng)) == want["runs_all"]
    assert sm.as_tuples(device_plan(cols, seq_genome, status != 0, rng)) == want["runs_kept"]
    for n, n_seq, per_genome in ((400, 6, 2), (1_500, 24, 3), (1_500, 9, 1)):
        cols, seq_genome, kept = random_case(rng, n, n_seq, per_genome, span=600, longest=80)     # (dense: many equal positions)
        for k in (None, kept):
            assert sm.same_rows(device_plan(cols, seq_genome, k, rng), sm.sharing(cols, seq_genome, None, k)[0])


# ---- the host side of the library ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib
    from sweepga_amd.sharing import RUN_DTYPE
    structs = (("swg_depth_run", _lib.SwgDepthRun), ("swg_depth_list", _lib.SwgDepthList), ("swg_sharing_request", _lib.SwgSharingRequest))
    prints = ['printf("%%zu\\n", sizeof(%s));' % name for name, _ in structs]
    prints += ['printf("%%zu\\n", offsetof(%s, %s));' % (name, f) for name, cls in structs for f, _ in cls._fields_]
    prints += ['printf("%zu\\n", offsetof(swg_sharing_request, set[1]));',
               'printf("%u %u %u %u\\n", SWG_SHARING_RUNS_ALL, SWG_SHARING_RUNS_KEPT, SWG_SHARING_SPECTRUM_ALL, SWG_SHARING_SPECTRUM_KEPT);']
    prints += ['printf("%%zu\\n", sizeof(%s));' % s for s in ("swg_records", "swg_breadth_counts", "swg_interval_request")]
    prints.append('printf("%d\\n", SWG_ABI_VERSION);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(cls) for _, cls in structs] + [getattr(cls, f).offset for _, cls in structs for f, _ in cls._fields_]
    want += [_lib.SwgSharingRequest.set.offset + C.sizeof(_lib.SwgDepthList), 1, 2, 4, 8]
    want += [128, 24, 200, 1]      # the structures that existed before keep their sizes
    assert got == want
    assert got[:3] == [16, 40, 88] and RUN_DTYPE.itemsize == 16
    assert [RUN_DTYPE.fields[f][1] for f, _ in _lib.SwgDepthRun._fields_] == got[3:7] == [0, 4, 8, 12]
    from sweepga_amd import sharing
    assert (sharing.RUNS_ALL, sharing.RUNS_KEPT, sharing.SPECTRUM_ALL, sharing.SPECTRUM_KEPT) == (1, 2, 4, 8)


def test_symbols_are_exported_and_declared(lib):
    import sweepga_amd
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_sharing_records", "swg_sharing_records_device", "swg_paf_sharing"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    assert lib.swg_abi_version() == 1
    for name in ("RUN_DTYPE", "Sharing", "sharing_records", "sharing_records_device"):
        assert hasattr(sweepga_amd, name)


def test_refusals_that_need_no_device(lib):
    from sweepga_amd import PafFile, _lib
    cols, seq_genome, seq_len, status, _ = hand_case()
    rec = _lib.SwgRecords()
    rec.n = len(status)
    for k, a in cols.items():
        setattr(rec, k, a.ctypes.data)
    rec.n_seq = len(seq_genome)
    for fn in (lib.swg_sharing_records, lib.swg_sharing_records_device):
        for want, reserved, st in ((0xf, 0, status), (0xf, 1, status), (0, 0, status), (1 << 4, 0, status), (0x2, 0, None), (0x8, 0, None)):
            req = _lib.SwgSharingRequest()
            req.want, req.reserved = want, reserved
            req.set[0].n = req.set[1].n = 12345
            # (a NULL context is refused before any pointer is looked at; the other faults are refusals with any context)
            assert fn(None, C.byref(rec), seq_genome.ctypes.data, 3, seq_len.ctypes.data, st.ctypes.data if st is not None else None, C.byref(req)) == -1
            assert int(req.set[0].n) == int(req.set[1].n) == 12345
    marker = C.create_string_buffer(1)

    def slots(table=True, bed=True):
        p = (C.c_void_p * 2)()
        p[0], p[1] = (C.addressof(marker) if table else None), (C.addressof(marker) if bed else None)
        return p, (C.c_uint64 * 2)(7, 7)
    with PafFile(text="a#1#x\t100\t0\t50\t+\tb#1#y\t200\t10\t60\t50\t50\t60\n") as paf:
        one = np.ones(1, dtype=np.uint8)
        p, n = slots()
        assert lib.swg_paf_sharing(None, paf.handle, one.ctypes.data, 0, p, n) == -1 and not p[0] and not p[1] and list(n) == [0, 0]
        assert b"NULL context" in lib.swg_alnstats_last_error()
        p, n = slots()
        assert lib.swg_paf_sharing(None, paf.handle, None, 0, p, n) == -1 and not p[0] and not p[1]
        assert b"status" in lib.swg_alnstats_last_error()
        p, n = slots(False, False)
        assert lib.swg_paf_sharing(None, paf.handle, one.ctypes.data, 0, p, n) == -1
        assert lib.swg_paf_sharing(None, paf.handle, one.ctypes.data, 0, None, n) == -1
        assert lib.swg_paf_sharing(None, None, one.ctypes.data, 0, p, n) == -1
    ln = "\t".join(["a#1#x", str(2**33), str(2**32), str(2**32 + 50), "+", "b#1#y", "900", "10", "60", "50", "50", "60"]) + "\n"
    with PafFile(text=ln) as paf:       # rebased columns: refused before a context is looked at
        p, n = slots()
        assert lib.swg_paf_sharing(None, paf.handle, np.ones(1, dtype=np.uint8).ctypes.data, 0, p, n) in (-1, -6)


def test_a_paf_without_records_gives_the_header_and_an_empty_bed_without_a_device(lib):
    from sweepga_amd import PafFile, Sharing
    header = b"genome\tlength\tprivate_all\tshared_all\tcore_all\tprivate_kept\tshared_kept\tcore_kept\n"
    for text in ("", "# nothing\nfew\tfields\n"):
        with PafFile(text=text) as paf:
            assert paf.n == 0
            for detailed in (False, True):
                s = Sharing.from_paf(None, paf, np.zeros(0, dtype=np.uint8), detailed=detailed)
                assert s.table == header and s.bed == b""
            only = Sharing.from_paf(None, paf, np.zeros(0, dtype=np.uint8), table=False)
            assert only.table is None and only.bed == b""
            assert sm.paf_texts(text, np.zeros(0, dtype=bool)) == (header, b"")


def test_command_line_lists_the_flags_and_wants_values(lib):
    from sweepga_amd import build
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--sharing REPORT" in r.stdout and "--sharing-detailed" in r.stdout and "--sharing-bed FILE" in r.stdout
    for flag in ("--sharing", "--sharing-bed"):
        r = subprocess.run([build.CLI, "in.paf", flag + "="], capture_output=True, text=True)
        assert r.returncode == 2 and "empty value for " + flag in r.stderr
        r = subprocess.run([build.CLI, "in.paf", flag], capture_output=True, text=True)
        assert r.returncode == 2 and flag in r.stderr
    r = subprocess.run([build.CLI, "in.paf", "--sharing-detailed"], capture_output=True, text=True)
    assert r.returncode == 2 and "--sharing-detailed needs --sharing" in r.stderr


def test_command_line_refuses_64_bit_columns_before_it_filters(lib, tmp_path):
    """A value >= 2^32 rebases the columns; the sharing flags say so right after the parse -- exit 3 -- and nothing is begun."""
    from sweepga_amd import build
    ln = "\t".join(["a#1#x", str(2**33), str(2**32), str(2**32 + 50), "+", "b#1#y", "900", "10", "60", "50", "50", "60"]) + "\n"
    inp, out, rep = tmp_path / "in.paf", tmp_path / "out.paf", tmp_path / "sharing.tsv"
    inp.write_text(ln)
    for flag in ("--sharing", "--sharing-bed"):
        for extra in ([], ["--no-filter"]):
            r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), flag, str(rep), *extra], capture_output=True, text=True)
            assert r.returncode == 3 and "--sharing" in r.stderr and "2^32" in r.stderr, r.stderr
            assert r.stdout == "" and not out.exists() and not rep.exists()
