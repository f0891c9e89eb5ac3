"""The mosaic without a GPU: the two models of tests/mosaic_model.py against answers derived by hand and against each other, the
device plan of csrc/swg_mosaic.hip walked through in numpy at tiles of 2, 4 and 8 slots, and the host side of the feature -- header,
ctypes mirrors, exported symbols, the refusals that need no device, a record-free PAF, the command line, the two texts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import mosaic_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = mm.COLS
SEQ_NAMES = ["A#1#a1", "A#1#a2", "B#1#b1", "C#1#c1"]
GENOME_NAMES = ["A#1#", "B#1#", "C#1#"]


def hand_case():
    """Sequences a1 = 0, a2 = 1 (genome A = 0), b1 = 2 (genome B = 1), c1 = 3 (genome C = 2).  -> (columns with matches, strand,
    seq_genome, status, expected): expected[axis, set] = (rows, share), all worked out by hand."""
    a1, a2, b1, c1 = 0, 1, 2, 3
    seq_genome = np.array([0, 0, 1, 2], dtype=np.uint32)
    rows = [
        # (q, t, qs, qe, ts, te, matches, status, strand)
        (a1, b1, 0, 1_000, 0, 1_000, 100, 1, 0),          # 0  light and long ...
        (a1, c1, 300, 400, 0, 100, 500, 1, 1),            # 1  ... with a heavy short one nested in it: record 0 owns two rows on a1
        (a1, b1, 600, 700, 2_000, 2_100, 100, 1, 0),      # 2  as heavy as record 0 and nested in it: the lower index wins, no cut
        (a1, c1, 1_000, 1_100, 200, 300, 50, 1, 0),       # 3  touches record 0 at 1000
        (a1, b1, 1_000, 1_000, 500, 500, 900, 1, 0),      # 4  zero length where a row begins: adds nothing on either axis
        (a1, a2, 0, 2_000, 0, 2_000, 9_999, 1, 0),        # 5  intra-genome: ignored, however heavy
        (a1, b1, 1_100, 1_300, 3_000, 3_200, 70, 0, 0),   # 6  dropped by the filter ...
        (a1, c1, 1_200, 1_250, 400, 450, 60, 1, 0),       # 7  ... so [1100, 1300) of ALL is kept in part: [1200, 1250), by a lighter record
        (a2, b1, 1_300, 1_500, 1_000, 1_200, 80, 1, 0),   # 8  a2's first begin is a1's last end (ALL): 1300 on another sequence
        (b1, c1, 900, 1_100, 50, 250, 200, 1, 0),         # 9  b1 as a query; on c1 it lies over the end of record 1 and the begin of record 3
    ]
    arr = np.array(rows, dtype=np.int64)
    cols = {k: arr[:, i].astype(np.uint32) for i, k in enumerate(COLS + ("matches",))}
    status, strand = arr[:, 7].astype(np.uint8), arr[:, 8].astype(np.uint8)
    q_all = [(a1, 0, 300, 0), (a1, 300, 400, 1), (a1, 400, 1_000, 0), (a1, 1_000, 1_100, 3), (a1, 1_100, 1_300, 6), (a2, 1_300, 1_500, 8),
             (b1, 900, 1_100, 9)]
    q_kept = [(a1, 0, 300, 0), (a1, 300, 400, 1), (a1, 400, 1_000, 0), (a1, 1_000, 1_100, 3), (a1, 1_200, 1_250, 7), (a2, 1_300, 1_500, 8),
              (b1, 900, 1_100, 9)]
    t_kept = [(b1, 0, 1_000, 0), (b1, 1_000, 1_200, 8), (b1, 2_000, 2_100, 2), (c1, 0, 100, 1), (c1, 100, 250, 9), (c1, 250, 300, 3), (c1, 400, 450, 7)]
    t_all = t_kept[:3] + [(b1, 3_000, 3_200, 6)] + t_kept[3:]
    want = {
        (0, "all"): (q_all, [[0, 1_300, 200], [0, 0, 200], [0, 0, 0]]), (0, "kept"): (q_kept, [[0, 1_100, 250], [0, 0, 200], [0, 0, 0]]),
        (1, "all"): (t_all, [[0, 0, 0], [1_500, 0, 0], [200, 150, 0]]), (1, "kept"): (t_kept, [[0, 0, 0], [1_300, 0, 0], [200, 150, 0]]),
        "bases": {(0, "all"): 1_700, (0, "kept"): 1_550, (1, "all"): 1_850, (1, "kept"): 1_650},
    }
    return cols, strand, seq_genome, status, want


# the texts of the hand case, set kept, query axis, by matches (the PAF interns a1, b1, c1, a2: a2's row comes last)
HAND_ROWS = ("A#1#a1\t0\t300\tB#1#b1\t+\t0\t100\t0\t1000\n"
             "A#1#a1\t300\t400\tC#1#c1\t-\t1\t500\t0\t100\n"
             "A#1#a1\t400\t1000\tB#1#b1\t+\t0\t100\t0\t1000\n"
             "A#1#a1\t1000\t1100\tC#1#c1\t+\t3\t50\t200\t300\n"
             "A#1#a1\t1200\t1250\tC#1#c1\t+\t7\t60\t400\t450\n"
             "B#1#b1\t900\t1100\tC#1#c1\t+\t9\t200\t50\t250\n"
             "A#1#a2\t1300\t1500\tB#1#b1\t+\t8\t80\t1000\t1200\n")
HAND_SHARE = "genome\tother_genome\tbases\nA#1#\tB#1#\t1100\nA#1#\tC#1#\t250\nB#1#\tC#1#\t200\n#total\t1550\n"
# ... by length on the target axis, set all: on c1 record 9 (200 bases) now beats record 1 (100 bases)
HAND_ROWS_T_LEN = ("B#1#b1\t0\t1000\tA#1#a1\t+\t0\t1000\t0\t1000\n"
                   "B#1#b1\t1000\t1200\tA#1#a2\t+\t8\t200\t1300\t1500\n"
                   "B#1#b1\t2000\t2100\tA#1#a1\t+\t2\t100\t600\t700\n"
                   "B#1#b1\t3000\t3200\tA#1#a1\t+\t6\t200\t1100\t1300\n"
                   "C#1#c1\t0\t50\tA#1#a1\t-\t1\t100\t300\t400\n"
                   "C#1#c1\t50\t250\tB#1#b1\t+\t9\t200\t900\t1100\n"
                   "C#1#c1\t250\t300\tA#1#a1\t+\t3\t100\t1000\t1100\n"
                   "C#1#c1\t400\t450\tA#1#a1\t+\t7\t50\t1200\t1250\n")
HAND_SHARE_T_LEN = "genome\tother_genome\tbases\nB#1#\tA#1#\t1500\nC#1#\tA#1#\t150\nC#1#\tB#1#\t200\n#total\t1850\n"


def hand_paf():
    """The hand case as PAF text (its names intern in the order a1, b1, c1, a2: ids differ from hand_case's, names do not)."""
    cols, strand, seq_genome, status, _ = hand_case()
    lines = []
    for k in range(len(status)):
        q, t = int(cols["q_id"][k]), int(cols["t_id"][k])
        lines.append("\t".join([SEQ_NAMES[q], "5000", str(cols["q_start"][k]), str(cols["q_end"][k]), "-" if strand[k] else "+", SEQ_NAMES[t], "5000",
                                str(cols["t_start"][k]), str(cols["t_end"][k]), str(cols["matches"][k]), "5000", "60"]))
    return "\n".join(lines) + "\n", status


def check_hand(get, want):
    """get(axis, set) -> (rows, share)"""
    for axis in (0, 1):
        for name in ("all", "kept"):
            rows, share = get(axis, name)
            assert mm.as_tuples(rows) == want[axis, name][0], (axis, name)
            assert np.asarray(share).tolist() == want[axis, name][1], (axis, name)
            assert mm.bases_of(rows) == want["bases"][axis, name] == int(np.asarray(share).sum()), (axis, name)


@pytest.mark.parametrize("per_base", [True, False])
def test_models_against_hand_derived_answers(per_base):
    cols, strand, seq_genome, status, want = hand_case()

    def get(axis, name):
        rows = mm.mosaic(cols, seq_genome, None if name == "all" else status != 0, None, axis, per_base=per_base)
        mm.check_rows(rows, cols, axis)
        return rows, mm.share_of(rows, cols, seq_genome, axis, 3)
    check_hand(get, want)
    # one genome: nothing counts
    assert len(mm.mosaic(cols, np.zeros(4, dtype=np.uint32), None, None, 0, per_base=per_base)) == 0
    # by length on the target axis: on c1 record 9 (200 bases) beats record 1 (100)
    rows = mm.mosaic(cols, seq_genome, None, None, 1, by_length=True, per_base=per_base)
    assert mm.as_tuples(rows)[4:7] == [(3, 0, 50, 1), (3, 50, 250, 9), (3, 250, 300, 3)]


def random_case(rng, n, n_seq, per_genome, span=400, longest=120, weights=6):
    """Dense: many equal positions, equal weights (`weights` distinct values), zero-length and intra-genome records."""
    q, t = rng.integers(0, n_seq, n), rng.integers(0, n_seq, n)
    seq_genome = (np.arange(n_seq) // per_genome).astype(np.uint32)
    qs, ts = rng.integers(0, span, n), rng.integers(0, span, n)
    qe = qs + rng.integers(0, longest, n) * (rng.random(n) < 0.9)
    te = ts + rng.integers(0, longest, n) * (rng.random(n) < 0.9)
    cols = {k: v.astype(np.uint32) for k, v in zip(COLS + ("matches",), (q, t, qs, qe, ts, te, rng.integers(0, weights, n)))}
    return cols, seq_genome, rng.random(n) < 0.5


def test_the_two_models_agree_on_random_records():
    rng = np.random.default_rng(7)
    for n, n_seq, per_genome in ((1, 2, 1), (60, 4, 2), (400, 6, 2), (1_500, 24, 3), (1_500, 9, 1)):
        cols, seq_genome, kept = random_case(rng, n, n_seq, per_genome, span=3_000, longest=400, weights=50)
        for axis in (0, 1):
            for mask in (None, kept):
                for by_length in (False, True):
                    a = mm.mosaic(cols, seq_genome, mask, None, axis, by_length, per_base=True)
                    b = mm.mosaic(cols, seq_genome, mask, None, axis, by_length, per_base=False)
                    assert mm.same_rows(a, b)
                    mm.check_rows(a, cols, axis)
                    sh = mm.share_of(a, cols, seq_genome, axis)
                    assert int(sh.sum()) == mm.bases_of(a) and not np.diag(sh).any()
    # with pairwise different weights the record order does not matter
    cols, seq_genome, kept = random_case(rng, 500, 6, 2)
    cols["matches"] = rng.permutation(500).astype(np.uint32)
    perm = rng.permutation(500)
    a = mm.mosaic(cols, seq_genome, kept, None, 0)
    b = mm.mosaic({k: v[perm] for k, v in cols.items()}, seq_genome, kept[perm], None, 0)
    b["record"] = perm[b["record"]]
    assert mm.same_rows(a, b) and len(a) > 50


# ---- the device plan ---------------------------------------------------------------------------------------------------------
END_FLAG = 1 << 31


def range_put(tbl, lo, hi, p):
    """P on [lo, hi) of a sparse table (tbl[level][position]): level floor(log2(hi - lo)), at lo and at hi - 2^level."""
    if lo >= hi:
        return
    k = (hi - lo).bit_length() - 1
    assert k < len(tbl) and hi <= len(tbl[k]), (k, lo, hi, len(tbl), len(tbl[0]))
    tbl[k][lo] = max(tbl[k][lo], p)
    tbl[k][hi - (1 << k)] = max(tbl[k][hi - (1 << k)], p)


def push_down(tbl):
    for k in range(len(tbl) - 1, 0, -1):
        half = 1 << (k - 1)
        for j in range(len(tbl[k])):
            v = max(tbl[k - 1][j], tbl[k][j])
            if j >= half:
                v = max(v, tbl[k][j - half])
            tbl[k - 1][j] = v


def device_plan(cols, seq_genome, mask, w, axis, T, rng, seen=None):
    """The steps of csrc/swg_mosaic.hip one after the other in numpy, the order inside equal keys randomised: keys, sort, slots,
    a / b, the coarse table over tiles of T slots with its push-down, per tile the sparse table of the partial ranges with its
    push-down, winners, breaks, openers, rows.  seen: a set that collects which paths were walked."""
    seen = seen if seen is not None else set()
    g = np.asarray(seq_genome).astype(np.int64)
    seq, other, s, e = mm.axis_columns(cols, axis)
    n, n_seq = len(seq), len(g)
    use = (g[seq] != g[other]) & (e > s)
    if mask is not None:
        use &= mask
    P = [(int(w[r]) << 32) | (mm.TOP - r) for r in range(n)]
    keys, vals = [], []
    for r in range(n):
        kb = ke = n_seq << 32
        if use[r]:
            kb, ke = (int(seq[r]) << 32) | int(s[r]), (int(seq[r]) << 32) | int(e[r])
        keys += [kb, ke]
        vals += [r, r | END_FLAG]
    keys, vals = np.array(keys, dtype=np.uint64), np.array(vals, dtype=np.int64)
    order = np.lexsort((rng.random(2 * n), keys))
    keys, vals = keys[order], vals[order]
    flag = np.concatenate([[True], keys[1:] != keys[:-1]])
    slot = np.cumsum(flag) - 1
    B = int(flag.sum())
    bound = keys[flag]
    first = np.concatenate([np.flatnonzero(flag), [2 * n]])
    a, b = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for p in range(2 * n):
        (b if vals[p] & END_FLAG else a)[vals[p] & ~END_FLAG] = slot[p]
    assert ((a < b) == use).all() and (a[~use] == b[~use]).all()
    tl = T.bit_length() - 1
    n_tiles = (B + T - 1) // T
    levels = max(1, n_tiles.bit_length())
    coarse = [[0] * n_tiles for _ in range(levels)]
    for r in range(n):
        if a[r] < b[r]:
            fw, ew = (a[r] + T - 1) >> tl, b[r] >> tl
            if fw < ew:
                seen.add(("coarse", int(ew - fw).bit_length() - 1))
                range_put(coarse, int(fw), int(ew), P[r])
    push_down(coarse)
    winner = [0] * B
    for t in range(n_tiles):
        lo, hi = t * T, min(t * T + T, B)
        lds = [[0] * T for _ in range(max(tl, 1))]
        stop = first[hi]
        if hi == B and int(bound[B - 1]) >> 32 == n_seq:     # the sentinel's entries put nothing and are not walked
            stop = first[B - 1]
            seen.add("sentinel")
        if stop - first[lo] > T:
            seen.add("long tile")
        for p in range(first[lo], stop):
            r, at = int(vals[p] & ~END_FLAG), int(slot[p]) - lo
            if vals[p] & END_FLAG:
                if a[r] < lo:
                    seen.add("tail")
                    range_put(lds, 0, at, P[r])
            else:
                to = int(min(b[r], hi)) - lo
                if at == 0 and to == T:
                    seen.add("whole")
                else:
                    seen.add("head" if b[r] > hi else "inside")
                    range_put(lds, at, to, P[r])
        push_down(lds)
        for i in range(hi - lo):
            winner[lo + i] = max(lds[0][i], coarse[0][t])
    breaks = [i for i in range(B) if i == 0 or winner[i] != winner[i - 1]]
    openers = [j for j, i in enumerate(breaks) if winner[i]]
    rows = np.zeros(len(openers), dtype=mm.ROW_DTYPE)
    for k, j in enumerate(openers):
        key, nxt = int(bound[breaks[j]]), int(bound[breaks[j + 1]])     # (a next break always exists)
        assert key >> 32 == nxt >> 32
        rows[k] = (key >> 32, key & mm.TOP, nxt & mm.TOP, mm.TOP - (winner[breaks[j]] & mm.TOP))
    return rows


@pytest.mark.parametrize("T", [2, 4, 8])
def test_the_device_plan_walked_through_in_numpy(T):
    rng = np.random.default_rng(T)
    cols, strand, seq_genome, status, want = hand_case()
    for axis in (0, 1):
        for name, mask in (("all", None), ("kept", status != 0)):
            assert mm.as_tuples(device_plan(cols, seq_genome, mask, cols["matches"], axis, T, rng)) == want[axis, name][0]
    seen, n_inputs = set(), 0
    for n, n_seq, per_genome, span in ((1, 2, 1, 50), (12, 3, 1, 60), (40, 4, 2, 150), (300, 2, 1, 3_000), (90, 6, 2, 300)):
        for _ in range(24):      # 120 inputs per tile size, none skipped
            cols, seq_genome, kept = random_case(rng, n, n_seq, per_genome, span=span, longest=max(2, span // 2))
            if n == 300:       # one light record over everything: many whole tiles under heavier short ones
                cols["q_start"][0], cols["q_end"][0], cols["t_start"][0], cols["t_end"][0] = 0, span + 200, 0, span + 200
                cols["q_id"][0], cols["t_id"][0], cols["matches"][0] = 0, 1, 0
            axis = int(rng.integers(0, 2))
            mask = kept if rng.random() < 0.5 else None
            by_length = bool(rng.random() < 0.3)
            w = mm.weights(cols, axis, None, by_length)
            got = device_plan(cols, seq_genome, mask, w, axis, T, rng, seen)
            assert mm.same_rows(got, mm.mosaic(cols, seq_genome, mask, None, axis, by_length)), (T, n, n_seq)
            n_inputs += 1
    assert n_inputs == 120
    assert {"tail", "whole", "head", "inside", "long tile", "sentinel"} <= seen and {k for what, k in (x for x in seen if isinstance(x, tuple))} >= {0, 1, 2, 3}, seen


# ---- the host side of the library ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from sweepga_amd import build, _lib
    build.build()
    return _lib.load()


def test_structures_match_the_header(lib, tmp_path):
    from sweepga_amd import _lib, mosaic
    structs = (("swg_mosaic_row", _lib.SwgMosaicRow), ("swg_mosaic_request", _lib.SwgMosaicRequest))
    prints = ['printf("%%zu\\n", sizeof(%s));' % name for name, _ in structs]
    prints += ['printf("%%zu\\n", offsetof(%s, %s));' % (name, f) for name, cls in structs for f, _ in cls._fields_]
    prints += ['printf("%u %u %d %d\\n", SWG_MOSAIC_ROWS, SWG_MOSAIC_SHARE, SWG_IV_ALL, SWG_IV_KEPT);']
    prints += ['printf("%%zu\\n", sizeof(%s));' % s for s in ("swg_records", "swg_sharing_request", "swg_depth_run")]
    prints.append('printf("%d\\n", SWG_ABI_VERSION);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sweepga_gpu.h"\nint main(void){' + "".join(prints) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])   # plain C
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(cls) for _, cls in structs] + [getattr(cls, f).offset for _, cls in structs for f, _ in cls._fields_]
    want += [1, 2, 0, 1, 128, 88, 16, 1]      # the structures that existed before keep their sizes
    assert got == want
    assert got[:2] == [16, 64] and mosaic.ROW_DTYPE.itemsize == 16
    assert [mosaic.ROW_DTYPE.fields[f][1] for f, _ in _lib.SwgMosaicRow._fields_] == got[2:6] == [0, 4, 8, 12]
    # no implicit padding: the fields' sizes add up to the structure's
    assert got[6:16] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56]
    assert (mosaic.ROWS, mosaic.SHARE) == (1, 2) and mosaic.ROW_DTYPE == mm.ROW_DTYPE


def test_symbols_are_exported_and_declared(lib):
    import sweepga_amd
    from sweepga_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in ("swg_mosaic_records", "swg_mosaic_records_device", "swg_paf_mosaic"):
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None and (s + "(") in hdr
    assert lib.swg_abi_version() == 1
    for name in ("ROW_DTYPE", "Mosaic", "mosaic_records", "mosaic_records_device"):
        assert hasattr(sweepga_amd, name)


def test_refusals_that_need_no_device(lib):
    from sweepga_amd import PafFile, _lib
    cols, strand, seq_genome, status, _ = hand_case()
    rec = _lib.SwgRecords()
    rec.n = len(status)
    for k, a in cols.items():
        setattr(rec, k, a.ctypes.data)
    rec.n_seq = len(seq_genome)
    share = np.zeros((3, 3), dtype=np.uint64)
    for fn in (lib.swg_mosaic_records, lib.swg_mosaic_records_device):
        for want, axis, set_, reserved, st in ((3, 0, 1, 0, status), (3, 0, 1, 1, status), (0, 0, 1, 0, status), (4, 0, 1, 0, status), (3, 2, 1, 0, status),
                                               (3, 0, 2, 0, status), (3, 0, 1, 0, None)):
            req = _lib.SwgMosaicRequest()
            req.want, req.axis, req.set, req.reserved = want, axis, set_, reserved
            req.n = req.bases = 12345
            req.share = C.cast(share.ctypes.data, C.POINTER(C.c_uint64))
            # (no context exists without a device: a NULL one is refused first, whatever the request holds, and nothing is written;
            # what each faulty request answers under a real context is pinned by tests/test_gpu_mosaic.py::test_limits_and_refusals)
            assert fn(None, C.byref(rec), seq_genome.ctypes.data, 3, st.ctypes.data if st is not None else None, C.byref(req)) == -1
            assert int(req.n) == int(req.bases) == 12345
    marker = C.create_string_buffer(1)

    def slots(rows=True, share=True):
        p = (C.c_void_p * 2)()
        p[0], p[1] = (C.addressof(marker) if rows else None), (C.addressof(marker) if share else None)
        return p, (C.c_uint64 * 2)(7, 7)
    with PafFile(text="a#1#x\t100\t0\t50\t+\tb#1#y\t200\t10\t60\t50\t50\t60\n") as paf:
        one = np.ones(1, dtype=np.uint8)
        p, n = slots()
        assert lib.swg_paf_mosaic(None, paf.handle, one.ctypes.data, 0, 1, 0, p, n) == -1 and not p[0] and not p[1] and list(n) == [0, 0]
        assert b"NULL context" in lib.swg_alnstats_last_error()
        p, n = slots()
        assert lib.swg_paf_mosaic(None, paf.handle, None, 0, 1, 0, p, n) == -1 and not p[0] and not p[1]
        assert b"status" in lib.swg_alnstats_last_error()
        for axis, set_ in ((2, 1), (0, 2)):
            p, n = slots()
            assert lib.swg_paf_mosaic(None, paf.handle, one.ctypes.data, axis, set_, 0, p, n) == -1 and not p[0] and not p[1]
        p, n = slots(False, False)
        assert lib.swg_paf_mosaic(None, paf.handle, one.ctypes.data, 0, 1, 0, p, n) == -1
        assert lib.swg_paf_mosaic(None, paf.handle, one.ctypes.data, 0, 1, 0, None, n) == -1
        assert lib.swg_paf_mosaic(None, None, one.ctypes.data, 0, 1, 0, p, n) == -1
    ln = "\t".join(["a#1#x", str(2**33), str(2**32), str(2**32 + 50), "+", "b#1#y", "900", "10", "60", "50", "50", "60"]) + "\n"
    with PafFile(text=ln) as paf:       # rebased columns: refused before a context is looked at
        p, n = slots()
        assert lib.swg_paf_mosaic(None, paf.handle, np.ones(1, dtype=np.uint8).ctypes.data, 0, 1, 0, p, n) == -6 and not p[0] and not p[1]
        assert b"2^32" in lib.swg_alnstats_last_error()


def test_a_paf_without_records_gives_the_header_only_texts_without_a_device(lib):
    from sweepga_amd import Mosaic, PafFile
    header = b"genome\tother_genome\tbases\n#total\t0\n"
    for text in ("", "# nothing\nfew\tfields\n"):
        with PafFile(text=text) as paf:
            assert paf.n == 0
            for axis in ("query", "target"):
                for by in ("matches", "length"):
                    m = Mosaic.from_paf(None, paf, np.zeros(0, dtype=np.uint8), axis=axis, by=by)
                    assert m.rows == b"" and m.share == header
            only = Mosaic.from_paf(None, paf, None, set="all", share=False)
            assert only.share is None and only.rows == b""
            assert mm.paf_texts(text, np.zeros(0, dtype=bool)) == (b"", header)


def test_command_line_lists_the_flags_and_wants_values(lib):
    from sweepga_amd import build
    r = subprocess.run([build.CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for line in ("--mosaic FILE ", "--mosaic-share FILE ", "--mosaic-axis query|target ", "--mosaic-set kept|all ", "--mosaic-by matches|length "):
        assert "\n  " + line in r.stdout, line
    for flag in ("--mosaic", "--mosaic-share"):
        r = subprocess.run([build.CLI, "in.paf", flag + "="], capture_output=True, text=True)
        assert r.returncode == 2 and "empty value for " + flag in r.stderr
        r = subprocess.run([build.CLI, "in.paf", flag], capture_output=True, text=True)
        assert r.returncode == 2 and flag in r.stderr
    for flag, good in (("--mosaic-axis", "target"), ("--mosaic-set", "all"), ("--mosaic-by", "length")):
        for bad in ("", "both", "Kept"):
            r = subprocess.run([build.CLI, "in.paf", "--mosaic", "x.bed", flag + "=" + bad], capture_output=True, text=True)
            assert r.returncode == 2 and "invalid value for " + flag in r.stderr, (flag, bad, r.stderr)
        r = subprocess.run([build.CLI, "in.paf", flag, good], capture_output=True, text=True)      # an option without a report
        assert r.returncode == 2 and "need --mosaic or --mosaic-share" in r.stderr, (flag, r.stderr)


def test_command_line_refuses_64_bit_columns_before_it_filters(lib, tmp_path):
    """A value >= 2^32 rebases the columns; the mosaic flags say so right after the parse -- exit 3 -- and nothing is begun."""
    from sweepga_amd import build
    ln = "\t".join(["a#1#x", str(2**33), str(2**32), str(2**32 + 50), "+", "b#1#y", "900", "10", "60", "50", "50", "60"]) + "\n"
    inp, out, rep = tmp_path / "in.paf", tmp_path / "out.paf", tmp_path / "mosaic.bed"
    inp.write_text(ln)
    for flag in ("--mosaic", "--mosaic-share"):
        for extra in ([], ["--no-filter"]):
            r = subprocess.run([build.CLI, str(inp), "--output-file", str(out), flag, str(rep), *extra], capture_output=True, text=True)
            assert r.returncode == 3 and "--mosaic" in r.stderr and "2^32" in r.stderr, r.stderr
            assert r.stdout == "" and not out.exists() and not rep.exists()


def test_texts_against_text_written_out():
    text, status = hand_paf()
    assert tuple(t.decode() for t in mm.paf_texts(text, status != 0)) == (HAND_ROWS, HAND_SHARE)
    assert tuple(t.decode() for t in mm.paf_texts(text, status != 0, axis=1, set_="all", by="length")) == (HAND_ROWS_T_LEN, HAND_SHARE_T_LEN)
    # from the hand case's own answers (other ids, same names)
    cols, strand, seq_genome, status, want = hand_case()
    rows = np.array(want[0, "kept"][0], dtype=mm.ROW_DTYPE)
    got = mm.rows_text(SEQ_NAMES, rows, cols, strand, cols["matches"], 0).decode()
    assert sorted(got.splitlines()) == sorted(HAND_ROWS.splitlines())
    assert mm.share_text(GENOME_NAMES, np.array(want[0, "kept"][1]), 1_550).decode() == HAND_SHARE
