"""Tree sparsification on records (include/sweepga_gpu.h: swg_tree_select_*, swg_filter_subset*, swg_paf_tree_select), the parts
that need no GPU: the exported symbols, the handles' two-part-prefix genome table, THE selection function (shared by the text
tool and the record routes) fed with sums computed in numpy against the oracle's text pass, the text tool after the refactoring,
and the flags that send a PAF handle to the text route (where the mask needs no device either)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import orc
from tests.test_tree_filter_cpu import line, oracle_tree, product_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["swg_tree_select_pairs", "swg_tree_select_records", "swg_tree_select_records_device", "swg_filter_subset",
               "swg_filter_subset_device", "swg_filter_subset_multi", "swg_paf_tree_select", "swg_paf_tree_needs_text",
               "swg_aln_tree_select", "swg_paf_num_genomes_two", "swg_paf_genome_two_prefix", "swg_aln_num_genomes_two",
               "swg_aln_genome_two_prefix"]
GRID = [(1, 0, 0.0), (2, 1, 0.0), (0, 2, 0.0), (3, 0, 0.3), (0, 0, 0.3), (1, 1, 1.0), (50, 0, 0.0), (0, 0, 0.0)]


def genome_two(name):
    """extract_genome_prefix, src/tree_filter.rs:15-24, restated"""
    parts = name.split("#")
    return parts[0] + "#" + parts[1] + "#" if len(parts) >= 2 else name


def open_paf(text):
    from sweepga_amd import _lib
    lib = _lib.load()
    raw = text.encode()
    h = C.c_void_p()
    assert lib.swg_paf_open_buffer(raw, len(raw), 2, C.byref(h)) == 0, lib.swg_paf_last_error()
    return lib, h


def test_symbols_are_exported_and_declared():
    from sweepga_amd import _lib, sparsify  # noqa: F401  (the mirror imports)
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "sweepga_gpu.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _lib.SYMBOLS
        getattr(lib, s)
        assert re.search(r"\b" + s + r"\(", header), s
    # the documented signatures, as the binding states them
    assert len(lib.swg_tree_select_records.argtypes) == 10 and len(lib.swg_tree_select_records_device.argtypes) == 10
    assert len(lib.swg_filter_subset_device.argtypes) == 7 and len(lib.swg_filter_subset.argtypes) == 7
    assert len(lib.swg_paf_tree_select.argtypes) == 9 and len(lib.swg_aln_tree_select.argtypes) == 7
    # NULL arguments come back as errors, not crashes
    assert lib.swg_tree_select_records(None, None, None, 0, None, 1, 0, 0.0, None, None) == -1
    assert lib.swg_filter_subset_device(None, None, None, None, None, None, None) == -1
    assert lib.swg_paf_tree_select(None, None, 1, 0, 0.0, 0, None, None, None) == -1


def test_handle_prefix_table_is_extract_genome_prefix():
    from sweepga_amd import sparsify
    names = ["plain", "a#b", "HG002#1#chr1", "HG002#1#chr2", "x#y#z#w", "x#y#q", "a#", "#", "##", "HG002#2#chr1", "a#b#"]
    rows = [line(names[i], names[(i * 3 + 1) % len(names)], 90, 100) for i in range(len(names))]
    lib, h = open_paf("\n".join(rows) + "\n")
    try:
        rec = lib.swg_paf_records(h).contents
        n_seq = lib.swg_paf_num_sequences(h)
        seq = [lib.swg_paf_sequence_name(h, i).decode() for i in range(n_seq)]
        assert sorted(seq) == sorted(names)
        pre = sparsify.handle_prefixes(h)
        assert len(pre) == rec.n_genome_two == len(set(genome_two(s) for s in seq))
        g = np.ctypeslib.as_array(C.cast(rec.seq_genome_two, C.POINTER(C.c_uint32)), (n_seq,))
        assert [pre[g[i]] for i in range(n_seq)] == [genome_two(s) for s in seq]
        assert [sparsify.genome_two(s) for s in seq] == [genome_two(s) for s in seq]
        assert genome_two("HG002#1#chr1") == "HG002#1#" and genome_two("a#b") == "a#b#" and genome_two("plain") == "plain"
        assert lib.swg_paf_genome_two_prefix(h, len(pre)) is None
    finally:
        lib.swg_paf_close(h)


def random_rows(rng, n_rows, tie_heavy=True):
    genomes = [f"g{i}#{h}#" for i in range(int(rng.integers(2, 9))) for h in (1, 2)][:int(rng.integers(2, 12))]
    names = [g + f"chr{c}" for g in genomes for c in range(3)] + ["plain1", "plain2", "x#y", "z#1", "lonely#1#a", "lonely#1#b"]
    rows = []
    for _ in range(n_rows):
        q, t = rng.choice(names, 2)
        if q.startswith("lonely") or t.startswith("lonely"):     # a genome that only ever meets itself
            q, t = "lonely#1#a", "lonely#1#b"
        b = int(rng.choice([100, 1000, 1000, 5000])) if tie_heavy else int(rng.integers(50, 9000))
        m = int(b * rng.choice([0.5, 0.8, 0.8, 0.9, 0.95])) if tie_heavy else int(b * rng.random())
        rows.append((q, t, m, b))
    return rows


def select_by_numpy_sums(rows, kn, kf, rf):
    """The kept rows through swg_tree_select_pairs, with the sums of every unordered genome pair computed here."""
    from sweepga_amd import sparsify
    pre = sorted({genome_two(x) for r in rows for x in r[:2]}, key=lambda s: (len(s), s))   # any id order must do
    gid = {p: i for i, p in enumerate(pre)}
    gq = np.array([gid[genome_two(r[0])] for r in rows], dtype=np.int64)
    gt = np.array([gid[genome_two(r[1])] for r in rows], dtype=np.int64)
    m = np.array([r[2] for r in rows], dtype=np.uint64)
    b = np.array([r[3] for r in rows], dtype=np.uint64)
    G = len(pre)
    key = np.minimum(gq, gt) * G + np.maximum(gq, gt)
    inter = gq != gt
    keys, inv = np.unique(key[inter], return_inverse=True)
    sm = np.zeros(len(keys), dtype=np.uint64)
    sb = np.zeros(len(keys), dtype=np.uint64)
    np.add.at(sm, inv, m[inter])
    np.add.at(sb, inv, b[inter])
    # (the pairs are handed over in either id order: the function canonicalises by prefix)
    a_ids, b_ids = keys // G, keys % G
    flip = np.arange(len(keys)) % 2 == 1
    pa, pb = np.where(flip, b_ids, a_ids), np.where(flip, a_ids, b_ids)
    sel = sparsify.select_pairs(pre, pa, pb, sm, sb, kn, kf, rf)
    chosen = set(keys[sel != 0].tolist())
    return [i for i in range(len(rows)) if inter[i] and int(key[i]) in chosen]


@pytest.mark.parametrize("seed", range(6))
def test_shared_selection_keeps_the_oracles_pairs(seed):
    rng = np.random.default_rng(100 + seed)
    rows = random_rows(rng, int(rng.integers(1, 2500)), tie_heavy=seed % 2 == 0)
    text = "".join(line(*r) + "\n" for r in rows)
    lines = text.split("\n")
    for kn, kf, rf in GRID:
        want = oracle_tree(text, kn, kf, rf)
        got = "".join(lines[i] + "\n" for i in select_by_numpy_sums(rows, kn, kf, rf))
        assert got == want, (seed, kn, kf, rf)
        assert product_tree(text, kn, kf, rf) == want, (seed, kn, kf, rf)   # the text tool calls the same function


def test_selection_ties_fall_to_the_smaller_prefix():
    # every pair has identity 0.9: tree:1 keeps, for each genome, the neighbour with the smallest prefix
    rows = [(a + "c", b + "c", 900, 1000) for a, b in (("B#1#", "A#1#"), ("C#1#", "A#1#"), ("C#1#", "B#1#"), ("D#1#", "C#1#"), ("D#1#", "B#1#"))]
    text = "".join(line(*r) + "\n" for r in rows)
    kept = select_by_numpy_sums(rows, 1, 0, 0.0)
    assert kept == [0, 1, 4]          # A -> B, B -> A, C -> A, D -> B
    assert oracle_tree(text, 1, 0, 0.0) == "".join(line(*rows[i]) + "\n" for i in kept)
    # farthest = last of the same order: A -> C (row 1), B -> D (row 4), C -> D (row 3), D -> C
    assert select_by_numpy_sums(rows, 0, 1, 0.0) == [1, 3, 4]
    assert oracle_tree(text, 0, 1, 0.0) == "".join(line(*rows[i]) + "\n" for i in (1, 3, 4))


def test_selection_rejects_what_it_cannot_answer():
    from sweepga_amd import _lib, sparsify
    pre = ["a#1#", "b#1#"]
    with pytest.raises(_lib.SwgError) as e:
        sparsify.select_pairs(pre, [0], [1], [1 << 53], [1 << 54], 1)
    assert e.value.code == -5        # SWG_ERR_RANGE: the reference's f64 sums are other numbers there
    assert sparsify.select_pairs(pre, [0], [1], [(1 << 53) - 1], [(1 << 53) - 1], 1).tolist() == [1]
    for a, b in (([0], [0]), ([0], [2]), ([0, 1], [1, 0])):   # equal genomes, an id out of range, a pair listed twice
        with pytest.raises(_lib.SwgError) as e:
            sparsify.select_pairs(pre, a, b, [1] * len(a), [1] * len(a), 1)
        assert e.value.code == -1
    assert sparsify.select_pairs(pre, [], [], [], [], 1).tolist() == []


IRREGULAR = {
    "regular": (line("A#1#c", "B#1#c", 900, 1000) + "\tcg:Z:900=100X", 0),
    "cg total differs from column 10": (line("A#1#c", "B#1#c", 900, 1000) + "\tcg:Z:800=200X", 1),
    "#-led line with 11 fields": ("#" + line("A#1#c", "B#1#c", 900, 1000), 1),
    "column 10 does not parse": (line("A#1#c", "B#1#c", 900, 1000).replace("\t900\t", "\tx\t"), 1),
    "column 11 does not parse": (line("A#1#c", "B#1#c", 900, 1000).replace("\t900\t1000\t", "\t900\t\t"), 1),
    "a value of 2^32 or more": (f"A#1#c\t9000000000\t5000000000\t5000001000\t+\tB#1#c\t1000\t0\t1000\t900\t1000\t60", 1),
    "#-led line with 3 fields": ("#a\tb\tc", 0),
    "column 3 does not parse (not read by the tree pass)": (line("A#1#c", "B#1#c", 900, 1000).replace("\t0\t1000\t+", "\tx\t1000\t+"), 0),
}


@pytest.mark.parametrize("what", list(IRREGULAR))
def test_irregular_flags_and_the_text_route(what):
    from sweepga_amd import sparsify
    odd, flagged = IRREGULAR[what]
    rng = np.random.default_rng(5)
    rows = [line(*r) for r in random_rows(rng, 300)]
    rows.insert(150, odd)
    text = "\n".join(rows) + "\n"
    lib, h = open_paf(text)
    try:
        assert lib.swg_paf_tree_needs_text(h) == flagged, what
        if not flagged:
            return
        # the text route needs no device: the mask is the set of lines the oracle keeps, through the records' line numbers
        n = lib.swg_paf_records(h).contents.n
        ranks = np.ctypeslib.as_array(C.cast(lib.swg_paf_ranks(h), C.POINTER(C.c_uint64)), (n,))
        lines = text.split("\n")
        for kn, kf, rf in GRID:
            keep, n_kept, route = sparsify.paf_tree_select(None, h, kn, kf, rf)
            assert route == sparsify.ROUTE_TEXT and n_kept == int(keep.sum())
            assert "".join(lines[int(ranks[i])] + "\n" for i in np.flatnonzero(keep)) == oracle_tree(text, kn, kf, rf), (what, kn, kf, rf)
    finally:
        lib.swg_paf_close(h)


def test_empty_handle_needs_no_device():
    from sweepga_amd import sparsify
    lib, h = open_paf("# nothing\n\n")
    try:
        keep, n_kept, route = sparsify.paf_tree_select(None, h, 1)
        assert len(keep) == 0 and n_kept == 0
    finally:
        lib.swg_paf_close(h)
