"""pair_sort's column output (csrc/swg_pair.hip): q_end, t_start, t_end -- and matches / block_len under an identity floor for
scaffolds -- go from input order to sorted order through two LDS buffers that take the columns in turn, one barrier per column.
What can go wrong there is a column read out of the wrong buffer, a buffer overwritten before its last reader, and the reuse of
both buffers by the next batch of a pair that needs several; a wrong column shows as a wrong status or chain number against
the CPU oracle.  Every case asserts from the library's launch table that the pair path ran, and under which kernel.
Sequences are 150 Mbp long, so that no coarse bin of the sort is denser than a batch and no call is handed to the global-sort
stage.  -m gpu only."""
import numpy as np
import pytest

from tests import gen, orc
from tests.test_gpu_pairs import permute, run_both

pytestmark = pytest.mark.gpu
SPAN = 150_000_000
COLS = ("qs", "qe", "ts", "te", "block_length", "identity", "matches", "strand")


@pytest.fixture(scope="module")
def sw():
    import sweepga_amd
    sweepga_amd.default_context(0)
    return sweepga_amd


def pairs_of(rng, sizes, minus_frac=0.1, all_minus=None):
    """One chromosome pair per size, pair after pair (pair-major), input order random inside a pair."""
    parts = []
    for k, n in enumerate(sizes):
        r = gen.random_records(rng, n, n_genomes=1, chrs_per_genome=1, span=SPAN, minus_frac=1.0 if k == all_minus else minus_frac,
                               zero_frac=0.0, self_frac=0.0)
        r.qname = [f"a{k}#1#c"] * n
        r.tname = [f"b{k}#1#c"] * n
        parts.append(r)
    total = sum(sizes)
    return orc.Records(sum((r.qname for r in parts), []), sum((r.tname for r in parts), []),
                       *[np.concatenate([getattr(r, c) for r in parts]) for c in COLS], np.arange(total, dtype=np.uint64))


def launched(sw, *labels):
    table = sw.default_context(0).profile_table()
    for lab in labels:
        assert lab in table, (lab, sorted(k for k in table if k.startswith("pair_")))
    return table


@pytest.fixture(scope="module")
def large_class():
    """4,097: the first size of the 1024-thread class; 16,384: one full batch; 16,385: two batches (the buffers are reused);
    20,000: all on the '-' strand; 32,768: the last size of the class.  89,634 records: the plan over runs, pair_sort_big."""
    return pairs_of(np.random.default_rng(4097), [4_097, 16_384, 16_385, 20_000, 32_768], all_minus=3)


@pytest.mark.parametrize("cfg", [{}, {"scaffold_gap": 20_000, "min_scaffold_length": 0},
                                 {"scaffold_gap": 60_000, "min_scaffold_length": 3_000, "scaffold_max_deviation": 10_000}])
def test_large_class_three_columns(sw, large_class, cfg):
    run_both(sw, large_class, cfg, expect_pair_path=True)
    table = launched(sw, "pair_sort_big")
    assert "pair_sort_s" not in table and "pair_sort_m" not in table


def test_large_class_five_columns(sw, large_class):
    """An identity floor for scaffolds: matches and block_len follow t_end through the two buffers."""
    for cfg in ({"scaffold_gap": 30_000, "min_scaffold_length": 500, "min_scaffold_identity": 0.85},
                {"min_scaffold_identity": 0.9}):
        run_both(sw, large_class, cfg, expect_pair_path=True)
        launched(sw, "pair_sort_big")


def test_large_class_behind_a_mapping_sweep(sw, large_class):
    """--num-mappings 1:1: the sweep's flags come in (alive_in / member_in), the records it dropped ride behind the members,
    and a pair has fewer members than records."""
    kept, _ = orc.apply_filters(orc.Config(mapping_filter_mode=orc.ONE_TO_ONE, scaffold_gap=0), large_class)
    assert 0 < int((kept != 0).sum()) < len(kept)
    for cfg in ({"mapping_filter_mode": "OneToOne"},
                {"mapping_filter_mode": "OneToOne", "scaffold_gap": 40_000, "min_scaffold_length": 2_000, "scaffold_max_deviation": 6_000},
                {"mapping_filter_mode": "OneToOne", "scaffold_gap": 30_000, "min_scaffold_length": 500, "min_scaffold_identity": 0.85}):
        run_both(sw, large_class, cfg, expect_pair_path=True)
        launched(sw, "pair_sort_big")


def test_small_and_medium_classes_of_a_large_input(sw):
    """1,024: the last size of the 64-thread class; 1,025 and 4,096: the first and the last of the 256-thread class."""
    rec = pairs_of(np.random.default_rng(1024), [1_024, 1_025, 4_096, 30_000, 30_000])
    for cfg in ({}, {"scaffold_gap": 100_000, "min_scaffold_length": 1_000, "min_scaffold_identity": 0.85}):
        run_both(sw, rec, cfg, expect_pair_path=True)
        launched(sw, "pair_sort_s", "pair_sort_m", "pair_sort_big")


def test_shuffled_input_through_the_record_list(sw):
    """At most 65,536 records in any order: the pairs are lists of record indices (PERM; the index buffer is 4 bytes wide).
    9,000 records are two batches of the 1024-thread shape there."""
    rng = np.random.default_rng(9000)
    rec = pairs_of(rng, [9_000, 2_000, 300, 4_097], minus_frac=0.3)
    rec = permute(rec, rng.permutation(len(rec.qname)))
    for cfg in ({}, {"scaffold_gap": 200_000, "min_scaffold_length": 1_000, "min_scaffold_identity": 0.85},
                {"mapping_filter_mode": "OneToOne", "scaffold_gap": 200_000, "min_scaffold_length": 1_000}):
        run_both(sw, rec, cfg, expect_pair_path=True)
        launched(sw, "pair_sort_pl", "pair_sort_pm", "pair_sort_ps")
