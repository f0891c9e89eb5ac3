"""tests/prim_model.py (the numpy references that tests/test_gpu_primitives_native.py holds the scans, the compaction and the
radix sorts against) on hand-written cases small enough to check by eye, and the build of the native driver without a GPU."""
import os

import numpy as np

from tests import prim_model as pm


def test_exclusive_sum_wraps_past_2_32():
    x = np.array([0xFFFFFFFF, 1, 1, 0xFFFFFFFF, 0x80000000, 0x80000000, 5], dtype=np.uint32)
    out, total = pm.exclusive_sum_u32(x)
    # running value: 0, -1, 0, 1, 0, 2^31, 0 (mod 2^32), then + 5
    assert out.dtype == np.uint32 and out.tolist() == [0, 0xFFFFFFFF, 0, 1, 0, 0x80000000, 0]
    assert total.dtype == np.uint64 and int(total) == 5  # the true sum is 3 * 2^32 + 5: the total wraps like the elements
    out, total = pm.exclusive_sum_u32(np.zeros(0, dtype=np.uint32))
    assert len(out) == 0 and int(total) == 0


def test_running_max_above_2_32():
    x = np.array([3, (7 << 32) | 1, 7 << 32, (7 << 32) | 2, 9, (1 << 63) | 5, 1 << 63, 0], dtype=np.uint64)
    want = [3, (7 << 32) | 1, (7 << 32) | 1, (7 << 32) | 2, (7 << 32) | 2, (1 << 63) | 5, (1 << 63) | 5, (1 << 63) | 5]
    got = pm.inclusive_max(x)
    assert got.dtype == np.uint64 and got.tolist() == want
    got32 = pm.inclusive_max(np.array([2, 1, 0xFFFFFFFE, 5, 0xFFFFFFFF], dtype=np.uint32))
    assert got32.dtype == np.uint32 and got32.tolist() == [2, 2, 0xFFFFFFFE, 0xFFFFFFFE, 0xFFFFFFFF]


def test_inclusive_sum_wraps_past_2_64():
    x = np.array([(1 << 64) - 1, 2, (1 << 63), (1 << 63), 7], dtype=np.uint64)
    assert pm.inclusive_sum_u64(x).tolist() == [(1 << 64) - 1, 1, (1 << 63) + 1, 1, 8]


def test_compaction_takes_every_non_zero_byte():
    flags = np.array([0, 0x01, 0, 0x7F, 0x80, 0, 0xFF, 0, 0x02], dtype=np.uint8)
    lst, total, tile_off = pm.compact(flags)
    assert lst.dtype == np.uint32 and lst.tolist() == [1, 3, 4, 6, 8]
    assert int(total) == 5 and tile_off.tolist() == [0]
    big = np.zeros(2 * 4096 + 3, dtype=np.uint8)
    big[[0, 4095, 4096, 8192, 8194]] = [1, 0x80, 0xFF, 0x7F, 2]
    lst, total, tile_off = pm.compact(big)
    assert lst.tolist() == [0, 4095, 4096, 8192, 8194] and int(total) == 5 and tile_off.tolist() == [0, 2, 3]
    lst, total, tile_off = pm.compact(np.zeros(0, dtype=np.uint8))
    assert len(lst) == 0 and int(total) == 0 and len(tile_off) == 0


def test_stable_sort_on_a_middle_bit_range_with_ties():
    # bits [4, 8) decide; the low nibble and everything above bit 8 only travel along
    keys = np.array([0x1A3, 0x02F, 0xFA0, 0x020, 0x0A1, 0x72E, 0x000, 0x3A2], dtype=np.uint64)
    vals = np.array([10, 11, 12, 13, 14, 15, 16, 17], dtype=np.uint32)
    k, v = pm.sort_pairs(keys, vals, 4, 8)
    # digits: A 2 A 2 A 2 0 A -> 0 first, the 2s in input order, then the As in input order
    assert k.tolist() == [0x000, 0x02F, 0x020, 0x72E, 0x1A3, 0xFA0, 0x0A1, 0x3A2]
    assert v.tolist() == [16, 11, 13, 15, 10, 12, 14, 17]
    k, v = pm.sort_pairs(keys, vals, 8, 8)  # an empty range orders nothing
    assert k.tolist() == keys.tolist() and v.tolist() == vals.tolist()


def test_packed_and_words_sorts():
    keys = np.array([0x2FF, 0x101, 0x2FF, 0x100, 0x7FF], dtype=np.uint64)  # key_bits = 10: bit 10 of the last key is not sorted on
    vals = np.array([3, 1, 2, 0, 3], dtype=np.uint32)
    got = pm.sort_packed(keys, vals, 10, 2)
    # order of the low 10 bits: 0x100 (3), 0x101 (1), then 0x2FF (0), 0x2FF (2) and 0x7FF (4, low bits 0x3FF) last
    assert got.tolist() == [(1 << 2) | 0, (1 << 2) | 1, (2 << 2) | 3, (2 << 2) | 2, (7 << 2) | 3]
    assert pm.sort_packed(keys, None, 10, 3).tolist() == [(1 << 3) | 3, (1 << 3) | 1, (2 << 3) | 0, (2 << 3) | 2, (7 << 3) | 4]
    words = np.array([(5 << 4) | 9, (1 << 4) | 2, (13 << 4) | 1, (1 << 4) | 15, (5 << 4) | 0], dtype=np.uint64)
    # sorted_bits = 3 above 4 value bits: 13 counts as 5
    assert pm.sort_words(words, 3, 4).tolist() == [(1 << 4) | 2, (1 << 4) | 15, (5 << 4) | 9, (13 << 4) | 1, (5 << 4) | 0]


def test_first_difference_names_the_index():
    want = np.array([5, 6, 7, 8], dtype=np.uint32)
    assert pm.first_difference("c", "out", want.copy(), want) is None
    msg = pm.first_difference("case7", "out", np.array([5, 6, 9, 1], dtype=np.uint32), want)
    assert "case7" in msg and "index 2" in msg and "0x9" in msg and "0x7" in msg
    assert "3 elements" in pm.first_difference("c", "out", want[:3], want)
    assert pm.first_difference("c", "total", np.uint64(4), np.uint64(4)) is None
    assert "0x5" in pm.first_difference("c", "total", np.uint64(5), np.uint64(4))


def test_prim_check_builds_without_a_gpu():
    from sweepga_amd import build
    exe = build.build_prim_check()
    assert exe == build.PRIM_CHECK and os.access(exe, os.X_OK)
    assert os.path.getmtime(exe) >= os.path.getmtime(build.PRIM_CHECK_SRC)
