"""The arithmetic behind the fused walk's keys beyond tests/test_walk_keys_cpu.py (sweepga_amd/csrc/swg_chain.hip, walk_key_loop), on
the CPU: a key is bit 62 | d << 16 | low with a non-zero low part -- the ring slot's byte offset, a multiple of 4 that grows with
j -- and a score kept in key space is d << 16 with the low part zero.  Then `d < score` and `key < score << 16` are the same
test, clearing the low bits of the smallest key gives the smallest d in key space, and keys whose low parts grow with j order
like (d, j).  numpy over 10^6 random triples plus the edges."""
import numpy as np

KEY_BIT = np.uint64(1) << np.uint64(62)
LOW = np.uint64(0xFFFF)
N = 1_000_000
D_MAX = 1 << 45          # d = q_gap^2 + r_gap^2 with gaps up to 2^22


def key(d, low):
    return KEY_BIT | (d << np.uint64(16)) | low


def score(s):
    return KEY_BIT | (s << np.uint64(16))


def triples():
    rng = np.random.default_rng(45)
    d = rng.integers(0, D_MAX, N).astype(np.uint64)
    s = rng.integers(0, D_MAX, N).astype(np.uint64)
    s[::3] = d[::3] + rng.integers(0, 3, len(d[::3])).astype(np.uint64)          # scores at, one and two above the distance
    s[1::7] = np.maximum(d[1::7], 1) - np.uint64(1)                               # ... and one below
    low = (np.uint64(4) * rng.integers(1, 256, N).astype(np.uint64))
    edge_d = np.array([0, 0, 1, 1, D_MAX - 1, D_MAX - 1, D_MAX - 1, 0, D_MAX - 2], dtype=np.uint64)
    edge_s = np.array([0, 1, 1, 0, D_MAX - 1, D_MAX - 2, D_MAX, D_MAX, D_MAX - 1], dtype=np.uint64)
    edge_l = np.array([4, 1020, 4, 1020, 4, 1020, 4, 1020, 1020], dtype=np.uint64)
    return np.concatenate((d, edge_d)), np.concatenate((low, edge_l)), np.concatenate((s, edge_s))


def test_low_parts_are_the_slot_offsets():
    _, low, _ = triples()
    assert int(low.min()) == 4 and int(low.max()) == 1020 and not (low % np.uint64(4)).any()


def test_a_key_is_below_a_score_exactly_when_its_distance_is():
    d, low, s = triples()
    assert np.array_equal(d < s, key(d, low) < score(s))
    assert np.array_equal(d < s, ((d << np.uint64(16)) | low) < (s << np.uint64(16)))      # (without bit 62 on either side)
    assert (d == s).sum() > 50_000 and (d + np.uint64(1) == s).sum() > 50_000                # the borders are there


def test_clearing_the_low_bits_of_the_smallest_key_gives_the_smallest_distance():
    d, low, _ = triples()
    n = len(d) // 8 * 8
    k = key(d[:n], low[:n]).reshape(-1, 8)
    assert np.array_equal(k.min(axis=1) & ~LOW, score(d[:n].reshape(-1, 8).min(axis=1)))
    # ties on d: the smallest key is still that d
    t = key(np.repeat(d[:n // 8], 8), low[:n]).reshape(-1, 8)
    assert np.array_equal(t.min(axis=1) & ~LOW, score(d[:n // 8]))


def test_low_parts_that_grow_with_j_keep_the_d_then_j_order():
    rng = np.random.default_rng(46)
    for trial in range(2_000):
        n = int(rng.integers(1, 256))
        i0 = int(rng.integers(0, 256))                       # the element's own slot: the low part is 4 * (i0 + j - i), unwrapped
        d = rng.integers(0, D_MAX if trial % 2 else 6, n).astype(np.uint64)      # (every other trial: many ties on d)
        off = np.arange(1, n + 1, dtype=np.uint64)
        for low in (np.uint64(4) * (off - np.uint64(1)) + np.uint64(4), np.uint64(4) * (np.uint64(i0) + off)):
            assert int(low.max()) < 1 << 16 and int(low.min()) > 0
            o = np.argsort(key(d, low), kind="stable")
            want = np.lexsort((off, d))
            assert np.array_equal(o, want), trial
    f = key(np.array([0, D_MAX - 1], dtype=np.uint64), np.array([4, 2044], dtype=np.uint64)).view(np.float64)
    assert np.all(np.isfinite(f)) and f[0] < f[1] and f[0] >= np.finfo(np.float64).tiny     # positive normal doubles, as before
