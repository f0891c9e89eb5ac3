"""Arguments for the checks of the logarithm (sweepga_amd/csrc/swg_log.h) against libm: every kind of double a caller
can hand it.  Shared by the CPU check (tests/test_abi_cpu.py) and the device check (tests/test_gpu_sweep.py)."""
import numpy as np

# glibc's log takes its near-1 branch when bits(x) - WIN_LO < WIN_HI - WIN_LO.  The two bounds are the immediates of that
# comparison in the platform libm's `__log_fma` (glibc 2.35: add 0xc012000000000000, compare with 0x000308ffffffffff),
# i.e. 1 - 0x1p-4 and 1 + 0x1.09p-4, as in sysdeps/ieee754/dbl-64/e_log.c.
WIN_LO = 0x3FEE000000000000
WIN_HI = 0x3FF1090000000000
ONE = 0x3FF0000000000000
# integer ranges (first, stride, count): one that ends just under 2^53, one that covers [2^63, 2^64)
INT_RANGE_53 = (1, (1 << 31) - 1, 1 << 22)
INT_RANGE_64 = (1 << 63, (1 << 41) - 2039, 1 << 22)
assert INT_RANGE_53[0] + (INT_RANGE_53[2] - 1) * INT_RANGE_53[1] < 1 << 53
assert INT_RANGE_64[0] + (INT_RANGE_64[2] - 1) * INT_RANGE_64[1] < 1 << 64


def _bits(b):
    return np.asarray(b, dtype=np.uint64).view(np.float64)


def mash_counts(max_union):
    """(inter, union) of every pair of counts 1 <= inter <= union <= max_union"""
    un = np.repeat(np.arange(1, max_union + 1, dtype=np.int64), np.arange(1, max_union + 1))
    start = np.cumsum(np.arange(0, max_union, dtype=np.int64))  # index of the first pair of every union
    inter = np.arange(len(un), dtype=np.int64) - np.repeat(start, np.arange(1, max_union + 1)) + 1
    return inter, un


def mash_ratio(inter, un):
    """2J / (1 + J) as mash_dist_kernel computes it: quotient, product, sum, quotient, each rounded once"""
    j = inter.astype(np.float64) / un.astype(np.float64)
    return (2.0 * j) / (1.0 + j)


def window(rng, n):
    """n doubles inside the near-1 window, uniform over its bit patterns"""
    return _bits(rng.integers(WIN_LO, WIN_HI, n, dtype=np.uint64))


def window_edges():
    """first and last double of the window below 1 and above 1, the neighbours just outside, 1 and 1 +- 1 ulp"""
    return _bits([WIN_LO - 1, WIN_LO, WIN_LO + 1, ONE - 2, ONE - 1, ONE, ONE + 1, ONE + 2, WIN_HI - 2, WIN_HI - 1, WIN_HI, WIN_HI + 1])


def binades(rng, n):
    """n positive normal doubles: exponent uniform over all 2046 normal binades, mantissa uniform"""
    e = rng.integers(1, 2047, n, dtype=np.uint64)
    m = rng.integers(0, 1 << 52, n, dtype=np.uint64)
    return _bits((e << np.uint64(52)) | m)


def integers(rng, n):
    """integers as f64: uniform below 2^53, every magnitude up to 2^53, and [2^63, 2^64) (rounded as a u64 -> f64 cast)"""
    a = rng.integers(1, 1 << 53, n, dtype=np.uint64, endpoint=True)
    b = rng.integers(0, 1 << 53, n, dtype=np.uint64) >> rng.integers(0, 53, n, dtype=np.uint64)
    c = rng.integers(1 << 63, (1 << 64) - 1, n, dtype=np.uint64, endpoint=True)
    return np.concatenate([a, np.maximum(b, np.uint64(1)), c, np.array([1, 2, 3, (1 << 53) - 1, 1 << 53, 1 << 63, (1 << 64) - 1], dtype=np.uint64)]).astype(np.float64)


def specials(rng):
    """+-0, negatives, subnormals (the extremes and 4096 random ones), the smallest normals, +-inf and NaNs"""
    sub = rng.integers(1, 1 << 52, 4096, dtype=np.uint64) >> rng.integers(0, 52, 4096, dtype=np.uint64)
    fixed = [0, 1 << 63, 0xBFF0000000000000, 0xC08F400000000000, (1 << 63) | 1, 0xFFF0000000000000,  # 0 -0 -1 -1000 -5e-324 -inf
             1, 2, 3, (1 << 52) - 1, 1 << 51, 1 << 52, (1 << 52) + 1,                                  # subnormals, 0x1p-1022
             0x7FEFFFFFFFFFFFFF, 0x7FF0000000000000, 0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001]
    return _bits(np.concatenate([np.array(fixed, dtype=np.uint64), np.maximum(sub, np.uint64(1))]))
