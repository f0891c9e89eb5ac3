"""Plain numpy references of the primitives in sweepga_amd/csrc/swg_sort.hip: the four scans, the byte-flag compaction and the
three radix sorts.  All arithmetic is in uint64 / Python ints; every expected array is fully determined (the sorts are stable),
so a comparison is np.array_equal -- first_difference() below names the first element that differs."""
import numpy as np

U32 = 0xFFFFFFFF
FLAG_TILE = 4096  # swg_flags_count counts per tile of this many flags


def exclusive_sum_u32(x):
    """swg_exclusive_scan_u32: out[i] = (x[0] + ... + x[i-1]) mod 2^32, and the total = (x[0] + ... + x[n-1]) mod 2^32,
    zero-extended into a u64 -- the library accumulates in 32 bits and widens only the result, so the total wraps like the
    elements do (n = 0: an empty output and a total of 0)."""
    x = np.asarray(x, dtype=np.uint32)
    inc = np.cumsum(x.astype(np.uint64), dtype=np.uint64)  # < 2^64 for any n < 2^32
    out = np.zeros(len(x), dtype=np.uint64)
    out[1:] = inc[:-1]
    total = int(inc[-1]) & U32 if len(x) else 0
    return (out & np.uint64(U32)).astype(np.uint32), np.uint64(total)


def inclusive_max(x):
    """swg_inclusive_max_scan_u32 / _u64: out[i] = max(x[0..i]); the dtype of x is kept."""
    x = np.asarray(x)
    assert x.dtype in (np.uint32, np.uint64)
    return np.maximum.accumulate(x) if len(x) else x.copy()


def inclusive_sum_u64(x):
    """swg_inclusive_sum_scan_u64: out[i] = (x[0] + ... + x[i]) mod 2^64 (unsigned numpy sums wrap)."""
    x = np.asarray(x, dtype=np.uint64)
    return np.cumsum(x, dtype=np.uint64)


def compact(flags):
    """swg_flags_count + swg_flags_compact over byte flags (any non-zero byte is set): the ascending positions of the set
    flags as u32, their number, and tile_off = the exclusive running count per tile of 4096 flags."""
    flags = np.asarray(flags, dtype=np.uint8)
    lst = np.flatnonzero(flags).astype(np.uint32)
    nb = (len(flags) + FLAG_TILE - 1) // FLAG_TILE
    padded = np.zeros(nb * FLAG_TILE, dtype=np.uint64)
    padded[:len(flags)] = flags != 0
    per_tile = padded.reshape(nb, FLAG_TILE).sum(axis=1, dtype=np.uint64)
    tile_off = np.zeros(nb, dtype=np.uint64)
    tile_off[1:] = np.cumsum(per_tile, dtype=np.uint64)[:-1]
    return lst, np.uint64(len(lst)), tile_off.astype(np.uint32)


def _mask(bits):
    return np.uint64((1 << bits) - 1)


def _digits(words, shift, bits):
    words = np.asarray(words, dtype=np.uint64)
    if bits <= 0:
        return np.zeros(len(words), dtype=np.uint64)
    return (words >> np.uint64(shift)) & _mask(bits)


def sort_pairs(keys, vals, begin_bit, end_bit):
    """swg_radix_sort_pairs: (key, value) pairs in the stable order of the key bits [begin_bit, end_bit); the other key bits
    travel along untouched.  An empty bit range, or n <= 1, leaves the input as it is."""
    keys, vals = np.asarray(keys, dtype=np.uint64), np.asarray(vals, dtype=np.uint32)
    order = np.argsort(_digits(keys, begin_bit, end_bit - begin_bit), kind="stable")
    return keys[order], vals[order]


def sort_packed(keys, vals, key_bits, val_bits):
    """swg_radix_sort_packed: the stable order of the key bits [0, key_bits); what comes out is one word per element,
    ((key >> 8) << val_bits) | value, in that order.  vals is None: the values are the identity."""
    keys = np.asarray(keys, dtype=np.uint64)
    vals = np.arange(len(keys), dtype=np.uint64) if vals is None else np.asarray(vals, dtype=np.uint32).astype(np.uint64)
    order = np.argsort(_digits(keys, 0, key_bits), kind="stable")
    return (((keys >> np.uint64(8)) << np.uint64(val_bits)) | vals)[order]


def sort_words(words, sorted_bits, val_bits):
    """swg_radix_sort_words: the words themselves in the stable order of their bits [val_bits, val_bits + sorted_bits)."""
    words = np.asarray(words, dtype=np.uint64)
    return words[np.argsort(_digits(words, val_bits, sorted_bits), kind="stable")]


def first_difference(case, what, got, want):
    """None when got equals want element for element; else one line naming the case, the first index that differs and the two
    values there (or the two lengths)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"{case}: {what} has {got.shape[0] if got.ndim else 1} elements, want {want.shape[0] if want.ndim else 1}"
    if got.ndim == 0:
        return None if got == want else f"{case}: {what}: got {int(got):#x}, want {int(want):#x}"
    ne = got != want
    if not ne.any():
        return None
    i = int(np.argmax(ne))
    return f"{case}: {what} differs first at index {i} of {len(want)}: got {int(got[i]):#x}, want {int(want[i]):#x}"
