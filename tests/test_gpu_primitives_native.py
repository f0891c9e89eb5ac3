"""The scans, the byte-flag compaction and the radix sorts of csrc/swg_sort.hip, each on its own, against tests/prim_model.py.

tests/native/prim_check.cpp (sweepga_amd/bin/prim_check) runs a list of cases in one process and one context and writes every
output to a file; everything is checked here, element for element, with no tolerance (every expected array is fully determined:
the sorts are stable).  One driver process per group; the sort knobs are read once per process, so each knob is a group.

What the shapes are for:
  scans    tile = 4096 elements (4 waves x 1024, rows of 256, 4 elements per lane): sizes around the 4-element vector, a row, a
           wave's span, a tile, several tiles, and 4096^2 - 1 / 4096^2 / 4096^2 + 1 (the last is the first size with three levels
           of the reduce / recurse / down-sweep; each of these sizes is a group of its own so that no group moves more than one
           input and one output of it); pointers 1-3 elements off 16-byte alignment take the scalar load / store path that
           aligned arena blocks never reach; u32 sums wrap modulo 2^32, the total included.
  compact  every class of non-zero byte, flag pointers off 16-byte alignment, tile_off and the poison behind the list's end.
  sorts    tile = 8192; skew (one digit holding whole tiles, constant passes, the all-ones key that the padding lanes of the last
           tile also carry), every mix of 8- and 9-bit digits the plans produce, bit ranges off bit 0, value arrays that are not
           the identity (duplicates included: only the stable order gives the expected array), caller-made histograms."""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

from tests import prim_model as pm

pytestmark = pytest.mark.gpu

SWG_OK, SWG_ERR_UNSUPPORTED = 0, -6
POISON32 = 0xA5A5A5A5
SEED = 20261018


@pytest.fixture(scope="module")
def prim_check():
    from sweepga_amd import build
    return build.build_prim_check()


class Group:
    """The cases of one driver process: input files, the case list, and per case what to expect."""

    def __init__(self, env=None):
        self.env = dict(env or {})
        self.files = {}   # file name -> array
        self.names = set()
        self.cases = []   # (name, operation, {key: value}, expected return code, check(outputs) -> [messages])

    def data(self, name, arr):
        self.files.setdefault(name, arr)
        return name

    def add(self, name, op, params, check, rc=SWG_OK):
        assert name not in self.names and " " not in name and "." not in name
        self.names.add(name)
        self.cases.append((name, op, params, rc, check))


def rand_bits(rng, n, bits, dtype=np.uint64):
    """n uniform values below 2^bits."""
    if bits <= 0:
        return np.zeros(n, dtype=dtype)
    x = rng.integers(0, 1 << 64, size=n, dtype=np.uint64, endpoint=False) >> np.uint64(64 - bits)
    return x.astype(dtype)


# ---- scans ----------------------------------------------------------------------------------------------------------------
SCAN_SIZES = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 3 * 4096 + 2]
SCAN_LARGE = [4096 * 4096 - 1, 4096 * 4096, 4096 * 4096 + 1]
SCAN_OPS = {  # operation -> (dtype, model, is a sum, has a total)
    "scan_excl_sum_u32": (np.uint32, pm.exclusive_sum_u32, True, True),
    "scan_incl_max_u32": (np.uint32, lambda x: (pm.inclusive_max(x), None), False, False),
    "scan_incl_max_u64": (np.uint64, lambda x: (pm.inclusive_max(x), None), False, False),
    "scan_incl_sum_u64": (np.uint64, lambda x: (pm.inclusive_sum_u64(x), None), True, False),
}
# the two largest sizes run only where three levels and wide elements matter most; 4096^2 - 1 runs for every operation
SCAN_LARGE_OPS = {"scan_excl_sum_u32": SCAN_LARGE, "scan_incl_max_u64": SCAN_LARGE, "scan_incl_max_u32": SCAN_LARGE[:1],
                  "scan_incl_sum_u64": SCAN_LARGE[:1]}


def scan_patterns(rng, n, dtype, is_sum):
    """(label, data) for one size."""
    bits = 32 if dtype == np.uint32 else 64
    top = (1 << bits) - 1
    out = [("uniform", rand_bits(rng, n, bits, dtype)),  # u64: the high 32 bits are set, as in unit << 32 | end
           ("zeros", np.zeros(n, dtype=dtype)),
           ("ones", np.ones(n, dtype=dtype)),
           ("allbits", np.full(n, top, dtype=dtype))]
    if is_sum:  # +1 / -1 events, balanced: the running value keeps coming back to 0 and dips below it (wraps)
        half = rng.permutation(n) < n // 2
        out.append(("plusminus", np.where(half, dtype(1), dtype(top))))
        out.append(("updown", np.where(np.arange(n) % 2 == 0, dtype(1), dtype(top))))
    else:
        out.append(("descending", (np.uint64(top) - np.arange(n, dtype=np.uint64) * np.uint64(3)).astype(dtype)))
        out.append(("ascending", (np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1 << (bits - 8))).astype(dtype)))
        for at in (4095, 4096):
            if at < n:
                x = rand_bits(rng, n, bits - 1, dtype)
                x[at] = top
                out.append((f"peak{at}", x))
    for at in sorted({p for p in (0, 1023, 1024, 4095, 4096, n - 1) if 0 <= p < n}):
        x = np.zeros(n, dtype=dtype)
        x[at] = top - 6
        out.append((f"single{at}", x))
    return out


def scan_check(name, model, x, want_total):
    def check(outs):
        want, total = model(x)
        msgs = [pm.first_difference(name, "out", outs["out"](x.dtype), want)]
        if want_total:
            msgs.append(pm.first_difference(name, "total", outs["total"](np.uint64)[0], total))
        return msgs
    return check


def scan_group(op, large_n=None):
    def make():
        dtype, model, is_sum, has_total = SCAN_OPS[op]
        rng = np.random.default_rng([SEED, sorted(SCAN_OPS).index(op), large_n or 0])
        g = Group()

        def add(name, x, **kw):
            want_total = kw.pop("want_total", True) and has_total
            params = dict(n=len(x), in_off=0, out_off=0, in_place=0, want_total=int(want_total))
            params.update(kw)
            params["in"] = g.data(name + ".in", x)
            g.add(name, op, params, scan_check(name, model, x, want_total))

        if large_n is not None:  # random data, aligned, out of place
            add(f"n{large_n}_uniform", rand_bits(rng, large_n, 32 if dtype == np.uint32 else 64, dtype))
            return g
        for n in SCAN_SIZES:
            for label, x in scan_patterns(rng, n, dtype, is_sum):
                add(f"n{n}_{label}", x)
                if label == "uniform":
                    add(f"n{n}_{label}_inplace", x, in_place=1)
                    if has_total:
                        add(f"n{n}_{label}_nototal", x, want_total=False)
        # addressing: pointers off their 16-byte alignment (the scalar path of load_vec4 / store_vec4)
        for n in (4097, 8193):
            x = rand_bits(rng, n, 32 if dtype == np.uint32 else 64, dtype)
            for off in range(16 // np.dtype(dtype).itemsize):
                add(f"n{n}_off{off}_inplace", x, in_off=off, out_off=off, in_place=1)
                add(f"n{n}_off{off}_both", x, in_off=off, out_off=off)
                if off:
                    add(f"n{n}_off{off}_out", x, out_off=off, want_total=False)
                    add(f"n{n}_off{off}_in", x, in_off=off)
        return g
    return make


# ---- compaction -----------------------------------------------------------------------------------------------------------
FLAG_SIZES = [0, 1, 15, 16, 17, 4095, 4096, 4097, 8193, 1_000_003]
FLAG_BYTES = np.array([0x01, 0x02, 0x7F, 0x80, 0xFF], dtype=np.uint8)  # every class nonzero_bytes() tells from 0


def compact_check(name, flags):
    def check(outs):
        lst, total, tile_off = pm.compact(flags)
        got = outs["list"](np.uint32)
        k = int(total)
        return [pm.first_difference(name, "total", outs["total"](np.uint64)[0], total),
                pm.first_difference(name, "list", got[:k], lst),
                pm.first_difference(name, "list slots behind the total", got[k:], np.full(len(flags) - k, POISON32, dtype=np.uint32)),
                pm.first_difference(name, "tile_off", outs["tile_off"](np.uint32), tile_off)]
    return check


def compact_group():
    rng = np.random.default_rng([SEED, 100])
    g = Group()

    def add(name, set_mask, off=0):
        flags = np.where(set_mask, rng.choice(FLAG_BYTES, size=len(set_mask)), 0).astype(np.uint8)
        g.add(name, "compact", {"n": len(flags), "in_off": off, "in": g.data(name + ".in", flags)}, compact_check(name, flags))

    for n in FLAG_SIZES:
        idx = np.arange(n)
        add(f"n{n}_none", np.zeros(n, dtype=bool))
        add(f"n{n}_all", np.ones(n, dtype=bool))
        add(f"n{n}_last", idx == n - 1)
        for at in (4095, 4096):
            if at < n:
                add(f"n{n}_only{at}", idx == at)
        for pct in (1, 50, 99):
            add(f"n{n}_random{pct}", rng.random(n) < pct / 100.0)
    for n in (4097, 8193):
        for off in (0, 1, 7, 8, 15):  # bytes
            add(f"n{n}_off{off}", rng.random(n) < 0.5, off=off)
    return g


# ---- sorts ----------------------------------------------------------------------------------------------------------------
SORT_SIZES = [2, 3, 8191, 8192, 8193, 3 * 8192 + 1, 200_003]
SORT_DIST_SIZES = [8193, 200_003]
DISTS = ["constant", "allones", "two", "sorted", "reversed", "top", "low", "skew", "uniform"]
VAL_BITS = [1, 7, 20, 32]


def digits_of(rng, dist, n, w, top_w=8):
    """n values below 2^w (the bits a sort looks at) drawn from one of the key distributions; top_w / the low digit: how many
    bits the plans' top and bottom digits have at most."""
    full = (1 << w) - 1
    if dist == "constant":
        return np.full(n, int(rand_bits(rng, 1, w)[0]), dtype=np.uint64)
    if dist == "allones":
        return np.full(n, full, dtype=np.uint64)
    if dist == "two":
        ab = np.array([int(rand_bits(rng, 1, w)[0]), full ^ (full >> 1) if w > 1 else 1], dtype=np.uint64)
        return ab[rng.integers(0, 2, size=n)]
    if dist == "sorted":
        return np.sort(rand_bits(rng, n, w))
    if dist == "reversed":
        return np.sort(rand_bits(rng, n, w))[::-1].copy()
    if dist == "top":  # only the top digit varies
        t = min(top_w, w)
        return (rand_bits(rng, n, t) << np.uint64(w - t)) | (rand_bits(rng, 1, w - t)[0] if w > t else np.uint64(0))
    if dist == "low":  # only the lowest digit varies
        t = min(8, w)
        return rand_bits(rng, n, t) | ((rand_bits(rng, 1, w - t)[0] << np.uint64(t)) if w > t else np.uint64(0))
    if dist == "skew":  # geometric: value lengths thin out by halves; and half of all keys are one value
        x = rand_bits(rng, n, w) >> np.minimum(rng.geometric(0.25, size=n), w - 1).astype(np.uint64)
        x[rng.random(n) < 0.5] = x[0]
        return x
    assert dist == "uniform"
    return rand_bits(rng, n, w)


def sort_shapes(plans):
    """(n, distribution, plan) over: every size x every plan with uniform keys; every distribution x every plan at 8193;
    every distribution at 200 003 with the plans taken in turn (and all of them under uniform keys, from the first part)."""
    out = [(n, "uniform", p) for n in SORT_SIZES for p in plans]
    out += [(SORT_DIST_SIZES[0], d, p) for d in DISTS[:-1] for p in plans]
    out += [(SORT_DIST_SIZES[1], d, plans[i % len(plans)]) for i, d in enumerate(DISTS[:-1])]
    return out


PAIR_PLANS = [(0, 8), (0, 17), (5, 29), (32, 64)]  # begin_bit, end_bit


def pairs_check(name, keys, vals, b, e):
    def check(outs):
        wk, wv = pm.sort_pairs(keys, vals, b, e)
        return [pm.first_difference(name, "keys", outs["keys"](np.uint64), wk),
                pm.first_difference(name, "vals", outs["vals"](np.uint32), wv)]
    return check


def pairs_group(env=None, prehist=True):
    def make():
        rng = np.random.default_rng([SEED, 200])
        g = Group(env)

        def add(name, keys, vals, b, e, use_prehist=0):
            g.add(name, "sort_pairs", {"n": len(keys), "begin_bit": b, "end_bit": e, "use_prehist": use_prehist,
                                       "in": g.data(name.replace("_prehist", "") + ".keys_in", keys),
                                       "in1": g.data(name.replace("_prehist", "") + ".vals_in", vals)}, pairs_check(name, keys, vals, b, e))

        for i, (n, dist, (b, e)) in enumerate(sort_shapes(PAIR_PLANS)):
            w = e - b
            # the bits outside [b, e) are random: they travel along, and tell equal digits apart (stability shows in the keys too)
            outside = rand_bits(rng, n, 64) & np.uint64(((1 << 64) - 1) ^ (((1 << w) - 1) << b))
            keys = (digits_of(rng, dist, n, w) << np.uint64(b)) | outside
            vb = VAL_BITS[i % 4]
            vals = rand_bits(rng, n, vb, np.uint32)
            name = f"n{n}_{dist}_b{b}_e{e}_v{vb}"
            add(name, keys, vals, b, e)
            if prehist and (b, e) == (5, 29) and n in SORT_DIST_SIZES and dist in ("uniform", "skew", "allones"):
                add(name + "_prehist", keys, vals, b, e, use_prehist=1)
        # nothing to do: OK, and the buffers as they were
        k, v = rand_bits(rng, 8193, 64), rand_bits(rng, 8193, 20, np.uint32)
        add("n1_nothing_to_sort", k[:1], v[:1], 0, 64)
        add("n8193_empty_bit_range", k, v, 24, 24)
        return g
    return make


PACKED_KEY_BITS = [9, 16, 25, 26, 41, 44, "widest"]  # 44 = 8 + 9+9+9+9, 41 = 8 + 9+8+8+8, 26 = 8 + 9+9, 25 = 8 + 9+8


def packed_plans(kb, identity, n):
    """(key_bits, val_bits) of one entry of PACKED_KEY_BITS, for every value width with key_bits - 8 + val_bits <= 64; "widest":
    key_bits = 64 - val_bits + 8, capped at the 64 bits a key has.  Identity values need n <= 2^val_bits."""
    out = []
    for vb in VAL_BITS:
        k = min(64, 64 - vb + 8) if kb == "widest" else kb
        if k - 8 + vb <= 64 and (not identity or n <= (1 << vb)):
            out.append((k, vb))
    return out


def packed_check(name, keys, vals, kb, vb):
    def check(outs):
        return [pm.first_difference(name, "words", outs["words"](np.uint64), pm.sort_packed(keys, vals, kb, vb))]
    return check


def packed_group(identity):
    def make():
        rng = np.random.default_rng([SEED, 300 + int(identity)])
        g = Group()

        def add(name, keys, vals, kb, vb, use_prehist=0, rc=SWG_OK):
            params = {"n": len(keys), "key_bits": kb, "val_bits": vb, "identity_vals": int(identity), "use_prehist": use_prehist,
                      "in": g.data(name.replace("_prehist", "") + ".keys_in", keys)}
            if not identity:
                params["in1"] = g.data(name.replace("_prehist", "") + ".vals_in", vals)
            g.add(name, "sort_packed", params, packed_check(name, keys, None if identity else vals, kb, vb), rc)

        turn = 0
        for n, dist, kb_label in sort_shapes(PACKED_KEY_BITS):
            plans = packed_plans(kb_label, identity, n)
            # the small sizes and the distributions at 8193 take every value width, the 200 003 cases take them in turn
            if n == SORT_DIST_SIZES[1]:
                turn += 1
                plans = plans[turn % len(plans):][:1]
            for kb, vb in plans:
                keys = digits_of(rng, dist, n, kb, top_w=9)
                vals = rand_bits(rng, n, vb, np.uint32)
                name = f"n{n}_{dist}_k{kb}_v{vb}"
                add(name, keys, vals, kb, vb)
                if kb in (41, 44) and n in SORT_DIST_SIZES and dist in ("uniform", "skew", "allones") and vb == 20:
                    add(name + "_prehist", keys, vals, kb, vb, use_prehist=1)
        add("n8193_key_bits_8_unsupported", rand_bits(rng, 8193, 8), rand_bits(rng, 8193, 20, np.uint32), 8, 20, rc=SWG_ERR_UNSUPPORTED)
        return g
    return make


WORD_SORTED_BITS = [8, 16, 17, 27, 33, 36]  # 17 = 8+9, 27 = 9+9+9, 33 = 8+8+8+9, 36 = 9+9+9+9


def words_check(name, words, sb, vb):
    def check(outs):
        return [pm.first_difference(name, "words", outs["words"](np.uint64), pm.sort_words(words, sb, vb))]
    return check


def words_group():
    rng = np.random.default_rng([SEED, 400])
    g = Group()

    def add(name, words, sb, vb, use_prehist=0, rc=SWG_OK):
        g.add(name, "sort_words", {"n": len(words), "sorted_bits": sb, "val_bits": vb, "use_prehist": use_prehist,
                                   "in": g.data(name.replace("_prehist", "") + ".in", words)}, words_check(name, words, sb, vb), rc)

    def make_words(dist, n, sb, vb):
        w = (digits_of(rng, dist, n, sb, top_w=9) << np.uint64(vb)) | rand_bits(rng, n, vb)
        if dist == "uniform" and sb + vb < 64:  # bits above the sorted ones travel along
            w |= rand_bits(rng, n, 64 - sb - vb) << np.uint64(sb + vb)
        return w

    turn = 0
    for n, dist, sb in sort_shapes(WORD_SORTED_BITS):
        vbs = [vb for vb in VAL_BITS if sb + vb <= 64]
        if n == SORT_DIST_SIZES[1]:
            turn += 1
            vbs = vbs[turn % len(vbs):][:1]
        for vb in vbs:
            name = f"n{n}_{dist}_s{sb}_v{vb}"
            words = make_words(dist, n, sb, vb)
            add(name, words, sb, vb)
            if sb in (33, 36) and n in SORT_DIST_SIZES and dist in ("uniform", "skew", "allones") and vb == 20:
                add(name + "_prehist", words, sb, vb, use_prehist=1)
    add("n1_unsupported", rand_bits(rng, 1, 56), 36, 20, rc=SWG_ERR_UNSUPPORTED)
    add("n8193_65_bits_unsupported", rand_bits(rng, 8193, 64), 33, 32, rc=SWG_ERR_UNSUPPORTED)
    return g


GROUPS = {op: scan_group(op) for op in SCAN_OPS}
GROUPS.update({f"{op}_n{n}": scan_group(op, n) for op, sizes in SCAN_LARGE_OPS.items() for n in sizes})
GROUPS.update({
    "compact": compact_group,
    "sort_pairs": pairs_group(),
    "sort_packed": packed_group(False),
    "sort_packed_identity": packed_group(True),
    "sort_words": words_group,
    "pairs_fallback": pairs_group({"SWG_SORT_FALLBACK": "1"}, prehist=False),
    "pairs_wide": pairs_group({"SWG_SORT_WIDE": "1"}),
})


def run_group(exe, g, work):
    """Writes the group's files and case list into `work`, runs the driver once and returns every failed check as a line."""
    for fname, arr in g.files.items():
        arr.tofile(os.path.join(work, fname))
    with open(os.path.join(work, "cases.txt"), "w") as f:
        for name, op, params, _, _ in g.cases:
            f.write(" ".join([name, op] + [f"{k}={v}" for k, v in params.items()]) + "\n")
    env = dict(os.environ)
    for knob in ("SWG_SORT_FALLBACK", "SWG_SORT_WIDE", "SWG_SORT_PAIRS", "SWG_SORT_BITS8", "SWG_SORT_DROP"):
        env.pop(knob, None)
    env.update(g.env)
    r = subprocess.run([exe, os.path.join(work, "cases.txt"), work], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, f"prim_check ended with status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}"
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("case ")]
    assert [ln[1] for ln in lines] == [c[0] for c in g.cases], "the driver did not report every case, in order"
    failures = []
    for ln, (name, _, _, want_rc, check) in zip(lines, g.cases):
        rc, guards, files = (ln[i].split("=", 1)[1] for i in (2, 3, 4))
        if int(rc) != want_rc:
            failures.append(f"{name}: returned {rc}, want {want_rc}")
            continue
        if guards != "ok":
            failures.append(f"{name}: guard bytes overwritten: {guards}")
        if want_rc != SWG_OK:
            if files != "-":
                failures.append(f"{name}: wrote {files} although it declined")
            continue
        outs = {fn.rsplit(".", 1)[1]: (lambda dt, fn=fn: np.fromfile(os.path.join(work, fn), dtype=dt)) for fn in files.split(",")}
        failures += [m for m in check(outs) if m]
    return failures


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_primitives_equal_the_model(prim_check, tmp_path, group):
    g = GROUPS[group]()
    work = str(tmp_path / "w")
    os.makedirs(work)
    t0 = time.perf_counter()
    try:
        failures = run_group(prim_check, g, work)
    finally:
        shutil.rmtree(work, ignore_errors=True)  # up to a few hundred MB per group
    print(f"\nprimitives group {group}: {len(g.cases)} cases, {time.perf_counter() - t0:.2f} s")
    assert not failures, f"{len(failures)} of {len(g.cases)} cases failed; the first:\n" + "\n".join(failures[:20])
