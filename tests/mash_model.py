"""Independent numpy restatement of the reference's `--joblist` path, written from the Rust text:
FASTA reading (src/main.rs:791-830, 963-990), MinHash sketches (src/mash.rs:78-131), haplotype keys and groups
(src/pansn.rs:58-86, 112-123), merge_sketches (src/knn_graph.rs:568-582), Mash distance (src/mash.rs:39-73), selection
(src/knn_graph.rs:243-393, 400-560), jobs (src/main.rs:848-960) and their text (src/joblist.rs:102-145).
SipHash-1-3 is vectorised over k-mers; tests/test_tree_filter_cpu.py's scalar `siphash` is its reference."""
import math

import numpy as np

U = np.uint64
IV = (U(0x736f6d6570736575), U(0x646f72616e646f6d), U(0x6c7967656e657261), U(0x7465646279746573))


def _rotl(x, r):
    return (x << U(r)) | (x >> U(64 - r))


def _round(v0, v1, v2, v3):
    v0 = v0 + v1; v1 = _rotl(v1, 13) ^ v0; v0 = _rotl(v0, 32)
    v2 = v2 + v3; v3 = _rotl(v3, 16) ^ v2
    v0 = v0 + v3; v3 = _rotl(v3, 21) ^ v0
    v2 = v2 + v1; v1 = _rotl(v1, 17) ^ v2; v2 = _rotl(v2, 32)
    return v0, v1, v2, v3


def sip13_blocks(words, total_len):
    """SipHash-1-3, zero keys, over messages given as full 8-byte words (list of uint64 arrays) + the final block's
    tail bytes already folded into words[-1] with the length byte; total_len is only for the caller's bookkeeping."""
    n = len(words[0])
    v0, v1, v2, v3 = (np.full(n, c, dtype=np.uint64) for c in IV)
    with np.errstate(over="ignore"):
        for m in words:
            v3 = v3 ^ m
            v0, v1, v2, v3 = _round(v0, v1, v2, v3)
            v0 = v0 ^ m
        v2 = v2 ^ U(0xff)
        for _ in range(3):
            v0, v1, v2, v3 = _round(v0, v1, v2, v3)
    return v0 ^ v1 ^ v2 ^ v3


def _hash_windows(byts, starts, k):
    """<[u8] as Hash> of every window byts[s:s+k]: le64(k), then the bytes (mash.rs:109-113)"""
    n = len(starts)
    words = [np.full(n, k, dtype=np.uint64)]
    nfull, rem = divmod(k, 8)
    for w in range(nfull):
        m = np.zeros(n, dtype=np.uint64)
        for b in range(8):
            m |= byts[starts + 8 * w + b].astype(np.uint64) << U(8 * b)
        words.append(m)
    m = np.full(n, (8 + k) << 56, dtype=np.uint64)
    for b in range(rem):
        m |= byts[starts + 8 * nfull + b].astype(np.uint64) << U(8 * b)
    words.append(m)
    return sip13_blocks(words, 8 + k)


_UP = np.arange(256, dtype=np.uint8)
_UP[ord("a"):ord("z") + 1] -= 32
_IS_BASE = np.zeros(256, dtype=bool)
_IS_BASE[[ord(c) for c in "ACGT"]] = True
_IS_BASE = _IS_BASE[_UP]
_COMP = _UP.copy()  # reverse_complement_kmer, mash.rs:120-131: complement of the upper case, other bytes as they are
for a, b in ("AT", "TA", "CG", "GC"):
    _COMP[_UP == ord(a)] = ord(b)


def sketch(seq, k, s):
    """KmerSketch::from_sequence (mash.rs:78-107): bottom s of min(h_fwd, h_rev), multiplicity kept."""
    arr = np.frombuffer(bytes(seq), dtype=np.uint8)
    if len(arr) < k:
        return np.zeros(0, dtype=np.uint64)
    bad = np.concatenate([[0], np.cumsum(~_IS_BASE[arr])])
    nwin = len(arr) - k + 1
    starts = np.nonzero(bad[k:k + nwin] - bad[:nwin] == 0)[0]
    if len(starts) == 0:
        return np.zeros(0, dtype=np.uint64)
    out = []
    for c0 in range(0, len(starts), 1 << 20):
        st = starts[c0:c0 + (1 << 20)]
        hf = _hash_windows(arr, st, k)
        rc = _COMP[arr[::-1]]  # window [s, s+k) reversed = rc[L-s-k, L-s)
        hr = _hash_windows(rc, len(arr) - st - k, k)
        h = np.minimum(hf, hr)
        out.append(np.sort(h)[:s])
    return np.sort(np.concatenate(out))[:s]


def merge(parts, s):  # merge_sketches, knn_graph.rs:568-582
    v = np.unique(np.concatenate([np.asarray(p, dtype=np.uint64) for p in parts] + [np.zeros(0, dtype=np.uint64)]))
    return v[:s]


def jaccard_counts(a, b):  # mash.rs:39-56: sets
    sa, sb = set(int(x) for x in a), set(int(x) for x in b)
    return len(sa & sb), len(sa | sb)


def mash_distance(a, b, k):  # mash.rs:58-73
    return distance_from_counts(*jaccard_counts(a, b), k)


def distance_from_counts(inter, union, k):
    j = 0.0 if union == 0 else inter / union
    if j <= 0.0:
        return 1.0
    ratio = (2.0 * j) / (1.0 + j)
    if ratio <= 0.0:
        return 1.0
    return (-1.0 / k) * math.log(ratio)


def distance_matrix(sketches, k):  # distance_matrix_from_sketches, mash.rs:188-202
    n = len(sketches)
    d = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1, n):
            d[i, j] = d[j, i] = mash_distance(sketches[i], sketches[j], k)
    return d


# ---- selection ---------------------------------------------------------------------------------------------------
def sip13_pair(i, j):
    """DefaultHasher: write_usize(i), write_usize(j) -- vectorised over arrays i, j (knn_graph.rs:369-376)"""
    i = np.asarray(i, dtype=np.uint64)
    j = np.asarray(j, dtype=np.uint64)
    return sip13_blocks([i, j, np.full(i.shape, 16 << 56, dtype=np.uint64)], 16)


def random_threshold(f):  # (f * u64::MAX as f64) as u64, saturating
    t = f * 18446744073709551616.0
    if not t > 0.0:
        return 0
    return 2**64 - 1 if t >= 18446744073709551616.0 else int(t)


def random_pairs(n, f):  # generate_random_pairs, knn_graph.rs:362-386
    thr = random_threshold(f)
    out = []
    for i in range(n):
        j = np.arange(i + 1, n, dtype=np.uint64)
        if len(j):
            h = sip13_pair(np.full(len(j), i, dtype=np.uint64), j)
            out += [(i, int(x)) for x in j[h <= U(thr)]]
    return out


def build_knn_graph(d, kk, farthest):  # knn_graph.rs:337-360: stable sort by partial_cmp
    n = len(d)
    pairs = []
    for i in range(n):
        nb = [(float(d[i][j]), j) for j in range(n) if j != i]
        nb = sorted(nb, key=lambda t: t[0], reverse=farthest)  # Python's sort is stable in both directions
        pairs += [(i, j) for _, j in nb[:min(kk, len(nb))]]
    return pairs


def tree_pairs(d, kn, kf, rf):  # extract_tree_pairs_from_matrix, knn_graph.rs:243-286
    n = len(d)
    if n < 2:
        return []
    allp = []
    if kn > 0:
        allp += build_knn_graph(d, kn, False)
    if kf > 0:
        allp += build_knn_graph(d, kf, True)
    if rf > 0.0:
        allp += random_pairs(n, rf)
    return sorted(set((min(a, b), max(a, b)) for a, b in allp))


def estimate_tree_pair_count(n, kn, kf, rf):  # knn_graph.rs:388-399
    total = n * (n - 1) // 2
    return min(n * min(kn, max(n - 1, 0)) + n * min(kf, max(n - 1, 0)) + int(round_half_away(total * rf)), total)


def round_half_away(x):
    return math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5)


def parse_strategy(s):  # SparsificationStrategy::from_str, knn_graph.rs:59-160 (the shapes the tests use)
    try:
        f = float(s)
        return ("random", f)
    except ValueError:
        pass
    if s in ("none", "all"):
        return ("none",)
    if s == "auto":
        return ("auto",)
    if s.startswith("random:"):
        return ("random", float(s[7:]))
    if s.startswith("giant:") or s.startswith("connectivity:"):
        return ("giant", float(s.split(":", 1)[1]))
    if s.startswith("tree:") or s.startswith("knn:"):
        p = s.split(":", 1)[1].split(":")
        return ("tree", int(p[0]), int(p[1]) if len(p) > 1 else 0, float(p[2]) if len(p) > 2 else 0.0)
    if s.startswith("wfmash:"):
        return ("wfmash",)
    raise ValueError(s)


def needs_sketches(st):
    return st[0] in ("auto", "giant", "tree")


def select(st, d, n):  # select_pairs (:400-489, sequences = None) / select_pairs_from_sketches (:498-560)
    allp = [(i, j) for i in range(n) for j in range(i + 1, n)]
    if st[0] in ("none", "wfmash"):
        return allp
    if st[0] == "random":
        return random_pairs(n, st[1])
    if st[0] == "auto":
        if n <= 10:
            return allp
        if n <= 50:
            return select(("giant", 0.99), d, n)
        return tree_pairs(d, 5, 2, 0.05)
    if st[0] == "giant":
        target = math.ceil(float(n) * math.log(float(n)) / 2.0 * (-math.log(st[1])))
        total = n * (n - 1) // 2
        frac = 1.0 if total == 0 else min(target / total, 1.0)
        kn = max(math.ceil(frac * n), 2)
        return tree_pairs(d, kn, 1, 0.01)
    return tree_pairs(d, st[1], st[2], st[3])


# ---- names, FASTA, jobs ------------------------------------------------------------------------------------------
WS = b" \t\n\x0b\x0c\r"


def pansn_key(name):  # extract_pansn_key(name, Haplotype), pansn.rs:58-86; None -> whole name (:117)
    t = name.lstrip(">").strip(WS.decode())
    t = t.split()[0] if t.split() else ""
    base = t.split(":")[0]
    if not base:
        return name
    parts = base.split("#")
    if not parts[0]:
        return name
    if len(parts) > 1 and parts[1]:
        return parts[0] + "#" + parts[1]
    return parts[0]


def read_fasta_bytes(data):
    """(names, sequences) of one file's bytes: BufRead::lines + trim (main.rs:791-830, 963-990)"""
    lines = data.split(b"\n")
    had_nl = [True] * (len(lines) - 1) + [False]
    if lines and lines[-1] == b"":
        lines, had_nl = lines[:-1], had_nl[:-1]
    lines = [ln[:-1] if nl and ln.endswith(b"\r") else ln for ln, nl in zip(lines, had_nl)]
    names, seqs, cur, have = [], [], b"", False
    for ln in lines:
        if ln.startswith(b">"):
            tok = ln[1:].split()
            names.append((tok[0] if tok else b"").decode())
            if have:
                seqs.append(cur)
                cur = b""
            have = True
        else:
            cur += ln.strip(WS)
    if have:
        seqs.append(cur)
    return names, seqs


def sanitize(s):  # joblist.rs:102-113
    return "".join("_" if c in '/\\#: \t*?"<>|' else c for c in s)


def emit(jobs, output_dir, threads, block_length):
    """write_wfmash_pansn_commands (joblist.rs:124-145); jobs = [(target_hap, query_hap, target_fa, query_fa)]"""
    out = []
    for t, q, tf, qf in jobs:
        name = f"{sanitize(t)}_vs_{sanitize(q)}.paf"
        path = name if output_dir == "" else (output_dir + name if output_dir.endswith("/") else output_dir + "/" + name)
        cmd = f"wfmash -t {threads}"
        if block_length > 0:
            cmd += f" -l {block_length}"
        cmd += f" -T {t} -Q {q} {tf}"
        if qf != tf:
            cmd += f" {qf}"
        out.append(cmd + f" > {path}\n")
    return "".join(out)


def joblist(paths, strategy="none", k=15, s=1000, threads=8, block_length=0, output_dir=".", reader=None):
    """pansn_joblist_jobs (main.rs:848-960) + emit.  reader(path) -> bytes of the (decompressed) file."""
    reader = reader or (lambda p: open(p, "rb").read())
    names, files, seqs = [], [], []
    for p in paths:
        nm, sq = read_fasta_bytes(reader(p))
        names += nm
        seqs += sq
        files += [p] * len(nm)
    hap_of = [pansn_key(n) for n in names]
    keys = sorted(set(hap_of), key=lambda x: x.encode())
    if not names or len(keys) == len(names):
        return None  # the reference's non-PanSN fallback
    idx = {h: i for i, h in enumerate(keys)}
    groups = [[] for _ in keys]
    for c, h in enumerate(hap_of):
        groups[idx[h]].append(c)
    st = parse_strategy(strategy)
    d = None
    if needs_sketches(st):
        cs = [sketch(x, k, s) for x in seqs]
        hs = [merge([cs[c] for c in g], s) for g in groups]
        d = distance_matrix(hs, k)
    pairs = set(select(st, d, len(keys)))
    pairs |= {(h, h) for h in range(len(keys))}
    jobs = [(keys[i], keys[j], files[groups[i][0]], files[groups[j][0]]) for i, j in sorted(pairs)]
    return emit(jobs, output_dir, threads, block_length)
