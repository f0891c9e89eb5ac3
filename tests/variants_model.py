"""Literal model of the variant calls: per entry the CIGAR is walked op by op with tests/lift_exact_model.py's
parser over Python byte strings -- no prefix sums, no searches.  Every entry it checks is held against three consequences of the
definitions: the sums' invariants, the X / I / D counts of tests/diffs_model.py, and the consensus property (the variants applied
to the target interval give the query interval).  Below the model: a generator of targets, queries and CIGARs from a list of
edits, and the texts of the PAF seam."""
import numpy as np

from tests import diffs_model as dm
from tests import lift_exact_model as em
from tests import lift_model as lm

SNP, INS, DEL = 1, 2, 4
MINUS = 256
ANY = 0xFFFFFFFF
SUBS = tuple(r + ">" + a for r in "ACGT" for a in "ACGT" if r != a)
SUMS = ("entries", "compared", "snvs") + SUBS + ("same", "m_equal", "n_columns", "n_ins", "ins_bases", "n_del", "del_bases", "long_indels", "unanchored")
FIELDS = ("n_variants", "pool_bytes", "n_pairs", "ops", "cigar_bad", "usable", "no_sequence", "out_of_sequence", "columns")
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def norm(b):
    """A, C, G or T for those letters in either case, N for every other byte (b: an int)"""
    ch = chr(b).upper()
    return ch if ch in "ACGT" else "N"


def norm_seq(s):
    return "".join(norm(b) for b in s)


def revcomp(s):
    """of a normalised string"""
    return "".join(_COMP[ch] for ch in reversed(s))


def entry_variants(text, minus, q_start, q_end, t_start, t_end, T, Q, record=0, max_indel=0, check=True):
    """One usable entry -> (variants as (record, kind_flags, pos, REF, ALT, q_pos) with the alleles as str, sums as a dict without
    `entries`).  T, Q: the target's and the query's bytes."""
    ops = em.parse(text)[1]
    out, sums, right = [], dict.fromkeys(SUMS[1:], 0), {}
    kf = MINUS if minus else 0
    x = y = x_columns = 0

    def column(w):
        return _COMP[norm(Q[q_end - 1 - w])] if minus else norm(Q[q_start + w])

    for l, ch in ops:
        p = t_start + y
        if ch in "XM":
            for b in range(l):
                r, a = norm(T[p + b]), column(x + b)
                sums["compared"] += 1
                x_columns += ch == "X"
                if r == "N" or a == "N":
                    sums["n_columns"] += 1
                elif r == a:
                    sums["same" if ch == "X" else "m_equal"] += 1
                else:
                    sums["snvs"] += 1
                    sums[r + ">" + a] += 1
                    out.append((record, SNP | kf, p + b, r, a, q_end - 1 - (x + b) if minus else q_start + x + b))
        elif ch == "I" and l > 0:
            sums["n_ins"] += 1
            sums["ins_bases"] += l
            ins = "".join(column(x + b) for b in range(l))
            if max_indel and l > max_indel:
                sums["long_indels"] += 1
            elif p > 0:
                out.append((record, INS | kf, p - 1, norm(T[p - 1]), norm(T[p - 1]) + ins, q_end - x - l if minus else q_start + x))
            else:
                right[len(out)] = 0
                out.append((record, INS | kf, 0, norm(T[0]), ins + norm(T[0]), q_end - x - l if minus else q_start + x))
        elif ch == "D" and l > 0:
            sums["n_del"] += 1
            sums["del_bases"] += l
            if p == 0 and l == len(T):
                sums["unanchored"] += 1
            elif max_indel and l > max_indel:
                sums["long_indels"] += 1
            elif p > 0:
                out.append((record, DEL | kf, p - 1, norm_seq(T[p - 1:p + l]), norm(T[p - 1]), q_end - x if minus else q_start + x))
            else:
                right[len(out)] = l
                out.append((record, DEL | kf, 0, norm_seq(T[0:l + 1]), norm(T[l]), q_end - x if minus else q_start + x))
        if ch in "M=XI":
            x += l
        if ch in "M=XDN":
            y += l
    if check:
        check_entry(text, out, right, sums, x_columns, minus, q_start, q_end, t_start, t_end, T, Q, max_indel)
    return out, sums


def consensus(T, lo, variants, right):
    """The variants (ascending, as the model lists them) applied from right to left to T, the normalised target from base lo on (the
    anchor of an entry's first op lies one base in front of t_start, that of a deletion at base 0 at t_end at the latest).  right: {index:
    anchor} of the indels at a contig's first base, which are anchored on the base BEHIND them; None where a later variant touches
    that anchor (two records over one base: applying both is not defined)."""
    seq = T
    for k, anchor in right.items():
        if any(v[2] <= anchor for v in variants[k + 1:]):
            return None
    for _, kf, pos, ref, alt, _ in reversed(variants):
        at = pos - lo
        assert at >= 0 and seq[at:at + len(ref)] == ref, (pos, ref, alt)
        seq = seq[:at] + alt + seq[at + len(ref):]
    return seq


def check_entry(text, variants, right, sums, x_columns, minus, q_start, q_end, t_start, t_end, T, Q, max_indel):
    """The three invariants of the definitions for one usable entry."""
    assert sums["compared"] == sums["snvs"] + sums["same"] + sums["m_equal"] + sums["n_columns"]
    assert sums["snvs"] == sum(sums[s] for s in SUBS)
    _, d = dm.entry_diffs(text, minus, q_start, q_end, t_start, t_end, check=False)
    assert (x_columns, sums["n_ins"], sums["ins_bases"], sums["n_del"], sums["del_bases"]) == (d["snp_bases"], d["n_ins"], d["ins_bases"], d["n_del"], d["del_bases"])
    assert sums["compared"] == d["snp_bases"] + d["m_columns"]
    if max_indel == 0 and sums["n_columns"] == 0 and sums["unanchored"] == 0 and d["n_skip"] == 0:
        want = norm_seq(Q[q_start:q_end])
        lo, hi = max(t_start - 1, 0), min(t_end + 1, len(T))
        got = consensus(norm_seq(T[lo:hi]), lo, variants, right)
        assert got is None or got == norm_seq(T[lo:t_start]) + (revcomp(want) if minus else want) + norm_seq(T[t_end:hi]), (text, minus, got, want)


def variant_records(cols, strand, seq_genome, n_genome, cigars, seqs, kept=None, set_=0, t_genome=None, q_genome=None, max_indel=0, check=True):
    """cigars: {record: text}; seqs: one bytes per sequence (empty: absent).  -> dict: variants (tuples in the order of VARIANT_DTYPE),
    pool (bytes), pairs [(q_genome, t_genome) + SUMS, ascending] and the request's counts."""
    c = {k: np.asarray(cols[k]).astype(np.int64) for k in lm.COLS}
    variants, pool, pairs = [], [], {}
    n = dict.fromkeys(FIELDS, 0)
    at = 0
    for i in sorted(cigars):
        q_start, q_end, t_start, t_end = (int(c[k][i]) for k in ("q_start", "q_end", "t_start", "t_end"))
        state = em.entry_state(cigars[i], q_end - q_start, t_end - t_start)
        n["cigar_bad"] += bool(state & 15)
        if state or not (set_ == 0 or bool(kept[i])):
            continue
        q, t = int(c["q_id"][i]), int(c["t_id"][i])
        key = (int(seq_genome[q]), int(seq_genome[t]))
        assert key[0] < n_genome and key[1] < n_genome
        if t_genome not in (None, ANY, key[1]) or q_genome not in (None, ANY, key[0]):
            continue
        if not (len(seqs[q]) and len(seqs[t])):
            n["no_sequence"] += 1
            continue
        if not (t_end <= len(seqs[t]) and q_end <= len(seqs[q])):
            n["out_of_sequence"] += 1
            continue
        n["usable"] += 1
        got, sums = entry_variants(cigars[i], int(strand[i]) != 0, q_start, q_end, t_start, t_end, seqs[t], seqs[q], record=i, max_indel=max_indel,
                                   check=check)
        acc = pairs.setdefault(key, dict.fromkeys(SUMS, 0))
        acc["entries"] += 1
        for name, v in sums.items():
            acc[name] += v
        for record, kf, pos, ref, alt, q_pos in got:
            variants.append((record, kf, pos, len(ref), len(alt), q_pos, at))
            pool.append(ref + alt)
            at += len(ref) + len(alt)
    plist = [key + tuple(acc[s] for s in SUMS) for key, acc in sorted(pairs.items())]
    n.update(n_variants=len(variants), pool_bytes=at, n_pairs=len(plist), columns=sum(p[3] for p in plist),
             ops=sum(sum(ch not in "0123456789" for ch in (t.decode("latin-1") if isinstance(t, bytes) else t)) for t in cigars.values()))
    return dict(n, variants=variants, pool="".join(pool).encode(), pairs=plist)


def variants_array(variants):
    from sweepga_amd.variants import VARIANT_DTYPE
    out = np.zeros(len(variants), dtype=VARIANT_DTYPE)
    for k, row in enumerate(variants):
        out[k] = row
    return out


def pairs_array(pairs):
    from sweepga_amd.variants import PAIR_DTYPE
    out = np.zeros(len(pairs), dtype=PAIR_DTYPE)
    for k, row in enumerate(pairs):
        out[k] = row
    return out


# ---- the generator -------------------------------------------------------------------------------------------------------------------
IUPAC = b"RYSWKMBDHVN-*"


def random_bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).tobytes())


def plant(rng, seq, lower=0.0, iupac=0.0):
    """seq (bytes) with a share of its bytes in lower case and a share replaced by IUPAC codes, N and foreign bytes"""
    a = np.frombuffer(seq, dtype=np.uint8).copy()
    if iupac:
        hit = rng.random(a.size) < iupac
        a[hit] = rng.choice(np.frombuffer(IUPAC, dtype=np.uint8), size=int(hit.sum()))
    if lower:
        hit = (rng.random(a.size) < lower) & (a >= 65) & (a <= 90)
        a[hit] |= 0x20
    return a.tobytes()


def derive(rng, T, t_start, edits, minus, fuse=False, fake=0.0):
    """The query side of an alignment of T from t_start on.  edits: (length, letter) with letters of "=XID" -- a list of ops, in fact.
    Under X every base differs from the target's (with probability `fake` per base it is EQUAL: an X over equal bases; `fake` may
    be a function of the X column's number within the call instead; a target byte that is no base gets any base).  fuse: runs of = and X become one M.  -> (CIGAR text, the query interval's bytes on the
    forward strand, t_end)"""
    out, ops, p, k = [], [], t_start, 0
    for l, ch in edits:
        if ch == "=":
            out.append(T[p:p + l].upper())
        elif ch == "X":
            for b in T[p:p + l].upper():
                k += 1
                if chr(b) not in "ACGT" or (fake(k - 1) if callable(fake) else rng.random() < fake):
                    out.append(bytes([b]) if chr(b) in "ACGT" else random_bases(rng, 1))
                else:
                    out.append(bytes([b"ACGT"[(b"ACGT".index(b) + int(rng.integers(1, 4))) % 4]]))
        elif ch == "I":
            out.append(random_bases(rng, l))
        if ch in "=XD":
            p += l
        if fuse and ch in "=X":
            if ops and ops[-1][1] == "M":
                ops[-1] = (ops[-1][0] + l, "M")
            else:
                ops.append((l, "M"))
        else:
            ops.append((l, ch))
    walk = b"".join(out)
    if minus:
        walk = bytes(reversed(walk.translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))))
    return "".join("%d%s" % op for op in ops), walk, p


def random_edits(rng, n_ops, max_len=6, letters="=XID"):
    """n_ops ops; no two I or D directly behind one another of the same letter (adjacent ops of one kind are legal but dull)"""
    edits, last = [], ""
    for _ in range(n_ops):
        ch = letters[int(rng.integers(len(letters)))]
        if ch == last and ch in "ID":
            ch = "="
        edits.append((int(rng.integers(1, max_len + 1)), ch))
        last = ch
    return edits


def random_case(rng, n_records, n_targets=2, n_queries=2, n_ops=12, max_len=6, fuse=0.3, fake=0.1, lower=0.2, iupac=0.02, genomes=2, flank=5):
    """Records over n_targets target and n_queries query sequences (the targets first): every record gets its own stretch of its
    target and of its query, queries are built from the pieces.  -> (cols, strand, seq_genome, cigars {record: text}, seqs)"""
    edits = [random_edits(rng, int(rng.integers(1, n_ops + 1)), max_len) for _ in range(n_records)]
    t_of = rng.integers(0, n_targets, n_records)
    q_of = rng.integers(0, n_queries, n_records)
    need = [sum(l for l, ch in e if ch in "=XD") for e in edits]
    t_at, t_len = [], [0] * n_targets
    for i in range(n_records):
        gap = int(rng.integers(0, flank + 1)) if t_len[t_of[i]] or rng.random() < 0.7 else 0     # some records start at base 0
        t_at.append(t_len[t_of[i]] + gap)
        t_len[t_of[i]] = t_at[i] + need[i]
    T = [plant(rng, random_bases(rng, max(t_len[t] + int(rng.integers(0, flank + 1)), 1)), lower, iupac) for t in range(n_targets)]
    Q = [[] for _ in range(n_queries)]
    q_len = [0] * n_queries
    cols = {k: np.zeros(n_records, dtype=np.int64) for k in lm.COLS}
    strand = rng.integers(0, 2, n_records).astype(np.uint8)
    cigars = {}
    for i in range(n_records):
        text, walk, t_end = derive(rng, T[t_of[i]], t_at[i], edits[i], bool(strand[i]), rng.random() < fuse, fake)
        lead = random_bases(rng, int(rng.integers(0, flank + 1)))
        q = int(q_of[i])
        cols["q_id"][i], cols["t_id"][i] = n_targets + q, int(t_of[i])
        cols["q_start"][i], cols["q_end"][i] = q_len[q] + len(lead), q_len[q] + len(lead) + len(walk)
        cols["t_start"][i], cols["t_end"][i] = t_at[i], t_end
        Q[q] += [lead, plant(rng, walk, lower, 0.0)]
        q_len[q] += len(lead) + len(walk)
        cigars[i] = text
    seqs = T + [b"".join(parts) + random_bases(rng, 1 + int(rng.integers(0, flank + 1))) for parts in Q]
    seq_genome = np.array([s % genomes for s in range(n_targets + n_queries)], dtype=np.uint32)
    return {k: v.astype(np.uint32) for k, v in cols.items()}, strand, seq_genome, cigars, seqs


# ---- the texts of swg_paf_vcf_text ---------------------------------------------------------------------------------------------------
VCF_COUNTS = ("records", "usable", "bad", "untagged", "variants", "snvs", "n_ins", "n_del", "same", "n_columns", "m_equal", "long_indels", "unanchored",
              "no_sequence", "out_of_sequence", "length_mismatch", "batches")
SUMMARY_HEADER = ("#query_genome\ttarget_genome\tentries\tcompared\tsnvs\t" + "\t".join(SUBS) +
                  "\tsame\tm_equal\tn_columns\tins\tins_bases\tdel\tdel_bases\tlong_indels\tunanchored\tts\ttv\n")
INFO_LINES = ('##INFO=<ID=QNAME,Number=1,Type=String,Description="Query sequence">\n'
              '##INFO=<ID=QSTART,Number=1,Type=Integer,Description="0-based position on the forward strand of the query">\n'
              '##INFO=<ID=QSTRAND,Number=1,Type=String,Description="Strand of the query in the mapping">\n'
              '##INFO=<ID=REC,Number=1,Type=Integer,Description="Record of the input, from 0">\n')


def escape(name):
    """';', '=', ',', '%' and bytes <= 0x20 percent-encoded"""
    return "".join("%%%02X" % ord(ch) if ord(ch) <= 0x20 or ch in ";=,%" else ch for ch in name)


def vcf_header(contigs, sample=None):
    """contigs: (name, length) in sequence-id order"""
    out = "##fileformat=VCFv4.2\n##source=sweepga-gpu\n" + "".join("##contig=<ID=%s,length=%d>\n" % c for c in contigs) + INFO_LINES
    if sample is not None:
        out += '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
    return out + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO" + ("\tFORMAT\t" + sample if sample is not None else "") + "\n"


def vcf_line(t_name, q_name, pos, ref, alt, q_pos, minus, record, genotype=False):
    return "%s\t%d\t.\t%s\t%s\t.\t.\tQNAME=%s;QSTART=%d;QSTRAND=%s;REC=%d%s\n" % (t_name, pos + 1, ref, alt, escape(q_name), q_pos, "-" if minus else "+", record,
                                                                                  "\tGT\t1" if genotype else "")


def summary_text(genome_name, pairs):
    out = [SUMMARY_HEADER]
    for p in pairs:
        sub = dict(zip(SUBS, p[5:17]))
        ts = sub["A>G"] + sub["G>A"] + sub["C>T"] + sub["T>C"]
        out.append("\t".join([genome_name[p[0]], genome_name[p[1]]] + [str(v) for v in p[2:]] + [str(ts), str(p[4] - ts)]) + "\n")
    return "".join(out)


def paf_texts(paf_text, kept, fasta, set_=1, ref=None, query=None, max_indel=10000):
    """(VCF text, summary text, counts without `batches`) as swg_paf_vcf_text gives them; kept None = no status; fasta: (name, bytes)
    records in file order (of two with one name the first counts); ref / query: a genome name with or without its trailing '#'.  A
    PAF without records of the set gives two empty texts."""
    from tests import ucsc_chain_model as um
    cols, strand, names = lm.parse_paf(paf_text)
    lines = um.paf_lines(paf_text)
    sel = [i for i in range(len(strand)) if set_ == 0 or kept[i]]
    counts = dict.fromkeys(VCF_COUNTS[:-1], 0)
    counts["records"] = len(sel)
    if not sel:
        return "", "", counts
    size = {}
    for ln in lines:
        f = ln.split("\t")
        size[f[0]] = int(f[1])
        size[f[5]] = int(f[6])
    genomes, seq_genome = [], []
    for nm in names:
        g = dm.prefix_two(nm)
        if g not in genomes:
            genomes.append(g)
        seq_genome.append(genomes.index(g))
    have = {}
    for nm, seq in fasta:
        have.setdefault(nm, seq)
    named = {int(cols[c][i]) for i in sel for c in ("q_id", "t_id")}
    seqs = []
    for s, nm in enumerate(names):
        seq = have.get(nm, b"") if s in named else b""
        if s in named and nm in have and len(seq) != size[nm]:
            counts["length_mismatch"] += 1
            seq = b""
        seqs.append(seq)

    def genome_id(name):
        return None if name is None else next(g for g, have_ in enumerate(genomes) if have_ in (name, name + "#"))
    tags = {i: em.last_cigar_tag(lines[i]) for i in sel}
    cig = {i: tags[i] or "" for i in sel}
    got = variant_records(cols, strand, seq_genome, len(genomes), cig, seqs, None, 0, genome_id(ref), genome_id(query), max_indel, check=False)
    # the contigs: the targets of the usable entries -- the model's own rule, entry by entry
    contigs = set()
    for i in sel:
        q, t = int(cols["q_id"][i]), int(cols["t_id"][i])
        rec = tuple(int(cols[c][i]) for c in ("q_start", "q_end", "t_start", "t_end"))
        if em.entry_state(cig[i], rec[1] - rec[0], rec[3] - rec[2]) == 0 and genome_id(ref) in (None, seq_genome[t]) and genome_id(query) in (None, seq_genome[q]) \
                and len(seqs[q]) and len(seqs[t]) and rec[1] <= len(seqs[q]) and rec[3] <= len(seqs[t]):
            contigs.add(t)
    order = sorted(range(len(got["variants"])), key=lambda k: (int(cols["t_id"][got["variants"][k][0]]), got["variants"][k][2], k))
    sample = genomes[genome_id(query)] if query is not None else None
    out = [vcf_header([(names[t], size[names[t]]) for t in sorted(contigs)], sample)]
    for k in order:
        record, kf, pos, ref_len, alt_len, q_pos, at = got["variants"][k]
        alleles = got["pool"][at:at + ref_len + alt_len].decode()
        out.append(vcf_line(names[int(cols["t_id"][record])], names[int(cols["q_id"][record])], pos, alleles[:ref_len], alleles[ref_len:], q_pos, kf & MINUS, record,
                            sample is not None))
    counts.update(usable=got["usable"], bad=got["cigar_bad"], untagged=sum(tags[i] is None for i in sel), variants=got["n_variants"],
                  no_sequence=got["no_sequence"], out_of_sequence=got["out_of_sequence"])
    for p in got["pairs"]:
        for name, v in zip(SUMS, p[2:]):
            if name in counts:
                counts[name] += v
    return "".join(out), summary_text(genomes, got["pairs"]), counts
