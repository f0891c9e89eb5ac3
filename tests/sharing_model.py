"""Sharing restated independently of sweepga_amd/csrc/swg_sharing.hip: cover(s, g) is the union, over both axes, of the
inter-genome records between sequence s and genome g; depth(s, x) is the number of genomes g whose cover holds x.  Two
formulations, neither the device's (no sort key of segment and start, no running maximum, no +1 / -1 events of merged intervals,
no prefix sum of deltas):

  per base   a boolean array per (sequence, genome), summed over the genomes; runs from np.diff, spectrum from np.bincount.  Small
             coordinates only.
  sweep      per sequence one walk over the positions where a record begins or ends, with one counter per genome: depth is the
             number of counters above 0.

sharing() gives the runs (RUN_DTYPE rows ordered by (seq, start)) and the spectrum ([G, G]) of one set; joint_runs() the
(n_all, n_kept) stretches of the BED; table_text() / bed_text() the two texts of swg_paf_sharing."""
import numpy as np

RUN_DTYPE = np.dtype([("seq", "<u4"), ("start", "<u4"), ("end", "<u4"), ("depth", "<u4")])
FIELDS = ("seq", "start", "end", "depth")
COLS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")
PER_BASE_LIMIT = 5_000   # bases per sequence up to which the per-base form is the default


def pieces(cols, seq_genome, mask=None):
    """{seq: [(start, end, genome of the other side)]} of the counted records of non-zero length, both axes."""
    g = np.asarray(seq_genome).astype(np.int64)
    q, t = np.asarray(cols["q_id"]).astype(np.int64), np.asarray(cols["t_id"]).astype(np.int64)
    use = g[q] != g[t]
    if mask is not None:
        use &= np.asarray(mask).astype(bool)
    out = {}
    for seq, other, s, e in ((q, g[t], cols["q_start"], cols["q_end"]), (t, g[q], cols["t_start"], cols["t_end"])):
        s, e = np.asarray(s).astype(np.int64), np.asarray(e).astype(np.int64)
        for k in np.flatnonzero(use & (e > s)):
            out.setdefault(int(seq[k]), []).append((int(s[k]), int(e[k]), int(other[k])))
    return out


def depth_per_base(ivs, length):
    row = {g: k for k, g in enumerate(sorted({g for _, _, g in ivs}))}   # (a row per genome that occurs)
    cover = np.zeros((len(row), length), dtype=bool)
    for s, e, g in ivs:
        cover[row[g], s:e] = True
    return cover.sum(axis=0)


def stretches(depth):
    """[(start, end, value)] of the maximal stretches of one value in a per-base array."""
    if len(depth) == 0:
        return []
    cut = np.flatnonzero(np.diff(depth)) + 1
    begins, ends = np.concatenate([[0], cut]), np.concatenate([cut, [len(depth)]])
    return [(int(a), int(b), depth[a]) for a, b in zip(begins, ends)]


def depth_by_sweep(ivs):
    """[(start, end, depth)] with depth >= 1, maximal: one counter per genome, looked at behind every position's changes."""
    changes = {}
    for s, e, g in ivs:
        changes.setdefault(s, []).append((g, 1))
        changes.setdefault(e, []).append((g, -1))
    count, depth, out, begun, held = {}, 0, [], None, 0
    for pos in sorted(changes):
        for g, d in changes[pos]:
            was = count.get(g, 0) > 0
            count[g] = count.get(g, 0) + d
            depth += (count[g] > 0) - was
        if depth != held:
            if held:
                out.append((begun, pos, held))
            begun, held = pos, depth
    assert held == 0 and not any(count.values())
    return out


def sharing(cols, seq_genome, seq_len=None, mask=None, n_genome=None, per_base=None, spectrum=True):
    """(runs, spectrum) of the set `mask` selects (None: every record); spectrum=False: (runs, None)."""
    seq_genome = np.asarray(seq_genome).astype(np.int64)
    G = int(n_genome) if n_genome is not None else int(seq_genome.max()) + 1
    by_seq = pieces(cols, seq_genome, mask)
    rows, want_spectrum = [], spectrum
    spectrum = np.zeros((G, G) if want_spectrum else (1, 1), dtype=np.uint64)
    for seq in sorted(by_seq):
        ivs = by_seq[seq]
        top = max(e for _, e, _ in ivs)
        small = top <= PER_BASE_LIMIT if per_base is None else per_base
        if small:
            depth = depth_per_base(ivs, top)
            found = [(a, b, int(d)) for a, b, d in stretches(depth) if d > 0]
            if want_spectrum:
                spectrum[seq_genome[seq], :] += np.bincount(depth, minlength=G).astype(np.uint64) * (np.arange(G) > 0)
        else:
            found = depth_by_sweep(ivs)
            for a, b, d in found if want_spectrum else ():
                spectrum[seq_genome[seq], d] += np.uint64(b - a)
        rows += [(seq, a, b, d) for a, b, d in found]
    if not want_spectrum:
        spectrum = None
    elif seq_len is not None:
        seq_len = np.asarray(seq_len).astype(np.uint64)
        for g in range(G):
            spectrum[g, 0] = seq_len[seq_genome == g].sum() - spectrum[g, 1:].sum()
    out = np.zeros(len(rows), dtype=RUN_DTYPE)
    for k, r in enumerate(rows):
        out[k] = r
    return out, spectrum


def joint_runs(cols, seq_genome, kept, n_genome=None):
    """[(seq, start, end, n_all, n_kept)]: the maximal stretches of constant (n_all, n_kept) with n_all >= 1, by (seq, start) --
    swept with two rows of per-genome counters, not merged from the two run lists."""
    seq_genome = np.asarray(seq_genome).astype(np.int64)
    G = int(n_genome) if n_genome is not None else int(seq_genome.max()) + 1
    every, held = pieces(cols, seq_genome), pieces(cols, seq_genome, kept)
    out = []
    for seq in sorted(every):
        changes = {}
        for which, ivs in ((0, every[seq]), (1, held.get(seq, []))):
            for s, e, g in ivs:
                changes.setdefault(s, []).append((which, g, 1))
                changes.setdefault(e, []).append((which, g, -1))
        count = [{}, {}]
        now, state, begun = [0, 0], (0, 0), None
        for pos in sorted(changes):
            for which, g, d in changes[pos]:
                was = count[which].get(g, 0) > 0
                count[which][g] = count[which].get(g, 0) + d
                now[which] += (count[which][g] > 0) - was
            if tuple(now) != state:
                if state[0]:
                    out.append((seq, begun, pos, state[0], state[1]))
                begun, state = pos, tuple(now)
        assert state == (0, 0)
    return out


def as_tuples(rows):
    return [tuple(int(r[f]) for f in FIELDS) for r in rows]


def same_rows(got, want):
    return len(got) == len(want) and all(np.array_equal(np.asarray(got[f]).astype(np.uint64), np.asarray(want[f]).astype(np.uint64)) for f in FIELDS)


def table_text(genome_names, spectrum_all, spectrum_kept, detailed=False):
    G = len(genome_names)
    lines = ["genome\tlength\tprivate_all\tshared_all\tcore_all\tprivate_kept\tshared_kept\tcore_kept\n"]
    if G == 0:
        return lines[0].encode()
    total = [0] * 7
    for g in range(G):
        row = [int(spectrum_all[g].sum())]
        for sp in (spectrum_all, spectrum_kept):
            core = int(sp[g, G - 1]) if G > 1 else 0
            row += [int(sp[g, 0]), int(sp[g].sum()) - int(sp[g, 0]) - core, core]
        total = [a + b for a, b in zip(total, row)]
        lines.append(genome_names[g] + "\t" + "\t".join(map(str, row)) + "\n")
    lines.append("#total\t" + "\t".join(map(str, total)) + "\n")
    if detailed:
        lines.append("#spectrum\n")
        for g in range(G):
            for name, sp in (("all", spectrum_all), ("kept", spectrum_kept)):
                lines += ["%s\t%s\t%d\t%d\n" % (genome_names[g], name, d, int(sp[g, d])) for d in range(G) if sp[g, d]]
    return "".join(lines).encode("utf-8", errors="surrogateescape")


def bed_text(seq_names, joint):
    return "".join("%s\t%d\t%d\t%d\t%d\n" % (seq_names[s], a, b, na, nk) for s, a, b, na, nk in joint).encode("utf-8", errors="surrogateescape")


def last_lengths(text):
    """{name: length} under the last-seen rule: the last line that names a sequence has the last word, its target column after its
    query column."""
    out = {}
    for ln in text.split("\n"):
        f = ln.rstrip("\r").split("\t")
        if len(f) < 11:
            continue
        out[f[0]] = int(f[1])
        out[f[5]] = int(f[6])
    return out


def paf_texts(text, kept, detailed=False):
    """(table, bed) of a PAF text under its last-'#' genome map; kept: a boolean mask over its records."""
    from tests.intervals_model import parse_paf
    cols, seq_genome, names, genomes = parse_paf(text)
    if len(cols["q_id"]) == 0:
        return table_text([], None, None), b""
    lengths = last_lengths(text)
    seq_len = np.array([lengths[nm] for nm in names], dtype=np.uint64)
    G = len(genomes)
    _, sp_all = sharing(cols, seq_genome, seq_len, None, G)
    _, sp_kept = sharing(cols, seq_genome, seq_len, kept, G)
    return table_text(genomes, sp_all, sp_kept, detailed), bed_text(names, joint_runs(cols, seq_genome, kept, G))
