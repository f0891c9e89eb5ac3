"""The components of include/sweepga_gpu.h, written from the definition with dictionaries and a plain
union-find: links between sequence pairs from the records that take part, `joined` under the two thresholds, connected components
over the joined links numbered by their smallest member, the sums inside and across components, and the report text.  Shares no
code with the library."""
COLUMNS = ("q_id", "t_id", "q_start", "q_end", "t_start", "t_end")
HEADER = "sequence\tlength\tcomponent\tcomponent_sequences\tcomponent_length\tlinks\trecords\tbases\n"


def need(ppm, length):
    """ceil(ppm * length / 10^6)"""
    return -((-ppm * length) // 1_000_000)


def components(cols, status, seq_len, min_bases=0, min_share_ppm=0):
    """-> {"links": [(a, b, n_records, joined, a_bases, b_bases, first_record)] ascending (a, b),
           "components": [(id, first_seq, n_seq, n_links, length, n_records, bases)] ascending id,
           "seq_component": [id per sequence], "cross": (links, records, bases)}"""
    n_seq = len(seq_len)
    q, t = [int(x) for x in cols["q_id"]], [int(x) for x in cols["t_id"]]
    span = [[int(e) - int(s) for s, e in zip(cols[a + "_start"], cols[a + "_end"])] for a in "qt"]
    table = {}
    for i in range(len(q)):
        if (status is not None and int(status[i]) == 0) or q[i] == t[i]:
            continue
        if q[i] >= n_seq or t[i] >= n_seq:
            raise ValueError("a sequence id >= n_seq")
        a, b = min(q[i], t[i]), max(q[i], t[i])
        row = table.setdefault((a, b), [0, 0, 0, i])
        row[0] += span[0][i] if q[i] == a else span[1][i]
        row[1] += span[1][i] if q[i] == a else span[0][i]
        row[2] += 1
    links = []
    parent = list(range(n_seq))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for (a, b), (ab, bb, cnt, first) in sorted(table.items()):
        joined = max(ab, bb) >= min_bases and (ab >= need(min_share_ppm, int(seq_len[a])) or bb >= need(min_share_ppm, int(seq_len[b])))
        links.append((a, b, cnt, int(joined), ab, bb, first))
        if joined:
            ra, rb = find(a), find(b)
            parent[max(ra, rb)] = min(ra, rb)     # the root is the smallest member
    roots = [s for s in range(n_seq) if parent[s] == s]
    number = {r: k + 1 for k, r in enumerate(roots)}          # ascending smallest member
    seq_component = [number[find(s)] for s in range(n_seq)]
    rows = [[number[r], r, 0, 0, 0, 0, 0] for r in roots]
    for s in range(n_seq):
        rows[seq_component[s] - 1][2] += 1
        rows[seq_component[s] - 1][4] += int(seq_len[s])
    cross = [0, 0, 0]
    for a, b, cnt, _, ab, bb, _ in links:
        if seq_component[a] == seq_component[b]:
            row = rows[seq_component[a] - 1]
            row[3] += 1
            row[5] += cnt
            row[6] += ab + bb
        else:
            cross[0] += 1
            cross[1] += cnt
            cross[2] += ab + bb
    return {"links": links, "components": [tuple(r) for r in rows], "seq_component": seq_component, "cross": tuple(cross)}


def last_lengths(text, names):
    """Per name, the length on the record line that mentions it last (a record line has at least 11 columns; column 7 is read
    after column 2)."""
    length = {}
    for ln in text.split("\n"):
        f = ln.rstrip("\r").split("\t")
        if len(f) >= 11:
            length[f[0]] = int(f[1])
            length[f[5]] = int(f[6])
    return [length[x] for x in names]


def report(names, seq_len, res, detailed):
    own = [[0, 0, 0] for _ in names]
    for a, b, cnt, _, ab, bb, _ in res["links"]:
        for s in (a, b):
            own[s][0] += 1
            own[s][1] += cnt
            own[s][2] += ab + bb
    out = [HEADER]
    for s, name in enumerate(names):
        c = res["components"][res["seq_component"][s] - 1]
        out.append("\t".join([name] + [str(x) for x in (int(seq_len[s]), c[0], c[2], c[4], *own[s])]) + "\n")
    if detailed:
        out.append("#links\n")
        for a, b, cnt, joined, ab, bb, _ in res["links"]:
            out.append("\t".join([names[a], names[b], str(cnt), str(ab), str(bb), str(joined)]) + "\n")
    out.append("#cross\t%d\t%d\t%d\n" % res["cross"])
    return "".join(out).encode()


def as_model(r):
    """A sweepga_amd.components.Components in the model's form."""
    return {"links": [tuple(int(l[k]) for k in ("a", "b", "n_records", "joined", "a_bases", "b_bases", "first_record")) for l in r.links],
            "components": [tuple(int(c[k]) for k in ("id", "first_seq", "n_seq", "n_links", "length", "n_records", "bases")) for c in r.components],
            "seq_component": [int(x) for x in r.seq_component], "cross": tuple(int(x) for x in r.cross)}
