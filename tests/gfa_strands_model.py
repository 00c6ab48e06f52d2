"""The bidirected GFA 1 text of a shrunk graph (strand twins merged into one segment, +/- links), restated in plain Python from host
arrays; include/katome_gpu.h fixes the format byte for byte:
    H\\tVN:Z:1.0\\n
    S\\t<r>\\t<bases of r>\\tLN:i:<bases>\\tKC:i:<w_r * kmers_r>\\tew:i:<w_r>[\\trc:i:<j>\\trw:i:<w_j>]\\n     one per representative r
    L\\t<x>\\t<ox>\\t<y>\\t<oy>\\t<k-1>M\\n                                                                     canonical, distinct, sorted
What the tests of katome_dev_contigs_gfa_strands / katome_dev_gfa_strands_arrays / katome_gfa_strands_* compare the library's bytes
with, and expand(): the way back from a merged text to the two-strand text of gfa_model.gfa_text."""
import gfa_model

COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
NO_TWIN = -1


def revcomp(s):
    return "".join(COMPLEMENT[c] for c in reversed(s))


def twins(k, seqs):
    """twin[i] = the j with seqs[j] == revcomp(seqs[i]), found through j's first k-mer, or NO_TWIN"""
    by_first = {}
    for i, s in enumerate(seqs):
        assert s[:k] not in by_first, "segments %d and %d start with the same k-mer" % (by_first[s[:k]], i)
        by_first[s[:k]] = i
    out = []
    for s in seqs:
        j = by_first.get(revcomp(s[-k:]), NO_TWIN)
        out.append(j if j != NO_TWIN and seqs[j] == revcomp(s) else NO_TWIN)
    return out


def canonical_link(a, b, twin):
    """(a, b) -> the smaller of its two spellings (x, ox, y, oy), orientations as 0 = '+' and 1 = '-'"""
    rep = lambda i: i if twin[i] == NO_TWIN else min(i, twin[i])
    o = lambda i: 1 if twin[i] != NO_TWIN and twin[i] < i else 0
    flip = lambda i: 0 if twin[i] == i else 1 - o(i)           # (a self-twin stays at +)
    return min((rep(a), o(a), rep(b), o(b)), (rep(b), flip(b), rep(a), flip(a)))


def strands_text(k, src, dst, weight, kmers, seqs):
    """-> (the file's bytes, names, segment_off, link_first, twin)"""
    assert len(src) == len(dst) == len(weight) == len(kmers) == len(seqs)
    twin = twins(k, seqs)
    out, names, segment_off, at = ["H\tVN:Z:1.0\n"], [], [], 11
    for i, s in enumerate(seqs):
        assert len(s) == int(kmers[i]) + k - 1
        if twin[i] != NO_TWIN and twin[i] < i:
            continue
        line = "S\t%d\t%s\tLN:i:%d\tKC:i:%d\tew:i:%d" % (i, s, len(s), int(weight[i]) * int(kmers[i]), int(weight[i]))
        if twin[i] != NO_TWIN:
            line += "\trc:i:%d\trw:i:%d" % (twin[i], int(weight[twin[i]]))
        line += "\n"
        names.append(i)
        segment_off.append(at + 3 + len(str(i)))
        at += len(line)
        out.append(line)
    lks = sorted({canonical_link(a, b, twin) for a, b in gfa_model.links(src, dst)})
    count = {}
    for x, _, _, _ in lks:
        count[x] = count.get(x, 0) + 1
    link_first = [0]
    for r in names:
        link_first.append(link_first[-1] + count.get(r, 0))
    out += ["L\t%d\t%s\t%d\t%s\t%dM\n" % (x, "+-"[ox], y, "+-"[oy], k - 1) for x, ox, y, oy in lks]
    return "".join(out).encode(), names, segment_off, link_first, twin


def parse(text):
    """-> (segments: list of (name, sequence, tags), links: list of (x, ox, y, oy, overlap)) of a merged text"""
    lines = text.decode().split("\n")
    assert lines[0] == "H\tVN:Z:1.0" and lines[-1] == ""
    segments, lks = [], []
    for ln in lines[1:-1]:
        f = ln.split("\t")
        if f[0] == "S":
            assert not lks, "segments come before links"
            segments.append((int(f[1]), f[2], dict((t[:2], int(t[5:])) for t in f[3:])))
        else:
            assert f[0] == "L" and f[2] in "+-" and f[4] in "+-" and f[5].endswith("M")
            lks.append((int(f[1]), f[2], int(f[3]), f[4], int(f[5][:-1])))
    return segments, lks


def expand(text, k=None):
    """a merged text back as the two-strand text: a representative and its rc / rw twin become two segments, an L line the (a, b)
    pairs of its two spellings (one where they coincide, or where the other strand of an end was never there) -> bytes.  k is read
    off the links' overlaps where there are any; without links and without k a segment's k-mers are KC / ew"""
    segments, lks = parse(text)
    if lks:
        assert k in (None, lks[0][4] + 1)
        k = lks[0][4] + 1
    seq, weight, n_kmers, minus, self_twin = {}, {}, {}, {}, set()
    for name, s, tags in segments:
        assert tags["LN"] == len(s)
        seq[name], weight[name] = s, tags["ew"]
        n_kmers[name] = len(s) - k + 1 if k else tags["KC"] // tags["ew"]
        assert tags["KC"] == tags["ew"] * n_kmers[name]
        if "rc" not in tags:
            continue
        j = tags["rc"]
        if j == name:
            self_twin.add(name)
            assert revcomp(s) == s and tags["rw"] == tags["ew"]
        else:
            assert j > name
            seq[j], weight[j], n_kmers[j], minus[name] = revcomp(s), tags["rw"], n_kmers[name], j
    strand = lambda r, o: r if o == "+" else minus.get(r)
    flip = lambda r, o: "+" if r in self_twin else "-+"[o == "-"]
    pairs = set()
    for x, ox, y, oy, _ in lks:
        for a, b in ((strand(x, ox), strand(y, oy)), (strand(y, flip(y, oy)), strand(x, flip(x, ox)))):
            if a is not None and b is not None:
                pairs.add((a, b))
    assert sorted(seq) == list(range(len(seq))), "every merged edge is a segment or a segment's rc"
    out = ["H\tVN:Z:1.0\n"]
    out += ["S\t%d\t%s\tLN:i:%d\tKC:i:%d\tew:i:%d\n" % (i, seq[i], len(seq[i]), weight[i] * n_kmers[i], weight[i]) for i in range(len(seq))]
    out += ["L\t%d\t+\t%d\t+\t%dM\n" % (a, b, k - 1) for a, b in sorted(pairs)]
    return "".join(out).encode()
