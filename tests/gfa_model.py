"""The GFA 1 text of a shrunk graph, restated in plain Python from host arrays (include/katome_gpu.h fixes the format byte for byte):
    H\\tVN:Z:1.0\\n
    S\\t<i>\\t<bases of edge i>\\tLN:i:<bases>\\tKC:i:<weight_i * kmers_i>\\tew:i:<weight_i>\\n    i = 0 .. n_edges - 1
    L\\t<a>\\t+\\t<b>\\t+\\t<k-1>M\\n                                                              every (a, b) with dst[a] == src[b], sorted
What the tests of katome_dev_contigs_gfa / katome_dev_gfa_arrays / katome_gfa_* compare the library's bytes with."""


def compress_edge(seq):
    """compress.rs:250-271: the pad byte, then the bases 2 bits each, first base in the top bits, zero padding"""
    pad = (4 - len(seq) % 4) % 4
    codes = ["ACGT".index(c) for c in seq] + [0] * pad
    return bytes([pad] + [codes[i] << 6 | codes[i + 1] << 4 | codes[i + 2] << 2 | codes[i + 3] for i in range(0, len(codes), 4)])


def decompress_edge(raw):
    """compress.rs:283-293"""
    pad = raw[0]
    bases = "".join("ACGT"[(x >> s) & 3] for x in raw[1:] for s in (6, 4, 2, 0))
    return bases[:len(bases) - pad]


def links(src, dst):
    """every (a, b) with dst[a] == src[b], by a, then b"""
    out_of = {}
    for b, v in enumerate(src):
        out_of.setdefault(int(v), []).append(b)
    return [(a, b) for a, v in enumerate(dst) for b in out_of.get(int(v), [])]


def gfa_text(k, src, dst, weight, kmers, seqs):
    """-> (the file's bytes, segment_off, link_first)"""
    assert len(src) == len(dst) == len(weight) == len(kmers) == len(seqs)
    out, segment_off, at = ["H\tVN:Z:1.0\n"], [], 11
    for i, s in enumerate(seqs):
        assert len(s) == int(kmers[i]) + k - 1
        line = "S\t%d\t%s\tLN:i:%d\tKC:i:%d\tew:i:%d\n" % (i, s, len(s), int(weight[i]) * int(kmers[i]), int(weight[i]))
        segment_off.append(at + 3 + len(str(i)))
        at += len(line)
        out.append(line)
    ab = links(src, dst)
    link_first = [0] * (len(seqs) + 1)
    for a, _ in ab:
        link_first[a + 1] += 1
    for a in range(len(seqs)):
        link_first[a + 1] += link_first[a]
    out += ["L\t%d\t+\t%d\t+\t%dM\n" % (a, b, k - 1) for a, b in ab]
    return "".join(out).encode(), segment_off, link_first


def parse(text):
    """-> (segments: list of (name, sequence, tags), links: list of (a, b, overlap)) of a GFA text this library wrote"""
    lines = text.decode().split("\n")
    assert lines[0] == "H\tVN:Z:1.0" and lines[-1] == ""
    segments, lks = [], []
    for ln in lines[1:-1]:
        f = ln.split("\t")
        if f[0] == "S":
            assert not lks, "segments come before links"
            segments.append((int(f[1]), f[2], dict((t[:2], int(t[5:])) for t in f[3:])))
        else:
            assert f[0] == "L" and f[2] == f[4] == "+" and f[5].endswith("M")
            lks.append((int(f[1]), int(f[3]), int(f[5][:-1])))
    return segments, lks
