"""Unitig coverage restated in plain Python, independent of how shrink walks: from a graph's host arrays the table k-mer -> weight,
and for every merged edge's sequence the sum, smallest and largest weight of its len - k + 1 k-mers, each looked up by its bases.
Also the coverage form of the GFA text (include/katome_gpu.h): gfa_model.gfa_text's output with every S line's tags replaced by
    LN:i:<bases>  KC:i:<kmer_sum>  ew:i:<weight>  mn:i:<kmer_min>  mx:i:<kmer_max>"""
import gfa_model
from helpers import CODE, words_to_int


def kmer_weights(edge_key, key_words, edge_weight):
    """edge_key: [n_edges][key_words] unsigned words (most significant first), edge_weight: [n_edges] -> {k-mer as an integer: weight}"""
    assert len(edge_key) == len(edge_weight)
    table = {}
    for words, w in zip(edge_key, edge_weight):
        words = [int(x) for x in words]
        assert len(words) == key_words
        table[words_to_int(words)] = int(w)
    assert len(table) == len(edge_weight), "a k-mer is the key of two edges"
    return table


def coverage(table, k, seqs):
    """-> [(sum, min, max)] per sequence; every one of its k-mers must be an edge of the graph"""
    mask = (1 << (2 * k)) - 1
    out = []
    for s in seqs:
        assert len(s) >= k
        v, ws = 0, []
        for j, ch in enumerate(s):
            v = ((v << 2) | CODE[ch]) & mask
            if j >= k - 1:
                assert v in table, "k-mer %s of a merged edge is no edge of the graph" % s[j - k + 1:j + 1]
                ws.append(table[v])
        assert len(ws) == len(s) - k + 1
        out.append((sum(ws), min(ws), max(ws)))
    return out


def gfa_coverage_text(k, src, dst, weight, kmers, seqs, kmer_sum, kmer_min, kmer_max):
    """-> (the file's bytes, segment_off, link_first): header, names, bases and L lines are gfa_model.gfa_text's"""
    assert len(kmer_sum) == len(kmer_min) == len(kmer_max) == len(seqs)
    plain, _, link_first = gfa_model.gfa_text(k, src, dst, weight, kmers, seqs)
    lines = plain.decode().split("\n")
    assert lines[-1] == ""
    out, segment_off, at = [], [], 0
    for ln in lines[:-1]:
        f = ln.split("\t")
        if f[0] == "S":
            i = int(f[1])
            assert f[2] == seqs[i] and f[3] == "LN:i:%d" % len(seqs[i]) and f[5] == "ew:i:%d" % int(weight[i]) and len(f) == 6
            f = f[:4] + ["KC:i:%d" % int(kmer_sum[i]), f[5], "mn:i:%d" % int(kmer_min[i]), "mx:i:%d" % int(kmer_max[i])]
            segment_off.append(at + 3 + len(f[1]))
        ln = "\t".join(f) + "\n"
        at += len(ln)
        out.append(ln)
    return "".join(out).encode(), segment_off, link_first
