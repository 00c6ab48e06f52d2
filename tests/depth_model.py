"""katome_dev_depth restated on strings (include/katome_gpu.h has the rules): a dict from k-mer string to (edge index, weight), and
every window of every query walked exactly by those rules."""
from helpers import int_to_kmer, revcomp_str, words_to_int

ABSENT, INVALID, REVERSE = 2 ** 64 - 1, 2 ** 64 - 2, 1 << 63
U32 = 2 ** 32 - 1


def edge_dict(key_rows, k, weights):
    """a graph's key rows (lists of unsigned words, most significant first) and weights -> {k-mer: (index, weight)}"""
    d = {}
    for e, (row, w) in enumerate(zip(key_rows, weights)):
        d.setdefault(int_to_kmer(words_to_int(row), k), (e, int(w)))
    return d


def depth(edges, k, queries, either_strand=False):
    """queries: strings (ASCII rules: only upper-case ACGT are bases).  -> dict with window_edge (all windows, query after query),
    seq_present / seq_invalid / seq_sum / seq_min / seq_max / seq_window_off, the totals and edge_hits {index: count}"""
    window_edge, present, invalid, sums, mins, maxs, off, hits = [], [], [], [], [], [], [0], {}
    for q in queries:
        p = i = s = 0
        mn, mx = U32, 0
        for w in range(max(0, len(q) - k + 1)):
            km = q[w:w + k]
            if any(ch not in "ACGT" for ch in km):
                window_edge.append(INVALID)
                i += 1
                continue
            found, rev = edges.get(km), 0
            if found is None and either_strand:
                found, rev = edges.get(revcomp_str(km)), REVERSE
            if found is None:
                window_edge.append(ABSENT)
                continue
            e, wt = found
            window_edge.append(e | rev)
            hits[e] = hits.get(e, 0) + 1
            p, s, mn, mx = p + 1, s + wt, min(mn, wt), max(mx, wt)
        present.append(p); invalid.append(i); sums.append(s); mins.append(mn); maxs.append(mx)
        off.append(len(window_edge))
    return dict(window_edge=window_edge, seq_present=present, seq_invalid=invalid, seq_sum=sums, seq_min=mins, seq_max=maxs, seq_window_off=off,
                n_seqs=len(queries), n_windows=len(window_edge), n_present=sum(present), n_invalid=sum(invalid), weight_sum=sum(sums),
                n_edges=len(edges), n_edges_hit=len(hits), edge_hits=hits)
