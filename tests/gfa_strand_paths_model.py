"""The path region of the assembly's BIDIRECTED GFA and the paths' mirrors, restated in plain Python from (src, dst, twin, pieces)
(include/katome_gpu.h fixes the format):
    P\\tkatome_<c>\\t<r0><o0>,<r1><o1>,...,<rn><on>\\t*\\n     run 0 of contig c
    P\\tkatome_<c>.<r>\\t...\\t*\\n                             run r = 1, 2, ... of contig c
A piece with shrunk edge i reads <rep i><o i> as gfa_strands_model defines them: rep = min(i, twin i), or i without a twin
(NO_TWIN); '-' only where twin(i) < i.  The runs are gfa_paths_model.runs', decided on the two-strand arrays.  What the tests of
katome_dev_gfa_strand_paths_arrays / katome_dev_collapse_gfa_strands / katome_assemble_gfa_strands_* compare the library with."""
import gfa_model
import gfa_paths_model
from gfa_strands_model import NO_TWIN, canonical_link

WHOLE = gfa_paths_model.WHOLE
NO_MIRROR = -1


def _twin(twin, i):
    """twin[i] as an edge index or NO_TWIN, whether the array spells none as -1 or as 2^64 - 1"""
    t = int(twin[i])
    return NO_TWIN if t < 0 or t >= 2 ** 63 else t


def oriented(i, twin):
    """-> (rep, '+' or '-')"""
    t = _twin(twin, i)
    return (t, "-") if t != NO_TWIN and t < i else (i, "+")


def path_text(src, dst, twin, pieces):
    """-> (the region's bytes, path_line_off, path_contig, path_first_piece, n_jumps); the offset arrays have one entry more than paths"""
    lines, line_off, contig, first, at = [], [], [], [], 0
    for c, r, p, ids in gfa_paths_model.runs(src, dst, pieces):
        name = "katome_%d" % c if r == 0 else "katome_%d.%d" % (c, r)
        line = "P\t%s\t%s\t*\n" % (name, ",".join("%d%s" % oriented(i, twin) for i in ids))
        line_off.append(at)
        contig.append(c)
        first.append(p)
        at += len(line)
        lines.append(line)
    n_contigs = sum(1 for w in pieces if int(w) & WHOLE)
    return "".join(lines).encode(), line_off + [at], contig, first + [len(pieces)], len(lines) - n_contigs


def mirrors(src, dst, twin, pieces):
    """the definition, quadratic and obvious: mirror[j] = the smallest q with as many pieces as j and id_q[t] == twin(id_j[n - 1 - t])
    for every t (an edge without a twin matches nothing), or NO_MIRROR"""
    return mirrors_of_paths([ids for _, _, _, ids in gfa_paths_model.runs(src, dst, pieces)], twin)


def mirrors_of_paths(paths, twin):
    """the same from every path's edge ids"""
    out = []
    for ids in paths:
        want = [_twin(twin, i) for i in reversed(ids)]
        out.append(next((q for q, other in enumerate(paths) if NO_TWIN not in want and other == want), NO_MIRROR))
    return out


def parse(text):
    """-> list of (contig, run, [(rep, o)]) of a merged path region this library wrote"""
    out = []
    for ln in text.decode().split("\n")[:-1]:
        f = ln.split("\t")
        assert len(f) == 4 and f[0] == "P" and f[1].startswith("katome_") and f[3] == "*", ln
        c, _, r = f[1][7:].partition(".")
        assert all(s[-1] in "+-" for s in f[2].split(","))
        out.append((int(c), int(r or 0), [(int(s[:-1]), s[-1]) for s in f[2].split(",")]))
    assert text == b"" or text.endswith(b"\n")
    return out


def expand(text, twin):
    """a merged path region back as the two-strand one: <r>+ is edge r, <r>- its twin -> bytes"""
    lines = []
    for c, r, steps in parse(text):
        ids = []
        for rep, o in steps:
            i = rep if o == "+" else _twin(twin, rep)
            assert i != NO_TWIN and (o == "+" or i > rep), "a '-' names a representative with a larger twin"
            ids.append(i)
        lines.append("P\t%s\t%s\t*\n" % ("katome_%d" % c if r == 0 else "katome_%d.%d" % (c, r), ",".join("%d+" % i for i in ids)))
    return "".join(lines).encode()


def pair_spellings(x, ox, y, oy, twin):
    """the two spellings of the step (x ox),(y oy) as L lines: as written, and its conjugate (flip leaves a self-twin at +)"""
    flip = lambda r, o: "+" if _twin(twin, r) == r else "-+"[o == "-"]
    return (x, ox, y, oy), (y, flip(y, oy), x, flip(x, ox))


def symmetric_graph(rng, n_edges, drop=0.1):
    """a random graph with a strand involution, for the tests: vertex v's other strand is v ^ 1, the twin of an edge (u, v) is
    (v ^ 1, u ^ 1) -- an edge (u, u ^ 1) is its own --, `drop` of the twins are left out (unpaired edges), and the edges are shuffled
    so that a twin lies below its edge as often as above -> (src, dst, twin)"""
    n_nodes = max(2, n_edges // 2) // 2 * 2
    pairs, tw = [(0, 1), (1, 0), (0, 0)], [0, 1, NO_TWIN]     # (two self-twins and an unpaired edge are always there)
    while len(pairs) < n_edges:
        u, v = int(rng.integers(n_nodes)), int(rng.integers(n_nodes))
        e = len(pairs)
        pairs.append((u, v))
        if v == u ^ 1:
            tw.append(e)
        elif rng.random() < drop:
            tw.append(NO_TWIN)
        else:
            pairs.append((v ^ 1, u ^ 1))
            tw += [e + 1, e]
    perm = rng.permutation(len(pairs)).tolist()                 # old index e -> new index perm[e]
    src, dst, twin = [0] * len(pairs), [0] * len(pairs), [0] * len(pairs)
    for e, (u, v) in enumerate(pairs):
        src[perm[e]], dst[perm[e]], twin[perm[e]] = u, v, NO_TWIN if tw[e] == NO_TWIN else perm[tw[e]]
    return src, dst, twin


def random_walks(rng, src, dst, twin, steps, mirrored=0.3):
    """pieces of random walks that mostly follow the edges (short and long runs, jumps, many contigs); now and then a finished contig
    is walked again from its other end on the other strand, where every edge of it has a twin -> pieces"""
    n = len(src)
    out_of = {}
    for e, v in enumerate(src):
        out_of.setdefault(v, []).append(e)
    contigs = [[int(rng.integers(n))]]
    for _ in range(steps):
        last = contigs[-1]
        nxt = out_of.get(dst[last[-1]], [])
        if rng.random() < 0.05:
            back = [_twin(twin, i) for i in reversed(last)]
            if NO_TWIN not in back and rng.random() < mirrored:
                contigs.append(back)
            contigs.append([int(rng.integers(n))])
        elif nxt and rng.random() < 0.95:
            last.append(int(rng.choice(nxt)))
        else:
            last.append(int(rng.integers(n)))
    return [i | (WHOLE if t == 0 else 0) for c in contigs for t, i in enumerate(c)]


def merged_links(src, dst, twin):
    """the L lines of the merged text as a set of (x, ox, y, oy)"""
    tw = [_twin(twin, i) for i in range(len(src))]
    return {(x, "+-"[ox], y, "+-"[oy]) for x, ox, y, oy in (canonical_link(a, b, tw) for a, b in gfa_model.links(src, dst))}
