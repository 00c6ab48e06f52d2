"""The path region of the assembly's GFA, restated in plain Python from (src, dst, pieces) (include/katome_gpu.h fixes the format):
    P\\tkatome_<c>\\t<s0>+,<s1>+,...,<sn>+\\t*\\n          run 0 of contig c
    P\\tkatome_<c>.<r>\\t<s..>+,...\\t*\\n                  run r = 1, 2, ... of contig c
Piece p names shrunk edge pieces[p] & ~WHOLE; it starts a run iff it has WHOLE (it begins a contig) or dst[id(p - 1)] != src[id(p)]
(a jump: the seam collapser.rs:181-193 leaves after a simple loop).  What the tests of katome_dev_gfa_paths_arrays /
katome_dev_collapse_gfa / katome_assemble_gfa_* compare the library's bytes with."""

WHOLE = 0x80000000


def runs(src, dst, pieces):
    """-> list of (contig, run index inside the contig, first piece, segment ids), in order"""
    out, contig = [], -1
    for p, w in enumerate(pieces):
        w = int(w)
        i = w & ~WHOLE
        assert 0 <= i < len(src), "a piece names no edge"
        if w & WHOLE:
            contig += 1
            out.append((contig, 0, p, [i]))
            continue
        assert p > 0, "the first piece begins a contig"
        before = int(pieces[p - 1]) & ~WHOLE
        if int(dst[before]) != int(src[i]):
            out.append((contig, out[-1][1] + 1, p, [i]))
        else:
            out[-1][3].append(i)
    return out


def path_text(src, dst, pieces):
    """-> (the region's bytes, path_line_off, path_contig, path_first_piece, n_jumps); the offset arrays have one entry more than paths"""
    lines, line_off, contig, first, at = [], [], [], [], 0
    for c, r, p, ids in runs(src, dst, pieces):
        name = "katome_%d" % c if r == 0 else "katome_%d.%d" % (c, r)
        line = "P\t%s\t%s\t*\n" % (name, ",".join("%d+" % i for i in ids))
        line_off.append(at)
        contig.append(c)
        first.append(p)
        at += len(line)
        lines.append(line)
    n_contigs = sum(1 for w in pieces if int(w) & WHOLE)
    return "".join(lines).encode(), line_off + [at], contig, first + [len(pieces)], len(lines) - n_contigs


def parse(text):
    """-> list of (contig, run, segment ids) of a path region this library wrote"""
    out = []
    for ln in text.decode().split("\n")[:-1]:
        f = ln.split("\t")
        assert len(f) == 4 and f[0] == "P" and f[1].startswith("katome_") and f[3] == "*", ln
        c, _, r = f[1][7:].partition(".")
        assert all(s.endswith("+") for s in f[2].split(","))
        out.append((int(c), int(r or 0), [int(s[:-1]) for s in f[2].split(",")]))
    assert text == b"" or text.endswith(b"\n")
    return out
