"""The strand-unique assembly restated in plain Python (include/katome_gpu.h, katome_dev_collapse_unique, has the definitions):
    contig c      the pieces from the c-th piece with WHOLE up to the next such piece; its ids a_0 .. a_{n-1}
    mirror(c)     the smallest q with n_q == n and id_q[t] == twin(a_{n-1-t}) for every t; an edge without a twin: no mirror
    kept          c is kept iff mirror(c) is none or mirror(mirror(c)) <= mirror(c)
    text          the kept records of the full text, in order, under their original numbers
What the tests of katome_dev_unique_contigs_arrays / katome_dev_collapse_unique compare the library with."""
WHOLE = 0x80000000
NO_TWIN = 0xFFFFFFFF
NO_MIRROR = -1


def _twin(twin, i):
    """twin[i] as an edge index or NO_TWIN, whether the array spells none as -1, as 2^32 - 1 or as 2^64 - 1"""
    t = int(twin[i])
    return NO_TWIN if t < 0 or t == NO_TWIN or t >= 2 ** 63 else t


def contigs_of(pieces):
    """-> every contig's ids"""
    out = []
    for w in pieces:
        w = int(w) & 0xFFFFFFFF
        if w & WHOLE:
            out.append([])
        out[-1].append(w & ~WHOLE)
    return out


def pieces_of(contigs):
    return [i | (WHOLE if t == 0 else 0) for c in contigs for t, i in enumerate(c)]


def mirrors(contigs, twin):
    """quadratic, by the definition -> list, NO_MIRROR for none"""
    out = []
    for ids in contigs:
        want = [_twin(twin, i) for i in reversed(ids)]
        out.append(next((q for q, other in enumerate(contigs) if NO_TWIN not in want and list(other) == want), NO_MIRROR))
    return out


def kept(mirror):
    """-> the kept contigs, ascending"""
    return [c for c, m in enumerate(mirror) if m == NO_MIRROR or mirror[m] <= m]


def records(full, layout, lengths=None):
    """the full text cut into its records -> list of bytes.  "fasta": by its own lines, each checked to be ">katome_<c>\\n<bases>\\n";
    "plain": by `lengths`, every contig's bases"""
    if layout == "fasta":
        lines = full.split(b"\n")
        assert lines[-1] == b"" and len(lines) % 2 == 1
        out = []
        for c in range(len(lines) // 2):
            assert lines[2 * c] == b">katome_%d" % c and set(lines[2 * c + 1]) <= set(b"ACGT")
            out.append(lines[2 * c] + b"\n" + lines[2 * c + 1] + b"\n")
        return out
    assert lengths is not None and sum(lengths) == len(full)
    out, at = [], 0
    for n in lengths:
        out.append(full[at:at + n])
        at += n
    return out


def unique_text(full, kept_list, layout, lengths=None):
    """the full text's records, filtered"""
    rec = records(full, layout, lengths)
    return b"".join(rec[c] for c in kept_list)


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def kept_by_strings(strings):
    """the keep rule on contig STRINGS (a collapse without seams): contig c's mirror is the first contig that reads revcomp(c), its
    first copy the first contig that reads as c does -> (kept, mirror)"""
    first = {}
    for c, s in enumerate(strings):
        first.setdefault(s, c)
    mirror = [first.get(revcomp(s), NO_MIRROR) for s in strings]
    return [c for c, m in enumerate(mirror) if m == NO_MIRROR or first[strings[c]] <= m], mirror
