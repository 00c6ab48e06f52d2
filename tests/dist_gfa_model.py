"""The numbered form of the GFA 1 text, restated in plain Python: one PART of a text whose other parts are written elsewhere
(katome_dev_gfa_part_arrays, katome_dist_contigs_gfa; include/katome_gpu.h fixes the layout).  Segment i of a part is named
first + i, its links are (first + i, b) for the global numbers b the caller lists for it, and the header line is there or not.
gfa_model.gfa_text is the form with first = 0, the header and the links of one graph; tests/test_dist_gfa_host.py holds the two
against each other."""
import gfa_model

HEADER = b"H\tVN:Z:1.0\n"
TILE = 8192                      # output bytes a workgroup of the writer owns at a time (gfa.hip)


def part_text(k, weight, kmers, seqs, first, with_header, link_first, link_b):
    """-> (S part: the header if asked for, then the segments' lines; L part; segment_off relative to the S part)"""
    assert len(weight) == len(kmers) == len(seqs) == len(link_first) - 1 and link_first[0] == 0 and link_first[-1] == len(link_b)
    s_part, segment_off = [HEADER.decode()] if with_header else [], []
    at = len(HEADER) if with_header else 0
    for i, s in enumerate(seqs):
        assert len(s) == int(kmers[i]) + k - 1
        line = "S\t%d\t%s\tLN:i:%d\tKC:i:%d\tew:i:%d\n" % (first + i, s, len(s), int(weight[i]) * int(kmers[i]), int(weight[i]))
        segment_off.append(at + 3 + len(str(first + i)))
        at += len(line)
        s_part.append(line)
    l_part = ["L\t%d\t+\t%d\t+\t%dM\n" % (first + a, int(b), k - 1) for a in range(len(seqs)) for b in link_b[link_first[a]:link_first[a + 1]]]
    return "".join(s_part).encode(), "".join(l_part).encode(), segment_off


def link_table(src, dst, first=0):
    """the links of one graph as a part's table: (link_first, link_b) with b numbered from `first`"""
    ab = gfa_model.links(src, dst)
    link_first = [0] * (len(src) + 1)
    for a, _ in ab:
        link_first[a + 1] += 1
    for a in range(len(src)):
        link_first[a + 1] += link_first[a]
    return link_first, [first + b for _, b in ab]


def whole_text(k, parts):
    """the ranks' parts, in rank order, as the whole text: parts = [(weight, kmers, seqs, link_first, link_b)], link_b global"""
    first, s_all, l_all = 0, [], []
    for r, (weight, kmers, seqs, link_first, link_b) in enumerate(parts):
        s, l, _ = part_text(k, weight, kmers, seqs, first, r == 0, link_first, link_b)
        s_all.append(s)
        l_all.append(l)
        first += len(seqs)
    return b"".join(s_all) + b"".join(l_all)


def padded(part):
    """a part as it lies in the device buffer: zeros up to the next multiple of 16"""
    return part + b"\0" * (-len(part) % 16)


def lines_across_tiles(part, width_of_numbers):
    """the lines of a part that lie across a multiple of TILE and hold a number of `width_of_numbers` digits"""
    out, at = [], 0
    for line in part.split(b"\n")[:-1]:
        end = at + len(line) + 1
        if at // TILE != (end - 1) // TILE and any(len(f) == width_of_numbers and f.isdigit() for f in line.split(b"\t")):
            out.append(line)
        at = end
    return out


# ---- the directory by new node id (katome_amd/csrc/dist_gfa_dir.h) ------------------------------------------------------------
def directory(total, world):
    """-> (per, [(base, range) per rank]): vertex v of [0, total) lives on rank v // per, per = ceil(total / world), at least 1"""
    per = max(1, -(-total // world))
    ranges = []
    for r in range(world):
        base = min(total, r * per)
        ranges.append((base, min(total, base + per) - base))
    return per, ranges
