"""The Python model of the bidirected GFA (tests/gfa_strands_model.py) against texts written out by hand, and expand() -- the way
back to the two-strand text -- against gfa_model.gfa_text on symmetric graphs; and the bit work of gfa_strands.hip (strand_bits.h: the
end k-mers, the comparison a word at a time, the canonical link) through a host build.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gfa_model
import gfa_strands_model as sm

H = "H\tVN:Z:1.0\n"


def _text(k, src, dst, weight, seqs):
    return sm.strands_text(k, src, dst, weight, [len(s) - k + 1 for s in seqs], seqs)


def test_a_pair():
    assert sm.revcomp("ACGG") == "CCGT"
    text, names, seg, first, twin = _text(3, [0, 2], [1, 3], [5, 7], ["ACGG", "CCGT"])
    assert text.decode() == H + "S\t0\tACGG\tLN:i:4\tKC:i:10\tew:i:5\trc:i:1\trw:i:7\n"
    assert (names, seg, first, twin) == ([0], [11 + 4], [0, 0], [1, 0])


def test_a_self_twin_with_a_link_into_it():
    # edge 0 = ACGT is its own reverse complement (k = 4); TTACG runs into it, and it runs into CGTAA = revcomp(TTACG)
    text, names, seg, first, twin = _text(4, [1, 0, 2], [2, 1, 3], [9, 2, 3], ["ACGT", "TTACG", "CGTAA"])
    assert twin == [0, 2, 1] and names == [0, 1]
    # (1, 0) spells 1 + 0 +, its conjugate 0 + 1 - (the self-twin stays at +); (0, 2) spells 0 + 1 - itself: one line
    assert text.decode() == (H + "S\t0\tACGT\tLN:i:4\tKC:i:9\tew:i:9\trc:i:0\trw:i:9\n" + "S\t1\tTTACG\tLN:i:5\tKC:i:4\tew:i:2\trc:i:2\trw:i:3\n" +
                             "L\t0\t+\t1\t-\t3M\n")
    assert first == [0, 1, 1]


def test_a_hairpin():
    # GGAT ends in AT, its own reverse complement, so it links to its twin ATCC: x + x -, whose two spellings coincide
    text, names, _, first, twin = _text(3, [0, 1], [1, 2], [4, 6], ["GGAT", "ATCC"])
    assert twin == [1, 0] and names == [0] and first == [0, 1]
    assert text.decode() == H + "S\t0\tGGAT\tLN:i:4\tKC:i:8\tew:i:4\trc:i:1\trw:i:6\n" + "L\t0\t+\t0\t-\t2M\n"


def test_a_near_twin_stays_two_segments():
    # GAAACGT has the end k-mers and the length of revcomp(ACGATTC) = GAATCGT, and another base in the middle
    assert sm.revcomp("ACGATTC") == "GAATCGT"
    text, names, _, first, twin = _text(3, [0, 2], [1, 3], [1, 1], ["ACGATTC", "GAAACGT"])
    assert twin == [sm.NO_TWIN, sm.NO_TWIN] and names == [0, 1] and first == [0, 0, 0]
    assert text.decode() == H + "S\t0\tACGATTC\tLN:i:7\tKC:i:5\tew:i:1\n" + "S\t1\tGAAACGT\tLN:i:7\tKC:i:5\tew:i:1\n"


def test_a_link_without_its_mirror_is_still_written():
    # A -> B on one strand only (B' does not run into A'), and D' -> C' on the other strand only
    a, b, c, d = "ACCA", "CATT", "GGCA", "TTGA"
    seqs = [a, b, sm.revcomp(a), sm.revcomp(b), c, d, sm.revcomp(d), sm.revcomp(c)]
    src, dst = [0, 1, 4, 5, 7, 9, 11, 12], [1, 2, 3, 6, 8, 10, 12, 13]
    text, names, _, first, twin = _text(3, src, dst, [1] * 8, seqs)
    assert twin == [2, 3, 0, 1, 7, 6, 5, 4] and names == [0, 1, 4, 5]
    assert text.decode().split("\n")[5:] == ["L\t0\t+\t1\t+\t2M", "L\t4\t+\t5\t+\t2M", ""]
    assert first == [0, 1, 1, 2, 2]


def _symmetric(rng, k, n_pairs, n_vertex_pairs, self_twins=0):
    """a graph closed under reverse complement: vertex v mirrors v + n_vertex_pairs, edge (s, d) comes with (mirror d, mirror s)"""
    mirror = lambda v: (v + n_vertex_pairs) % (2 * n_vertex_pairs)
    seqs, src, dst, used = [], [], [], set()

    def fresh(n):
        while True:
            s = "".join(rng.choice(list("ACGT"), n))
            heads = {s[:k], sm.revcomp(s[-k:])}
            if len(heads) == 2 and not heads & used:
                used.update(heads)
                return s
    for _ in range(n_pairs):
        s, a, b = fresh(int(rng.integers(k, k + 12))), int(rng.integers(0, 2 * n_vertex_pairs)), int(rng.integers(0, 2 * n_vertex_pairs))
        seqs += [s, sm.revcomp(s)]; src += [a, mirror(b)]; dst += [b, mirror(a)]
    for _ in range(self_twins):
        while True:
            h = "".join(rng.choice(list("ACGT"), k))
            if h not in used and h != sm.revcomp(h):
                break
        used.add(h)
        a = int(rng.integers(0, 2 * n_vertex_pairs))
        seqs.append(h + sm.revcomp(h)); src.append(a); dst.append(mirror(a))
    p = [int(x) for x in rng.permutation(len(seqs))]
    return 2 * n_vertex_pairs, [src[i] for i in p], [dst[i] for i in p], [int(x) for x in rng.integers(1, 1000, len(p))], [seqs[i] for i in p]


@pytest.mark.parametrize("k,self_twins", [(3, 0), (4, 2), (5, 0), (11, 0), (12, 3)])
def test_expand_gives_the_two_strand_text_back(k, self_twins):
    rng = np.random.default_rng(100 + k)
    for _ in range(20):
        n_nodes, src, dst, weight, seqs = _symmetric(rng, k, 8, 3, self_twins)
        kmers = [len(s) - k + 1 for s in seqs]
        text, names, _, first, twin = sm.strands_text(k, src, dst, weight, kmers, seqs)
        assert all(t != sm.NO_TWIN for t in twin) and sum(t == i for i, t in enumerate(twin)) == self_twins
        two_strand = gfa_model.gfa_text(k, src, dst, weight, kmers, seqs)[0]
        assert sm.expand(text, k) == two_strand
        # a link and its mirror are one line, a link that is its own mirror stays one: 2 * lines - self-conjugate = links
        lks = sm.parse(text)[1]
        own = sum(1 for x, ox, y, oy, _ in lks if (x, ox, y, oy) == _conjugate(x, ox, y, oy, twin))
        assert 2 * len(lks) - own == two_strand.count(b"\nL\t") and first[-1] == len(lks)


def _conjugate(x, ox, y, oy, twin):
    flip = lambda r, o: "+" if twin[r] == r else "-+"[o == "-"]
    return (y, flip(y, oy), x, flip(x, ox))


# ---- strand_bits.h, built for the host (tests/hostshim/strand_bits_host.cpp) ---------------------------------------------------
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "hostshim", "strand_bits_host.cpp")
    hdrs = [os.path.join(os.path.dirname(HERE), "katome_amd", "csrc", h) for h in ("strand_bits.h", "kmer_bits.h")]
    so = os.path.join(HERE, "hostshim", "libstrand_bits_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.hs_strand_first_kmer.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.hs_strand_last_kmer_revcomp.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.hs_strand_first_difference.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.hs_strand_first_difference.restype = C.c_int64
    lib.hs_strand_canonical_link.argtypes = [C.c_uint32] * 4 + [C.POINTER(C.c_uint64)]
    return lib


def _kmer(s):
    return sum("ACGT".index(c) << (2 * (len(s) - 1 - i)) for i, c in enumerate(s))


@pytest.mark.parametrize("k", [3, 4, 11, 16, 17, 31, 32, 33, 48, 63])
def test_end_kmers_at_every_pad_and_alignment(shim, k):
    rng = np.random.default_rng(k)
    out = (C.c_uint64 * 2)()
    for n in list(range(k, k + 9)) + [k + 40, 200]:
        s = "".join(rng.choice(list("ACGT"), n))
        packed = gfa_model.compress_edge(s)[1:]
        for shift in range(4):
            shim.hs_strand_first_kmer(packed, len(packed), shift, k, out)
            assert (out[0] << 64 | out[1]) == _kmer(s[:k])
            shim.hs_strand_last_kmer_revcomp(packed, len(packed), shift, n, k, out)
            assert (out[0] << 64 | out[1]) == _kmer(sm.revcomp(s[-k:]))


def test_the_comparison_finds_the_word_of_every_single_difference(shim):
    rng = np.random.default_rng(9)
    for n in [3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 100]:
        s = "".join(rng.choice(list("ACGT"), n))
        t = sm.revcomp(s)
        ps, pt = gfa_model.compress_edge(s)[1:], gfa_model.compress_edge(t)[1:]
        for si in range(4):
            for sj in range(4):
                assert shim.hs_strand_first_difference(ps, pt, len(ps), si, sj, n) == -1
        for at in range(n):                           # base `at` of s faces base n - 1 - at of t
            bad = list(t)
            bad[n - 1 - at] = "ACGT"[("ACGT".index(bad[n - 1 - at]) + 1 + at % 3) % 4]
            pb = gfa_model.compress_edge("".join(bad))[1:]
            assert shim.hs_strand_first_difference(ps, pb, len(ps), at % 4, (at + n) % 4, n) == at // 16 * 16


def test_the_canonical_link_is_the_models(shim):
    rng = np.random.default_rng(3)
    none, out = 0xFFFFFFFF, (C.c_uint64 * 2)()
    for _ in range(200):
        n = 12
        twin = [sm.NO_TWIN] * n
        p = [int(x) for x in rng.permutation(n)]
        for a, b in zip(p[0:8:2], p[1:8:2]):
            twin[a], twin[b] = b, a
        twin[p[8]] = p[8]                              # a self-twin; p[9:] stay without a twin
        for a in range(n):
            for b in range(n):
                x, ox, y, oy = sm.canonical_link(a, b, twin)
                shim.hs_strand_canonical_link(a, b, twin[a] if twin[a] != sm.NO_TWIN else none, twin[b] if twin[b] != sm.NO_TWIN else none, out)
                assert (out[0], out[1]) == (2 * x + ox, 2 * y + oy)
