"""No-GPU checks of the unitig coverage: the Python model (tests/coverage_model.py) on three hand-written graphs, and the library's
entry points (five functions and the struct they share) -- exported, declared in include/katome_gpu.h with the prototypes the issue fixes, bound with as many arguments --
with KATOME_FLAG_PATH_COVERAGE == 8."""
import ctypes as C
import os
import re

import pytest

import coverage_model
import gfa_model
from helpers import ROOT, int_to_words, kmer_to_int


def _graph(k, kmers_with_weights):
    nw = 1 if k <= 32 else 2
    keys = [int_to_words(kmer_to_int(s), nw) for s, _ in kmers_with_weights]
    return coverage_model.kmer_weights(keys, nw, [w for _, w in kmers_with_weights])


def test_model_on_a_line():
    """ACGTTGCA at k = 4: five k-mers in a row; the whole line, and the line shrunk in two pieces"""
    k, seq, ws = 4, "ACGTTGCA", [3, 9, 2, 7, 7]
    table = _graph(k, [(seq[i:i + k], w) for i, w in enumerate(ws)])
    assert coverage_model.coverage(table, k, [seq]) == [(28, 2, 9)]
    assert coverage_model.coverage(table, k, [seq[:5], seq[2:]]) == [(12, 3, 9), (16, 2, 7)]
    with pytest.raises(AssertionError):
        coverage_model.coverage(table, k, ["ACGTA"])               # CGTA is no edge


def test_model_on_a_cycle_and_a_self_loop():
    """a circle of 6 bases at k = 3 spelled once from any start (6 k-mers, each once); AAAA at k = 3 is one k-mer seen twice in the label
    of a self-loop spelling AAA only once"""
    k, circle, ws = 3, "ACGGTC", [5, 1, 4, 2 ** 32 - 1, 6, 2]
    table = _graph(k, [((circle + circle)[i:i + k], w) for i, w in enumerate(ws)])
    for r in range(6):
        rot = circle[r:] + circle[:r]
        assert coverage_model.coverage(table, k, [rot + rot[:k - 1]]) == [(2 ** 32 - 1 + 18, 1, 2 ** 32 - 1)]
    assert coverage_model.coverage(_graph(k, [("AAA", 30)]), k, ["AAA"]) == [(30, 30, 30)]


def test_model_on_a_fork_with_two_word_keys_and_the_text():
    """k = 33 (two key words): a stem that forks; sums past 32 bits; the S lines of the coverage text against a text written by hand"""
    k = 33
    stem = "ACGT" * 8 + "ACCA"              # 36 bases: 4 k-mers
    left, right = stem[-(k - 1):] + "GT", stem[-(k - 1):] + "TTG"
    edges = [(stem[i:i + k], w) for i, w in enumerate([2 ** 32 - 1, 2 ** 32 - 1, 1, 7])]
    edges += [(left[i:i + k], w) for i, w in enumerate([5, 6])] + [(right[i:i + k], w) for i, w in enumerate([9, 8, 10])]
    table = _graph(k, edges)
    seqs = [stem, left, right]
    cov = coverage_model.coverage(table, k, seqs)
    assert cov == [(2 * (2 ** 32 - 1) + 8, 1, 2 ** 32 - 1), (11, 5, 6), (27, 8, 10)]
    src, dst, weight, kmers = [0, 1, 1], [1, 2, 3], [2 ** 32 - 1, 5, 9], [4, 2, 3]
    text, seg, first = coverage_model.gfa_coverage_text(k, src, dst, weight, kmers, seqs, *zip(*cov))
    want = ("H\tVN:Z:1.0\n"
            "S\t0\t%s\tLN:i:36\tKC:i:8589934598\tew:i:4294967295\tmn:i:1\tmx:i:4294967295\n"
            "S\t1\t%s\tLN:i:34\tKC:i:11\tew:i:5\tmn:i:5\tmx:i:6\n"
            "S\t2\t%s\tLN:i:35\tKC:i:27\tew:i:9\tmn:i:8\tmx:i:10\n"
            "L\t0\t+\t1\t+\t32M\nL\t0\t+\t2\t+\t32M\n" % (stem, left, right)).encode()
    assert text == want and first == [0, 2, 2, 2]
    assert [text[o:o + 4].decode() for o in seg] == [s[:4] for s in seqs]
    plain = gfa_model.gfa_text(k, src, dst, weight, kmers, seqs)[0]
    assert plain.count(b"\n") == text.count(b"\n") and b"mn:i:" not in plain


def _header():
    text = open(os.path.join(ROOT, "include", "katome_gpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


PROTOTYPES = {
    "katome_dev_shrink_coverage": "int katome_dev_shrink_coverage(katome_builder *b, uint32_t mode, katome_dev_contigs *out, katome_dev_coverage *cov, "
                                  "double *host_ms, void *stream);",
    "katome_dist_shrink_coverage": "int katome_dist_shrink_coverage(katome_dist_builder *d, katome_dist_contigs *out, katome_dev_coverage *cov, "
                                   "katome_dist_shrink_stats *stats, void *stream);",
    "katome_dev_contigs_gfa_coverage": "int katome_dev_contigs_gfa_coverage(katome_builder *b, const katome_dev_contigs *contigs, katome_dev_gfa *out, void *stream);",
    "katome_dev_gfa_coverage_arrays": "int katome_dev_gfa_coverage_arrays(int device, uint32_t k, uint64_t n_nodes, uint64_t n_edges, const uint64_t *d_edge_src, "
                                      "const uint64_t *d_edge_dst, const uint32_t *d_edge_weight, const uint32_t *d_edge_kmers, const uint64_t *d_kmer_sum, "
                                      "const uint32_t *d_kmer_min, const uint32_t *d_kmer_max, const uint64_t *d_edge_label_off, const uint8_t *d_edge_label, "
                                      "uint64_t label_bytes, uint64_t *d_segment_off, uint64_t *d_link_first, uint8_t *d_text, uint64_t text_cap, "
                                      "uint64_t *n_links, uint64_t *text_bytes, void *stream);",
    "katome_dist_contigs_gfa_coverage": "int katome_dist_contigs_gfa_coverage(katome_dist_builder *d, katome_dist_gfa *out, void *stream);",
}


def test_library_exports_the_coverage_entries_with_the_headers_prototypes():
    from katome_amd import _lib, build
    lib = C.CDLL(_lib.lib_path())
    header = " ".join(_header().split())
    for name, proto in PROTOTYPES.items():
        assert hasattr(lib, name), name
        assert proto in header, name
        n_args = proto[proto.index("(") + 1:].count(",") + 1
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and len(args) == n_args, name
    # the struct they share, field for field
    assert "typedef struct { uint64_t n_edges; uint64_t *d_kmer_sum; uint32_t *d_kmer_min, *d_kmer_max; } katome_dev_coverage;" in header
    assert [f for f, _ in _lib.DevCoverage._fields_] == ["n_edges", "d_kmer_sum", "d_kmer_min", "d_kmer_max"] and C.sizeof(_lib.DevCoverage) == 32
    assert re.search(r"#define KATOME_FLAG_PATH_COVERAGE 8u\b", header) and build.FLAG_PATH_COVERAGE == 8
    assert build.make_settings(31, path_coverage=True).flags == 8 and build.make_settings(31).flags == 0
    assert lib.katome_abi_version() == 2           # only functions were added
