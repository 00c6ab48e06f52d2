"""The strand-unique assembly's definitions (tests/unique_model.py) on hand-written cases, and the keep rule on the oracle's contigs of
the three fixtures built on both strands.  No GPU: the model is what tests/test_gpu_unique.py compares the library with."""
import json
import os

import pytest

import unique_model as model

NO = model.NO_TWIN
# edges 0 .. 9 and their twins 10 .. 19, two self-twins 20 and 21, two edges without a twin 22 and 23
TWIN = [10 + i for i in range(10)] + list(range(10)) + [20, 21] + [NO, NO]
A, A_ = [0, 1, 2], [12, 11, 10]


def both(*contigs):
    m = model.mirrors([list(c) for c in contigs], TWIN)
    return m, model.kept(m)


def test_pair_orders():
    assert both(A, A_) == ([1, 0], [0])
    assert both(A_, A) == ([1, 0], [0])


def test_copies_keep_one_strand_with_all_its_copies():
    assert both(A, A_, A, A_) == ([1, 0, 1, 0], [0, 2])
    assert both(A, A, A_) == ([2, 2, 0], [0, 1])
    assert both(A_, A, A) == ([1, 0, 0], [0])
    # mirror(j) >= j, the per-path rule, keeps an irregular subset of the copies
    from katome_amd.device import unique_paths
    assert unique_paths([1, 0, 1, 0]) == [0] and unique_paths([2, 2, 0]) == [0, 1] and unique_paths([1, 0, 0]) == [0]


def test_self_mirrors_and_self_twins():
    assert both([3, 13]) == ([0], [0])                                     # [a, twin a]
    assert both([20]) == ([0], [0]) and both([3, 21, 13]) == ([0], [0])    # a self-twin piece
    assert both([3, 13], [3, 13]) == ([0, 0], [0, 1])                      # copies of a self-mirror are all kept
    assert both([20, 4], [14, 20]) == ([1, 0], [0])


def test_edges_without_a_twin_have_no_mirror():
    assert both([22]) == ([-1], [0])
    assert both([0, 22], [22, 10]) == ([-1, -1], [0, 1])
    assert both([0, 22], [0, 22]) == ([-1, -1], [0, 1])


def test_near_mirrors_and_permutations():
    assert both(A, [12, 14, 10]) == ([-1, -1], [0, 1])                     # differs in one piece
    assert both(A, [12, 11]) == ([-1, -1], [0, 1]) and both([0, 1], [10, 11]) == ([-1, -1], [0, 1])      # another length; the same pieces in another order
    assert both(A, [10, 12, 11], A_) == ([2, -1, 0], [0, 1])


def test_all_kept_without_twins():
    contigs = [A, A_, A, [5]]
    m = model.mirrors(contigs, [NO] * 24)
    assert m == [-1] * 4 and model.kept(m) == [0, 1, 2, 3]
    assert model.mirrors([], TWIN) == [] and model.kept([]) == []


def test_text_filter():
    full = b">katome_0\nACG\n>katome_1\nCGT\n>katome_2\nT\n"
    assert model.unique_text(full, [0, 2], "fasta") == b">katome_0\nACG\n>katome_2\nT\n"
    assert model.unique_text(b"ACGCGTT", [0, 2], "plain", [3, 3, 1]) == b"ACGT"
    assert model.unique_text(full, [], "fasta") == b"" and model.unique_text(b"", [], "fasta") == b""
    assert model.contigs_of(model.pieces_of([A, [5], A_])) == [A, [5], A_]


def test_string_rule_agrees_with_the_piece_rule():
    """where every contig is one piece, the rule on strings and the rule on pieces are one rule"""
    seq = ["AAC", "GTT", "ACGT", "AAC", "GGG", "GTT", "ACGT"]
    twin = [1, 0, 2, NO]                                                   # AAC <-> GTT, ACGT its own, GGG alone (CCC is not there)
    ids = {"AAC": 0, "GTT": 1, "ACGT": 2, "GGG": 3}
    m = model.mirrors([[ids[s]] for s in seq], twin)
    assert (model.kept(m), m) == model.kept_by_strings(seq) == ([0, 2, 3, 4, 6], [1, 0, 2, 1, -1, 0, 2])


@pytest.mark.parametrize("i", [0, 1, 2])
def test_fixtures_on_both_strands(oracle, golden_dir, i):
    """the oracle's collapse of a reverse_complement build: every contig is mirrored, half of them are kept (2 of 4, 91 of 182, 233 of
    466) -- derived here from the strings: reverse complement, first occurrence"""
    with open(os.path.join(golden_dir, "pinned.json")) as f:
        pinned = json.load(f)
    path, k = os.path.join(golden_dir, pinned["fixtures"][i]), pinned["k"]
    strings = oracle.build_files([path], k, True, stages="C").collapsed
    keep, mirror = model.kept_by_strings(strings)
    assert (len(keep), len(strings)) == [(2, 4), (91, 182), (233, 466)][i]
    assert len(keep) < len(strings) and all(m != -1 for m in mirror)       # something is dropped: no vacuous pass
    # one strand per molecule: no kept string is the reverse complement of another kept string that is not itself, and every
    # dropped string's reverse complement is kept
    kept_set = {strings[c] for c in keep}
    assert all(model.revcomp(s) not in kept_set or model.revcomp(s) == s for s in kept_set)
    assert all(model.revcomp(strings[c]) in kept_set for c in range(len(strings)) if c not in keep)
    # ... with all its copies
    assert all((strings[c] in kept_set) == (c in keep) for c in range(len(strings)))
    one_strand = oracle.build_files([path], k, False, stages="C").collapsed
    assert len(model.kept_by_strings(one_strand)[0]) == len(one_strand) == [2, 92, 233][i]
