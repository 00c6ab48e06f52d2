"""tests/depth_model.py pinned on hand-written cases with literal expectations, and the new entries' place in the header and the binding."""
import os

import depth_model as dm
from depth_model import ABSENT as A, INVALID as I, REVERSE as R, U32
from helpers import ROOT, int_to_words, kmer_to_int

EDGES = {"ACGT": (0, 5), "CGTA": (1, 2), "GGGG": (2, 9)}


def test_six_bases_over_three_edges():
    r = dm.depth(EDGES, 4, ["ACGTAC"])
    assert r["window_edge"] == [0, 1, A] and r["seq_window_off"] == [0, 3]
    assert (r["seq_present"], r["seq_invalid"], r["seq_sum"], r["seq_min"], r["seq_max"]) == ([2], [0], [7], [2], [5])
    assert (r["n_windows"], r["n_present"], r["n_invalid"], r["weight_sum"], r["n_edges"], r["n_edges_hit"]) == (3, 2, 0, 7, 3, 2)
    assert r["edge_hits"] == {0: 1, 1: 1}


def test_n_in_the_middle_and_at_either_end():
    assert dm.depth(EDGES, 4, ["ACGTNACGTA"])["window_edge"] == [0, I, I, I, I, 0, 1]
    assert dm.depth(EDGES, 4, ["NACGTA"])["window_edge"] == [I, 0, 1]
    r = dm.depth(EDGES, 4, ["ACGTAN"])
    assert r["window_edge"] == [0, 1, I] and r["seq_invalid"] == [1] and r["n_invalid"] == 1 and r["seq_present"] == [2]


def test_lower_case_is_not_a_base():
    r = dm.depth(EDGES, 4, ["ACGtA"])
    assert r["window_edge"] == [I, I] and r["seq_present"] == [0]


def test_k_minus_one_and_k_bases():
    r = dm.depth(EDGES, 4, ["ACG", "ACGT", ""])
    assert r["seq_window_off"] == [0, 0, 1, 1] and r["window_edge"] == [0]
    assert r["seq_present"] == [0, 1, 0] and r["seq_min"] == [U32, 5, U32] and r["seq_max"] == [0, 5, 0]


def test_palindrome_is_found_forward():
    r = dm.depth({"ACGT": (0, 5)}, 4, ["ACGT"], either_strand=True)      # ACGT is its own reverse complement
    assert r["window_edge"] == [0]


def test_reverse_only_hit_carries_bit_63():
    assert dm.depth(EDGES, 4, ["TACG"])["window_edge"] == [A]
    r = dm.depth(EDGES, 4, ["TACG"], either_strand=True)                   # rc(TACG) = CGTA, edge 1
    assert r["window_edge"] == [1 | R] and r["seq_sum"] == [2] and r["edge_hits"] == {1: 1}
    assert dm.depth(EDGES, 4, ["CGTA"], either_strand=True)["window_edge"] == [1]


def test_zero_weight_edge_is_present():
    r = dm.depth({"AAAA": (0, 0)}, 4, ["AAAAA"])
    assert r["window_edge"] == [0, 0] and (r["seq_present"], r["seq_sum"], r["seq_min"], r["seq_max"]) == ([2], [0], [0], [0])
    assert r["edge_hits"] == {0: 2} and r["n_edges_hit"] == 1


def test_nothing_present():
    r = dm.depth(EDGES, 4, ["TTTTT"])
    assert (r["seq_present"], r["seq_min"], r["seq_max"], r["seq_sum"]) == ([0], [U32], [0], [0])


def test_edge_dict_from_key_rows():
    rows = [int_to_words(kmer_to_int(s), 1) for s in ("ACGT", "GGGG")]
    assert dm.edge_dict(rows, 4, [5, 9]) == {"ACGT": (0, 5), "GGGG": (1, 9)}
    s = "ACGTACGTACGTACGTACGTACGTACGTACGTACGTA"                              # 37 bases: two words
    assert dm.edge_dict([int_to_words(kmer_to_int(s), 2)], 37, [1]) == {s: (0, 1)}


def test_header_and_binding_name_the_entries():
    from katome_amd import _lib
    header = open(os.path.join(ROOT, "include", "katome_gpu.h")).read()
    for name in ("katome_dev_depth", "katome_dev_depth_arrays", "katome_dev_depth_index_bytes"):
        assert name + "(" in header and name in _lib.SYMBOLS
    assert "#define KATOME_DEPTH_REVERSE  0x8000000000000000ull" in header
    assert [f for f, _ in _lib.DevDepth._fields_][:7] == ["n_seqs", "n_windows", "n_present", "n_invalid", "n_edges", "n_edges_hit", "weight_sum"]
    L = _lib.lib()
    names = [L.katome_phase_name(i).decode() for i in range(L.katome_phase_count())]
    assert names[-3:] == ["depth", "k:depth_kernel", "k:depth_index"]
