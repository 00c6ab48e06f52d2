"""The Python model of the bidirected assembly GFA's path region and of the paths' mirrors (tests/gfa_strand_paths_model.py) against
hand-written strings, against the two-strand model through expand(), against the merged text's L lines, and the mirror definition
on the cases that decide it.  No GPU."""
import numpy as np
import pytest

import gfa_paths_model
import gfa_strand_paths_model as model

WHOLE, NO = model.WHOLE, model.NO_TWIN


def test_model_reproduces_hand_written_strings():
    # a chain 0 -> 1 -> 2 -> 3 and its other strand 3' -> 2' -> 1' -> 0': edges 0, 1, 2 forward, 3 = twin 2, 4 = twin 1, 5 = twin 0
    src, dst = [0, 1, 2, 13, 12, 11], [1, 2, 3, 12, 11, 10]
    twin = [5, 4, 3, 2, 1, 0]
    pieces = [0 | WHOLE, 1, 2, 3 | WHOLE, 4, 5, 1 | WHOLE]
    text, off, contig, first, jumps = model.path_text(src, dst, twin, pieces)
    assert text == b"P\tkatome_0\t0+,1+,2+\t*\nP\tkatome_1\t2-,1-,0-\t*\nP\tkatome_2\t1+\t*\n"
    assert (off, contig, first, jumps) == ([0, 22, 44, 60], [0, 1, 2], [0, 3, 6, 7], 0)
    assert model.parse(text) == [(0, 0, [(0, "+"), (1, "+"), (2, "+")]), (1, 0, [(2, "-"), (1, "-"), (0, "-")]), (2, 0, [(1, "+")])]
    assert model.expand(text, twin) == gfa_paths_model.path_text(src, dst, pieces)[0]
    assert model.mirrors(src, dst, twin, pieces) == [1, 0, model.NO_MIRROR]
    # no pieces: an empty region
    assert model.path_text(src, dst, twin, []) == (b"", [0], [], [0], 0)
    # a self-twin and an unpaired edge are +; rep's digits, not the id's, make the name: edge 12's twin is 3
    src, dst = [0] * 13, [1] * 13
    twin = [NO] * 13
    twin[3], twin[12], twin[7] = 12, 3, 7
    text, off, contig, first, jumps = model.path_text(src, dst, twin, [12 | WHOLE, 7 | WHOLE, 11, 3])
    assert text == b"P\tkatome_0\t3-\t*\nP\tkatome_1\t7+\t*\nP\tkatome_1.1\t11+\t*\nP\tkatome_1.2\t3+\t*\n"
    assert (off, contig, first, jumps) == ([0, 16, 32, 51, 69], [0, 1, 1, 1], [0, 1, 2, 3, 4], 2)
    # twin as the library hands it back: 2^64 - 1 for none
    assert model.path_text(src, dst, [2 ** 64 - 1 if t == NO else t for t in twin], [12 | WHOLE, 11 | WHOLE])[0] == b"P\tkatome_0\t3-\t*\nP\tkatome_1\t11+\t*\n"
    for bad in ([0], [13 | WHOLE]):
        with pytest.raises(AssertionError):
            model.path_text(src, dst, twin, bad)


@pytest.mark.parametrize("seed", range(6))
def test_random_symmetric_graphs(seed):
    """expand() of the merged region is the two-strand region; the run structure is the two-strand one; every step inside a line is an
    L line of the merged text in one of its two spellings"""
    rng = np.random.default_rng(seed)
    src, dst, twin = model.symmetric_graph(rng, int(rng.integers(20, 400)))
    assert all(t == NO or twin[t] == i for i, t in enumerate(twin)) and NO in twin and any(t == i for i, t in enumerate(twin)) and any(NO != t < i for i, t in enumerate(twin))
    pieces = model.random_walks(rng, src, dst, twin, 3000)
    text, off, contig, first, jumps = model.path_text(src, dst, twin, pieces)
    two = gfa_paths_model.path_text(src, dst, pieces)
    assert model.expand(text, twin) == two[0] and (contig, first, jumps) == two[2:] and jumps > 0
    assert b"-" in text and len(off) == len(contig) + 1 and off[-1] == len(text)
    links = model.merged_links(src, dst, twin)
    steps = 0
    for _, _, line in model.parse(text):
        for (x, ox), (y, oy) in zip(line, line[1:]):
            assert any(s in links for s in model.pair_spellings(x, ox, y, oy, twin)), (x, ox, y, oy)
            steps += 1
    assert steps > 1000
    mirror = model.mirrors(src, dst, twin, pieces)
    paths = [ids for _, _, _, ids in gfa_paths_model.runs(src, dst, pieces)]
    assert sum(q != model.NO_MIRROR for q in mirror) > 10
    for j, q in enumerate(mirror):                             # mirror is an involution up to duplicates: the mirror of my mirror spells me
        if q != model.NO_MIRROR:
            assert paths[mirror[q]] == paths[j] and mirror[q] <= j


def test_the_mirror_definition():
    # edges 0 .. 7 on one strand, 8 + i = twin(i); edge 16 is its own twin, edge 17 has none.  Everything follows everything (one vertex)
    n = 18
    src, dst = [0] * n, [0] * n
    twin = [8 + i for i in range(8)] + list(range(8)) + [16, NO]
    m = lambda *contigs: model.mirrors(src, dst, twin, [i | (WHOLE if t == 0 else 0) for c in contigs for t, i in enumerate(c)])
    assert m([0, 1, 2], [10, 9, 8]) == [1, 0]                                  # a pair
    assert m([3, 11]) == [0] and m([16]) == [0] and m([3, 16, 11]) == [0]      # self-mirrors: [a, twin a], a self-twin, both
    assert m([0, 1], [0, 1], [9, 8], [0, 1]) == [2, 2, 0, 2]                   # duplicates: the smallest index wins on both sides
    assert m([0, 1, 2], [10, 12, 8]) == [-1, -1]                               # a near-mirror that differs only in its middle piece
    assert m([0, 1, 2], [10, 9]) == [-1, -1] and m([0, 1], [8, 9]) == [-1, -1] # another length; the twins in the same order
    assert m([0, 17], [17, 8]) == [-1, -1] and m([17]) == [-1]                 # an edge without a twin matches nothing
    assert m() == []


NEW = ["katome_dev_gfa_strand_paths_arrays", "katome_dev_collapse_gfa_strands", "katome_assemble_gfa_strands_files", "katome_assemble_gfa_strands_packed",
       "katome_gfa_strand_paths_save", "katome_gfa_strand_paths_free"]


def test_entries_are_bound_and_exported():
    """the C entries, their ctypes prototypes, the profile names and the keyword arguments are there; the ABI version stays 2"""
    import ctypes as C
    import inspect
    import katome_amd
    from katome_amd import _lib, build, device
    raw = C.CDLL(_lib.lib_path())
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(raw, name), name
    L = katome_amd.lib()
    assert L.katome_abi_version() == 2
    names = [L.katome_phase_name(i).decode() for i in range(L.katome_phase_count())]
    assert names.index("gfa_paths") < names.index("gfa_strand_paths") < names.index("k:gfa_strand_paths_write_kernel")
    for f in (device.Builder.collapse_gfa, build.GpuGraph.assemble_gfa, build.GpuGraph.assemble_gfa_from_packed):
        assert inspect.signature(f).parameters["merge_strands"].default is False
    assert device.unique_paths([2, -1, 0, 3, 1]) == [0, 1, 3]
    # a null argument is refused before any device is asked for
    assert L.katome_dev_gfa_strand_paths_arrays(1 << 20, 0, None, None, None, None, 0, None, None, None, None, 0, None, 0, None, None) == -7
