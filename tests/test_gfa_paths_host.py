"""The Python model of the assembly GFA's path region (tests/gfa_paths_model.py) against hand-written strings, and the walk of
collapse_exact.h on a tandem repeat: after a simple loop the next piece does not start where the last one ended, so the contig
is two paths with a seam between them.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gfa_paths_model as model

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WHOLE = model.WHOLE
END = 0xFFFFFFFF


def test_model_reproduces_hand_written_strings():
    # a chain 0 -> 1 -> 2 -> 3 walked as one contig, then edge 1 alone
    src, dst = [0, 1, 2], [1, 2, 3]
    text, off, contig, first, jumps = model.path_text(src, dst, [0 | WHOLE, 1, 2, 1 | WHOLE])
    assert text == b"P\tkatome_0\t0+,1+,2+\t*\nP\tkatome_1\t1+\t*\n"
    assert (off, contig, first, jumps) == ([0, 22, 38], [0, 1], [0, 3, 4], 0)
    # no pieces: an empty region
    assert model.path_text(src, dst, []) == (b"", [0], [], [0], 0)
    # two jumps inside contig 1: runs .1 and .2; two-digit segment names
    src, dst = [0] * 11 + [5], [1] * 11 + [6]
    text, off, contig, first, jumps = model.path_text(src, dst, [11 | WHOLE, 10 | WHOLE, 3, 11])
    assert text == b"P\tkatome_0\t11+\t*\nP\tkatome_1\t10+\t*\nP\tkatome_1.1\t3+\t*\nP\tkatome_1.2\t11+\t*\n"
    assert (off, contig, first, jumps) == ([0, 17, 34, 52, 71], [0, 1, 1, 1], [0, 1, 2, 3, 4], 2)
    assert model.parse(text) == [(0, 0, [11]), (1, 0, [10]), (1, 1, [3]), (1, 2, [11])]
    # a self-loop walked three times is properly linked: one path
    assert model.path_text([4], [4], [0 | WHOLE, 0, 0])[0] == b"P\tkatome_0\t0+,0+,0+\t*\n"
    for bad in ([0], [7 | WHOLE]):
        with pytest.raises(AssertionError):
            model.path_text([0], [1], bad)


@pytest.fixture(scope="module")
def shim():
    """tests/hostshim/collapse_exact_host.cpp, as test_collapse_exact_host.py builds it"""
    src = os.path.join(HERE, "hostshim", "collapse_exact_host.cpp")
    hdrs = [os.path.join(ROOT, "katome_amd", "csrc", h) for h in ("shrink_exact.h", "collapse_exact.h", "contig_stats.h", "multi_route.h", "env.h")]
    so = os.path.join(HERE, "hostshim", "libcollapse_exact_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def collapse_on_host(shim, n_nodes, pairs, weights):
    """-> (pieces, src and dst of the shrunk edges they name, simple loops taken)"""
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    E = len(pairs)
    src, dst = np.array([e[0] for e in pairs], np.uint32), np.array([e[1] for e in pairs], np.uint32)
    w = np.array(weights, np.uint32)
    cap = int(w.sum())
    pieces, o_slot, chain, counts = np.zeros(cap + 1, np.uint32), np.zeros(E + 1, np.uint32), np.zeros(E + 1, np.uint32), np.zeros(16, np.uint64)
    assert shim.hs_collapse_exact(p(src), p(dst), None, p(w), C.c_uint32(E), C.c_uint32(n_nodes), C.c_int(0), p(pieces), C.c_uint64(cap), p(o_slot),
                                  p(chain), p(counts)) == 0
    n_shrunk, n_pieces, simple_loops = int(counts[0]), int(counts[2]), int(counts[9])
    s_src, s_dst = [], []
    for s in o_slot[:n_shrunk].tolist():         # a shrunk edge runs from its first edge's source to the target of the last one on its chain
        s_src.append(pairs[s][0])
        while chain[s] != END:
            s = int(chain[s])
        s_dst.append(pairs[s][1])
    return pieces[:n_pieces].tolist(), s_src, s_dst, simple_loops


def test_tandem_repeat_leaves_a_seam(shim):
    """0 -> 1 (1), 1 -> 2 (2), 2 -> 1 (1), 2 -> 3 (1): the walk enters the loop by 1 -> 2, returns by 2 -> 1 and continues from 2"""
    pieces, src, dst, simple_loops = collapse_on_host(shim, 4, [(0, 1), (1, 2), (2, 1), (2, 3)], [1, 2, 1, 1])
    assert pieces == [0 | WHOLE, 1, 2, 3, 1 | WHOLE] and simple_loops == 1
    assert (src, dst) == ([0, 1, 2, 2], [1, 2, 1, 3])
    assert dst[2] == 1 and src[3] == 2                      # piece 3 does not start where piece 2 ended
    text, off, contig, first, jumps = model.path_text(src, dst, pieces)
    assert text == b"P\tkatome_0\t0+,1+,2+\t*\nP\tkatome_0.1\t3+\t*\nP\tkatome_1\t1+\t*\n"
    assert [(c, r, len(ids)) for c, r, ids in model.parse(text)] == [(0, 0, 3), (0, 1, 1), (1, 0, 1)]
    assert (jumps, contig, first) == (1, [0, 0, 1], [0, 3, 4, 5])
