"""katome_amd/csrc/collapse_exact.h (the sequential half of `collapse`: the walk of collapser.rs:25-273 over petgraph's index
semantics, after ShrinkExact) against the oracle's literal restatement on hand-made graphs: the contigs string for string and in
order -- rebuilt here from the pieces the walk emits, the shrink's chains and random K-base labels --, what is left of the graph,
and the piece count, which is the sum of the shrunk edges' weights.  No GPU."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
END = 0xFFFFFFFF
WHOLE = 0x80000000
K = 6
COUNTS = ("shrunk_edges", "shrunk_nodes", "pieces", "contigs", "nodes_left", "edges_left", "steps", "ambiguity_cuts", "self_loops",
          "simple_loops", "scc_restarts", "nodes_removed", "ambiguity_moves", "weight_sum")


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "hostshim", "collapse_exact_host.cpp")
    hdrs = [os.path.join(ROOT, "katome_amd", "csrc", h) for h in ("shrink_exact.h", "collapse_exact.h", "contig_stats.h", "multi_route.h", "env.h")]
    so = os.path.join(HERE, "hostshim", "libcollapse_exact_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    return C.CDLL(so)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def run_host(shim, n_nodes, pairs, weights, literal=False):
    """-> (pieces, slot of every identity, chain_next, counts by name)"""
    E = len(pairs)
    src = np.array([e[0] for e in pairs], np.uint32)
    dst = np.array([e[1] for e in pairs], np.uint32)
    w = np.array(weights, np.uint32)
    cap = int(w.astype(np.uint64).sum())           # an upper bound of the shrunk weights' sum: every shrunk edge keeps one original weight
    pieces, o_slot, chain = np.zeros(cap + 1, np.uint32), np.zeros(E + 1, np.uint32), np.zeros(E + 1, np.uint32)
    counts = np.zeros(16, np.uint64)
    rc = shim.hs_collapse_exact(_p(src), _p(dst), None, _p(w), C.c_uint32(E), C.c_uint32(n_nodes), C.c_int(int(literal)), _p(pieces),
                                C.c_uint64(cap), _p(o_slot), _p(chain), _p(counts))
    assert rc == 0
    c = dict(zip(COUNTS, (int(x) for x in counts)))
    return pieces[:c["pieces"]].tolist(), o_slot[:c["shrunk_edges"]].tolist(), chain[:E].tolist(), c


def contigs_of(pieces, o_slot, chain, labels, k):
    """EdgeSlice::merge along the chains (the first edge's k bases, then one base per further edge), then name() + remainder()s"""
    seqs = []
    for s in o_slot:
        seq, c = labels[s], chain[s]
        while c != END:
            seq += labels[c][k - 1:]
            c = chain[c]
        seqs.append(seq)
    out = []
    for p in pieces:
        if p & WHOLE:
            out.append(seqs[p & ~WHOLE])
        else:
            out[-1] += seqs[p][k - 1:]
    return out


def check(shim, oracle, n_nodes, pairs, rng, weights=None, max_weight=4):
    labels = ["".join(rng.choice(list("ACGT"), K)) for _ in pairs]
    if weights is None:
        weights = [int(rng.integers(1, max_weight + 1)) for _ in pairs]
    edges = [(s, d, weights[e], e + 1) for e, (s, d) in enumerate(pairs)]
    want = oracle.run_from_edges(n_nodes, edges, "C", k=K, slot_ascii=[None] + labels)
    pieces, o_slot, chain, c = run_host(shim, n_nodes, pairs, weights)
    assert contigs_of(pieces, o_slot, chain, labels, K) == want.collapsed
    assert (c["nodes_left"], c["edges_left"]) == (want.n_nodes, want.n_edges) == (0, 0)
    assert c["pieces"] == c["weight_sum"] == sum(weights[s] for s in o_slot)
    assert c["contigs"] == len(want.collapsed) and c["steps"] + c["simple_loops"] == c["pieces"]
    lit = run_host(shim, n_nodes, pairs, weights, literal=True)        # the externals by a scan of all nodes: the same walk
    assert lit[0] == pieces and lit[3] == c
    return c


def test_in_file_cases(shim, golden_dir):
    """collapser.rs:333-467, k = 40: the strings and their order"""
    with open(os.path.join(golden_dir, "collapser_kat.json")) as f:
        kat = json.load(f)
    name, second, k = kat["name"], kat["second"], kat["k"]
    slots = [None, name[:k], name[1:k + 1], name[2:k + 2], name[3:k + 3], second[:k]]
    assert len(kat["cases"]) == 9
    for case in kat["cases"]:
        pairs = [(e[0], e[1]) for e in case["edges"]]
        labels = [slots[e[3]] for e in case["edges"]]
        pieces, o_slot, chain, c = run_host(shim, case["n_nodes"], pairs, [e[2] for e in case["edges"]])
        assert contigs_of(pieces, o_slot, chain, labels, k) == case["contigs"], case["name"]
        assert (c["nodes_left"], c["edges_left"]) == (0, 0) and c["pieces"] == c["weight_sum"]


SHAPES = [
    (4, [(0, 1), (1, 2), (2, 3)]),
    (6, [(0, 1), (1, 2), (2, 3), (2, 4), (4, 5)]),
    (6, [(0, 2), (1, 2), (2, 3), (3, 4), (4, 5)]),
    (5, [(0, 1), (1, 2), (2, 3), (3, 1), (3, 4)]),
    (4, [(0, 1), (1, 2), (2, 3), (3, 0)]),
    (3, [(0, 0), (0, 1), (1, 2)]),
    (4, [(0, 1), (1, 0), (1, 2), (2, 3)]),
    (5, [(2, 3), (3, 4), (4, 2), (0, 1)]),
    (7, [(1, 2), (2, 3), (3, 1), (4, 5), (5, 6), (6, 4)]),
    (3, [(0, 1), (0, 1), (1, 2)]),
]


def test_reference_in_file_shapes(shim, oracle):
    """the ten topologies test_shrink_exact_host.py takes from shrinker.rs:237-488, weights 1..4"""
    rng = np.random.default_rng(1)
    for n, pairs in SHAPES:
        for _ in range(4):
            check(shim, oracle, n, pairs, rng)


def tangle(seed):
    """the generator of test_shrink_exact_host.py::test_random_tangles, plus, on every other seed, the one shape it never makes: a simple
    loop (x -> s -> t -> y with t -> s back; taken when the edge back weighs less than s -> t) on nodes of its own, entered from a
    vertex without incoming edges or from the tangle"""
    rng = np.random.default_rng(100 + seed)
    n_nodes = int(rng.integers(2, 60))
    pairs = []
    for _ in range(int(rng.integers(1, 8))):                              # chains
        path = rng.choice(n_nodes, int(rng.integers(2, min(n_nodes, 12) + 1)), replace=False).tolist()
        pairs += list(zip(path[:-1], path[1:]))
        if rng.random() < 0.4:
            pairs.append((path[-1], path[0]))                             # closed into a cycle
    for _ in range(int(rng.integers(0, 6))):                              # cross links, self-loops, parallel edges
        pairs.append((int(rng.integers(n_nodes)), int(rng.integers(n_nodes))))
    if seed % 2:
        x, s, t, y = range(n_nodes, n_nodes + 4)
        n_nodes += 4
        pairs += [(x, s), (s, t), (t, s), (t, y)]
        if rng.random() < 0.5:
            pairs.append((int(rng.integers(n_nodes - 4)), x))
    order = rng.permutation(len(pairs))
    return rng, n_nodes, [pairs[i] for i in order]


N_TANGLES = 80


@pytest.fixture(scope="module")
def tangle_counts(shim, oracle):
    return [check(shim, oracle, n, pairs, rng) for rng, n, pairs in (tangle(seed) for seed in range(N_TANGLES))]


def test_random_tangles(tangle_counts):
    """every seed agrees with the oracle (check() asserts); over the seeds every branch of the walk was taken"""
    assert len(tangle_counts) == N_TANGLES >= 60
    for name in ("simple_loops", "self_loops", "ambiguity_cuts", "scc_restarts", "ambiguity_moves"):
        assert sum(c[name] for c in tangle_counts) > 0, name


def test_long_line_walked_twice(shim, oracle):
    """300 edges added back to front, weight 2: shrunk into one edge, walked twice (as the fixture data1 is)"""
    rng = np.random.default_rng(3)
    pairs = [(i, i + 1) for i in range(300)][::-1]
    c = check(shim, oracle, 301, pairs, rng, weights=[2] * 300)
    assert (c["shrunk_edges"], c["pieces"], c["contigs"]) == (1, 2, 2)


def test_long_cycles(shim, oracle):
    """a pure cycle only the SCC start can enter: 2 000 nodes against the oracle (which recurses), 20 000 -- a depth the reference's
    recursion is not given here -- in closed form: the shrink cuts a pure cycle of weight 1 into one self-loop of n edges at node 0,
    the walk takes it once: one contig of K - 1 + n bases"""
    rng = np.random.default_rng(5)
    n = 2000
    c = check(shim, oracle, n, [(i, (i + 1) % n) for i in range(n)], rng, weights=[1] * n)
    assert c["scc_restarts"] == 1
    n = 20000
    pairs = [(i, (i + 1) % n) for i in range(n)]
    labels = ["".join(rng.choice(list("ACGT"), K)) for _ in pairs]
    pieces, o_slot, chain, c = run_host(shim, n, pairs, [1] * n)
    got = contigs_of(pieces, o_slot, chain, labels, K)
    assert len(got) == 1 and len(got[0]) == K - 1 + n
    assert (c["nodes_left"], c["edges_left"], c["pieces"], c["scc_restarts"]) == (0, 0, 1, 1)


def test_unshrunk_cycle_is_walked_iteratively(shim):
    """the SCC search itself at depth: a ring of 20 000 nodes with an edge each way between neighbours is a graph shrink cannot merge
    (every vertex has two edges in and two out) without a vertex to start from, so tarjan's depth-first visit runs 20 000 deep"""
    n = 20000
    pairs = [(i, (i + 1) % n) for i in range(n)] + [((i + 1) % n, i) for i in range(n)]
    pieces, o_slot, chain, c = run_host(shim, n, pairs, [1] * len(pairs))
    assert c["shrunk_edges"] == len(pairs) and c["scc_restarts"] >= 1
    assert (c["nodes_left"], c["edges_left"], c["pieces"]) == (0, 0, len(pairs))


def test_assemble_route_gathers_whatever_the_environment_says(shim, monkeypatch):
    """katome_assemble_* over several GPUs: planned by plan_multi_route itself -- always the gather (the exact shrink and the walk
    are one GPU's), never the sharded shrink or stages, KATOME_E_ARG without the reference's numbering"""
    shim.hs_assemble_route.restype = C.c_uint32
    shim.hs_assemble_route.argtypes = [C.c_uint32, C.c_uint64, C.c_uint64]
    FIRST_SEEN, DEAD_PATHS, SHARE = 1, 2, 4
    for env in ({}, {"KATOME_DIST_SHRINK": "sharded"}, {"KATOME_DIST_SHRINK": "gather"}, {"KATOME_DIST_STAGES": "sharded"},
                {"KATOME_DIST_PRUNE": "gather"}):
        for name in ("KATOME_DIST_SHRINK", "KATOME_DIST_STAGES", "KATOME_DIST_PRUNE", "KATOME_COMM"):
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        for sizes in ((1000, 1000), (1 << 33, 1 << 33)):            # (a graph too big to gather: the gather itself refuses it)
            assert shim.hs_assemble_route(FIRST_SEEN, *sizes) == 16
            assert shim.hs_assemble_route(FIRST_SEEN | SHARE, *sizes) == 16 | 128
            assert shim.hs_assemble_route(FIRST_SEEN | DEAD_PATHS, *sizes) & (1 | 2 | 4 | 8 | 16) == 16
            assert shim.hs_assemble_route(0, *sizes) & 4 and shim.hs_assemble_route(DEAD_PATHS, *sizes) & 4
