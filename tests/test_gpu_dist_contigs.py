"""standardize_contigs on the SHARDED graph by list ranking (katome_amd/csrc/dist_contigs.hip, KATOME_DIST_CONTIGS=ranked):
against the oracle's petgraph index for index through the host entry with thread ranks on one card, against the table
route, with many chunks per round, with cycles of pass-through vertices and ranks without edges, through the Python API
with one process per rank, and the route choice and the failure knob."""
import math
import os

import numpy as np
import pytest

from helpers import pack_reads_ascii

pytestmark = pytest.mark.gpu

ARRAYS = ("edge_src", "edge_dst", "edge_weight", "edge_label", "edge_key", "node_key")


def _same(got, ref):
    """host arrays of a GpuGraph against the oracle's PtGraph: every edge at its index"""
    assert (got.n_nodes, got.n_edges) == (ref.n_nodes, ref.n_edges)
    assert np.array_equal(got.edge_src, ref.edge_src) and np.array_equal(got.edge_dst, ref.edge_dst)
    assert np.array_equal(got.edge_weight, ref.edge_weight)
    assert np.array_equal(got.edge_label, ref.edge_label)
    if got.edge_age is not None:
        assert np.array_equal(got.edge_age.astype(np.uint64) + 1, ref.edge_slot)


def _equal_graphs(a, b):
    assert (a.n_nodes, a.n_edges) == (b.n_nodes, b.n_edges)
    for name in ARRAYS:
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert (a.edge_age is None) == (b.edge_age is None)
    if a.edge_age is not None:
        assert np.array_equal(a.edge_age, b.edge_age)


def _input(k):
    """test_gpu_dist_stages._input: reads whose graph keeps edges through every stage"""
    return (3000, 200, 30000, 1e-3) if k > 40 else (2500, 110, 50000, 8e-3)


_SYNTH = {}


def _synth(oracle, k):
    """(ascii reads, packed reads, skip flags) of _input(k), made once"""
    key = k > 40
    if key not in _SYNTH:
        n, L, G, err = _input(k)
        ascii_reads = oracle.synth_reads(0, n, L, G, err, 1)
        has_n = (ascii_reads == ord("N")).any(axis=1)
        clean = ascii_reads.copy()
        clean[clean == ord("N")] = ord("A")
        _SYNTH[key] = (ascii_reads, pack_reads_ascii(clean).reshape(-1).copy(), has_n.astype(np.uint8))
    return _SYNTH[key]


def _circle_reads():
    """a random 300-base circle read as 60-bp reads every 7 bases"""
    rng = np.random.default_rng(21)
    circle = "".join("ACGT"[c] for c in rng.integers(0, 4, 300))
    return np.array([[ord(c) for c in (circle + circle)[s:s + 60]] for s in range(0, 300, 7)], dtype=np.uint8)


def _linear_circle_reads():
    """a linear random 20 000-base genome read error-free as 60-bp reads every 20 bases, and the circle: at k = 31 one contig
    of 19 970 edges per strand and 300 cycle edges per strand"""
    rng = np.random.default_rng(11)
    genome = "".join("ACGT"[c] for c in rng.integers(0, 4, 20000))
    linear = np.array([[ord(c) for c in genome[s:s + 60]] for s in range(0, 20000 - 60 + 1, 20)], dtype=np.uint8)
    return np.concatenate([linear, _circle_reads()])


def _contig_stats(src, dst):
    """(contigs, edges of the longest, edges on cycles of pass-through vertices, which edges those are) of a graph, as the
    table route reads it: a contig starts at an edge whose source is not a vertex with in = out = 1 and runs through such
    vertices"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    n = int(max(src.max(), dst.max())) + 1 if src.size else 0
    indeg, outdeg = np.bincount(dst, minlength=n), np.bincount(src, minlength=n)
    through = (indeg == 1) & (outdeg == 1)
    out_edge = np.zeros(n, np.int64)
    out_edge[src] = np.arange(src.size)
    through[src[src == dst]] = False                # (a self-loop at such a vertex stands alone)
    lengths, on_cycle = [], np.ones(src.size, bool)
    for e in np.nonzero(~through[src])[0].tolist():
        length, on_cycle[e] = 1, False
        while through[dst[e]]:
            e = int(out_edge[dst[e]])
            length, on_cycle[e] = length + 1, False
        lengths.append(length)
    return len(lengths), max(lengths, default=0), int(on_cycle.sum()), on_cycle


def _build(packed, n, L, skip, k, rc, n_dev, stages, thr=2, glen=3000):
    from katome_amd.build import GpuGraph
    g, _ = GpuGraph.create_from_packed(packed, n, L, skip=skip, reverse_complement=rc, k=k, first_seen_order=True, n_devices=n_dev,
                                       ranks_share_device=True, stages=stages, original_genome_length=glen, minimal_weight_threshold=thr)
    return g


@pytest.fixture
def ranked(monkeypatch):
    monkeypatch.setenv("KATOME_DIST_STAGES", "sharded")
    monkeypatch.setenv("KATOME_DIST_CONTIGS", "ranked")
    for name in ("KATOME_DIST_CONTIGS_CHUNK", "KATOME_DIST_CONTIGS_FAIL", "KATOME_DIST_CONTIGS_TABLE_LIMIT"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


_ORACLE = {}


def _oracle_lc(oracle, rc, stages):
    """the oracle's graph of the linear + circle input at k = 31, made once per (rc, stages)"""
    if (rc, stages) not in _ORACLE:
        _ORACLE[(rc, stages)] = oracle.build_ascii(_linear_circle_reads(), 31, rc, stages=stages)
    return _ORACLE[(rc, stages)]


# ---- 1. thread ranks against the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dev,k,rc,stages", [(2, 21, True, "c"), (3, 31, False, "cwc"), (4, 63, True, "dcwced"), (8, 40, False, "dcwced")])
def test_thread_ranks_match_oracle(oracle, ranked, n_dev, k, rc, stages):
    n, L, _, _ = _input(k)
    ascii_reads, packed, skip = _synth(oracle, k)
    g = _build(packed, n, L, skip, k, rc, n_dev, stages)
    oracle.set_genome_length(3000)
    ref = oracle.build_ascii(ascii_reads, k, rc, remove_weak_edges=2, stages=stages)
    assert ref.n_edges > 0
    _same(g, ref)
    if stages == "c":                                   # the stage did something: a route that does nothing cannot pass
        assert (oracle.build_ascii(ascii_reads, k, rc).edge_weight != ref.edge_weight).sum() > 1000


# ---- 2. both routes agree -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dev,k,rc,stages", [(3, 31, True, "c"), (4, 63, False, "dcwc")])
def test_both_routes_agree(oracle, ranked, n_dev, k, rc, stages):
    n, L, _, _ = _input(k)
    _, packed, skip = _synth(oracle, k)
    out = {}
    for route in ("table", "ranked"):
        ranked.setenv("KATOME_DIST_CONTIGS", route)
        out[route] = _build(packed, n, L, skip, k, rc, n_dev, stages)
    assert out["table"].n_edges > 0
    _equal_graphs(out["table"], out["ranked"])


# ---- 3. chunks ------------------------------------------------------------------------------------------------------------
def test_many_chunks_per_round(oracle, ranked):
    """64 questions per rank and exchange: hundreds of exchanges in the first rounds, the state updated in place between them
    (that the chunks happen: test_process_ranks_stats_and_route_choice counts the exchanges)"""
    reads = _linear_circle_reads()
    packed = pack_reads_ascii(reads).reshape(-1).copy()
    whole = _build(packed, len(reads), 60, None, 31, False, 3, "c")
    ranked.setenv("KATOME_DIST_CONTIGS_CHUNK", "64")
    chunked = _build(packed, len(reads), 60, None, 31, False, 3, "c")
    _same(chunked, _oracle_lc(oracle, False, "c"))
    _equal_graphs(chunked, whole)


# ---- 4. cycles and ranks without edges ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rc", [False, True])
def test_cycle_edges_stay_untouched(oracle, ranked, rc):
    reads = _linear_circle_reads()
    packed = pack_reads_ascii(reads).reshape(-1).copy()
    before, ref = _oracle_lc(oracle, rc, ""), _oracle_lc(oracle, rc, "c")
    contigs, longest, cycle_edges, on_cycle = _contig_stats(before.edge_src, before.edge_dst)
    assert (contigs, longest, cycle_edges) == ((2, 19970, 600) if rc else (1, 19970, 300))
    assert (before.edge_weight != ref.edge_weight).sum() == (2 if rc else 1) * 9970
    g = _build(packed, len(reads), 60, None, 31, rc, 8, "c")
    _same(g, ref)
    assert np.array_equal(g.edge_weight[on_cycle], before.edge_weight[on_cycle])      # the circle's edges: as they were


def test_circle_alone(oracle, ranked):
    """nothing but a cycle of pass-through vertices on 3 ranks: no contig, nothing changes, KATOME_OK"""
    reads = _circle_reads()
    packed = pack_reads_ascii(reads).reshape(-1).copy()
    before = oracle.build_ascii(reads, 31, False)
    assert _contig_stats(before.edge_src, before.edge_dst)[:3] == (0, 0, 300)
    g = _build(packed, len(reads), 60, None, 31, False, 3, "c")
    _same(g, before)
    _same(g, oracle.build_ascii(reads, 31, False, stages="c"))


# ---- 5. one PROCESS per rank over gloo ------------------------------------------------------------------------------------
def _process_rank(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch
    import torch.distributed as dist
    from katome_amd import shard as ks
    from katome_amd.build import KatomePanic
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        reads = _linear_circle_reads()
        first, count = ks.shard_range(len(reads), world, rank)
        packed = torch.from_numpy(np.concatenate([pack_reads_ascii(reads[first:first + count]).reshape(-1), np.zeros(32, np.uint8)])).cuda()
        comm = ks.Comm.over_torch(device=0)

        def build():
            b = ks.ShardedBuilder(comm, 31, False, 0, first_seen_order=True)
            b.add_reads(packed, first, count, 60, None, batch_reads=1024)
            b.finalize()
            return b
        for name in ("KATOME_DIST_CONTIGS_CHUNK", "KATOME_DIST_CONTIGS_FAIL"):
            os.environ.pop(name, None)
        os.environ["KATOME_DIST_CONTIGS"] = "ranked"
        b = build()
        try:
            b.standardize_stats()
            raise AssertionError("stats before any standardize_contigs")
        except KatomePanic as e:
            assert e.name == "E_ARG", e
        g = b.standardize_contigs()
        st = b.standardize_stats()
        out = dict(edge_id=g.edge_id.cpu().numpy(), weight=g.edge_weight.cpu().numpy().view(np.uint32), total_edges=g.total_edges,
                   stats=np.array([st[f] for f in ("route", "rank_rounds", "exchanges", "contigs", "longest_contig", "cycle_edges", "bytes_sent")]))
        del g
        b.close()
        # 64 questions per rank and exchange: the chunks of the links, of the rounds and of the means
        os.environ["KATOME_DIST_CONTIGS_CHUNK"] = "64"
        b = build()
        g = b.standardize_contigs()
        st = b.standardize_stats()
        out["chunked_stats"] = np.array([st[f] for f in ("route", "rank_rounds", "exchanges", "contigs", "longest_contig", "cycle_edges")])
        out["chunked_weight"] = g.edge_weight.cpu().numpy().view(np.uint32)
        out["chunked_id"] = g.edge_id.cpu().numpy()
        del g
        b.close()
        del os.environ["KATOME_DIST_CONTIGS_CHUNK"]
        # the table does not fit: without the variable the ranked route is taken, with table every rank gets E_OOM
        os.environ["KATOME_DIST_CONTIGS_TABLE_LIMIT"] = "1"
        del os.environ["KATOME_DIST_CONTIGS"]
        b = build()
        g = b.standardize_contigs()
        out["fallback_route"] = b.standardize_stats()["route"]
        out["fallback_weight"] = g.edge_weight.cpu().numpy().view(np.uint32)
        out["fallback_id"] = g.edge_id.cpu().numpy()
        del g
        b.close()
        os.environ["KATOME_DIST_CONTIGS"] = "table"
        b = build()
        try:
            b.standardize_contigs()
            out["table_status"] = "OK"
        except KatomePanic as e:
            out["table_status"] = e.name
        b.close()
        # nothing set: the table, as before
        del os.environ["KATOME_DIST_CONTIGS"], os.environ["KATOME_DIST_CONTIGS_TABLE_LIMIT"]
        b = build()
        g = b.standardize_contigs()
        out["unset_route"] = b.standardize_stats()["route"]
        out["unset_weight"] = g.edge_weight.cpu().numpy().view(np.uint32)
        out["unset_id"] = g.edge_id.cpu().numpy()
        del g
        b.close()
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
        comm.close()
    finally:
        dist.destroy_process_group()


def test_process_ranks_stats_and_route_choice(oracle, tmp_path):
    import socket
    import torch.multiprocessing as mp
    world = 3
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_process_rank, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    before, ref = _oracle_lc(oracle, False, ""), _oracle_lc(oracle, False, "c")
    contigs, longest, cycle_edges, _ = _contig_stats(before.edge_src, before.edge_dst)
    assert longest == 19970
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    for p in parts:
        route, rounds, exchanges, n_contigs, n_longest, n_cycle, sent = (int(x) for x in p["stats"])
        assert (route, n_contigs, n_longest, n_cycle) == (1, contigs, longest, cycle_edges)
        assert 1 <= rounds <= math.ceil(math.log2(longest)) + 2 and exchanges >= rounds
        assert int(p["total_edges"]) == ref.n_edges
        assert int(p["fallback_route"]) == 1 and str(p["table_status"]) == "E_OOM" and int(p["unset_route"]) == 0
    assert sum(int(p["stats"][6]) for p in parts) > 0
    # with 64 questions per exchange the first round alone needs this many exchanges: the rank with the most unresolved edges
    # holds at least a third of the edges that are not heads (the cycle edges ask too); far more than one per round
    first_round = math.ceil(math.ceil((ref.n_edges - contigs) / world) / 64)
    for p in parts:
        route, rounds, exchanges, n_contigs, n_longest, n_cycle = (int(x) for x in p["chunked_stats"])
        assert (route, n_contigs, n_longest, n_cycle) == (1, contigs, longest, cycle_edges)
        assert 1 <= rounds <= math.ceil(math.log2(longest)) + 2
        assert exchanges >= first_round > 4 * (math.ceil(math.log2(longest)) + 2) and exchanges > int(p["stats"][2])
    for ids, weights in (("edge_id", "weight"), ("chunked_id", "chunked_weight"), ("fallback_id", "fallback_weight"), ("unset_id", "unset_weight")):
        order = np.concatenate([p[ids] for p in parts])
        w = np.concatenate([p[weights] for p in parts])
        assert np.array_equal(np.sort(order), np.arange(ref.n_edges))
        assert np.array_equal(w[np.argsort(order, kind="stable")], ref.edge_weight)


# ---- 6. a failure reaches every rank; a value that names no route ---------------------------------------------------------
def test_failure_reaches_every_rank(oracle, ranked):
    from katome_amd.build import KatomePanic
    n, L, _, _ = _input(31)
    ascii_reads, packed, skip = _synth(oracle, 31)
    ranked.setenv("KATOME_DIST_CONTIGS_FAIL", "1")
    with pytest.raises(KatomePanic) as e:
        _build(packed, n, L, skip, 31, True, 4, "c")
    assert "rank 1" in str(e.value) and e.value.name == "E_UNSUPPORTED"
    ranked.delenv("KATOME_DIST_CONTIGS_FAIL")
    _same(_build(packed, n, L, skip, 31, True, 4, "c"), oracle.build_ascii(ascii_reads, 31, True, remove_weak_edges=2, stages="c"))
    ranked.setenv("KATOME_DIST_CONTIGS", "nonsense")
    with pytest.raises(KatomePanic) as e:
        _build(packed, n, L, skip, 31, True, 4, "c")
    assert e.value.name == "E_ARG"


# ---- 7. nothing else moved ------------------------------------------------------------------------------------------------
def test_without_the_variable_nothing_changes(oracle, ranked):
    """no variable set: the "dcwced" build equals the KATOME_DIST_CONTIGS=table build array for array (that the route read
    back is 0 then: test_process_ranks_stats_and_route_choice, where a builder can be asked)"""
    n, L, _, _ = _input(31)
    ascii_reads, packed, skip = _synth(oracle, 31)
    ranked.setenv("KATOME_DIST_CONTIGS", "table")
    table = _build(packed, n, L, skip, 31, True, 3, "dcwced")
    ranked.delenv("KATOME_DIST_CONTIGS")
    unset = _build(packed, n, L, skip, 31, True, 3, "dcwced")
    assert unset.n_edges > 0
    _equal_graphs(unset, table)
