"""The stages between the two prunings (standardize_contigs, remove_weak_edges, standardize_edges and the second
remove_dead_paths) on the SHARDED graph, no gather (katome_amd/csrc/dist_stages.hip): against the oracle's petgraph
index for index, through the host entry with thread ranks and through the Python API with one process per rank."""
import os

import numpy as np
import pytest

from helpers import pack_reads_ascii

pytestmark = pytest.mark.gpu


def _same(got, ref):
    """host arrays of a GpuGraph against the oracle's PtGraph: every edge at its index"""
    assert (got.n_nodes, got.n_edges) == (ref.n_nodes, ref.n_edges)
    assert np.array_equal(got.edge_src, ref.edge_src) and np.array_equal(got.edge_dst, ref.edge_dst)
    assert np.array_equal(got.edge_weight, ref.edge_weight)
    assert np.array_equal(got.edge_label, ref.edge_label)
    if got.edge_age is not None:
        # the oracle hands SEQUENCES slots out in the order edges are first added (pt_graph.rs:176-194): slot = age + 1
        assert np.array_equal(got.edge_age.astype(np.uint64) + 1, ref.edge_slot)


def _reads(oracle, n, L, glen, err, seed_read=0):
    ascii_reads = oracle.synth_reads(seed_read, n, L, glen, err, 1)
    has_n = (ascii_reads == ord("N")).any(axis=1)
    clean = ascii_reads.copy()
    clean[clean == ord("N")] = ord("A")
    return ascii_reads, pack_reads_ascii(clean).reshape(-1).copy(), has_n.astype(np.uint8)


def _input(k):
    """reads whose graph keeps edges through every stage: at k = 63 short reads leave only dead paths of < 2k edges"""
    return (3000, 200, 30000, 1e-3) if k > 40 else (2500, 110, 50000, 8e-3)


def _build(packed, n, L, skip, k, rc, n_dev, stages, thr, glen):
    from katome_amd.build import GpuGraph
    g, _ = GpuGraph.create_from_packed(packed, n, L, skip=skip, reverse_complement=rc, k=k, first_seen_order=True, n_devices=n_dev,
                                       ranks_share_device=True, stages=stages, original_genome_length=glen, minimal_weight_threshold=thr)
    return g


CASES = [  # n_devices, k, rc, stages, threshold, genome length (small: weights scale down; large: up)
    (2, 21, True, "c", 2, 3000),
    (3, 31, False, "w", 2, 3000),
    (4, 40, True, "e", 1, 3000),
    (8, 63, False, "e", 3, 5_000_000),
    (2, 63, True, "cwc", 3, 3000),
    (3, 21, False, "wd", 1, 3000),
    (4, 31, True, "ed", 2, 4_000_000),
    (8, 40, False, "dcwced", 2, 3000),
    (3, 63, True, "dcwced", 2, 6_000_000),
    (2, 31, True, "dcwced", 1, 3000),
]


@pytest.mark.parametrize("n_dev,k,rc,stages,thr,glen", CASES)
def test_thread_ranks_match_oracle(oracle, monkeypatch, n_dev, k, rc, stages, thr, glen):
    monkeypatch.setenv("KATOME_DIST_STAGES", "sharded")
    n, L, G, err = _input(k)
    ascii_reads, packed, skip = _reads(oracle, n, L, G, err)
    g = _build(packed, n, L, skip, k, rc, n_dev, stages, thr, glen)
    oracle.set_genome_length(glen)
    ref = oracle.build_ascii(ascii_reads, k, rc, remove_weak_edges=thr, stages=stages)
    assert ref.n_edges > 0
    _same(g, ref)


@pytest.mark.parametrize("name,k,rc,n_dev,thr,glen", [("data1.txt", 40, True, 2, 2, 3000), ("data2.txt", 21, False, 3, 1, 2500),
                                                     ("data3.txt", 31, True, 4, 2, 900000)])
def test_fixtures_match_oracle(oracle, golden_dir, monkeypatch, name, k, rc, n_dev, thr, glen):
    from katome_amd.build import GpuGraph, InputFileType, set_global_k_sizes
    monkeypatch.setenv("KATOME_DIST_STAGES", "sharded")
    path = os.path.join(golden_dir, name)
    set_global_k_sizes(k)
    g, rb = GpuGraph.create([path], InputFileType.Fastq, rc, thr, first_seen_order=True, stages="dcwced", original_genome_length=glen,
                            n_devices=n_dev, ranks_share_device=True)
    oracle.set_genome_length(glen)
    ref = oracle.build_files([path], k, rc, remove_weak_edges=thr, stages="dcwced")
    assert rb == ref.read_bytes
    _same(g, ref)


def test_standardize_edges_removes_every_edge(oracle, monkeypatch):
    """genome length = k and a threshold above every weight: p = 0 / 0 = NaN, every weight becomes 0 and every edge and
    node goes; the second remove_dead_paths then runs on ranks that hold nothing"""
    monkeypatch.setenv("KATOME_DIST_STAGES", "sharded")
    n, L, k = 600, 90, 31
    ascii_reads, packed, skip = _reads(oracle, n, L, 5000, 4e-3)
    g = _build(packed, n, L, skip, k, True, 4, "ed", 1 << 30, k)
    oracle.set_genome_length(k)
    ref = oracle.build_ascii(ascii_reads, k, True, remove_weak_edges=1 << 30, stages="ed")
    assert ref.n_edges == 0
    _same(g, ref)


def test_a_rank_without_edges(oracle, monkeypatch):
    """eight ranks; the first remove_dead_paths leaves only a cycle of five pass-through nodes (never walked, never
    standardized), so at least three ranks end each stage from there on with no edge while another holds some"""
    monkeypatch.setenv("KATOME_DIST_STAGES", "sharded")
    L, k = 60, 21
    period = np.frombuffer((b"ACGTT" * 20)[:L], np.uint8)
    ascii_reads = np.concatenate([oracle.synth_reads(0, 6, L, 2000, 2e-2, 1), np.stack([np.roll(period, -i) for i in range(4)])])
    has_n = (ascii_reads == ord("N")).any(axis=1)
    clean = ascii_reads.copy()
    clean[clean == ord("N")] = ord("A")
    g = _build(pack_reads_ascii(clean).reshape(-1).copy(), len(ascii_reads), L, has_n.astype(np.uint8), k, False, 8, "dcwced", 1, 400)
    oracle.set_genome_length(400)
    ref = oracle.build_ascii(ascii_reads, k, False, remove_weak_edges=1, stages="dcwced")
    assert 0 < ref.n_edges < 8 and oracle.build_ascii(ascii_reads, k, False).n_edges > 8 * ref.n_edges
    _same(g, ref)


@pytest.mark.parametrize("n_dev,k,rc,stages", [(3, 31, True, "dcwced"), (4, 63, False, "wdce")])
def test_sharded_equals_gathered(oracle, monkeypatch, n_dev, k, rc, stages):
    n, L, G, err = _input(k)
    _, packed, skip = _reads(oracle, n, L, G, err)
    out = {}
    for route in ("sharded", "gather"):
        monkeypatch.setenv("KATOME_DIST_STAGES", route)
        out[route] = _build(packed, n, L, skip, k, rc, n_dev, stages, 2, 3000)
    a, b = out["sharded"], out["gather"]
    assert (a.n_nodes, a.n_edges) == (b.n_nodes, b.n_edges) and a.n_edges > 0
    for name in ("edge_src", "edge_dst", "edge_weight", "edge_label", "edge_key", "node_key", "edge_age"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize("where", ["edges", "nodes"])
def test_failure_reaches_every_rank(oracle, monkeypatch, where):
    """rank 0's replay fails: every rank returns the error (nobody waits in a collective); a clean run follows"""
    from katome_amd.build import KatomePanic
    monkeypatch.setenv("KATOME_DIST_STAGES", "sharded")
    n, L, k = 2000, 100, 31
    ascii_reads, packed, skip = _reads(oracle, n, L, 50000, 8e-3)
    monkeypatch.setenv("KATOME_DIST_STAGES_FAIL", where)
    with pytest.raises(KatomePanic) as e:
        _build(packed, n, L, skip, k, True, 4, "w", 2, 3000)
    assert "KATOME_DIST_STAGES_FAIL" in str(e.value) or "rank 0 failed" in str(e.value)
    monkeypatch.delenv("KATOME_DIST_STAGES_FAIL")
    g = _build(packed, n, L, skip, k, True, 4, "w", 2, 3000)
    ref = oracle.build_ascii(ascii_reads, k, True, remove_weak_edges=2, stages="w")
    _same(g, ref)


# ---- one PROCESS per rank through the Python sharded API ---------------------------------------------------------------
def _process_rank(rank, world, port, k, rc, n_reads, read_len, genome, err, thr, glen, mode, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch
    import torch.distributed as dist
    from katome_amd import shard as ks
    from katome_amd.build import KatomePanic
    from oracle import oracle as o
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        ascii_reads = o.synth_reads(0, n_reads, read_len, genome, err, 1)
        has_n = (ascii_reads == ord("N")).any(axis=1)
        clean = ascii_reads.copy()
        clean[clean == ord("N")] = ord("A")
        first, count = ks.shard_range(n_reads, world, rank)
        packed = torch.from_numpy(np.concatenate([pack_reads_ascii(clean[first:first + count]).reshape(-1), np.zeros(32, np.uint8)])).cuda()
        skip = torch.from_numpy(np.concatenate([has_n[first:first + count].astype(np.uint8), np.zeros(16, np.uint8)])).cuda()
        comm = ks.Comm.over_torch(device=0)
        if mode == "args":
            # a packed-key builder and a gathered one get KATOME_E_ARG
            for first_seen in (False, True):
                b = ks.ShardedBuilder(comm, k, rc, 0, first_seen_order=first_seen)
                b.add_reads(packed, first, count, read_len, skip)
                b.finalize()
                if first_seen:
                    b.gather(0)
                for call in (b.standardize_contigs, lambda: b.prune_weak_edges(thr), lambda: b.standardize_edges(glen, thr)):
                    try:
                        call()
                        raise AssertionError("a stage ran on a %s builder" % ("gathered" if first_seen else "packed-key"))
                    except KatomePanic as e:
                        assert e.name == "E_ARG", e
                b.close()
            comm.close()
            return
        b = ks.ShardedBuilder(comm, k, rc, 0, first_seen_order=True)
        b.add_reads(packed, first, count, read_len, skip, batch_reads=1024)
        b.finalize()
        b.remove_dead_paths()
        b.standardize_contigs()
        b.prune_weak_edges(thr)
        b.standardize_contigs()
        b.standardize_edges(glen, thr)
        g, _ = b.remove_dead_paths()
        out = dict(total_nodes=g.total_nodes, total_edges=g.total_edges, edge_id=g.edge_id.cpu().numpy(), node_id=g.node_id.cpu().numpy(),
                   src=g.edge_src.cpu().numpy(), dst=g.edge_dst.cpu().numpy(), weight=g.edge_weight.cpu().numpy().view(np.uint32),
                   label=g.edge_label.cpu().numpy(), age=g.edge_age.cpu().numpy(), edge_key=g.edge_key.cpu().numpy().view(np.uint64),
                   node_key=g.node_key.cpu().numpy().view(np.uint64))
        cur = b.graph()
        assert cur.total_edges == g.total_edges and cur.n_edges == g.n_edges
        del g, cur
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
        b.close()
        comm.close()
    finally:
        dist.destroy_process_group()


def _spawn(world, *args):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_process_rank, args=(world, port) + args, nprocs=world, join=True)


@pytest.mark.parametrize("world,k,rc,thr,glen", [(2, 31, True, 2, 3000), (3, 40, False, 1, 2500), (4, 63, True, 2, 3000)])
def test_process_ranks_python_api(oracle, tmp_path, world, k, rc, thr, glen):
    """finalize -> remove_dead_paths -> standardize_contigs -> prune_weak_edges -> standardize_contigs -> standardize_edges ->
    remove_dead_paths, one process per rank over gloo; the shares put together by edge_id / node_id equal the oracle's "dcwced" """
    n_reads, L, G, err = _input(k)
    _spawn(world, k, rc, n_reads, L, G, err, thr, glen, "stages", str(tmp_path))
    oracle.set_genome_length(glen)
    ref = oracle.build_ascii(oracle.synth_reads(0, n_reads, L, G, err, 1), k, rc, remove_weak_edges=thr, stages="dcwced")
    assert ref.n_edges > 0
    parts = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(world)]
    TE, TN = ref.n_edges, ref.n_nodes
    src, dst, w, age = (np.full(TE, -1, np.int64) for _ in range(4))
    label = np.zeros((TE, ref.edge_label.shape[1]), np.uint8)
    seen_e, seen_n = np.zeros(TE, np.int64), np.zeros(TN, np.int64)
    for p in parts:
        assert (int(p["total_nodes"]), int(p["total_edges"])) == (TN, TE)
        ids = p["edge_id"].astype(np.int64)
        assert ids.size == 0 or (ids.min() >= 0 and ids.max() < TE)
        src[ids], dst[ids], w[ids], age[ids] = p["src"], p["dst"], p["weight"], p["age"]
        label[ids] = p["label"].reshape(len(ids), -1)[:, :label.shape[1]]
        np.add.at(seen_e, ids, 1)
        nids = p["node_id"].astype(np.int64)
        assert nids.size == 0 or (nids.min() >= 0 and nids.max() < TN)
        np.add.at(seen_n, nids, 1)
    assert (seen_e == 1).all() and (seen_n == 1).all()          # every index exactly once across the ranks
    assert np.array_equal(src, ref.edge_src.astype(np.int64)) and np.array_equal(dst, ref.edge_dst.astype(np.int64))
    assert np.array_equal(w, ref.edge_weight.astype(np.int64))
    assert np.array_equal(label, ref.edge_label)
    assert np.array_equal(age + 1, ref.edge_slot.astype(np.int64))


def test_argument_errors(tmp_path):
    """a packed-key builder and a gathered one: KATOME_E_ARG from every stage, on every rank"""
    _spawn(2, 31, True, 800, 100, 50000, 8e-3, 2, 3000, "args", str(tmp_path))
