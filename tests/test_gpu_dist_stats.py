"""CollectionStats and the weight spectrum of the SHARDED graph, no gather (katome_amd/csrc/dist_stats.hip): through the
staged host entry with thread ranks -- on the shares and on the gathered graph -- and through the Python API with one
process per rank, against the oracle's stats after every prefix of the stage string."""
import json
import os

import numpy as np
import pytest

from helpers import pack_reads_ascii
from test_gpu_stats import INPUTS, STAGES, THRESHOLD, _Case

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(oracle, k):
    if k not in _CASES:
        _CASES[k] = _Case(oracle, k)
    return _CASES[k]


def _staged(packed, n, L, skip, k, rc, n_dev, stages, thr, glen, first_seen=True):
    from katome_amd.build import GpuGraph
    g, _ = GpuGraph.create_from_packed(packed, n, L, skip=skip, reverse_complement=rc, k=k, first_seen_order=first_seen, n_devices=n_dev,
                                       ranks_share_device=True, stages=stages, original_genome_length=glen, minimal_weight_threshold=thr,
                                       stage_stats=True)
    return g


@pytest.mark.parametrize("route", ["sharded", "gather"])
@pytest.mark.parametrize("n_dev,k", [(2, 21), (3, 63), (8, 21)])
def test_thread_ranks_every_stage(oracle, monkeypatch, n_dev, k, route):
    monkeypatch.setenv("KATOME_DIST_STAGES", route)
    c = _case(oracle, k)
    g = _staged(c.packed, c.n, c.L, c.skip, k, c.rc, n_dev, STAGES, THRESHOLD, c.glen)
    assert len(g.stage_stats) == len(STAGES) + 1
    for i, got in enumerate(g.stage_stats):
        assert got == c.stats[i], (STAGES[:i], got, c.stats[i])
    assert (g.n_nodes, g.n_edges) == (c.stats[-1].node_count, c.stats[-1].edge_count)


def test_stage_stats_only_add_the_stats(oracle, monkeypatch):
    """on the shares the stats call rebuilds the links a stage dropped, which reorders the rank's nodes: the graph that comes
    back with stage_stats=True is still, array for array, the graph that comes back without it"""
    from katome_amd.build import GpuGraph
    monkeypatch.setenv("KATOME_DIST_STAGES", "sharded")
    for n_dev, k in ((3, 21), (2, 63)):
        c = _case(oracle, k)
        g = _staged(c.packed, c.n, c.L, c.skip, k, c.rc, n_dev, STAGES, THRESHOLD, c.glen)
        plain, _ = GpuGraph.create_from_packed(c.packed, c.n, c.L, skip=c.skip, reverse_complement=c.rc, k=k, first_seen_order=True,
                                               n_devices=n_dev, ranks_share_device=True, stages=STAGES, original_genome_length=c.glen,
                                               minimal_weight_threshold=THRESHOLD)
        assert not hasattr(plain, "stage_stats") and (plain.n_nodes, plain.n_edges) == (g.n_nodes, g.n_edges)
        for name in ("edge_src", "edge_dst", "edge_weight", "node_key"):
            assert np.array_equal(getattr(plain, name), getattr(g, name)), (n_dev, k, name)


def test_many_chunks_give_the_same_counts(oracle, monkeypatch):
    """KATOME_DIST_STATS_CHUNK=1000: dozens of exchanges per call; the in-degrees add up over them"""
    monkeypatch.setenv("KATOME_DIST_STAGES", "sharded")
    monkeypatch.setenv("KATOME_DIST_STATS_CHUNK", "1000")
    c = _case(oracle, 63)
    g = _staged(c.packed, c.n, c.L, c.skip, 63, c.rc, 3, "dw", THRESHOLD, c.glen)
    assert g.stage_stats == [c.stats[0], c.stats[1], _after(oracle, c, "dw")]


def _after(oracle, c, stages):
    from katome_amd.build import CollectionStats
    oracle.set_genome_length(c.glen)
    return CollectionStats(**oracle.build_ascii(c.ascii, c.k, c.rc, remove_weak_edges=THRESHOLD, stages=stages).stats)


def test_ranks_without_edges(oracle, monkeypatch):
    """the eight-rank input of test_gpu_dist_stages.py::test_a_rank_without_edges: after the first pruning only a cycle of five
    nodes is left, so most ranks describe a share with no edge at all"""
    from katome_amd.build import CollectionStats
    monkeypatch.setenv("KATOME_DIST_STAGES", "sharded")
    L, k = 60, 21
    period = np.frombuffer((b"ACGTT" * 20)[:L], np.uint8)
    ascii_reads = np.concatenate([oracle.synth_reads(0, 6, L, 2000, 2e-2, 1), np.stack([np.roll(period, -i) for i in range(4)])])
    has_n = (ascii_reads == ord("N")).any(axis=1)
    clean = ascii_reads.copy()
    clean[clean == ord("N")] = ord("A")
    g = _staged(pack_reads_ascii(clean).reshape(-1).copy(), len(ascii_reads), L, has_n.astype(np.uint8), k, False, 8, STAGES, 1, 400)
    oracle.set_genome_length(400)
    for i, got in enumerate(g.stage_stats):
        ref = oracle.build_ascii(ascii_reads, k, False, remove_weak_edges=1, stages=STAGES[:i])
        assert got == CollectionStats(**ref.stats), (STAGES[:i], got, ref.stats)
    assert 0 < g.stage_stats[-1].edge_count < 8


def test_packed_key_build_without_stages(oracle):
    """stats need no numbering: a packed-key build over three ranks, entry 0 alone, equal to the one-GPU value"""
    from katome_amd.build import GpuGraph
    c = _case(oracle, 21)
    g = _staged(c.packed, c.n, c.L, c.skip, 21, c.rc, 3, "", THRESHOLD, c.glen, first_seen=False)
    one, _ = GpuGraph.create_from_packed(c.packed, c.n, c.L, skip=c.skip, reverse_complement=c.rc, k=21, stage_stats=True)
    assert len(g.stage_stats) == 1 and g.stage_stats == one.stage_stats and g.stage_stats[0] == c.stats[0]


def test_failure_reaches_every_thread_rank(oracle, monkeypatch):
    from katome_amd.build import KatomePanic
    monkeypatch.setenv("KATOME_DIST_STAGES", "sharded")
    c = _case(oracle, 21)
    monkeypatch.setenv("KATOME_DIST_STATS_FAIL", "1")
    with pytest.raises(KatomePanic) as e:
        _staged(c.packed, c.n, c.L, c.skip, 21, c.rc, 4, "d", THRESHOLD, c.glen)
    assert e.value.name == "E_UNSUPPORTED" and "rank 1 of 4 failed" in str(e.value)
    monkeypatch.delenv("KATOME_DIST_STATS_FAIL")
    g = _staged(c.packed, c.n, c.L, c.skip, 21, c.rc, 4, "d", THRESHOLD, c.glen)
    assert g.stage_stats == c.stats[:2]


# ---- one PROCESS per rank through the Python sharded API ---------------------------------------------------------------
def _process_rank(rank, world, port, k, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch
    import torch.distributed as dist
    from katome_amd import shard as ks
    from katome_amd.build import KatomePanic
    from oracle import oracle as o
    rc, n_reads, read_len, genome, err, glen = INPUTS[k]
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
        out = {}

        def builder(first_seen):
            b = ks.ShardedBuilder(comm, k, rc, 0, first_seen_order=first_seen)
            b.add_reads(packed, first, count, read_len, skip, batch_reads=1024)
            return b

        def describe(b, name):
            st = b.stats()
            out[name] = dict(stats=[st.node_count, st.edge_count, st.max_edge_weight, st.avg_edge_weight, st.max_in_degree, st.max_out_degree,
                                    st.avg_out_degree, st.incoming_vert_count, st.outgoing_vert_count],
                             spectrum=[int(x) for x in b.weight_spectrum(16)])

        def refused(b):
            for call in (b.stats, lambda: b.weight_spectrum(16)):
                try:
                    call()
                    raise AssertionError("stats of a builder that is not finalized, or gathered")
                except KatomePanic as e:
                    assert e.name == "E_ARG", e

        b = builder(False)
        refused(b)                                            # before finalize
        b.finalize()
        describe(b, "by key")
        b.close()
        b = builder(True)
        refused(b)
        b.finalize()
        describe(b, "")
        b.remove_dead_paths()
        describe(b, "d")
        os.environ["KATOME_DIST_STATS_CHUNK"] = "1000"        # many chunks: the counts add up
        describe(b, "d in chunks")
        del os.environ["KATOME_DIST_STATS_CHUNK"]
        b.standardize_contigs()
        b.prune_weak_edges(THRESHOLD)
        b.standardize_contigs()
        b.standardize_edges(glen, THRESHOLD)
        b.remove_dead_paths()
        describe(b, STAGES)
        b.gather(0)
        refused(b)                                            # after gather
        b.close()
        # rank 1 fails after the first exchange: every rank gets the error that names it; a clean call on a fresh builder follows
        b = builder(True)
        b.finalize()
        os.environ["KATOME_DIST_STATS_FAIL"] = "1"
        try:
            b.stats()
            raise AssertionError("KATOME_DIST_STATS_FAIL=1 and no failure on rank %d" % rank)
        except KatomePanic as e:
            assert e.name == "E_UNSUPPORTED" and "rank 1 of %d failed" % world in str(e), e
        del os.environ["KATOME_DIST_STATS_FAIL"]
        b.close()
        b = builder(True)
        b.finalize()
        describe(b, "after a failure")
        x = b.exchange_stats()
        assert world == 1 or x["prune"]["bytes_out"] > 0      # the targets' addresses are accounted to the "prune" exchanges
        b.close()
        comm.close()
        with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
            json.dump(out, f)
    finally:
        dist.destroy_process_group()


def _spawn(world, *args):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_process_rank, args=(world, port) + args, nprocs=world, join=True)


@pytest.mark.parametrize("world,k", [(2, 31), (4, 63)])
def test_process_ranks_python_api(oracle, tmp_path, world, k):
    c = _case(oracle, k)
    _spawn(world, k, str(tmp_path))
    parts = [json.load(open(os.path.join(str(tmp_path), "rank%d.json" % r))) for r in range(world)]
    for p in parts[1:]:
        assert p == parts[0]                                  # identical on every rank
    got = parts[0]

    def check(name, i):
        s = got[name]["stats"]
        from katome_amd.build import CollectionStats
        assert CollectionStats(*s) == c.stats[i], (name, s, c.stats[i])
        assert got[name]["spectrum"] == [int(x) for x in c.spectrum[i]], name

    check("by key", 0)
    check("", 0)
    check("d", 1)
    check("d in chunks", 1)
    check(STAGES, len(STAGES))
    check("after a failure", 0)
