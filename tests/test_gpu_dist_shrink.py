"""Shrinkable::shrink in the traversal-free form on the SHARDED graph, no gather (katome_amd/csrc/dist_shrink.hip): through
the host entries with KATOME_DIST_SHRINK=sharded and thread ranks on one card, and through the Python API with one process
per rank.  In first-seen order the result equals the one-GPU fast form array for array; by packed key as a multiset."""
import os

import numpy as np
import pytest

from helpers import int_to_kmer, pack_reads_ascii, revcomp_str

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _clean(ascii_reads):
    clean = ascii_reads.copy()
    clean[clean == ord("N")] = ord("A")
    return clean


def _input(k):
    """as test_gpu_dist_stages.py: reads whose graph keeps edges through every stage"""
    return (3000, 200, 30000, 1e-3) if k > 40 else (2500, 110, 50000, 8e-3)


def _one_gpu(packed, n, L, k, rc, first_seen, stages="", thr=0, glen=0):
    """the one-GPU builder after the stage chain, and its fast shrink"""
    from katome_amd import device as kd
    b = kd.Builder(k, rc, first_seen_order=first_seen)
    p = torch.from_numpy(np.concatenate([packed, np.zeros(32, np.uint8)])).cuda()
    span = b.tile_span(L)
    if span > 1:
        b.insert_tiles(b.extract_tiles(p, n, L, span), span)
    else:
        b.insert(b.extract_fixed(p, n, L))
    b.finalize()
    for st in stages:
        if st == "d":
            b.remove_dead_paths()
        elif st == "c":
            b.standardize_contigs()
        elif st == "w":
            b.remove_weak_edges(thr)
        elif st == "e":
            b.standardize_edges(glen, thr)
    return b, b.shrink(mode="fast")


def _host(dc):
    """a DeviceContigs / RankContigs as host arrays"""
    return dict(src=dc.edge_src.cpu().numpy(), dst=dc.edge_dst.cpu().numpy(), weight=dc.edge_weight.cpu().numpy().view(np.uint32),
                kmers=dc.edge_kmers.cpu().numpy().view(np.uint32), off=dc.edge_label_off.cpu().numpy(), label=dc.edge_label.cpu().numpy(),
                node_key=dc.node_key.cpu().numpy().view(np.uint64))


def _same_as_one_gpu(c, ref):
    """GpuContigs (host entry) against the one-GPU fast form, array for array"""
    assert (c.n_nodes, c.n_edges) == (ref["node_key"].shape[0], ref["src"].shape[0])
    assert np.array_equal(c.edge_src, ref["src"].astype(np.uint64)) and np.array_equal(c.edge_dst, ref["dst"].astype(np.uint64))
    assert np.array_equal(c.edge_weight, ref["weight"]) and np.array_equal(c.edge_kmers, ref["kmers"])
    assert np.array_equal(c.edge_label_off.astype(np.int64), ref["off"]) and np.array_equal(c.edge_label, ref["label"])
    assert np.array_equal(c.node_key, ref["node_key"])


def _sharded(packed, n, L, k, rc, n_dev, first_seen, dead_paths=False):
    from katome_amd.build import GpuContigs
    c, _ = GpuContigs.create_from_packed(packed, n, L, reverse_complement=rc, k=k, first_seen_order=first_seen,
                                         remove_dead_paths=dead_paths, n_devices=n_dev, ranks_share_device=True)
    return c


def _checked_contigs(c, k):
    """GpuContigs -> sorted (sequence, weight), after checking every label against its end vertices and its length"""
    names = [int_to_kmer(int(r[0]) if c.key_words == 1 else (int(r[0]) << 64) | int(r[1]), k - 1) for r in c.node_key]
    assert len(set(names)) == len(names)
    for i, s in enumerate(c.edge_seq):
        assert len(s) == k + int(c.edge_kmers[i]) - 1
        assert names[int(c.edge_src[i])] == s[:k - 1] and names[int(c.edge_dst[i])] == s[-(k - 1):]
    assert set(c.edge_src.tolist()) | set(c.edge_dst.tolist()) == set(range(c.n_nodes))
    return c.contigs()


def _device_contigs(dc, k):
    names = [int_to_kmer(int(r[0]) if dc.key_words == 1 else (int(r[0]) << 64) | int(r[1]), k - 1)
             for r in dc.node_key.cpu().numpy().view(np.uint64)]
    seqs = dc.sequences()
    src, dst = dc.edge_src.cpu().tolist(), dc.edge_dst.cpu().tolist()
    for i, s in enumerate(seqs):
        assert names[src[i]] == s[:k - 1] and names[dst[i]] == s[-(k - 1):]
    return sorted(zip(seqs, dc.edge_weight.cpu().numpy().view(np.uint32).tolist()))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("n_dev,k,rc,chain", [(2, 21, True, ""), (3, 31, False, "d"), (4, 40, True, "d"), (8, 63, False, ""),
                                               (3, 63, True, "d"), (2, 31, True, ""), (4, 21, False, "d"), (8, 40, True, "d")])
def test_first_seen_host_entry_equals_one_gpu_fast(oracle, monkeypatch, n_dev, k, rc, chain):
    monkeypatch.setenv("KATOME_DIST_SHRINK", "sharded")
    n, L, G, err = _input(k)
    packed = pack_reads_ascii(_clean(oracle.synth_reads(0, n, L, G, err, 1))).reshape(-1).copy()
    b, dc = _one_gpu(packed, n, L, k, rc, True, chain)
    ref = _host(dc)
    assert ref["src"].shape[0] > 0
    c = _sharded(packed, n, L, k, rc, n_dev, True, dead_paths=chain == "d")
    _same_as_one_gpu(c, ref)
    b.close()


@pytest.mark.timeout(300)
def test_without_the_variable_nothing_changes(oracle, monkeypatch):
    """first-seen order gathers and runs the exact form; a packed-key build is refused"""
    from katome_amd.build import GpuContigs, KatomePanic
    monkeypatch.delenv("KATOME_DIST_SHRINK", raising=False)
    n, L, G, err = _input(31)
    packed = pack_reads_ascii(_clean(oracle.synth_reads(0, n, L, G, err, 1))).reshape(-1).copy()
    with pytest.raises(KatomePanic) as e:
        _sharded(packed, n, L, 31, True, 2, False)
    assert e.value.name == "E_ARG"
    c, _ = GpuContigs.create_from_packed(packed, n, L, reverse_complement=True, k=31, first_seen_order=True)
    g = _sharded(packed, n, L, 31, True, 3, True)
    assert np.array_equal(g.edge_src, c.edge_src) and np.array_equal(g.edge_label, c.edge_label)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("n_dev,k,rc", [(2, 31, True), (3, 21, False), (4, 63, True)])
def test_packed_key_multiset(oracle, monkeypatch, n_dev, k, rc):
    monkeypatch.setenv("KATOME_DIST_SHRINK", "sharded")
    n, L, G, err = _input(k)
    packed = pack_reads_ascii(_clean(oracle.synth_reads(0, n, L, G, err, 1))).reshape(-1).copy()
    b, dc = _one_gpu(packed, n, L, k, rc, False)
    want = _device_contigs(dc, k)
    c = _sharded(packed, n, L, k, rc, n_dev, False)
    assert _checked_contigs(c, k) == want and len(want) > 0
    b.close()


@pytest.mark.timeout(300)
def test_packed_key_ranks_without_edges(oracle, monkeypatch):
    """one read of four 31-mers on eight ranks: at least four ranks hold no edge"""
    monkeypatch.setenv("KATOME_DIST_SHRINK", "sharded")
    k, L = 31, 34
    reads = oracle.synth_reads(3, 1, L, 5000, 0.0, 0)
    packed = pack_reads_ascii(reads).reshape(-1).copy()
    b, dc = _one_gpu(packed, 1, L, k, False, False)
    c = _sharded(packed, 1, L, k, False, 8, False)
    got = _checked_contigs(c, k)
    assert got == _device_contigs(dc, k) == [(reads[0].tobytes().decode(), 1)]
    b.close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("i", [0, 1, 2])
@pytest.mark.parametrize("first_seen", [True, False])
def test_reference_counts(oracle, golden_dir, monkeypatch, i, first_seen):
    """tests/shrinker.rs:33-36: (2,1), (184,92), (466,233), and the oracle's merged edges"""
    import json
    from katome_amd.build import GpuContigs, InputFileType, set_global_k_sizes
    monkeypatch.setenv("KATOME_DIST_SHRINK", "sharded")
    pinned = json.load(open(os.path.join(golden_dir, "pinned.json")))
    path, k = os.path.join(golden_dir, pinned["fixtures"][i]), pinned["k"]
    set_global_k_sizes(k)
    c, _ = GpuContigs.create([path], InputFileType.Fastq, False, first_seen_order=first_seen, n_devices=3, ranks_share_device=True)
    assert [c.n_nodes, c.n_edges] == pinned["shrink"]["counts"][i]
    assert _checked_contigs(c, k) == oracle.build_files([path], k, False, stages="s").contigs()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("first_seen", [True, False])
@pytest.mark.parametrize("k,rc", [(21, True), (31, False)])
def test_cycle_of_inner_vertices(oracle, monkeypatch, first_seen, k, rc):
    """reads off a circular sequence only: one self-loop per strand spelling the circle; in first-seen order cut at the
    same vertex as on one GPU, by packed key compared up to rotation"""
    monkeypatch.setenv("KATOME_DIST_SHRINK", "sharded")
    rng = np.random.default_rng(k)
    circle = "".join("ACGT"[c] for c in rng.integers(0, 4, 300))
    L = 60
    reads = np.array([[ord(c) for c in (circle + circle)[s:s + L]] for s in range(0, 300, 7)], dtype=np.uint8)
    packed = pack_reads_ascii(reads).reshape(-1).copy()
    b, dc = _one_gpu(packed, len(reads), L, k, rc, first_seen)
    c = _sharded(packed, len(reads), L, k, rc, 3, first_seen)
    assert c.n_edges == (2 if rc else 1) and np.array_equal(c.edge_src, c.edge_dst)
    assert all(len(s) == 300 + k - 1 for s in c.edge_seq)

    def rot(s):                          # a circle rotated to its smallest form
        return min(s[i:] + s[:i] for i in range(len(s)))

    def canon(seq):                      # the circle a self-loop label spells
        return rot(seq[:len(seq) - (k - 1)])
    want = {rot(circle)} | ({rot(revcomp_str(circle))} if rc else set())
    assert {canon(s) for s in c.edge_seq} == want
    if first_seen:
        _same_as_one_gpu(c, _host(dc))
    else:
        assert sorted(canon(s) for s in c.edge_seq) == sorted(canon(s) for s in dc.sequences())
    b.close()


@pytest.mark.timeout(300)
def test_failure_reaches_every_rank(oracle, monkeypatch):
    """KATOME_DIST_SHRINK_FAIL=1: rank 1 fails after the first ranking round, the call returns its error; a clean run follows"""
    from katome_amd.build import KatomePanic
    monkeypatch.setenv("KATOME_DIST_SHRINK", "sharded")
    n, L, G, err = _input(31)
    packed = pack_reads_ascii(_clean(oracle.synth_reads(0, n, L, G, err, 1))).reshape(-1).copy()
    monkeypatch.setenv("KATOME_DIST_SHRINK_FAIL", "1")
    with pytest.raises(KatomePanic) as e:
        _sharded(packed, n, L, 31, True, 4, True)
    assert "rank 1" in str(e.value) and e.value.name == "E_UNSUPPORTED"
    monkeypatch.delenv("KATOME_DIST_SHRINK_FAIL")
    assert _sharded(packed, n, L, 31, True, 4, True).n_edges > 0


# ---- one process per rank, over gloo -------------------------------------------------------------------------------------
def _linear_reads(glen=20000, L=150, step=50, seed=11):
    rng = np.random.default_rng(seed)
    genome = "".join("ACGT"[c] for c in rng.integers(0, 4, glen))
    starts = list(range(0, glen - L + 1, step))
    if starts[-1] != glen - L:
        starts.append(glen - L)
    return genome, np.array([[ord(c) for c in genome[s:s + L]] for s in starts], dtype=np.uint8)


def _process_rank(rank, world, port, mode, k, rc, thr, glen, out_dir):
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
        if mode == "rounds":
            _, reads = _linear_reads()
        else:
            n, L, G, err = _input(k)
            reads = _clean(o.synth_reads(0, n, L, G, err, 1))
        L = reads.shape[1]
        first, count = ks.shard_range(len(reads), world, rank)
        packed = torch.from_numpy(np.concatenate([pack_reads_ascii(reads[first:first + count]).reshape(-1), np.zeros(32, np.uint8)])).cuda()
        comm = ks.Comm.over_torch(device=0)

        def build(first_seen=True):
            b = ks.ShardedBuilder(comm, k, rc, 0, first_seen_order=first_seen)
            b.add_reads(packed, first, count, L, None, batch_reads=1024)
            return b
        if mode == "errors":
            b = build()
            for step in ("before finalize", "after gather"):
                if step == "after gather":
                    b.finalize()
                    b.gather(0)
                try:
                    b.shrink()
                    raise AssertionError("shrink ran %s" % step)
                except KatomePanic as e:
                    assert e.name == "E_ARG", e
            b.close()
            os.environ["KATOME_DIST_SHRINK_FAIL"] = "1"
            b = build()
            b.finalize()
            try:
                b.shrink()
                raise AssertionError("the failure knob did not strike")
            except KatomePanic as e:
                assert e.name == "E_UNSUPPORTED" and "rank 1" in str(e), e
            del os.environ["KATOME_DIST_SHRINK_FAIL"]
            b.close()
            b = build()
            b.finalize()
            assert b.shrink().total_edges > 0
            b.close()
            np.savez(os.path.join(out_dir, "rank%d.npz" % rank), ok=np.ones(1))
            comm.close()
            return
        b = build()
        b.finalize()
        if mode == "chain":
            b.remove_dead_paths()
            b.standardize_contigs()
            b.prune_weak_edges(thr)
            b.standardize_contigs()
            b.standardize_edges(glen, thr)
            b.remove_dead_paths()
        c = b.shrink()
        h = _host(c)
        h.update(head=c.edge_head_id.cpu().numpy(), node_id=c.node_id.cpu().numpy(), seqs=np.array(c.sequences(), dtype=object),
                 total=np.array([c.total_nodes, c.total_edges]), stats=np.array([c.stats[f] for f in ("rank_rounds", "cycle_rounds", "longest_path")]))
        g = b.graph()                                        # the share is left as it was
        h["graph_edges"] = np.array([g.total_edges])
        del c, g
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **h)
        b.close()
        comm.close()
    finally:
        dist.destroy_process_group()


def _spawn(world, *args):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_process_rank, args=(world, port) + args, nprocs=world, join=True)


def _parts(tmp_path, world):
    return [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r), allow_pickle=True) for r in range(world)]


@pytest.mark.timeout(600)
def test_process_ranks_assembler_chain(oracle, tmp_path):
    """finalize -> d -> c -> w -> c -> e -> d -> shrink on three process ranks: the union ordered by head id equals the
    one-GPU chain's fast shrink, head ids name the head edges of the pruned graph, node ids place the nodes"""
    k, rc, thr, glen, world = 31, True, 2, 3000, 3
    _spawn(world, "chain", k, rc, thr, glen, str(tmp_path))
    n, L, G, err = _input(k)
    packed = pack_reads_ascii(_clean(oracle.synth_reads(0, n, L, G, err, 1))).reshape(-1).copy()
    b, dc = _one_gpu(packed, n, L, k, rc, True, "dcwced", thr, glen)
    ref = _host(dc)
    g1 = b.graph()
    parts = _parts(tmp_path, world)
    TN, TE = ref["node_key"].shape[0], ref["src"].shape[0]
    assert TE > 0 and all(tuple(p["total"]) == (TN, TE) for p in parts)
    assert all(int(p["graph_edges"][0]) == g1.n_edges for p in parts)
    head = np.concatenate([p["head"] for p in parts])
    order = np.argsort(head, kind="stable")
    assert np.array_equal(np.sort(head), np.unique(head))
    for name in ("src", "dst", "weight", "kmers"):
        assert np.array_equal(np.concatenate([p[name] for p in parts])[order], ref[name]), name
    seqs = np.concatenate([p["seqs"] for p in parts])[order].tolist()
    assert seqs == dc.sequences()
    # the head edge at its petgraph index spells the merged edge's first k bases and carries its weight
    glab, gw = g1.edge_label.cpu().numpy(), g1.edge_weight.cpu().numpy().view(np.uint32)
    for i, h in enumerate(np.sort(head).tolist()):
        bts = glab[h]
        first = "".join("ACGT"[(int(x) >> s) & 3] for x in bts[1:] for s in (6, 4, 2, 0))[:k]
        assert first == seqs[i][:k] and gw[h] == ref["weight"][i]
    nkey = np.zeros_like(ref["node_key"])
    seen = np.zeros(TN, np.int64)
    for p in parts:
        ids = p["node_id"].astype(np.int64)
        nkey[ids] = p["node_key"].reshape(len(ids), -1)
        np.add.at(seen, ids, 1)
    assert (seen == 1).all() and np.array_equal(nkey, ref["node_key"])
    b.close()


@pytest.mark.timeout(600)
def test_rounds_grow_with_the_log_of_the_longest_path(tmp_path):
    """error-free reads of a linear 20 kb genome on four ranks: one unitig per strand, spelling the genome; ranking rounds
    <= ceil(log2(longest path)) + 2 (walkers hopping along the path would need about 20 000)"""
    world, k = 4, 31
    _spawn(world, "rounds", k, True, 0, 0, str(tmp_path))
    genome, _ = _linear_reads()
    parts = _parts(tmp_path, world)
    seqs = sorted(np.concatenate([p["seqs"] for p in parts]).tolist())
    assert seqs == sorted([genome, revcomp_str(genome)])
    longest = len(genome) - k + 1
    for p in parts:
        rounds, cycle_rounds, lp = (int(x) for x in p["stats"])
        assert lp == longest and cycle_rounds == 0
        assert rounds <= int(np.ceil(np.log2(longest))) + 2


@pytest.mark.timeout(600)
def test_process_ranks_errors(tmp_path):
    """before finalize and after gather: KATOME_E_ARG; KATOME_DIST_SHRINK_FAIL=1: the same error naming rank 1 on every rank,
    then a clean build and shrink in the same processes"""
    _spawn(2, "errors", 31, True, 0, 0, str(tmp_path))
    assert all(int(p["ok"][0]) == 1 for p in _parts(tmp_path, 2))
