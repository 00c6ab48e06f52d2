"""The sharded build of reads of VARYING length (katome_dist_add_reads_var, dist.hip): through the host entries with
`settings.n_devices` (thread ranks sharing the card), through the C ABI at world size 1 over RCCL, and with one process per
rank.  Against the oracle's build_files of the same FASTQ: in the reference's numbering every array index for index, by packed
key the edge multiset with every node owned once.  The reads are drawn from several lengths, including reads of exactly k bases
and reads with N, which ingest drops."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import kmer_to_int, pack_reads_ascii  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _var_reads(k, n, seed=5, genome_len=3000, err=0.01):
    """reads of several lengths (k among them) cut from one genome, some with an N"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, genome_len)
    lens = [L for L in (k, k + 1, k + 7, 2 * k, 100, 150, 61) if L >= k]
    reads = []
    for i in range(n):
        L = lens[int(rng.integers(0, len(lens)))]
        at = int(rng.integers(0, genome_len - L))
        bases = genome[at:at + L].copy()
        flip = rng.random(L) < err
        bases[flip] = rng.integers(0, 4, int(flip.sum()))
        s = "".join("ACGT"[c] for c in bases)
        if rng.random() < 0.05:
            j = int(rng.integers(0, L))
            s = s[:j] + "N" + s[j + 1:]
        reads.append(s)
    return reads


def _fastq(tmp_path, reads, name="var.fq"):
    path = tmp_path / name
    path.write_text("".join("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)))
    return str(path)


def _same_arrays(g, ref):
    assert (g.n_nodes, g.n_edges) == (ref.n_nodes, ref.n_edges)
    assert np.array_equal(g.edge_label, ref.edge_label)
    assert np.array_equal(g.edge_weight, ref.edge_weight)
    assert np.array_equal(g.edge_src, ref.edge_src) and np.array_equal(g.edge_dst, ref.edge_dst)


def _same_multiset(g, ref, k):
    assert (g.n_nodes, g.n_edges) == (ref.n_nodes, ref.n_edges)
    assert g.multiset() == ref.multiset()
    ek, nk = g.key_ints("edge"), g.key_ints("node")
    assert len(set(ek)) == len(ek) and len(set(nk)) == len(nk)       # every k-mer on one rank, every node owned once
    mask = (1 << (2 * (k - 1))) - 1
    for e in range(g.n_edges):
        assert nk[int(g.edge_src[e])] == ek[e] >> 2 and nk[int(g.edge_dst[e])] == ek[e] & mask


# (world, k, rc, reads): 100 reads over 3 or 5 ranks leave the last rank without reads (shards are multiples of 64 reads)
HOST_CASES = [(2, 21, True, 400), (3, 31, True, 100), (5, 40, False, 300), (8, 63, True, 700), (3, 63, False, 250), (2, 31, False, 300)]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("route", ["local", "tiles"])
@pytest.mark.parametrize("first_seen", [True, False])
@pytest.mark.parametrize("world,k,rc,n", HOST_CASES)
def test_var_reads_through_the_host_entry(oracle, monkeypatch, tmp_path, world, k, rc, n, first_seen, route):
    from katome_amd.build import GpuGraph, InputFileType, set_global_k_sizes
    monkeypatch.setenv("KATOME_DIST_ROUTE", route)
    monkeypatch.setenv("KATOME_DIST_VAR_BATCH_WINDOWS", "1500")      # several batches per rank
    path = _fastq(tmp_path, _var_reads(k, n, seed=world * 100 + k))
    set_global_k_sizes(k)
    g, rb = GpuGraph.create([path], InputFileType.Fastq, rc, 0, first_seen_order=first_seen, n_devices=world, ranks_share_device=True)
    ref = oracle.build_files([path], k, rc)
    assert rb == ref.read_bytes
    if first_seen:
        _same_arrays(g, ref)
    else:
        _same_multiset(g, ref, k)


@pytest.mark.timeout(300)
def test_var_reads_as_a_world_of_one(oracle, monkeypatch, tmp_path):
    """KATOME_FORCE_SHARDED=1: one GPU through the sharded route (the RCCL transport, a world of one)"""
    from katome_amd.build import GpuGraph, InputFileType, set_global_k_sizes
    monkeypatch.setenv("KATOME_FORCE_SHARDED", "1")
    path = _fastq(tmp_path, _var_reads(31, 300, seed=9))
    set_global_k_sizes(31)
    g, _ = GpuGraph.create([path], InputFileType.Fastq, True, 0, first_seen_order=True, n_devices=1)
    _same_arrays(g, oracle.build_files([path], 31, True))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("stage_route", ["sharded", "gather"])
def test_stages_and_shrink_after_a_var_build(oracle, monkeypatch, tmp_path, stage_route):
    from katome_amd.build import GpuContigs, GpuGraph, InputFileType, set_global_k_sizes
    monkeypatch.setenv("KATOME_DIST_STAGES", stage_route)
    path = _fastq(tmp_path, _var_reads(31, 600, seed=21, genome_len=4000, err=2e-3))
    set_global_k_sizes(31)
    oracle.set_genome_length(4000)
    g, rb = GpuGraph.create([path], InputFileType.Fastq, True, 2, first_seen_order=True, stages="dcwced",
                            original_genome_length=4000, n_devices=3, ranks_share_device=True)
    ref = oracle.build_files([path], 31, True, remove_weak_edges=2, stages="dcwced")
    assert rb == ref.read_bytes
    _same_arrays(g, ref)
    one, _ = GpuContigs.create([path], InputFileType.Fastq, True, 0, first_seen_order=True)
    many, _ = GpuContigs.create([path], InputFileType.Fastq, True, 0, first_seen_order=True, n_devices=3, ranks_share_device=True)
    assert (many.n_nodes, many.n_edges) == (one.n_nodes, one.n_edges)
    assert many.contigs() == one.contigs()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("route", ["local", "tiles"])
def test_a_rank_whose_var_reads_are_refused_fails_every_rank(oracle, monkeypatch, tmp_path, route):
    """KATOME_DIST_ADD_FAIL on rank 1: its verdict travels with the first agreement of katome_dist_add_reads_var, every rank
    returns, the build names rank 1; the next build is fine"""
    from katome_amd.build import GpuGraph, InputFileType, KatomePanic, set_global_k_sizes
    monkeypatch.setenv("KATOME_DIST_ROUTE", route)
    monkeypatch.setenv("KATOME_DIST_ADD_FAIL", "1")
    path = _fastq(tmp_path, _var_reads(21, 400, seed=2))
    set_global_k_sizes(21)
    with pytest.raises(KatomePanic) as e:
        GpuGraph.create([path], InputFileType.Fastq, True, 0, n_devices=3, ranks_share_device=True)
    assert "rank 1 of 3" in str(e.value) and "KATOME_DIST_ADD_FAIL" in str(e.value)
    monkeypatch.delenv("KATOME_DIST_ADD_FAIL")
    g, _ = GpuGraph.create([path], InputFileType.Fastq, True, 0, n_devices=3, ranks_share_device=True)
    assert g.multiset() == oracle.build_files([path], 21, True).multiset()


# ---- the C ABI itself ---------------------------------------------------------------------------------------------------
def _pack_var(reads):
    """-> (packed bytes, byte_off[n + 1], lens[n]) in katome_dev_extract_var's layout (every read from a byte boundary)"""
    out, offs = [], [0]
    for s in reads:
        b = pack_reads_ascii(np.frombuffer(s.encode(), np.uint8)[None, :]).reshape(-1).tobytes()
        out.append(b)
        offs.append(offs[-1] + len(b))
    return np.frombuffer(b"".join(out), np.uint8), np.array(offs, np.int64), np.array([len(s) for s in reads], np.int32)


def _to_dev(reads):
    packed, off, lens = _pack_var(reads)
    return (torch.from_numpy(np.concatenate([packed, np.zeros(32, np.uint8)])).cuda(), torch.from_numpy(off).cuda(),
            torch.from_numpy(lens).cuda())


def _clean(reads):
    return [s for s in reads if "N" not in s]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("first_seen", [True, False])
def test_add_reads_var_at_world_one_over_rccl(oracle, tmp_path, first_seen):
    """ShardedBuilder.add_reads_var over Comm.rccl(0, 1, 0), the reads in three calls with explicit first_window (the
    window of the rank's first read; later calls continue after the earlier ones), small batches"""
    from katome_amd import shard as ks
    k, rc = 31, True
    reads = _clean(_var_reads(k, 500, seed=13))
    path = _fastq(tmp_path, reads)
    ref = oracle.build_files([path], k, rc)
    comm = ks.Comm.rccl(0, 1, 0)
    try:
        b = ks.ShardedBuilder(comm, k, rc, 0, first_seen_order=first_seen)
        for a, e in ((0, 120), (120, 121), (121, len(reads))):
            b.add_reads_var(*_to_dev(reads[a:e]), first_window=0, batch_windows=700)
        g = b.finalize()
        assert (g.total_nodes, g.total_edges) == (ref.n_nodes, ref.n_edges)
        if first_seen:
            root = b.gather(0)
            dg = root.graph()
            assert np.array_equal(dg.edge_src.cpu().numpy(), ref.edge_src) and np.array_equal(dg.edge_dst.cpu().numpy(), ref.edge_dst)
            assert np.array_equal(dg.edge_weight.cpu().numpy().view(np.uint32), ref.edge_weight)
            assert np.array_equal(dg.edge_label.cpu().numpy(), ref.edge_label)
            del dg, root
        else:
            keys = g.edge_key.cpu().numpy().view(np.uint64).reshape(-1)
            w = g.edge_weight.cpu().numpy().view(np.uint32)
            assert sorted(zip(keys.tolist(), w.tolist())) == sorted((kmer_to_int(s), x) for s, x in ref.multiset())
        del g
        b.close()
    finally:
        comm.close()


@pytest.mark.timeout(300)
def test_a_short_read_fails_the_call(oracle):
    from katome_amd import shard as ks
    from katome_amd.build import KatomePanic
    comm = ks.Comm.rccl(0, 1, 0)
    try:
        b = ks.ShardedBuilder(comm, 31, True, 0, first_seen_order=True)
        with pytest.raises(KatomePanic) as e:
            b.add_reads_var(*_to_dev(["ACGT" * 10, "ACGT" * 7]))
        assert e.value.name == "E_SHORT_READ"
        b.close()
    finally:
        comm.close()


def _fixed_dev(reads):
    L = len(reads[0])
    packed = pack_reads_ascii(np.frombuffer("".join(reads).encode(), np.uint8).reshape(len(reads), L)).reshape(-1)
    return torch.from_numpy(np.concatenate([packed, np.zeros(32, np.uint8)])).cuda(), len(reads), L


def _mixed_reads(k):
    """150-base reads and reads of varying length, N-free, from one genome"""
    var = _clean(_var_reads(k, 300, seed=41))
    rng = np.random.default_rng(42)
    genome = "".join("ACGT"[c] for c in np.random.default_rng(41).integers(0, 4, 3000))
    fixed = [genome[a:a + 150] for a in rng.integers(0, 3000 - 150, 256)]
    return fixed, var


@pytest.mark.timeout(300)
@pytest.mark.parametrize("order", ["fixed_first", "var_first"])
def test_first_seen_order_refuses_the_mix(oracle, order):
    """the one-GPU builder's rule: in the reference's numbering a build takes reads of one length or reads of varying length"""
    from katome_amd import shard as ks
    from katome_amd.build import KatomePanic
    fixed, var = _mixed_reads(31)
    comm = ks.Comm.rccl(0, 1, 0)
    try:
        b = ks.ShardedBuilder(comm, 31, True, 0, first_seen_order=True)
        packed, n, L = _fixed_dev(fixed)
        with pytest.raises(KatomePanic) as e:
            if order == "fixed_first":
                b.add_reads(packed, 0, n, L)
                b.add_reads_var(*_to_dev(var), first_window=n * (L - 30))
            else:
                b.add_reads_var(*_to_dev(var), first_window=0)
                b.add_reads(packed, len(var), n, L)
        assert e.value.name == "E_UNSUPPORTED" and "mixed" in e.value.message
        b.close()
    finally:
        comm.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("route", ["local", "tiles", "supermers"])
@pytest.mark.parametrize("order", ["fixed_first", "var_first"])
def test_packed_key_mixes_both_kinds_of_batch(oracle, tmp_path, monkeypatch, route, order):
    """by packed key a build may take reads of one length and reads of varying length, in either order: the multiset of all of
    them.  The supermer route is planned by a batch of one length and takes nothing else: reads of varying length after it are
    refused (KATOME_E_UNSUPPORTED); before it they plan the tiles route, which the batch of one length then takes too."""
    from katome_amd import shard as ks
    from katome_amd.build import KatomePanic
    monkeypatch.setenv("KATOME_DIST_ROUTE", route)
    k = 31
    fixed, var = _mixed_reads(k)
    ref = oracle.build_files([_fastq(tmp_path, fixed + var)], k, True)
    comm = ks.Comm.rccl(0, 1, 0)
    try:
        b = ks.ShardedBuilder(comm, k, True, 0)
        packed, n, L = _fixed_dev(fixed)
        if order == "fixed_first":
            b.add_reads(packed, 0, n, L)
            if route == "supermers":
                with pytest.raises(KatomePanic) as e:
                    b.add_reads_var(*_to_dev(var), first_window=n * (L - k + 1))
                assert e.value.name == "E_UNSUPPORTED" and "supermer" in e.value.message
                b.close()
                return
            b.add_reads_var(*_to_dev(var), first_window=n * (L - k + 1), batch_windows=2000)
        else:
            b.add_reads_var(*_to_dev(var), first_window=0, batch_windows=2000)
            b.add_reads(packed, len(var), n, L)
        assert b.route in ("local", "tiles")
        g = b.finalize()
        keys = g.edge_key.cpu().numpy().view(np.uint64).reshape(-1)
        w = g.edge_weight.cpu().numpy().view(np.uint32)
        assert (g.total_nodes, g.total_edges) == (ref.n_nodes, ref.n_edges)
        assert sorted(zip(keys.tolist(), w.tolist())) == sorted((kmer_to_int(s), x) for s, x in ref.multiset())
        del g
        b.close()
    finally:
        comm.close()


_RANK_SCRIPT = r'''
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch, torch.distributed as dist
from test_gpu_dist_var import _var_reads, _clean, _to_dev
from katome_amd import shard as ks
from katome_amd.build import KatomePanic
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
out_dir, k, first_seen, short = sys.argv[2], int(sys.argv[3]), sys.argv[4] == "1", sys.argv[5] == "1"
dist.init_process_group("gloo", rank=rank, world_size=world)
try:
    torch.cuda.set_device(0)
    reads = _clean(_var_reads(k, 600, seed=31))
    first, count = ks.shard_range(len(reads), world, rank)
    mine = reads[first:first + count]
    if short and rank == world - 1:
        mine = mine + ["ACGT"]
    comm = ks.Comm.over_torch(device=0)
    b = ks.ShardedBuilder(comm, k, True, 0, first_seen_order=first_seen)
    out = {}
    try:
        b.add_reads_var(*_to_dev(mine), batch_windows=900)
        g = b.finalize()
        out.update(total_nodes=g.total_nodes, total_edges=g.total_edges, edge_key=g.edge_key.cpu().numpy().view(np.uint64),
                   weight=g.edge_weight.cpu().numpy().view(np.uint32))
        del g
        if first_seen:
            root = b.gather(0)
            if root is not None:
                dg = root.graph()
                out.update(src=dg.edge_src.cpu().numpy(), dst=dg.edge_dst.cpu().numpy(), label=dg.edge_label.cpu().numpy(),
                           root_weight=dg.edge_weight.cpu().numpy().view(np.uint32))
                del dg
    except KatomePanic as e:
        out["error"] = e.name
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    b.close()
    comm.close()
finally:
    dist.destroy_process_group()
'''


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world,k,first_seen,short", [(2, 31, True, False), (3, 40, False, False), (4, 21, True, False), (3, 31, True, True)])
def test_process_per_rank(oracle, tmp_path, world, k, first_seen, short):
    """2-4 processes (katome_amd/launch.py) sharing the card, exchanges over gloo; first_window from the ranks' allreduce.  With a
    read shorter than k on the last rank, every rank gets E_SHORT_READ."""
    from katome_amd.launch import launch_ranks
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT)
    code, _ = launch_ranks(world, [sys.executable, str(script), ROOT, str(tmp_path), str(k), "1" if first_seen else "0",
                                   "1" if short else "0"], timeout=400)
    assert code == 0
    parts = [dict(np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))) for r in range(world)]
    if short:
        assert all(str(p["error"]) == "E_SHORT_READ" for p in parts)
        return
    reads = _clean(_var_reads(k, 600, seed=31))
    ref = oracle.build_files([_fastq(tmp_path, reads)], k, True)
    merged = {}
    for p in parts:
        assert (int(p["total_nodes"]), int(p["total_edges"])) == (ref.n_nodes, ref.n_edges)
        nw = 1 if 2 * k <= 62 else 2
        rows = p["edge_key"].reshape(-1, nw)
        for row, w in zip(rows, p["weight"]):
            key = int(row[0]) if nw == 1 else (int(row[0]) << 64) | int(row[1])
            assert key not in merged
            merged[key] = int(w)
    assert sorted(merged.items()) == sorted((kmer_to_int(s), w) for s, w in ref.multiset())
    if first_seen:
        r0 = parts[0]
        assert np.array_equal(r0["src"], ref.edge_src) and np.array_equal(r0["dst"], ref.edge_dst)
        assert np.array_equal(r0["root_weight"], ref.edge_weight) and np.array_equal(r0["label"], ref.edge_label)


def test_the_entry_is_exported():
    from katome_amd import _lib
    assert hasattr(_lib.lib(), "katome_dist_add_reads_var")
