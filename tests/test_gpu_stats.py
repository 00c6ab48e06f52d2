"""CollectionStats (stats/collections.rs:137-168) and the weight spectrum computed on the device: the raw-array primitives
against numpy, device.Builder.stats() / weight_spectrum() against the pinned constants, the oracle and katome_graph_stats
after every stage, and the staged host entries that fill one entry per stage."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from helpers import pack_reads_ascii

pytestmark = pytest.mark.gpu

STAGES = "dcwced"


def _t(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def _same(a, b):
    """two CollectionStats, field for field; the averages bit for bit (one f64 division of the same u64 sums), NaN equal to NaN"""
    for f in ("node_count", "edge_count", "max_edge_weight", "max_in_degree", "max_out_degree", "incoming_vert_count", "outgoing_vert_count"):
        assert getattr(a, f) == getattr(b, f), (f, a, b)
    for f in ("avg_edge_weight", "avg_out_degree"):
        x, y = getattr(a, f), getattr(b, f)
        assert (math.isnan(x) and math.isnan(y)) or x == y, (f, a, b)


def _np_stats(src, dst, w, n_nodes):
    from katome_amd.build import CollectionStats
    E = len(src)
    outd = np.bincount(src.astype(np.int64), minlength=n_nodes) if n_nodes else np.zeros(0, np.int64)
    ind = np.bincount(dst.astype(np.int64), minlength=n_nodes) if n_nodes else np.zeros(0, np.int64)
    total = int(w.astype(np.uint64).sum())
    return CollectionStats(node_count=n_nodes, edge_count=E, max_edge_weight=int(w.max()) if E else 0,
                           avg_edge_weight=float(total) / float(E) if E else float("nan"),
                           max_in_degree=int(ind.max()) if n_nodes else 0, max_out_degree=int(outd.max()) if n_nodes else 0,
                           avg_out_degree=float(int(outd.sum())) / float(n_nodes) if n_nodes else float("nan"),
                           incoming_vert_count=int((ind == 0).sum()), outgoing_vert_count=int((outd == 0).sum()))


def _arrays(name):
    rng = np.random.default_rng(11)
    u64, u32 = np.uint64, np.uint32
    if name == "nothing":
        return np.zeros(0, u64), np.zeros(0, u64), np.zeros(0, u32), 0
    if name == "five isolated nodes":
        return np.zeros(0, u64), np.zeros(0, u64), np.zeros(0, u32), 5
    if name == "one self-loop":
        return np.array([0], u64), np.array([0], u64), np.array([7], u32), 1
    if name in ("E=1", "E=63", "E=65"):
        E = int(name[2:])
        return rng.integers(0, 10, E).astype(u64), rng.integers(0, 10, E).astype(u64), rng.integers(0, 1000, E).astype(u32), 10
    if name == "70000 parallel edges":          # degrees pass 2^16, every add of a launch hits one address; a self-loop at 2
        src = np.concatenate([np.zeros(70000, u64), np.array([2], u64)])
        dst = np.concatenate([np.ones(70000, u64), np.array([2], u64)])
        return src, dst, np.full(70001, 3, u32), 3
    if name == "random multigraph":             # the weight sum passes 2^32; the nodes from 90 000 on are named by no edge
        N, E = 100_003, 300_007
        w = rng.integers(0, 1 << 32, E, dtype=np.uint64).astype(u32)
        w[12345] = 0xFFFFFFFF
        return rng.integers(0, 90_000, E).astype(u64), rng.integers(0, 90_000, E).astype(u64), w, N
    raise KeyError(name)


@pytest.mark.parametrize("name", ["nothing", "five isolated nodes", "one self-loop", "E=1", "E=63", "E=65", "70000 parallel edges",
                                  "random multigraph"])
def test_stats_arrays_against_numpy(name):
    from katome_amd import device as kd
    src, dst, w, n_nodes = _arrays(name)
    want = _np_stats(src, dst, w, n_nodes)
    got = kd.stats_arrays(_t(src), _t(dst), _t(w), n_nodes)
    print(name, got)
    _same(got, want)
    if name == "nothing":
        assert math.isnan(got.avg_edge_weight) and math.isnan(got.avg_out_degree)
    if name == "five isolated nodes":
        assert (got.incoming_vert_count, got.outgoing_vert_count, got.avg_out_degree) == (5, 5, 0.0) and math.isnan(got.avg_edge_weight)
    if name == "70000 parallel edges":
        assert (got.max_in_degree, got.max_out_degree, got.incoming_vert_count, got.outgoing_vert_count) == (70000, 70000, 1, 1)
    if name == "random multigraph":
        assert got.avg_edge_weight * got.edge_count > 2 ** 32 and got.incoming_vert_count > 10_003
    if len(w) > 4:                                # the same weights from an address that is no multiple of 16
        shifted = _t(np.concatenate([np.zeros(1, np.uint32), w]))[1:]
        _same(kd.stats_arrays(_t(src), _t(dst), shifted, n_nodes), want)


def _spectrum_weights(kind, n_bins):
    rng = np.random.default_rng(5)
    if kind == "all 1":
        return np.ones(1_000_003, np.uint32)
    if kind == "all at or above n_bins":
        return rng.integers(n_bins, 1 << 32, 100_003, dtype=np.uint64).astype(np.uint32)
    if kind == "the last two bins":
        return np.where(rng.integers(0, 3, 100_003) == 0, n_bins - 2, n_bins - 1).astype(np.uint32)
    if kind == "uniform":
        return rng.integers(0, 2 * n_bins, 200_003).astype(np.uint32)
    if kind == "none":
        return np.zeros(0, np.uint32)
    raise KeyError(kind)


@pytest.mark.parametrize("n_bins", [2, 16, 4096, 16384])
@pytest.mark.parametrize("kind", ["all 1", "all at or above n_bins", "the last two bins", "uniform", "none"])
def test_weight_spectrum_arrays_against_numpy(monkeypatch, kind, n_bins):
    from katome_amd import device as kd
    w = _spectrum_weights(kind, n_bins)
    want = np.bincount(np.minimum(w, n_bins - 1), minlength=n_bins).astype(np.uint64)
    got = kd.weight_spectrum_arrays(_t(w), n_bins)
    assert got.dtype == np.uint64 and got.shape == (n_bins,)
    assert int(got.sum()) == len(w)
    assert np.array_equal(got, want)
    if len(w) > 4:
        assert np.array_equal(kd.weight_spectrum_arrays(_t(np.concatenate([np.zeros(3, np.uint32), w]))[3:], n_bins), want)
        monkeypatch.setenv("KATOME_SPECTRUM_PLAIN", "1")      # one LDS add per record: the form the handling is measured against
        assert np.array_equal(kd.weight_spectrum_arrays(_t(w), n_bins), want)


# ---- the builder ---------------------------------------------------------------------------------------------------------
def _fixture_builder(path, k, first_seen):
    import torch
    from katome_amd import device as kd
    from katome_amd.build import InputFileType, ingest_files
    r = ingest_files([path], InputFileType.Fastq, k)
    assert r["fixed_len"]
    packed = torch.from_numpy(np.concatenate([r["packed"], np.zeros(32, np.uint8)])).cuda()
    b = kd.Builder(k, False, first_seen_order=first_seen)
    b.count_reads(packed, r["n_reads"], r["fixed_len"], None)
    b.finalize()
    return b


@pytest.mark.parametrize("first_seen", [False, True])
@pytest.mark.parametrize("i", [0, 1, 2])
def test_builder_stats_equal_the_pinned_constants(golden_dir, i, first_seen):
    """tests/build.rs:44-90 through device.Builder.stats()"""
    from katome_amd.build import CollectionStats
    pinned = json.load(open(os.path.join(golden_dir, "pinned.json")))
    b = _fixture_builder(os.path.join(golden_dir, pinned["fixtures"][i]), pinned["k"], first_seen)
    n, e = pinned["counts"]["values"][i]
    got = b.stats()
    assert got == CollectionStats(node_count=n, edge_count=e, **pinned["pt_graph_stats"]["values"][i])
    assert int(b.weight_spectrum(64).sum()) == e
    b.close()


INPUTS = {  # k: (reverse_complement, reads, read length, genome, error rate, original_genome_length); threshold 2
    21: (True, 2500, 110, 50000, 8e-3, 3000),
    31: (True, 2500, 110, 50000, 8e-3, 3000),
    63: (False, 3000, 200, 30000, 1e-3, 4_000_000),
}
THRESHOLD = 2


class _Case:
    """one input of test_gpu_dist_stages.py, and what the oracle's PtGraph looks like after every prefix of "dcwced" """

    def __init__(self, oracle, k):
        from katome_amd.build import CollectionStats
        self.k = k
        self.rc, self.n, self.L, G, err, self.glen = INPUTS[k]
        self.ascii = oracle.synth_reads(0, self.n, self.L, G, err, 1)
        has_n = (self.ascii == ord("N")).any(axis=1)
        clean = self.ascii.copy()
        clean[clean == ord("N")] = ord("A")
        self.packed = pack_reads_ascii(clean).reshape(-1).copy()
        self.skip = has_n.astype(np.uint8)
        oracle.set_genome_length(self.glen)
        self.stats, self.spectrum = [], []
        for i in range(len(STAGES) + 1):
            ref = oracle.build_ascii(self.ascii, k, self.rc, remove_weak_edges=THRESHOLD, stages=STAGES[:i])
            self.stats.append(CollectionStats(**ref.stats))
            self.spectrum.append(np.bincount(np.minimum(ref.edge_weight, 15), minlength=16).astype(np.uint64))
        # a stale or misplaced entry cannot pass: the stages change what is counted (at k = 21 all seven entries differ; at
        # k = 63 the second remove_dead_paths finds nothing left to remove)
        assert len({s.edge_count for s in self.stats}) >= (4 if k < 40 else 3) and len({s.max_edge_weight for s in self.stats}) >= 3
        assert all(a != b for a, b in zip(self.stats[:-2], self.stats[1:-1]))


_CASES = {}


@pytest.fixture
def case(oracle, request):
    k = request.param
    if k not in _CASES:
        _CASES[k] = _Case(oracle, k)
    return _CASES[k]


def _host_stats(dg):
    """katome_graph_stats over the arrays of a device graph copied out"""
    import katome_amd
    from katome_amd import _lib
    from katome_amd.build import collection_stats
    src = dg.edge_src.cpu().numpy().view(np.uint64).copy()
    dst = dg.edge_dst.cpu().numpy().view(np.uint64).copy()
    w = dg.edge_weight.cpu().numpy().view(np.uint32).copy()
    g = _lib.Graph()
    g.n_nodes, g.n_edges = dg.n_nodes, dg.n_edges
    g.edge_src, g.edge_dst = src.ctypes.data_as(_lib.u64p), dst.ctypes.data_as(_lib.u64p)
    g.edge_weight = w.ctypes.data_as(_lib.u32p)
    st = _lib.Stats()
    assert katome_amd.lib().katome_graph_stats(C.byref(g), C.byref(st)) == 0
    return collection_stats(st)


def _device_builder(c, first_seen=True):
    from katome_amd import device as kd
    b = kd.Builder(c.k, c.rc, first_seen_order=first_seen)
    b.count_reads(_t(np.concatenate([c.packed, np.zeros(32, np.uint8)])), c.n, c.L, _t(c.skip))
    return b


@pytest.mark.parametrize("case", [21, 63], indirect=True)
def test_builder_stats_after_every_stage(case):
    from katome_amd.build import KatomePanic
    b = _device_builder(case)
    for call in (b.stats, lambda: b.weight_spectrum(16)):
        with pytest.raises(KatomePanic) as e:
            call()
        assert e.value.name == "E_ARG"
    b.finalize()
    step = {"d": b.remove_dead_paths, "c": b.standardize_contigs, "w": lambda: b.remove_weak_edges(THRESHOLD),
            "e": lambda: b.standardize_edges(case.glen, THRESHOLD)}
    for i in range(len(STAGES) + 1):
        if i:
            step[STAGES[i - 1]]()
        got = b.stats()
        print(case.k, STAGES[:i], got)
        assert got == case.stats[i], (STAGES[:i], got, case.stats[i])
        dg = b.graph()
        assert (dg.n_nodes, dg.n_edges) == (got.node_count, got.edge_count)
        _same(got, _host_stats(dg))
        del dg
        assert np.array_equal(b.weight_spectrum(16), case.spectrum[i]), STAGES[:i]
    b.close()


@pytest.mark.parametrize("case", [21, 63], indirect=True)
def test_staged_host_entry_fills_one_entry_per_stage(case):
    from katome_amd.build import GpuGraph
    g, _ = GpuGraph.create_from_packed(case.packed, case.n, case.L, skip=case.skip, reverse_complement=case.rc, k=case.k, first_seen_order=True,
                                       stages=STAGES, original_genome_length=case.glen, minimal_weight_threshold=THRESHOLD, stage_stats=True)
    assert len(g.stage_stats) == 7
    for i, got in enumerate(g.stage_stats):
        assert got == case.stats[i], (STAGES[:i], got, case.stats[i])
    _same(g.stage_stats[-1], g.stats())                     # the last entry is the graph that was copied out
    plain, _ = GpuGraph.create_from_packed(case.packed, case.n, case.L, skip=case.skip, reverse_complement=case.rc, k=case.k, first_seen_order=True,
                                           stages=STAGES, original_genome_length=case.glen, minimal_weight_threshold=THRESHOLD)
    assert not hasattr(plain, "stage_stats") and np.array_equal(plain.edge_weight, g.edge_weight)


def test_files_entry_fills_one_entry_per_stage(oracle, golden_dir):
    """katome_build_files_staged_stats through GpuGraph.create: the FASTQ fixture at k 16 on both strands (39 607 edges before 'w',
    3 after it, of weight 661 after 'e', none after the last 'd'), every prefix of "dcwced" against the oracle, and the graph
    that comes back is the one the entry without stats gives"""
    from katome_amd.build import CollectionStats, GpuGraph, InputFileType, set_global_k_sizes
    path, k, glen = os.path.join(golden_dir, "data3.txt"), 16, 2000
    set_global_k_sizes(k)
    oracle.set_genome_length(glen)
    g, rb = GpuGraph.create([path], InputFileType.Fastq, True, THRESHOLD, first_seen_order=True, stages=STAGES, original_genome_length=glen,
                            stage_stats=True)
    assert len(g.stage_stats) == len(STAGES) + 1
    refs = [oracle.build_files([path], k, True, remove_weak_edges=THRESHOLD, stages=STAGES[:i]) for i in range(len(STAGES) + 1)]
    assert len({r.stats["edge_count"] for r in refs}) >= 3 and refs[-1].stats["edge_count"] == 0
    for i, (got, ref) in enumerate(zip(g.stage_stats, refs)):
        if ref.stats["edge_count"]:
            assert got == CollectionStats(**ref.stats), (STAGES[:i], got, ref.stats)
        else:                                               # (NaN averages: equal to nothing, so field by field)
            _same(got, CollectionStats(**ref.stats))
    assert rb == refs[0].read_bytes
    plain, _ = GpuGraph.create([path], InputFileType.Fastq, True, THRESHOLD, first_seen_order=True, stages="dcw", original_genome_length=glen)
    some, _ = GpuGraph.create([path], InputFileType.Fastq, True, THRESHOLD, first_seen_order=True, stages="dcw", original_genome_length=glen,
                              stage_stats=True)
    assert not hasattr(plain, "stage_stats") and some.stage_stats == g.stage_stats[:4] and plain.n_edges == 3
    for name in ("edge_src", "edge_dst", "edge_weight", "node_key"):
        assert np.array_equal(getattr(plain, name), getattr(some, name)), name


@pytest.mark.parametrize("case", [21], indirect=True)
def test_packed_key_builder_gives_the_same_stats(case):
    from katome_amd.build import GpuGraph
    a, b = _device_builder(case, True), _device_builder(case, False)
    a.finalize(); b.finalize()
    _same(a.stats(), b.stats())
    assert a.stats() == case.stats[0]
    assert np.array_equal(a.weight_spectrum(16), b.weight_spectrum(16))
    a.close(); b.close()
    # the host entry takes a packed-key build when no stage is asked for: stats need no numbering
    g, _ = GpuGraph.create_from_packed(case.packed, case.n, case.L, skip=case.skip, reverse_complement=case.rc, k=case.k, stage_stats=True)
    assert len(g.stage_stats) == 1 and g.stage_stats[0] == case.stats[0]


def test_emptied_graph(oracle):
    """genome length = k and a threshold above every weight ("ed"): every edge and node goes; NaN averages, zero counts"""
    from katome_amd import device as kd
    from katome_amd.build import GpuGraph
    n, L, k = 600, 90, 31
    ascii_reads = oracle.synth_reads(0, n, L, 5000, 4e-3, 1)
    has_n = (ascii_reads == ord("N")).any(axis=1)
    clean = ascii_reads.copy()
    clean[clean == ord("N")] = ord("A")
    packed, skip = pack_reads_ascii(clean).reshape(-1).copy(), has_n.astype(np.uint8)
    b = kd.Builder(k, True, first_seen_order=True)
    b.count_reads(_t(np.concatenate([packed, np.zeros(32, np.uint8)])), n, L, _t(skip))
    b.finalize()
    assert b.stats().edge_count > 0
    b.standardize_edges(k, 1 << 30)
    b.remove_dead_paths()
    g, _ = GpuGraph.create_from_packed(packed, n, L, skip=skip, reverse_complement=True, k=k, first_seen_order=True, stages="ed",
                                       original_genome_length=k, minimal_weight_threshold=1 << 30, stage_stats=True)
    for got in (b.stats(), g.stage_stats[1], g.stage_stats[2]):
        assert (got.node_count, got.edge_count, got.max_edge_weight, got.max_in_degree, got.max_out_degree) == (0, 0, 0, 0, 0)
        assert (got.incoming_vert_count, got.outgoing_vert_count) == (0, 0)
        assert math.isnan(got.avg_edge_weight) and math.isnan(got.avg_out_degree)
    assert g.stage_stats[0].edge_count > 0 and not b.weight_spectrum(16).any()
    b.close()
