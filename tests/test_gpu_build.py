"""GPU parity tests proper: the HIP build path, through the C ABI, against the oracle and against the
constants the reference's own tests pin (tests/golden/pinned.json).  Integer work: bit-exact."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from helpers import int_to_kmer, kmer_to_int, pack_reads_ascii, windows_multiset  # noqa: E402


def _build_files(paths, k, rc, ft=None):
    from katome_amd.build import GpuGraph, InputFileType, set_global_k_sizes
    set_global_k_sizes(k)
    return GpuGraph.create(paths, ft if ft is not None else InputFileType.Fastq, rc, 0)


def _check_graph_consistency(g, k, distinct=True):
    """structure every build must have, whatever the input (distinct=False: BFCounter input may list a k-mer on several lines,
    which stay parallel edges as in the reference)"""
    nw = g.key_words
    ek = g.key_ints("edge")
    nk = g.key_ints("node")
    assert ek == sorted(ek) and (not distinct or len(set(ek)) == len(ek))   # ascending (distinct) k-mers
    assert len(set(nk)) == len(nk)                                   # distinct (k-1)-mers
    n_src = len(set(g.edge_src.tolist()))                            # nodes with out-edges come first, ascending,
    assert nk[:n_src] == sorted(nk[:n_src]) and nk[n_src:] == sorted(nk[n_src:])   # then the out-edge-less ones, ascending
    assert set(g.edge_src.tolist()) == set(range(n_src))
    mask = (1 << (2 * (k - 1))) - 1
    for e in range(0, g.n_edges, max(1, g.n_edges // 500)):
        assert nk[int(g.edge_src[e])] == ek[e] >> 2                   # compress_kmer halves
        assert nk[int(g.edge_dst[e])] == ek[e] & mask
    used = set(g.edge_src.tolist()) | set(g.edge_dst.tolist())
    assert used == set(range(g.n_nodes))                             # every node is an endpoint
    assert nw == (1 if 2 * k <= 62 else 2)


@pytest.mark.parametrize("i", [0, 1, 2])
def test_reference_pinned_constants(golden_dir, i):
    """tests/build.rs:27-28,44-90 through the GPU path (k=40 -> 128-bit keys)"""
    from katome_amd.build import CollectionStats
    pinned = json.load(open(os.path.join(golden_dir, "pinned.json")))
    g, read_bytes = _build_files([os.path.join(golden_dir, pinned["fixtures"][i])], pinned["k"], False)
    assert read_bytes == pinned["read_bytes"]["values"][i]
    want = pinned["pt_graph_stats"]["values"][i]
    n, e = pinned["counts"]["values"][i]
    assert g.stats() == CollectionStats(node_count=n, edge_count=e, **want)
    _check_graph_consistency(g, 40)


@pytest.mark.parametrize("k", [3, 5, 16, 31, 32, 33, 40, 63])
@pytest.mark.parametrize("rc", [False, True])
def test_fixture_multiset_equals_oracle(oracle, golden_dir, k, rc):
    """bit-exact (k-mer, weight) multiset, labels and CollectionStats vs the oracle"""
    path = os.path.join(golden_dir, "data2.txt")
    g, read_bytes = _build_files([path], k, rc)
    ref = oracle.build_files([path], k, rc)
    assert read_bytes == ref.read_bytes
    assert (g.n_nodes, g.n_edges) == (ref.n_nodes, ref.n_edges)
    assert g.multiset() == ref.multiset()
    # labels: same bytes as the oracle's compress_edge-format slots, edge for edge
    ref_by_label = {bytes(row): int(w) for row, w in zip(ref.edge_label, ref.edge_weight)}
    got_by_label = {bytes(row): int(w) for row, w in zip(g.edge_label, g.edge_weight)}
    assert got_by_label == ref_by_label
    st, rs = g.stats(), ref.stats
    assert (st.max_edge_weight, st.max_in_degree, st.max_out_degree, st.incoming_vert_count, st.outgoing_vert_count) == \
        (rs["max_edge_weight"], rs["max_in_degree"], rs["max_out_degree"], rs["incoming_vert_count"], rs["outgoing_vert_count"])
    assert abs(st.avg_edge_weight - rs["avg_edge_weight"]) < 1e-12 and abs(st.avg_out_degree - rs["avg_out_degree"]) < 1e-12
    _check_graph_consistency(g, k)


def test_derived_goldens(golden_dir):
    derived = json.load(open(os.path.join(golden_dir, "derived.json")))
    for case in derived["cases"]:
        g, _ = _build_files([os.path.join(golden_dir, case["fixture"])], case["k"], case["rc"])
        assert [g.n_nodes, g.n_edges] == case["counts"], case
        assert int(g.edge_weight.astype(np.uint64).sum()) == case["weight_sum"]


def test_multifile_and_graph_topology_vs_oracle(oracle, golden_dir):
    """multi-file = concatenation (builder.rs:152); node/edge incidence isomorphic to the oracle's graph"""
    paths = [os.path.join(golden_dir, f) for f in ("data1.txt", "data3.txt")]
    g, rb = _build_files(paths, 40, True)
    ref = oracle.build_files(paths, 40, True)
    assert rb == ref.read_bytes and g.multiset() == ref.multiset()
    # edges as (source (k-1)-mer, target (k-1)-mer) pairs must agree with the oracle's node ids up to renaming
    nk = g.key_ints("node")
    ours = sorted((nk[int(s)], nk[int(d)]) for s, d in zip(g.edge_src, g.edge_dst))
    ref_kmers = ref.kmer_strings()
    node_name = {}
    for km, s, d in zip(ref_kmers, ref.edge_src, ref.edge_dst):
        node_name.setdefault(int(s), kmer_to_int(km[:-1]))
        node_name.setdefault(int(d), kmer_to_int(km[1:]))
        assert node_name[int(s)] == kmer_to_int(km[:-1]) and node_name[int(d)] == kmer_to_int(km[1:])
    theirs = sorted((node_name[int(s)], node_name[int(d)]) for s, d in zip(ref.edge_src, ref.edge_dst))
    assert ours == theirs and len(node_name) == g.n_nodes


@pytest.mark.parametrize("k,rc", [(11, True), (12, False), (33, True), (33, False), (63, True)])
def test_variable_length_reads_and_fasta(oracle, tmp_path, k, rc):
    """the file route with reads of unequal length (FASTQ, and the same reads as multi-line FASTA) against the oracle;
    k = 33 and 63: 128-bit keys (an accepted read shorter than k is fatal in the reference, so lengths start at k)"""
    rng = np.random.default_rng(5)
    lines, fa = [], []
    for i in range(300):
        n = int(rng.integers(max(12, k), 400))
        s = "".join("ACGT"[c] for c in rng.integers(0, 4, n))
        if i % 17 == 0:
            s = s[:5] + "N" + s[6:]
        lines += ["@r%d" % i, s, "+", "I" * n]
        fa += [">r%d" % i] + [s[j:j + 60] for j in range(0, n, 60)]
    fq = tmp_path / "var.fq"
    fq.write_text("\n".join(lines) + "\n")
    faf = tmp_path / "var.fa"
    faf.write_text("\n".join(fa) + "\n")
    from katome_amd.build import InputFileType
    ref = oracle.build_files([str(fq)], k, rc)
    g, rb = _build_files([str(fq)], k, rc)
    assert rb == ref.read_bytes and g.multiset() == ref.multiset()
    assert (g.n_nodes, g.n_edges) == (ref.n_nodes, ref.n_edges)
    g2, rb2 = _build_files([str(faf)], k, rc, InputFileType.Fasta)
    ref2 = oracle.build_files([str(faf)], k, rc, file_type=0)
    assert rb2 == ref2.read_bytes == rb and g2.multiset() == ref2.multiset() == g.multiset()
    _check_graph_consistency(g, k)


def test_error_paths_on_gpu_box(golden_dir):
    from katome_amd.build import KatomePanic
    with pytest.raises(KatomePanic) as e:      # tests/build.rs:33,129-139 (fails3)
        _build_files([os.path.join(golden_dir, "data_too_short_reads")], 40, False)
    assert e.value.name == "E_PATH"
    with pytest.raises(KatomePanic) as e:      # pt_graph.rs:278
        _build_files([os.path.join(golden_dir, "data_too_short_read.txt")], 40, False)
    assert e.value.name == "E_SHORT_READ" and e.value.message == "Read is too short!"
    g, rb = _build_files([os.path.join(golden_dir, "data_too_short_read.txt")], 7, False)
    assert (rb, g.n_edges, g.n_nodes) == (7, 1, 2)


def test_empty_and_all_skipped_inputs(tmp_path):
    from katome_amd.build import GpuGraph
    empty = tmp_path / "e.fq"
    empty.write_text("")
    g, rb = _build_files([str(empty)], 31, True)
    assert (rb, g.n_edges, g.n_nodes) == (0, 0, 0)
    alln = tmp_path / "n.fq"
    alln.write_text("@a\nACGTNNNN\n+\nIIIIIIII\n")
    g, rb = _build_files([str(alln)], 5, True)
    assert (rb, g.n_edges, g.n_nodes) == (0, 0, 0)
    packed = np.zeros((4, 38), np.uint8)
    g, rb = GpuGraph.create_from_packed(packed, 4, 150, skip=np.ones(4, np.uint8), reverse_complement=True, k=31)
    assert (rb, g.n_edges) == (0, 0)


@pytest.mark.parametrize("k,rc", [(31, True), (31, False), (63, True), (4, True), (6, True)])
def test_extraction_kernel_records(oracle, k, rc):
    """extract_fixed (LDS path) record for record vs the string-level windows"""
    from katome_amd import device as kd
    from helpers import revcomp_str, words_to_int
    n, L = 777, 150
    ascii_reads = oracle.synth_reads(5, n, L, 40000, 2e-2, 3)
    has_n = (ascii_reads == ord("N")).any(axis=1)
    clean = ascii_reads.copy()
    clean[clean == ord("N")] = ord("A")
    packed = torch.from_numpy(np.ascontiguousarray(pack_reads_ascii(clean)).reshape(-1)).cuda()
    skip = torch.from_numpy(has_n.astype(np.uint8)).cuda()
    b = kd.Builder(k, rc)
    rec = b.extract_fixed(packed, n, L, skip)
    torch.cuda.synchronize()
    nw = b.nw
    got = rec.cpu().numpy().view(np.uint64).reshape(n, L - k + 1, nw)
    for r in range(0, n, 13):
        s = bytes(clean[r]).decode()
        for w in range(L - k + 1):
            v = words_to_int(got[r, w])
            if has_n[r]:
                assert got[r, w, 0] == np.uint64(0xFFFFFFFFFFFFFFFF)
                continue
            km = s[w:w + k]
            want = kmer_to_int(km)
            if rc:
                want = min(want, kmer_to_int(revcomp_str(km)))
            assert v == want, (r, w)
    b.close()


@pytest.mark.parametrize("k,rc,n,L", [(31, True, 20000, 150), (31, False, 20000, 150), (40, True, 6000, 100),
                                      (6, True, 3000, 64), (63, True, 5000, 150), (32, True, 4000, 75)])
def test_synthetic_build_equals_oracle(oracle, k, rc, n, L):
    """SURVEY 8d workload shape (N-injection included) at a size the oracle finishes in seconds"""
    from katome_amd.build import GpuGraph
    ascii_reads = oracle.synth_reads(0, n, L, 200000, 1e-3, 1)
    has_n = (ascii_reads == ord("N")).any(axis=1)
    clean = ascii_reads.copy()
    clean[clean == ord("N")] = ord("C")
    g, rb = GpuGraph.create_from_packed(pack_reads_ascii(clean).reshape(-1), n, L, skip=has_n.astype(np.uint8),
                                        reverse_complement=rc, k=k)
    ref = oracle.build_ascii(ascii_reads, k, rc)
    assert rb == ref.read_bytes == int((~has_n).sum()) * L
    assert (g.n_nodes, g.n_edges) == (ref.n_nodes, ref.n_edges)
    ref_keys = np.array(sorted(kmer_to_int(s) for s in ref.kmer_strings()), dtype=object)
    assert g.key_ints("edge") == list(ref_keys)
    assert g.multiset() == ref.multiset()
    _check_graph_consistency(g, k)


def test_c2_in_full_equals_oracle(oracle):
    """BASELINE configs[1] in full -- 1 M synthetic 150 bp reads, k=31, both strands, 1 % of the reads hold an N -- through
    the host ABI (katome_build_packed) against the oracle's sequential build: the whole edge multiset (labels in
    compress_edge format + weights), node and edge counts, read bytes and the CollectionStats the reference's tests
    compare (stats/collections.rs:137-168).  The oracle needs a couple of minutes for its 2.4e8 insertions."""
    from katome_amd.build import GpuGraph
    from katome_amd.workloads import WORKLOADS
    wl = WORKLOADS["c2"]
    ascii_reads = oracle.synth_reads(0, wl.reads, wl.read_len, wl.genome_len, wl.err_rate, wl.n_inject_percent)
    has_n = (ascii_reads == ord("N")).any(axis=1)
    clean = ascii_reads.copy()
    clean[clean == ord("N")] = ord("C")
    g, rb = GpuGraph.create_from_packed(pack_reads_ascii(clean).reshape(-1), wl.reads, wl.read_len,
                                        skip=has_n.astype(np.uint8), reverse_complement=True, k=wl.k)
    del clean
    ref = oracle.build_ascii(ascii_reads, wl.k, True)
    assert rb == ref.read_bytes == int((~has_n).sum()) * wl.read_len and 0 < int(has_n.sum()) < wl.reads // 50
    assert (g.n_nodes, g.n_edges) == (ref.n_nodes, ref.n_edges) and g.n_edges > 9_000_000

    def ordered(labels, weights):           # rows sorted as byte strings; the weights follow their labels
        v = np.ascontiguousarray(labels).view("V%d" % labels.shape[1]).reshape(-1)
        o = np.argsort(v, kind="stable")
        return np.ascontiguousarray(labels)[o], np.asarray(weights)[o]
    gl, gw = ordered(g.edge_label, g.edge_weight)
    rl, rw = ordered(ref.edge_label, ref.edge_weight)
    assert np.array_equal(gl, rl) and np.array_equal(gw.astype(np.uint32), rw.astype(np.uint32))
    st = g.stats()
    for f in ("node_count", "edge_count", "max_edge_weight", "max_in_degree", "max_out_degree", "incoming_vert_count",
              "outgoing_vert_count"):
        assert getattr(st, f) == ref.stats[f], f
    assert round(st.avg_edge_weight, 2) == round(ref.stats["avg_edge_weight"], 2)          # stats/collections.rs:71-89
    assert round(st.avg_out_degree, 2) == round(ref.stats["avg_out_degree"], 2)
    # the same input in the reference's own numbering (petgraph indices in first-seen order, pt_graph.rs:149,194): the four
    # arrays of the oracle's sequential build, index for index -- 1.1e7 edges, where the renumbering's neighbour shortcuts and
    # left-out table writes (first_seen.hip) carry most nodes
    del g, gl, gw, rl, rw
    clean = ascii_reads.copy()
    clean[clean == ord("N")] = ord("C")
    g, rb = GpuGraph.create_from_packed(pack_reads_ascii(clean).reshape(-1), wl.reads, wl.read_len,
                                        skip=has_n.astype(np.uint8), reverse_complement=True, k=wl.k, first_seen_order=True)
    del clean
    assert rb == ref.read_bytes and (g.n_nodes, g.n_edges) == (ref.n_nodes, ref.n_edges)
    assert np.array_equal(g.edge_src, ref.edge_src) and np.array_equal(g.edge_dst, ref.edge_dst)
    assert np.array_equal(g.edge_weight, ref.edge_weight) and np.array_equal(g.edge_label, ref.edge_label)


def test_high_multiplicity_and_table_growth(oracle):
    """many duplicate reads -> heavy contention on few slots; tiny table hint -> the table must grow"""
    from katome_amd import device as kd
    n, L, k = 64, 150, 31
    base = oracle.synth_reads(0, n, L, 5000, 0.0, 0)
    reps = 300
    ascii_reads = np.tile(base, (reps, 1))
    packed = torch.from_numpy(pack_reads_ascii(ascii_reads).reshape(-1)).cuda()
    b = kd.Builder(k, True, table_slots_hint=2048)
    rec = b.extract_fixed(packed, n * reps, L)
    step = (n * (L - k + 1)) * 7
    for off in range(0, rec.numel(), step):
        b.insert(rec[off:off + step])
    dg = b.finalize()
    want = windows_multiset(base, k, True)
    assert dg.n_edges == len(want)
    w = dg.edge_weight.cpu().numpy().view(np.uint32)
    keys = dg.edge_key.cpu().numpy().view(np.uint64)[:, 0]
    want_sorted = sorted((kmer_to_int(s), c * reps) for s, c in want.items())
    assert [int(x) for x in keys] == [x for x, _ in want_sorted]
    assert [int(x) for x in w] == [c for _, c in want_sorted]
    b.close()
    # 128-bit keys under the same contention (claim/publish protocol of the two-word slots)
    b = kd.Builder(40, True, table_slots_hint=2048)
    rec = b.extract_fixed(packed, n * reps, L)
    for off in range(0, rec.numel(), step * 2):
        b.insert(rec[off:off + step * 2])
    dg = b.finalize()
    want = windows_multiset(base, 40, True)
    assert dg.n_edges == len(want)
    assert int(dg.edge_weight.cpu().numpy().view(np.uint32).astype(np.uint64).sum()) == sum(want.values()) * reps
    got = {(int(h) << 64) | int(l): int(c) for (h, l), c in zip(dg.edge_key.cpu().numpy().view(np.uint64), dg.edge_weight.cpu().numpy().view(np.uint32))}
    assert got == {kmer_to_int(s): c * reps for s, c in want.items()}
    b.close()


def test_properties_at_scale():
    """1M reads x 150 bp, k=31, rc (BASELINE config 2 size): size-independent invariants"""
    from katome_amd import device as kd
    n, L, k = 1_000_000, 150, 31
    packed, skip = kd.synth_reads(0, n, L, 1_000_000, 1e-3, 1)
    b = kd.Builder(k, True)
    rec = b.extract_fixed(packed, n, L, skip)
    b.insert(rec)
    dg = b.finalize()
    W = L - k + 1
    accepted = n - int(skip[:n].sum().item())
    assert 0 < n - accepted < n // 50
    # every window was counted on both strands: sum of weights = 2 * accepted * W (odd k: no self-complement)
    assert int(dg.edge_weight.to(torch.int64).sum().item()) == 2 * accepted * W
    keys = dg.edge_key[:, 0]
    assert bool((keys[1:] > keys[:-1]).all())                        # sorted, distinct
    nodes = dg.node_key[:, 0]
    n_src = int(dg.edge_src.max().item()) + 1
    assert bool((nodes[1:n_src] > nodes[:n_src - 1]).all()) and bool((nodes[n_src + 1:] > nodes[n_src:-1]).all())
    assert int(torch.unique(nodes).numel()) == dg.n_nodes
    assert bool((nodes[dg.edge_src] == (keys >> 2)).all())
    assert bool((nodes[dg.edge_dst] == (keys & ((1 << 60) - 1))).all())
    # strand symmetry: the reverse complement of every edge is an edge with the same weight
    from katome_amd.device import rank_in_sorted
    def rc64(x):
        y = torch.zeros_like(x)
        for i in range(k):
            y |= (3 - ((x >> (2 * i)) & 3)) << (2 * (k - 1 - i))
        return y
    r = rank_in_sorted(dg.edge_key.reshape(-1), rc64(keys).contiguous(), 62, 1)
    assert bool((r >= 0).all()) and bool((dg.edge_weight[r] == dg.edge_weight).all())
    # idempotence: a second build of the same input gives the same arrays
    b2 = kd.Builder(k, True)
    b2.insert(b2.extract_fixed(packed, n, L, skip))
    dg2 = b2.finalize()
    assert dg2.n_edges == dg.n_edges and dg2.n_nodes == dg.n_nodes
    assert torch.equal(dg2.edge_key, dg.edge_key) and torch.equal(dg2.edge_weight, dg.edge_weight)
    assert torch.equal(dg2.edge_src, dg.edge_src) and torch.equal(dg2.edge_dst, dg.edge_dst)
    assert torch.equal(dg2.edge_label, dg.edge_label)
    b.close(); b2.close()


def _need_whole_gpu(need_gib=200):
    """the at-size tests need most of an MI355X.  On a card of that size with less than that free, something an earlier test
    left behind holds the memory (library cache, a builder whose close() was put off by live views): that is a failure to
    look at, not a reason to skip -- the skip hid the k=63 at-size test from the driver's run in round 2."""
    from katome_amd import device as kd
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    kd.release_cache()
    free_b, total_b = torch.cuda.mem_get_info()
    import time
    for _ in range(60):                # (a child process that has just exited -- the full-size A/B build -- gets its memory unmapped by
        if free_b >= need_gib << 30:   # the driver over some seconds: that is not something "left behind")
            return
        time.sleep(0.5)
        free_b, total_b = torch.cuda.mem_get_info()
    msg = "needs %d GiB free, has %.1f of %.1f GiB; the library still holds %r" % (
        need_gib, free_b / 2**30, total_b / 2**30, kd.cache_stats())
    if total_b >= 250 << 30:
        pytest.fail(msg)
    pytest.skip(msg)


def _close_and_release(b):
    """close a builder whose views the caller has dropped, and give the library's cache back: nothing may stay behind"""
    from katome_amd import device as kd
    import gc
    import sys
    if sys.exc_info()[0] is not None:              # a failing test: its traceback keeps the views alive; report that failure, not this
        b.close()
        kd.release_cache()
        return
    gc.collect()                                   # views kept alive by reference cycles would put the close off
    b.close()
    assert not b._h, "Builder.close() was put off: %d views of its memory are still alive" % b._views
    torch.cuda.empty_cache()
    held = kd.release_cache()
    assert held < (1 << 30), "the library still holds %.1f GiB after release_cache(): %r" % (held / 2**30, kd.cache_stats())


def _chunked_all(fn, n, step=1 << 26):
    return all(bool(fn(i, min(n, i + step))) for i in range(0, n, step))


def test_properties_at_full_c3_size():
    """BASELINE configs[2] in full (200 M reads x 150 bp, k=31, both strands; the configuration `bench.py` times), through
    the route the bench takes (tiles of 30 windows, two expansion levels): invariants that do not need the oracle --
    every window counted on both strands, ascending distinct k-mers, endpoints = the k-mer's two (k-1)-mers, dense node
    ids, strand symmetry of the weights (sampled)"""
    from katome_amd import device as kd
    from katome_amd.workloads import WORKLOADS
    wl = WORKLOADS["c3"]
    _need_whole_gpu()
    packed, _skip = kd.synth_reads(0, wl.reads, wl.read_len, wl.genome_len, wl.err_rate, 0)
    b = kd.Builder(wl.k, True, table_slots_hint=int(wl.expected_distinct_canonical() * 2.2))

    def body():                                     # the views of the result die with this frame, before the close
        step = 4 << 20
        for r0 in range(0, wl.reads, step):
            b.count_reads(packed, min(step, wl.reads - r0), wl.read_len, None, first_read=r0)
        dg = b.finalize()
        E, N, k = dg.n_edges, dg.n_nodes, wl.k
        assert 1_500_000_000 < E < 1_700_000_000 and N < E
        total = 0
        for i in range(0, E, 1 << 27):
            total += int(dg.edge_weight[i:i + (1 << 27)].to(torch.int64).sum().item())
        assert total == 2 * wl.reads * wl.windows_per_read              # k odd: no k-mer is its own reverse complement
        keys, nodes = dg.edge_key[:, 0], dg.node_key[:, 0]
        assert _chunked_all(lambda a, z: (keys[a + 1:z + 1] > keys[a:min(z, E - 1)]).all(), E - 1)
        mask = (1 << (2 * (k - 1))) - 1
        assert _chunked_all(lambda a, z: (nodes[dg.edge_src[a:z]] == (keys[a:z] >> 2)).all(), E)
        assert _chunked_all(lambda a, z: (nodes[dg.edge_dst[a:z]] == (keys[a:z] & mask)).all(), E)
        n_src = int(dg.edge_src[-1].item()) + 1                           # sources are numbered along the sorted edges
        assert _chunked_all(lambda a, z: (nodes[a + 1:min(z + 1, n_src)] > nodes[a:min(z, n_src - 1)]).all(), n_src - 1)
        assert bool((nodes[n_src + 1:] > nodes[n_src:-1]).all())         # then the nodes without out-edges, ascending
        sample = torch.randint(0, E, (1 << 22,), device=keys.device)
        x = keys[sample]
        y = torch.zeros_like(x)
        for i in range(k):
            y |= (3 - ((x >> (2 * i)) & 3)) << (2 * (k - 1 - i))
        r = kd.rank_in_sorted(dg.edge_key.reshape(-1), y.contiguous(), 2 * k, 1)
        assert bool((r >= 0).all()) and bool((dg.edge_weight[r] == dg.edge_weight[sample]).all())
        return E, N, _array_checksums(dg)
    try:
        got = body()
    finally:
        del packed, _skip
        _close_and_release(b)
    # The same build by the OTHER counting implementation -- both tile levels in the HBM atomics tables (KATOME_SORTED_TILES=0),
    # the k-mers still by sorting -- in a process of its own (the switch is read once; this process has given its memory back):
    # position-weighted 64-bit checksums of edge_key / edge_weight / edge_src / edge_dst / node_key must agree at C3 in full
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", _FULL_C3_CHILD, root], env=dict(os.environ, KATOME_SORTED_TILES="0"),
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [x for x in out.stdout.splitlines() if x.startswith("FULLC3 ")][-1].split()
    assert (int(line[1]), int(line[2])) == got[:2]
    assert [int(x) for x in line[3:]] == got[2], (line, got)


def _array_checksums(dg):
    """sum of a[i] * (2 i + 1) mod 2^64 over every word of the graph's arrays, in chunks on the device"""
    out = []
    for a in (dg.edge_key.reshape(-1), dg.edge_weight, dg.edge_src, dg.edge_dst, dg.node_key.reshape(-1)):
        total = 0
        n = a.numel()
        for i in range(0, n, 1 << 27):
            z = min(n, i + (1 << 27))
            w = torch.arange(i, z, device=a.device, dtype=torch.int64) * 2 + 1
            total = (total + int((a[i:z].to(torch.int64) * w).sum().item())) & ((1 << 64) - 1)
        out.append(total)
    return out


_FULL_C3_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch
from katome_amd import device as kd
from katome_amd.workloads import WORKLOADS
from test_gpu_build import _array_checksums
wl = WORKLOADS["c3"]
packed, _ = kd.synth_reads(0, wl.reads, wl.read_len, wl.genome_len, wl.err_rate, 0)
b = kd.Builder(wl.k, True, table_slots_hint=int(wl.expected_distinct_canonical() * 2.2))
for r0 in range(0, wl.reads, 4 << 20):
    b.count_reads(packed, min(4 << 20, wl.reads - r0), wl.read_len, None, first_read=r0)
dg = b.finalize()
c = b.counts()
assert c["tile_slots"] > 0 and c["mid_tile_slots"] > 0, c            # the tile levels really were counted in their tables
print("FULLC3", dg.n_edges, dg.n_nodes, *_array_checksums(dg))
"""


def test_properties_at_c5_share_size():
    """100 M reads of BASELINE configs[4] (k=63, 128-bit keys; three-word tiles of 90 bases + left-over windows): the same
    invariants on two-word keys"""
    from katome_amd import device as kd
    from katome_amd.workloads import WORKLOADS
    wl = WORKLOADS["c5"].scaled(100_000_000)
    _need_whole_gpu()
    packed, _skip = kd.synth_reads(0, wl.reads, wl.read_len, wl.genome_len, wl.err_rate, 0)
    b = kd.Builder(wl.k, True, table_slots_hint=int(wl.expected_distinct_canonical() * 2.2))

    def body():
        span, tiles, rest = b.tile_plan(wl.read_len)
        assert (span, tiles, rest) == (28, 3, 4) and b.tile_words(span) == 3
        step = 4 << 20
        for r0 in range(0, wl.reads, step):
            b.count_reads(packed, min(step, wl.reads - r0), wl.read_len, None, first_read=r0)
        dg = b.finalize()
        E, N, k = dg.n_edges, dg.n_nodes, wl.k
        assert E > wl.genome_len and N < E
        assert int(dg.edge_weight.to(torch.int64).sum().item()) == 2 * wl.reads * wl.windows_per_read
        SIGN = -(1 << 63)

        def less(ah, al, bh, bl):                       # unsigned 128-bit a < b on (hi, lo) int64 pairs
            return (ah < bh) | ((ah == bh) & ((al ^ SIGN) < (bl ^ SIGN)))    # (hi < 2^62: signed compare is right)
        kh, kl = dg.edge_key[:, 0], dg.edge_key[:, 1]
        nh, nl = dg.node_key[:, 0], dg.node_key[:, 1]
        assert bool(less(kh[:-1], kl[:-1], kh[1:], kl[1:]).all())
        src_h, src_l = kh >> 2, ((kl >> 2) & ((1 << 62) - 1)) | (kh << 62)
        assert bool((nh[dg.edge_src] == src_h).all()) and bool((nl[dg.edge_src] == src_l).all())
        assert bool((nh[dg.edge_dst] == (kh & ((1 << (2 * (k - 1) - 64)) - 1))).all()) and bool((nl[dg.edge_dst] == kl).all())
        n_src = int(dg.edge_src[-1].item()) + 1
        assert bool(less(nh[:n_src - 1], nl[:n_src - 1], nh[1:n_src], nl[1:n_src]).all())
        assert bool(less(nh[n_src:-1], nl[n_src:-1], nh[n_src + 1:], nl[n_src + 1:]).all())
    try:
        body()
    finally:
        del packed, _skip
        _close_and_release(b)


def test_pruning_properties_at_scale():
    """20 M reads of C3 (161 M edges) in the reference's numbering, then remove_dead_paths: what does not need the oracle --
    the arrays stay one graph (endpoints = the k-mer's (k-1)-mers, ages distinct), nothing is invented (weights and k-mers
    come from the build), and the result is a fixpoint (a second call removes nothing, in one pass)"""
    from katome_amd import device as kd
    from katome_amd.workloads import WORKLOADS
    wl = WORKLOADS["c3"].scaled(20_000_000)
    packed, _skip = kd.synth_reads(0, wl.reads, wl.read_len, wl.genome_len, wl.err_rate, 0)
    b = kd.Builder(wl.k, True, first_seen_order=True, table_slots_hint=int(wl.expected_distinct_canonical() * 2.2))

    def body():
        step = 4 << 20
        for r0 in range(0, wl.reads, step):
            b.count_reads(packed, min(step, wl.reads - r0), wl.read_len, None, first_read=r0)
        dg = b.finalize()
        E0, N0 = dg.n_edges, dg.n_nodes
        # petgraph's numbering: node indices are handed out in the order the edge list first mentions them (source before
        # target) -- the renumbering's neighbour shortcuts and left-out table writes (first_seen.hip, assign_nodes_kernel) at a size
        # where they carry nearly every node
        mention = torch.stack([dg.edge_src, dg.edge_dst], 1).reshape(-1)
        first = torch.full((N0,), 2 * E0, dtype=torch.int64, device=mention.device)
        first.scatter_reduce_(0, mention, torch.arange(2 * E0, dtype=torch.int64, device=mention.device), "amin")
        assert bool((first[1:] > first[:-1]).all()) and int(first[-1].item()) < 2 * E0
        del mention, first
        k0 = dg.edge_key[:, 0]
        assert bool((dg.node_key[:, 0][dg.edge_src] == (k0 >> 2)).all())
        assert bool((dg.node_key[:, 0][dg.edge_dst] == (k0 & ((1 << (2 * (wl.k - 1))) - 1))).all())
        built = torch.sort(dg.edge_key[:, 0].clone()).values
        weight_of = dg.edge_weight.clone()
        dg, st = b.remove_dead_paths()
        E, N, k = dg.n_edges, dg.n_nodes, wl.k
        assert st["removed_edges"] == E0 - E and st["removed_nodes"] == N0 - N and 0 < E < E0 and st["host_ms"] == 0.0
        keys, nodes = dg.edge_key[:, 0], dg.node_key[:, 0]
        assert bool((nodes[dg.edge_src] == (keys >> 2)).all()) and bool((nodes[dg.edge_dst] == (keys & ((1 << (2 * (k - 1))) - 1))).all())
        assert int(torch.unique(nodes).numel()) == N and int(torch.unique(keys).numel()) == E
        age = dg.edge_age.to(torch.int64)
        assert int(torch.unique(age).numel()) == E and int(age.max().item()) < E0
        assert bool((weight_of[age] == dg.edge_weight).all())            # an edge keeps its weight; its age is its old index
        pos = torch.searchsorted(built, keys)
        assert bool((built[pos.clamp(max=E0 - 1)] == keys).all())
        touched = torch.zeros(N, dtype=torch.bool, device=keys.device)
        touched[dg.edge_src] = True; touched[dg.edge_dst] = True
        assert bool(touched.all())                                       # no node without an edge is left behind
        dg2, st2 = b.remove_dead_paths()
        assert (dg2.n_edges, dg2.n_nodes, st2["passes"], st2["removed_edges"]) == (E, N, 1, 0)
    try:
        body()
    finally:
        del packed, _skip
        _close_and_release(b)


@pytest.mark.parametrize("k,L,rc", [(31, 150, True), (31, 150, False), (31, 100, True), (32, 75, True), (12, 51, True),
                                    (40, 103, True), (5, 20, True)])
def test_tiled_counting_equals_plain_counting(oracle, k, L, rc):
    """tiles of `span` consecutive windows, counted and expanded, give the same table as one insert per window"""
    from katome_amd import device as kd
    n = 4000
    ascii_reads = oracle.synth_reads(3, n, L, 30000, 5e-3, 2)
    has_n = (ascii_reads == ord("N")).any(axis=1)
    clean = ascii_reads.copy()
    clean[clean == ord("N")] = ord("T")
    packed = torch.from_numpy(pack_reads_ascii(clean).reshape(-1).copy()).cuda()
    skip = torch.from_numpy(has_n.astype(np.uint8)).cuda()
    plain = kd.Builder(k, rc)
    plain.insert(plain.extract_fixed(packed, n, L, skip))
    ek0, ew0 = plain.edges()
    tiled = kd.Builder(k, rc, table_slots_hint=4096)
    span = tiled.tile_span(L)
    W = L - k + 1
    assert span == max([s for s in range(2, 33) if W % s == 0 and k + s - 1 <= 63] + [1])
    if span == 1:
        pytest.skip("no span divides the windows of this read length")
    half = (n // 2 // 64) * 64
    for first, cnt in ((0, half), (half, n - half)):
        tiled.insert_tiles(tiled.extract_tiles(packed, cnt, L, span, skip, first_read=first), span)
    ek1, ew1 = tiled.edges()
    torch.cuda.synchronize()
    assert torch.equal(ek0, ek1) and torch.equal(ew0, ew1)
    ref = oracle.build_ascii(ascii_reads, k, rc)
    assert ek1.shape[0] == ref.n_edges
    # the multi-GPU route: tiles -> (k-mer, weight) records -> weighted insert
    t2 = kd.Builder(k, rc)
    t2.insert_tiles(t2.extract_tiles(packed, n, L, span, skip), span)
    keys, weights = t2.expand_tiles()
    t3 = kd.Builder(k, rc)
    t3.insert(keys.clone(), weights.clone())
    ek2, ew2 = t3.edges()
    assert torch.equal(ek0, ek2) and torch.equal(ew0, ew2)
    for b in (plain, tiled, t2, t3):
        b.close()


def test_plain_path_when_tiles_disabled(oracle, golden_dir, monkeypatch):
    monkeypatch.setenv("KATOME_NO_TILES", "1")
    path = os.path.join(golden_dir, "data3.txt")
    g, _ = _build_files([path], 31, True)
    assert g.multiset() == oracle.build_files([path], 31, True).multiset()


@pytest.mark.parametrize("k,rc", [(31, False), (31, True), (40, True), (6, True)])
def test_bfcounter_input(oracle, golden_dir, tmp_path, k, rc):
    """InputFileType::BFCounter through the GPU path vs the oracle's create_bfc restatement"""
    from katome_amd.build import InputFileType
    import random
    path = os.path.join(golden_dir, "data3.txt")
    base = oracle.build_files([path], k, False)
    rng = random.Random(k)
    comp = str.maketrans("ACGT", "TGCA")
    lines = []
    seen = set()
    for km, w in base.multiset():            # one line per strand pair, orientation picked at random (as BFCounter does)
        r = km.translate(comp)[::-1]
        if min(km, r) in seen:
            continue
        seen.add(min(km, r))
        lines.append("%s\t%d" % (km if rng.random() < 0.5 else r, w + rng.randrange(3)))
    # the reference adds every line with add_edge, unconditionally (pt_graph.rs:200-213): a k-mer listed twice -- in the
    # same orientation or as its reverse complement -- stays as parallel edges, and so it must here
    lines += [lines[0], lines[3], "%s\t%d" % (lines[5].split("\t")[0].translate(comp)[::-1], 7)]
    if k % 2 == 0:
        pal = ("ACGT" * k)[:k // 2]
        lines.append("%s\t5" % (pal + pal.translate(comp)[::-1]))      # its own reverse complement: two parallel edges with rc
    bfc = tmp_path / "kmers.bfc"
    bfc.write_text("\n".join(lines) + "\n")
    for thr in (0, 2):
        g, rb = _build_files([str(bfc)], k, rc, InputFileType.BFCounter) if thr == 0 else (None, None)
        if thr:
            from katome_amd.build import GpuGraph, set_global_k_sizes
            set_global_k_sizes(k)
            g, rb = GpuGraph.create([str(bfc)], InputFileType.BFCounter, rc, thr)
        ref = oracle.build_bfc([str(bfc)], k, rc, thr)
        assert rb == ref.read_bytes
        assert g.multiset() == ref.multiset()
        assert (g.n_nodes, g.n_edges) == (ref.n_nodes, ref.n_edges)
        assert len(g.multiset()) > len(set(km for km, _ in g.multiset()))       # parallel edges really are there
        _check_graph_consistency(g, k, distinct=False)


def _fixture_on_device(golden_dir, name, k):
    from katome_amd.build import InputFileType, ingest_files
    r = ingest_files([os.path.join(golden_dir, name)], InputFileType.Fastq, k)
    assert r["fixed_len"] == 100
    return torch.from_numpy(r["packed"].copy()).cuda(), r["n_reads"], r["fixed_len"]


@pytest.mark.parametrize("i", [0, 1, 2])
def test_pinned_remove_weak_edges_on_gpu(golden_dir, i):
    """tests/pruner.rs:37-169 through the GPU path: the threshold is applied when the edges leave the table"""
    from katome_amd import device as kd
    pinned = json.load(open(os.path.join(golden_dir, "pinned.json")))
    p = pinned["remove_weak_edges"]
    packed, n, L = _fixture_on_device(golden_dir, pinned["fixtures"][i], 40)
    b = kd.Builder(40, False)
    b.insert(b.extract_fixed(packed, n, L))
    b.remove_weak_edges(p["thresholds"][i])
    dg = b.finalize()
    assert [dg.n_nodes, dg.n_edges] == p["counts"][i]
    b.close()


@pytest.mark.parametrize("k,rc,thr", [(31, True, 2), (31, True, 5), (12, False, 3), (40, True, 2), (6, True, 40)])
def test_remove_weak_edges_equals_oracle(oracle, k, rc, thr):
    from katome_amd import device as kd
    n, L = 3000, 150
    ascii_reads = oracle.synth_reads(0, n, L, 20000, 1e-2, 0)
    packed = torch.from_numpy(pack_reads_ascii(ascii_reads).reshape(-1).copy()).cuda()
    b = kd.Builder(k, rc)
    span = b.tile_span(L)
    if span > 1:
        b.insert_tiles(b.extract_tiles(packed, n, L, span), span)
    else:
        b.insert(b.extract_fixed(packed, n, L))
    b.remove_weak_edges(thr)
    dg = b.finalize()
    # reference: build, then Clean::remove_weak_edges(thr) (edges kept iff weight >= thr; isolated vertices dropped)
    full = oracle.build_ascii(ascii_reads, k, rc)
    want = sorted((kmer_to_int(s), w) for s, w in full.multiset() if w >= thr)
    nw = dg.key_words
    ek = dg.edge_key.cpu().numpy().view(np.uint64).reshape(-1, nw)
    keys = [int(r[0]) if nw == 1 else (int(r[0]) << 64) | int(r[1]) for r in ek]
    assert list(zip(keys, dg.edge_weight.cpu().numpy().view(np.uint32).tolist())) == want
    mask = (1 << (2 * (k - 1))) - 1
    assert dg.n_nodes == len({x >> 2 for x, _ in want} | {x & mask for x, _ in want})
    assert 0 < len(want) < full.n_edges
    b.close()


@pytest.mark.parametrize("k,rc", [(4, True), (6, True), (7, False), (31, True), (32, True), (40, True)])
def test_low_complexity_reads(oracle, tmp_path, k, rc):
    """homopolymers, short tandem repeats and reverse-palindromes: self-loops (a (k-1)-mer that is its own
    successor), k-mers equal to their reverse complement (even k), (k-1)-mers equal to their reverse complement
    (odd k), heavy multiplicity -- against the oracle's restatement of the reference"""
    L = 96
    seqs = ["A" * L, "T" * L, "AC" * (L // 2), "ACGT" * (L // 4), "AATT" * (L // 4), "G" * 40 + "C" * 56,
            ("ACGTTGCA" * 12)[:L], ("AAAAC" * 20)[:L], ("AT" * 48), ("GATC" * 24)]
    lines = []
    for rep in range(7):
        for i, s in enumerate(seqs):
            lines += ["@r%d_%d" % (rep, i), s, "+", "I" * L]
    fq = tmp_path / "lowc.fq"
    fq.write_text("\n".join(lines) + "\n")
    g, rb = _build_files([str(fq)], k, rc)
    ref = oracle.build_files([str(fq)], k, rc)
    assert rb == ref.read_bytes
    assert g.multiset() == ref.multiset()
    assert (g.n_nodes, g.n_edges) == (ref.n_nodes, ref.n_edges)
    st, rs = g.stats(), ref.stats
    assert (st.max_edge_weight, st.max_in_degree, st.max_out_degree, st.incoming_vert_count, st.outgoing_vert_count) == \
        (rs["max_edge_weight"], rs["max_in_degree"], rs["max_out_degree"], rs["incoming_vert_count"], rs["outgoing_vert_count"])
    _check_graph_consistency(g, k)


def _assert_same_as_reference_order(g, ref):
    """edge for edge, node id for node id: the arrays the reference's petgraph would hold"""
    assert (g.n_nodes, g.n_edges) == (ref.n_nodes, ref.n_edges)
    assert np.array_equal(g.edge_label, ref.edge_label)          # same edge at every index
    assert np.array_equal(g.edge_weight, ref.edge_weight)
    assert np.array_equal(g.edge_src, ref.edge_src) and np.array_equal(g.edge_dst, ref.edge_dst)


@pytest.mark.parametrize("name,k,rc", [("data1.txt", 40, False), ("data2.txt", 40, False), ("data3.txt", 40, True),
                                       ("data2.txt", 31, True), ("data3.txt", 31, False), ("data2.txt", 16, True),
                                       ("data2.txt", 63, True), ("data3.txt", 6, True)])
def test_first_seen_order_fixtures(oracle, golden_dir, name, k, rc):
    """KATOME_FLAG_FIRST_SEEN_ORDER: petgraph's own edge and node numbering (pt_graph.rs:149,194), through plain
    counting (k=40, 63), one-level tiles (k=31: span 14, k=16: span 17 -> ...) and low k with heavy multiplicity"""
    from katome_amd.build import GpuGraph, InputFileType, set_global_k_sizes
    path = os.path.join(golden_dir, name)
    set_global_k_sizes(k)
    g, rb = GpuGraph.create([path], InputFileType.Fastq, rc, 0, first_seen_order=True)
    ref = oracle.build_files([path], k, rc)
    assert rb == ref.read_bytes
    _assert_same_as_reference_order(g, ref)


@pytest.mark.parametrize("k,rc,n,L,npct", [(31, True, 6000, 150, 1), (31, False, 6000, 150, 0), (12, True, 3000, 51, 2),
                                           (40, True, 4000, 103, 1), (33, True, 2500, 92, 0), (5, True, 500, 36, 0)])
def test_first_seen_order_synthetic(oracle, k, rc, n, L, npct):
    """two-level tiles (L=150, k=31: span 30 -> 6), other spans, plain counting, skipped reads, several batches"""
    from katome_amd import device as kd
    ascii_reads = oracle.synth_reads(0, n, L, 40000, 3e-3, npct)
    has_n = (ascii_reads == ord("N")).any(axis=1)
    clean = ascii_reads.copy()
    clean[clean == ord("N")] = ord("A")
    packed = torch.from_numpy(pack_reads_ascii(clean).reshape(-1).copy()).cuda()
    skip = torch.from_numpy(has_n.astype(np.uint8)).cuda()
    b = kd.Builder(k, rc, first_seen_order=True, table_slots_hint=1 << 16)      # small tables: growth on the way
    span = b.tile_span(L)
    step = 1024
    for r0 in range(0, n, step):
        nr = min(step, n - r0)
        if span > 1:
            b.insert_tiles(b.extract_tiles(packed, nr, L, span, skip, first_read=r0), span)
        else:
            b.insert(b.extract_fixed(packed, nr, L, skip, first_read=r0))
    dg = b.finalize()
    ref = oracle.build_ascii(ascii_reads, k, rc)
    assert (dg.n_nodes, dg.n_edges) == (ref.n_nodes, ref.n_edges)
    assert np.array_equal(dg.edge_label.cpu().numpy(), ref.edge_label)
    assert np.array_equal(dg.edge_weight.cpu().numpy().view(np.uint32), ref.edge_weight)
    assert np.array_equal(dg.edge_src.cpu().numpy().view(np.uint64), ref.edge_src)
    assert np.array_equal(dg.edge_dst.cpu().numpy().view(np.uint64), ref.edge_dst)
    b.close()


@pytest.mark.parametrize("k,rc", [(31, True), (40, False)])
def test_first_seen_order_when_most_nodes_have_no_out_edge(oracle, k, rc):
    """reads of exactly k bases: every read is one edge between two nodes nothing continues, so the nodes without out-edges
    outnumber the room the node numbering keeps behind the sources (node keys and first touches are re-housed) and the
    targets set aside by the merge outnumber their buffer (the collecting pass runs instead) -- node_ids.hip node_ids_t"""
    from katome_amd import device as kd
    n = 160_000
    rng = np.random.default_rng(k)
    ascii_reads = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(n, k))]
    ascii_reads[1::5] = ascii_reads[0:-1:5][:len(ascii_reads[1::5])]              # some reads twice: weights above 1
    packed = torch.from_numpy(pack_reads_ascii(ascii_reads).reshape(-1).copy()).cuda()
    b = kd.Builder(k, rc, first_seen_order=True, table_slots_hint=1 << 19)
    b.insert(b.extract_fixed(packed, n, k, None, first_read=0))
    dg = b.finalize()
    ref = oracle.build_ascii(ascii_reads, k, rc)
    assert (dg.n_nodes, dg.n_edges) == (ref.n_nodes, ref.n_edges) and dg.n_nodes > 1.9 * dg.n_edges * 0.95
    assert np.array_equal(dg.edge_weight.cpu().numpy().view(np.uint32), ref.edge_weight)
    assert np.array_equal(dg.edge_src.cpu().numpy().view(np.uint64), ref.edge_src)
    assert np.array_equal(dg.edge_dst.cpu().numpy().view(np.uint64), ref.edge_dst)
    assert np.array_equal(dg.edge_label.cpu().numpy(), ref.edge_label)
    b.close()


_AB_SCRIPT = r"""
import sys, hashlib, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import pack_reads_ascii
from oracle import oracle as o
from katome_amd import device as kd
for first_seen in (False, True):
    reads = o.synth_reads(5, 5000, 150, 30000, 3e-3, 0)
    packed = torch.from_numpy(pack_reads_ascii(reads).reshape(-1).copy()).cuda()
    b = kd.Builder(31, True, first_seen_order=first_seen, table_slots_hint=1 << 16)
    b.count_reads(packed, 5000, 150, None, first_read=0)
    dg = b.finalize()
    h = hashlib.sha256()
    for t in (dg.edge_key, dg.edge_weight, dg.edge_src, dg.edge_dst, dg.node_key, dg.edge_label):
        h.update(t.cpu().numpy().tobytes())
    print("AB", int(first_seen), dg.n_nodes, dg.n_edges, h.hexdigest())
    b.close()
"""


def test_round_one_paths_give_the_same_arrays(tmp_path):
    """the A/B switches: edge-by-edge target look-up, node sort in first-seen builds, all radix passes --
    each in a process of its own (the switches are read once), byte for byte against the default paths"""
    import subprocess
    script = tmp_path / "ab.py"
    script.write_text(_AB_SCRIPT)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(extra):
        env = dict(os.environ, **extra)
        out = subprocess.run([sys.executable, str(script), root], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        return sorted(line for line in out.stdout.splitlines() if line.startswith("AB "))
    want = run({})
    assert len(want) == 2
    # (KATOME_SORTED_COUNT=2: the last level counted by sorting however small the input -- by default only from 4 M records on)
    for extra in ({"KATOME_DST_RANK": "1"}, {"KATOME_SORT_NODES": "1"}, {"KATOME_FULL_SORT": "1"},
                  {"KATOME_DST_RANK": "1", "KATOME_SORT_NODES": "1"}, {"KATOME_SORTED_COUNT": "2"}, {"KATOME_SORTED_COUNT": "0"},
                  {"KATOME_RUN_SORT": "1"},         # (the run sort staged in LDS instead of by wave shuffles)
                  # the tile levels: all three by sorting (the default from 4 M records on), the big tiles in their table, both in tables
                  {"KATOME_SORTED_COUNT": "2", "KATOME_SORTED_TILES": "1"}, {"KATOME_SORTED_COUNT": "2", "KATOME_SORTED_TILES": "0"},
                  {"KATOME_SORTED_COUNT": "2", "KATOME_MID_SPAN": "10"},
                  # the first partition pass of a level counts its digits itself instead of the records kernel on the way; the passes'
                  # tiles in plain order
                  {"KATOME_SORTED_COUNT": "2", "KATOME_FUSED_HIST": "0"}, {"KATOME_SORTED_COUNT": "2", "KATOME_XCD_TILES": "0"},
                  # the k-mers counted in 8-byte LDS slots, one visit per record (lds_count.hip lds_count_packed_kernel; by default only
                  # where a group would take two visits), and never
                  {"KATOME_SORTED_COUNT": "2", "KATOME_LC_PACKED": "2"}, {"KATOME_SORTED_COUNT": "2", "KATOME_LC_PACKED": "0"},
                  # the tile levels' two-word keys whole in the LDS slots (lds_count_full_kernel; by default a sample decides), and never
                  {"KATOME_SORTED_COUNT": "2", "KATOME_LC_FULL": "1"}, {"KATOME_SORTED_COUNT": "2", "KATOME_LC_FULL": "0"}):
        assert run(extra) == want, extra


_PACKED_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import pack_reads_ascii
from oracle import oracle as o
from katome_amd import device as kd
for k, rc, L, n, many in ((31, True, 150, 4000, 0), (31, False, 100, 3000, 0), (21, True, 60, 5000, 0), (16, False, 40, 3000, 0), (31, True, 40, 2000, 70000),
                          (30, False, 64, 2500, 0), (30, True, 64, 2500, 0)):
    reads = o.synth_reads(k + n, n, L, 20000, 2e-3, 0)
    if many:                                   # one read `many` times: a k-mer whose count does not fit the slot's 16 bits
        reads = np.concatenate([reads, np.repeat(reads[:1], many, axis=0)])
    packed = torch.from_numpy(pack_reads_ascii(reads).reshape(-1).copy()).cuda()
    b = kd.Builder(k, rc)
    b.count_reads(packed, len(reads), L, None, first_read=0)
    dg = b.finalize()
    ref = o.build_ascii(reads, k, rc)
    lab = dg.edge_label.cpu().numpy().reshape(dg.n_edges, -1)
    got = sorted((bytes(r), int(w)) for r, w in zip(lab, dg.edge_weight.cpu().numpy().view(np.uint32)))
    want = sorted((bytes(r), int(w)) for r, w in zip(ref.edge_label, ref.edge_weight))
    print("PACKED", k, int(rc), many, int((dg.n_nodes, dg.n_edges) == (ref.n_nodes, ref.n_edges) and got == want), max(w for _, w in want))
    b.close()
"""


def test_kmers_counted_in_eight_byte_lds_slots(tmp_path):
    """lds_count_packed_kernel (lds_count.hip): the k-mer level's records counted in one visit -- a slot is the low 48 bits of the k-mer's
    (bijective) hash and a 16-bit count, the read-out inverts the hash.  Forced at small sizes (KATOME_LC_PACKED=2) against the
    oracle: both strand modes, k with one-word keys, a k-mer seen 70 001 times (the count does not fit: the library says so under
    KATOME_LC_TRACE and counts with the 12-byte slots), and even k with both strands, which stays with the 12-byte slots"""
    import subprocess
    script = tmp_path / "packed.py"
    script.write_text(_PACKED_SCRIPT)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, KATOME_SORTED_COUNT="2", KATOME_LC_PACKED="2", KATOME_LC_TRACE="1")
    out = subprocess.run([sys.executable, str(script), root], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    rows = [line.split() for line in out.stdout.splitlines() if line.startswith("PACKED ")]
    assert len(rows) == 7 and all(r[4] == "1" for r in rows), rows
    assert out.stderr.count("8-byte slots, 1 visit(s) per record: code 0") >= 5, out.stderr[-800:]        # (levels of one-word tiles take them too)
    assert out.stderr.count("a count beyond 16 bits") == 1 and int(rows[4][5]) > 0xFFFF, out.stderr[-800:]


_FULL_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import pack_reads_ascii
from oracle import oracle as o
from katome_amd import device as kd
SALT = 0x9E3779B97F4A7C15
salt_bases = np.frombuffer(b"ACGT", np.uint8)[[(SALT >> (2 * (31 - i))) & 3 for i in range(32)]]
for k, rc, L, n, salted in ((31, True, 150, 4000, 0), (31, False, 150, 3000, 1), (40, True, 150, 3000, 0), (40, False, 120, 3000, 0), (63, True, 150, 3000, 0),
                            (47, True, 100, 3000, 0), (33, False, 64, 2500, 0)):
    reads = o.synth_reads(k + n, n, L, 20000, 2e-3, 0)
    if salted:              # the last 32 bases of a read's first tile (k + span - 1 = 60 bases) spell the salt: that tile cannot be stored
        reads[:40, 28:60] = salt_bases
    packed = torch.from_numpy(pack_reads_ascii(reads).reshape(-1).copy()).cuda()
    b = kd.Builder(k, rc)
    b.count_reads(packed, len(reads), L, None, first_read=0)
    dg = b.finalize()
    ref = o.build_ascii(reads, k, rc)
    lab = dg.edge_label.cpu().numpy().reshape(dg.n_edges, -1)
    got = sorted((bytes(r), int(w)) for r, w in zip(lab, dg.edge_weight.cpu().numpy().view(np.uint32)))
    want = sorted((bytes(r), int(w)) for r, w in zip(ref.edge_label, ref.edge_weight))
    print("FULL", k, int(rc), salted, int((dg.n_nodes, dg.n_edges) == (ref.n_nodes, ref.n_edges) and got == want))
    b.close()
"""


def test_two_word_keys_counted_with_whole_keys_in_the_lds_slots(tmp_path):
    """lds_count_full_kernel (lds_count.hip): two-word keys -- the tiles of k <= 31, the k-mers of k = 32..63 -- counted in LDS slots that
    hold the whole key, claimed word by word.  Forced at small sizes (KATOME_LC_FULL=1; by default a sample of 256 groups decides)
    against the oracle: both strand modes, even and odd k, tiles whose second word equals the salt that marks "not set" (the level
    falls back to the fingerprint slots: code 7 under KATOME_LC_TRACE)"""
    import subprocess
    script = tmp_path / "full.py"
    script.write_text(_FULL_SCRIPT)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for per in ("7", "4"):               # (the table of 7168 slots and the one of 4096 for groups of few distinct keys)
        env = dict(os.environ, KATOME_SORTED_COUNT="2", KATOME_LC_FULL="1", KATOME_LC_FULL_PER=per, KATOME_LC_TRACE="1")
        out = subprocess.run([sys.executable, str(script), root], env=env, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
        rows = [line.split() for line in out.stdout.splitlines() if line.startswith("FULL ")]
        assert len(rows) == 7 and all(r[4] == "1" for r in rows), rows
        assert out.stderr.count("whole keys in the slots (%s per thread): code 0" % per) >= 5, out.stderr[-1500:]
        assert out.stderr.count("whole keys in the slots (%s per thread): code 7" % per) >= 1, out.stderr[-1500:]
        # (the tile levels of k >= 32 are three-word keys: lds_count_full3_kernel, tables of 5 or 3 slots per thread)
        assert out.stderr.count("whole three-word keys in the slots (%s per thread): code 0" % ("5" if per == "7" else "3")) >= 4, out.stderr[-1500:]


_KEPT_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import pack_reads_ascii
from oracle import oracle as o
from katome_amd import device as kd
n, L, k = 6000, 150, 31
reads = o.synth_reads(11, n, L, 25000, 4e-3, 3)
has_n = (reads == ord("N")).any(axis=1)
clean = reads.copy()
clean[clean == ord("N")] = ord("A")
packed = torch.from_numpy(pack_reads_ascii(clean).reshape(-1).copy()).cuda()
skip = torch.from_numpy(has_n.astype(np.uint8)).cuda()
ref = o.build_ascii(reads, k, True)
want = {bytes(row): int(w) for row, w in zip(ref.edge_label, ref.edge_weight)}
for batch, plain in ((100, False), (100, True), (6000, False)):
    b = kd.Builder(k, True, table_slots_hint=1 << 14)
    for i, r0 in enumerate(range(0, n, batch)):
        if plain and i % 7 == 3:     # a batch counted window by window in between: its records wait with the tiles' (left-over windows do the same)
            b.insert(b.extract_fixed(packed, min(batch, n - r0), L, skip, first_read=r0))
        else:
            b.count_reads(packed, min(batch, n - r0), L, skip, first_read=r0)
    dg = b.finalize()
    c = b.counts()
    lab = dg.edge_label.cpu().numpy().reshape(dg.n_edges, -1)
    got = {bytes(row): int(w) for row, w in zip(lab, dg.edge_weight.cpu().numpy())}
    print("KEPT", batch, int(plain), dg.n_edges, int(len(got) == dg.n_edges and got == want), c["tile_slots"], c["kmer_slots"])
    b.close()
# the reference's numbering: the tiles are kept as TAGGED records; array for array against the oracle's petgraph
ref_fs = o.build_ascii(reads, k, True)
for batch in (100, 6000):
    b = kd.Builder(k, True, first_seen_order=True, table_slots_hint=1 << 14)
    for r0 in range(0, n, batch):
        b.count_reads(packed, min(batch, n - r0), L, skip, first_read=r0)
    dg = b.finalize()
    c = b.counts()
    lab = dg.edge_label.cpu().numpy().reshape(dg.n_edges, -1)
    same = (dg.n_nodes, dg.n_edges) == (ref_fs.n_nodes, ref_fs.n_edges) and np.array_equal(lab, ref_fs.edge_label) and \
        np.array_equal(dg.edge_weight.cpu().numpy(), ref_fs.edge_weight) and np.array_equal(dg.edge_src.cpu().numpy(), ref_fs.edge_src) and \
        np.array_equal(dg.edge_dst.cpu().numpy(), ref_fs.edge_dst)
    print("SEEN", batch, dg.n_edges, int(same), c["tile_slots"], c["kmer_slots"])
    b.close()
# no read skipped: katome_dev_count_tiles makes the records where they are kept -- all batches; then with a skip array (of zeros)
# for every third batch, whose records go through the buffer and the copy, and the two-call boundary in between
reads2 = o.synth_reads(12, n, L, 25000, 4e-3, 0)
packed2 = torch.from_numpy(pack_reads_ascii(reads2).reshape(-1).copy()).cuda()
none_skipped = torch.zeros(n, dtype=torch.uint8, device="cuda")
ref2 = o.build_ascii(reads2, k, True)
want2 = {bytes(row): int(w) for row, w in zip(ref2.edge_label, ref2.edge_weight)}
for mixed in (False, True):
    b = kd.Builder(k, True, table_slots_hint=1 << 14)
    span = b.tile_plan(L)[0]
    for i, r0 in enumerate(range(0, n, 250)):
        if mixed and i % 3 == 1:
            b.count_tiles(packed2, 250, L, span, none_skipped, first_read=r0)
        elif mixed and i % 3 == 2:
            b.insert_tiles(b.extract_tiles(packed2, 250, L, span, None, first_read=r0), span)
        else:
            b.count_tiles(packed2, 250, L, span, None, first_read=r0)
    dg = b.finalize()
    c = b.counts()
    lab = dg.edge_label.cpu().numpy().reshape(dg.n_edges, -1)
    got = {bytes(row): int(w) for row, w in zip(lab, dg.edge_weight.cpu().numpy())}
    print("INPLACE", int(mixed), dg.n_edges, int(len(got) == dg.n_edges and got == want2), c["tile_slots"], c["kmer_slots"])
    b.close()
"""


_WIDE_TILES_SCRIPT = r"""
import sys, hashlib, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import pack_reads_ascii
from oracle import oracle as o
from katome_amd import device as kd
# (k, read length, reverse complement): k = 40 at 150 bp -- the reference's example setting -- and k = 63 (BASELINE config 5) make
# THREE-word tiles of two-word k-mers; k = 33 at 50 bp one two-word tile of two-word k-mers; k = 50 at 100 bp three-word tiles and
# left-over windows; k = 36 without the reverse strand
for k, L, rc in ((40, 150, True), (63, 150, True), (33, 50, True), (50, 100, True), (36, 150, False)):
    n = 4000
    reads = o.synth_reads(20 + k, n, L, 20000, 4e-3, 3)
    has_n = (reads == ord("N")).any(axis=1)
    clean = reads.copy()
    clean[clean == ord("N")] = ord("A")
    packed = torch.from_numpy(pack_reads_ascii(clean).reshape(-1).copy()).cuda()
    skip = torch.from_numpy(has_n.astype(np.uint8)).cuda()
    ref = o.build_ascii(reads, k, rc)
    want = {bytes(row): int(w) for row, w in zip(ref.edge_label, ref.edge_weight)}
    for batch in (500, 4000):
        b = kd.Builder(k, rc, table_slots_hint=1 << 14)
        span, tiles, rest = b.tile_plan(L)
        for r0 in range(0, n, batch):
            # (alternately with and without a skip array: without one the records are made where they are kept)
            use_skip = skip if (r0 // batch) % 2 == 0 or has_n[r0:r0 + batch].any() else None
            b.count_reads(packed, min(batch, n - r0), L, use_skip, first_read=r0)
        dg = b.finalize()
        c = b.counts()
        lab = dg.edge_label.cpu().numpy().reshape(dg.n_edges, -1)
        got = {bytes(row): int(w) for row, w in zip(lab, dg.edge_weight.cpu().numpy())}
        h = hashlib.sha256()
        for t in (dg.edge_key, dg.edge_weight, dg.edge_src, dg.edge_dst, dg.node_key, dg.edge_label):
            h.update(t.cpu().numpy().tobytes())
        ok = len(got) == dg.n_edges and got == want and (dg.n_nodes, dg.n_edges) == (ref.n_nodes, ref.n_edges)
        print("W3", k, L, batch, b.tile_words(span), dg.n_edges, int(ok), "tables" if (c["tile_slots"] or c["mid_tile_slots"] or c["kmer_slots"]) else "sorted", h.hexdigest())
        b.close()
"""


def test_three_word_tiles_and_two_word_kmers_counted_by_sorting(tmp_path):
    """round 4: the tile levels of k = 32..63 at 150 bp (three-word tiles: the reference's example k = 40, BASELINE config 5's k = 63)
    and of two-word tiles over two-word k-mers are counted by sorting like the headline shape's -- no table is touched -- and give the
    oracle's graph; the same builds with the round-3 rule (KATOME_SORTED_WIDE=0: those levels in the HBM tables) byte for byte"""
    import subprocess
    script = tmp_path / "wide.py"
    script.write_text(_WIDE_TILES_SCRIPT)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(extra):
        env = dict(os.environ, KATOME_SORTED_COUNT="2", **extra)
        out = subprocess.run([sys.executable, str(script), root], env=env, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
        return [line.split() for line in out.stdout.splitlines() if line.startswith("W3 ")]
    new, old = run({}), run({"KATOME_SORTED_WIDE": "0"})
    assert len(new) == len(old) == 10
    for a, b in zip(new, old):
        assert a[6] == "1" and b[6] == "1", (a, b)              # both equal the oracle's multiset and counts
        assert a[7] == "sorted", a                                 # every level by sorting: no tile table, no k-mer table
        assert a[8] == b[8], (a, b)                                # ... and byte for byte what the tables give
    assert {int(a[4]) for a in new} == {2, 3}                      # two- and three-word tiles both ran
    assert any(b[7] == "tables" for b in old)


_BUDGET_SCRIPT = r"""
import sys, hashlib, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import pack_reads_ascii
from oracle import oracle as o
from katome_amd import device as kd
# thin coverage: 6000 reads over a genome so long that tiles hardly repeat -- every level multiplies its records
for k, L in ((31, 150), (40, 150)):
    n = 6000
    reads = o.synth_reads(31 + k, n, L, int(sys.argv[2]) if len(sys.argv) > 2 else 600000, 2e-3, 0)
    packed = torch.from_numpy(pack_reads_ascii(reads).reshape(-1).copy()).cuda()
    ref = o.build_ascii(reads, k, True)
    want = {bytes(row): int(w) for row, w in zip(ref.edge_label, ref.edge_weight)}
    b = kd.Builder(k, True, table_slots_hint=0)
    for r0 in range(0, n, 1500):
        b.count_reads(packed, 1500, L, None, first_read=r0)
    dg = b.finalize()
    c = b.counts()
    lab = dg.edge_label.cpu().numpy().reshape(dg.n_edges, -1)
    got = {bytes(row): int(w) for row, w in zip(lab, dg.edge_weight.cpu().numpy())}
    h = hashlib.sha256()
    for t in (dg.edge_key, dg.edge_weight, dg.edge_src, dg.edge_dst, dg.node_key, dg.edge_label):
        h.update(t.cpu().numpy().tobytes())
    ok = len(got) == dg.n_edges and got == want and (dg.n_nodes, dg.n_edges) == (ref.n_nodes, ref.n_edges)
    print("BUDGET", k, int(ok), int(c["tile_slots"] > 0), int(c["mid_tile_slots"] > 0), int(c["kmer_slots"] > 0), c["distinct_tiles"], c["distinct_mid_tiles"], h.hexdigest())
    b.close()
"""


def test_levels_that_do_not_fit_the_card_by_sorting_are_counted_in_tables(tmp_path):
    """input whose tiles hardly repeat (coverage of a few fold instead of C3's 300) multiplies records level by level; a level whose
    records, scratch and output would not fit what the card has free goes the table way from there on (count_routes.hip level_fits) instead of
    dying in an allocation: forced at a small size with KATOME_LEVEL_BUDGET -- (a) nothing fits: the mid tiles and the k-mers in
    tables, (b) the mid level fits, the k-mer level does not: in parts by sorting when that is allowed, else the distinct mid tiles
    go into their table with their counts and the k-mers are counted in theirs, (c) everything fits: no table.  The oracle's graph
    each time, byte for byte the same arrays"""
    import subprocess
    script = tmp_path / "budget.py"
    script.write_text(_BUDGET_SCRIPT)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(budget, parts="0", trace=None, genome=600000):
        env = dict(os.environ, KATOME_SORTED_COUNT="2", KATOME_LEVEL_SLACK="0", KATOME_LEVEL_PARTS=parts, KATOME_LEVEL_TRACE="1")
        if budget is not None:
            env["KATOME_LEVEL_BUDGET"] = str(budget)
        out = subprocess.run([sys.executable, str(script), root, str(genome)], env=env, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
        if trace is not None:
            trace.append(out.stderr)
        return [line.split() for line in out.stdout.splitlines() if line.startswith("BUDGET ")]
    everything = run(None)
    assert [r[2:6] for r in everything] == [["1", "0", "0", "0"]] * 2                 # all three levels by sorting
    nothing = run(1)
    assert [r[2:6] for r in nothing] == [["1", "1", "1", "1"]] * 2                    # big tiles, mid tiles, k-mers in tables
    for full, tight in zip(everything, nothing):
        assert full[8] == tight[8]
    # between the two needs: the mid level's records (distinct big tiles x sub-tiles x 3 x record size) fit, the k-mer level's do not
    for i, row in enumerate(everything):
        k = int(row[1])
        nwm, nw = (2, 1) if k == 31 else (2, 2)
        n_sub, span2 = (5, 6) if k == 31 else (3, 9)
        need_mid = int(row[6]) * n_sub * (8 * nwm + 4) * 3
        need_last = int(row[7]) * span2 * (8 * nw + 4) * 4
        assert need_mid < need_last
        mid = run((need_mid + need_last) // 2)[i]
        assert mid[2:6] == ["1", "0", "1", "1"], mid                                   # mid tiles and k-mers in tables, no big-tile table
        assert mid[8] == row[8]
    # The k-mer level IN PARTS (the default; count_routes.hip kmer_records_in_parts): when its records do not fit at once but repeat -- reads at
    # 22-fold coverage here --, the last tile level's list is cut, every part's k-mers are counted by sorting and the parts' lists are
    # counted once more: no table at all; with parts switched off the same budget sends the level to the tables
    deeper = run(None, genome=40000)
    assert [r[2:6] for r in deeper] == [["1", "0", "0", "0"]] * 2
    for i, row in enumerate(deeper):
        k = int(row[1])
        nw, span2 = (1, 6) if k == 31 else (2, 9)
        need_last = int(row[7]) * span2 * (8 * nw + 4) * 4
        said = []
        parts = run(int(0.85 * need_last), parts="1", trace=said, genome=40000)[i]
        assert parts[2:6] == ["1", "0", "0", "0"] and parts[8] == row[8], (parts, said[0][-600:])
        assert "k-mers: counted in" in said[0] and "parts of" in said[0], said[0][-600:]
        tables = run(int(0.85 * need_last), parts="0", genome=40000)[i]
        assert tables[2:6] == ["1", "0", "1", "1"] and tables[8] == row[8], tables


def test_tile_records_kept_aside_grow_and_can_still_go_into_the_table(tmp_path):
    """the big tiles of a build by packed key are kept aside as records and counted by sorting (kept_records.hip keep_tile_recs): sixty
    batches (room for sixteen to begin with, doubled when that is too little), reads with N in them (their records are dropped),
    batches counted window by window in between -- and, in processes of their own, a limit on what may be kept that is reached
    half-way (the records kept so far go into the tile table, later batches too) and a level below that gives up (the distinct big
    tiles go into the tile table with their counts); and `katome_dev_count_tiles`, which makes a batch's records where they are kept
    when no read is skipped, alone and mixed with batches that go through a buffer -- against the oracle; the same limits and
    give-ups for a build in the reference's numbering (tagged tile records), array for array against the oracle's petgraph"""
    import subprocess
    script = tmp_path / "kept.py"
    script.write_text(_KEPT_SCRIPT)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for limit in (None, "9000", "mid", "last"):
        env = dict(os.environ, KATOME_SORTED_COUNT="2")
        if limit in ("mid", "last"):          # that level gives up: the distinct big tiles go into the tile table with their counts
            env["KATOME_SORTED_FAIL"] = limit
        elif limit:
            env["KATOME_TILE_RECS_LIMIT"] = limit
        out = subprocess.run([sys.executable, str(script), root], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        inplace = [line.split() for line in out.stdout.splitlines() if line.startswith("INPLACE ")]
        assert len(inplace) == 2 and all(r[3] == "1" for r in inplace), (limit, inplace)
        assert inplace[0][2] == inplace[1][2]
        seen = [line.split() for line in out.stdout.splitlines() if line.startswith("SEEN ")]
        assert len(seen) == 2 and all(r[3] == "1" for r in seen), (limit, seen)
        if limit is None:
            assert all(r[4] == "0" and r[5] == "0" for r in seen), seen      # no table at any level
        elif limit in ("9000", "mid"):
            assert all(r[4] != "0" for r in seen), (limit, seen)             # the tile table took over
        rows = [line.split() for line in out.stdout.splitlines() if line.startswith("KEPT ")]
        assert len(rows) == 3
        for r in rows:
            assert r[4] == "1", (limit, r)
        assert rows[0][3] == rows[1][3] == rows[2][3]
        if limit == "last":
            assert rows[0][6] != "0" and rows[2][6] != "0"     # the k-mer records went into the k-mer table, counts and all
        elif limit:
            assert rows[0][5] != "0" and rows[2][5] != "0"     # the tile table took over (6000 reads are 24000 tiles)
        else:
            assert rows[0][5] == "0" and rows[2][5] == "0"     # no tile table: counted by sorting


_WIDE_SCRIPT = r"""
import sys, hashlib, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from helpers import pack_reads_ascii
from oracle import oracle as o
from katome_amd import device as kd
for k, L, rc, weak, first_seen in ((31, 101, True, 0, False), (40, 150, True, 0, False), (40, 150, False, 2, False), (63, 150, True, 0, False), (40, 77, True, 0, False),
                                   (33, 126, True, 3, False), (47, 150, False, 0, False), (32, 150, True, 0, False), (62, 131, True, 0, False), (31, 150, True, 2, False),
                                   # the reference's numbering: whole tiles (31/150), left-over windows (31/101, 40/150), two-word k-mers, one strand
                                   (31, 150, True, 0, True), (31, 101, True, 0, True), (40, 150, True, 0, True), (63, 150, True, 0, True), (40, 150, False, 0, True),
                                   (16, 50, True, 0, True)):
    n = 4000
    reads = o.synth_reads(7, n, L, 20000, 4e-3, 2)              # 2 % of the reads carry an N: skipped (builder.rs:155-158), their records invalid
    has_n = (reads == ord("N")).any(axis=1)
    clean = reads.copy()
    clean[clean == ord("N")] = ord("A")
    packed = torch.from_numpy(pack_reads_ascii(clean).reshape(-1).copy()).cuda()
    skip = torch.from_numpy(has_n.astype(np.uint8)).cuda()
    b = kd.Builder(k, rc, first_seen_order=first_seen, table_slots_hint=1 << 14)
    if weak:
        b.remove_weak_edges(weak)
    for r0 in range(0, n, 1536):
        b.count_reads(packed, min(1536, n - r0), L, skip, first_read=r0)
    dg = b.finalize()
    c = b.counts()
    h = hashlib.sha256()
    for t in (dg.edge_key, dg.edge_weight, dg.edge_src, dg.edge_dst, dg.node_key, dg.edge_label):
        h.update(t.cpu().numpy().tobytes())
    ref = o.build_ascii(reads, k, rc, remove_weak_edges=weak or None)
    lab = dg.edge_label.cpu().numpy().reshape(dg.n_edges, -1)
    if first_seen:            # array for array: petgraph's own numbering
        same = (dg.n_nodes, dg.n_edges) == (ref.n_nodes, ref.n_edges) and np.array_equal(lab, ref.edge_label) and \
            np.array_equal(dg.edge_weight.cpu().numpy(), ref.edge_weight) and np.array_equal(dg.edge_src.cpu().numpy(), ref.edge_src) and \
            np.array_equal(dg.edge_dst.cpu().numpy(), ref.edge_dst)
    else:
        ms = {bytes(row): int(w) for row, w in zip(ref.edge_label, ref.edge_weight)}
        got = {bytes(row): int(w) for row, w in zip(lab, dg.edge_weight.cpu().numpy())}
        same = len(got) == dg.n_edges and got == ms
    print("WIDE", k, L, int(rc), weak, int(first_seen), dg.n_nodes, dg.n_edges, c["distinct_kmers"], int(c["kmer_slots"] == 0), int(same), h.hexdigest())
    b.close()
"""


def test_two_word_kmers_and_left_over_windows_counted_by_sorting(tmp_path):
    """k = 32..63 (the reference's example configuration runs k = 40: config.txt), reads whose windows are not a whole number of
    tiles (the left-over windows join the tiles' records; reads with N leave invalid ones) and first-seen-order builds (records
    tagged with their packed sequence numbers) go through the sorted last level too: forced at a small size
    (KATOME_SORTED_COUNT=2), byte for byte against the table route (=0) and against the oracle -- as a multiset, and array for
    array where the build keeps the reference's numbering"""
    import subprocess
    script = tmp_path / "wide.py"
    script.write_text(_WIDE_SCRIPT)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(mode):
        env = dict(os.environ, KATOME_SORTED_COUNT=mode)
        out = subprocess.run([sys.executable, str(script), root], env=env, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        return [line.split() for line in out.stdout.splitlines() if line.startswith("WIDE ")]
    by_sort, by_table = run("2"), run("0")
    assert len(by_sort) == len(by_table) == 16
    for a, t in zip(by_sort, by_table):
        assert a[10] == "1" and t[10] == "1", (a, t)            # the oracle's graph (first-seen order: array for array)
        assert a[9] == "1" and t[9] == "0", (a, t)              # ... reached without / with the k-mer table
        assert a[:9] == t[:9] and a[11] == t[11], (a, t)        # the same arrays


_OPTIMISM_SCRIPT = r"""
import sys, hashlib, torch
sys.path.insert(0, sys.argv[1])
from katome_amd import device as kd
from katome_amd.workloads import WORKLOADS
first_seen = sys.argv[2] == "1"
w = WORKLOADS["c3"].scaled(int(sys.argv[3]))
packed, skip = kd.synth_reads(0, w.reads, w.read_len, w.genome_len, w.err_rate, w.n_inject_percent, device=0)
b = kd.Builder(w.k, True, first_seen_order=first_seen, table_slots_hint=int(1.8 * w.expected_distinct_canonical()))
step = 1 << 24
for r0 in range(0, w.reads, step):
    b.count_reads(packed, min(step, w.reads - r0), w.read_len, None, first_read=r0)
del packed
dg = b.finalize()
c = b.counts()
# (order-sensitive checksums on the device: the arrays are gigabytes)
sums = []
for t in (dg.edge_key, dg.edge_weight, dg.edge_src, dg.edge_dst):
    v = t.reshape(-1).to(torch.int64)
    pos = torch.arange(v.numel(), device=v.device, dtype=torch.int64)
    sums.append(int(((v ^ (pos * -7046029254386353131)) * 6364136223846793005 + pos).sum().item()))
    del v, pos
print("OPT", dg.n_nodes, dg.n_edges, c["distinct_kmers"], int(c["kmer_slots"] == 0), "%x-%x-%x-%x" % tuple(x & (2**64 - 1) for x in sums))
"""


@pytest.mark.parametrize("first_seen", [False, True])
def test_optimistic_sub_rounds_fall_back_to_the_guaranteed_number(tmp_path, first_seen):
    """the sorted last level first tries fewer sub-rounds than a group of distinct records needs (lds_count.hip, lc_optimism); an
    attempt that fills its LDS table gives up and the guaranteed number runs.  Half of C3 (groups of 11 k records): with
    KATOME_LC_OPTIMISM=0.05 and two probes of patience the first attempt is one round and must fail over (the library says so
    under KATOME_LC_TRACE); =1 never tries; the default tries and succeeds -- the same arrays all three times"""
    _need_whole_gpu(80)
    import subprocess
    script = tmp_path / "opt.py"
    script.write_text(_OPTIMISM_SCRIPT)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    seen = set()
    # (a first attempt can only be short of rounds when a group does not fit one table: 11 k records by packed key, 4 k in the
    # reference's numbering, whose slots are wider)
    reads = "50000000" if first_seen else "100000000"
    for optimism in ("0.05", "1", None):
        env = dict(os.environ, KATOME_LC_TRACE="1")
        env.pop("KATOME_LC_OPTIMISM", None)
        env.pop("KATOME_LC_PROBE_LIMIT", None)
        if optimism:
            env["KATOME_LC_OPTIMISM"] = optimism
        if optimism == "0.05":
            env["KATOME_LC_PROBE_LIMIT"] = "2"          # half-full tables need more probes than that: the first attempt must give up
        out = subprocess.run([sys.executable, str(script), root, "1" if first_seen else "0", reads], env=env, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        assert ("counting again" in out.stderr) == (optimism == "0.05"), (optimism, out.stderr[-600:])
        line = [l for l in out.stdout.splitlines() if l.startswith("OPT ")][-1].split()
        assert line[4] == "1", line                       # counted by sorting, no k-mer table
        seen.add(tuple(line))
    assert len(seen) == 1, seen


def test_first_seen_order_refuses_fixed_batches_of_two_lengths(oracle):
    """window i of read r is number r * 2W + i in the reference's order: a second fixed-length batch with another W would number
    past the first one's reads -- an error, not a graph (reads of several lengths have their own entry points)"""
    from katome_amd import device as kd
    from katome_amd.build import KatomePanic
    reads = oracle.synth_reads(3, 64, 100, 5000, 0.0, 0)
    packed = torch.from_numpy(pack_reads_ascii(reads).reshape(-1).copy()).cuda()
    shorter = torch.from_numpy(pack_reads_ascii(reads[:, :90]).reshape(-1).copy()).cuda()
    b = kd.Builder(31, True, first_seen_order=True)
    b.count_reads(packed, 64, 100, None, first_read=0)
    with pytest.raises(KatomePanic, match="fixed-length batches of 100 and 90"):
        b.count_reads(shorter, 64, 90, None, first_read=0)
    b.close()


def test_first_seen_order_bfcounter(oracle, golden_dir, tmp_path):
    from katome_amd.build import GpuGraph, InputFileType, set_global_k_sizes
    base = oracle.build_files([os.path.join(golden_dir, "data1.txt")], 31, False)
    bfc = tmp_path / "k.bfc"
    ms = list(reversed(base.multiset()))
    comp = str.maketrans("ACGT", "TGCA")
    ms += [ms[2], (ms[4][0].translate(comp)[::-1], 9), ms[2]]         # repeated lines: parallel edges (pt_graph.rs:200-213)
    bfc.write_text("".join("%s\t%d\n" % (km, w) for km, w in ms))
    set_global_k_sizes(31)
    for rc in (False, True):
        g, _ = GpuGraph.create([str(bfc)], InputFileType.BFCounter, rc, 0, first_seen_order=True)
        _assert_same_as_reference_order(g, oracle.build_bfc([str(bfc)], 31, rc, 0))
        # ... and the reference's first pruning on such a graph (no per-base adjacency slots with parallel edges)
        g, _ = GpuGraph.create([str(bfc)], InputFileType.BFCounter, rc, 0, first_seen_order=True, remove_dead_paths=True)
        _assert_same_as_reference_order(g, oracle.build_bfc([str(bfc)], 31, rc, 0, remove_dead_paths=True))


@pytest.mark.parametrize("k,L,rc,first_seen", [(31, 101, True, False), (31, 101, True, True), (21, 76, False, True), (40, 77, True, False),
                                               (33, 126, True, True), (16, 50, True, False), (31, 150, True, True), (63, 150, True, False),
                                               (31, 36, True, True), (12, 13, False, True),
                                               # three-word tiles (64..95 bases): k = 63 -> 3 tiles of 28 + 4 windows, mid tiles of 69
                                               # bases; k = 40 -> tiles of 66 bases broken into two-word mid tiles; k = 47, plain order
                                               (63, 150, True, True), (40, 150, True, True), (47, 150, False, False), (62, 131, True, True)])
def test_read_lengths_that_are_not_whole_tiles(oracle, k, L, rc, first_seen):
    """the library's plan for any read length: tiles from the front + the windows left over (101 bp at k=31: 71 windows =
    5 tiles of 14 + 1); same graph as the oracle, in the reference's numbering too; several batches"""
    from katome_amd import device as kd
    n = 3000
    ascii_reads = oracle.synth_reads(0, n, L, 30000, 4e-3, 2)
    has_n = (ascii_reads == ord("N")).any(axis=1)
    clean = ascii_reads.copy()
    clean[clean == ord("N")] = ord("A")
    packed = torch.from_numpy(pack_reads_ascii(clean).reshape(-1).copy()).cuda()
    skip = torch.from_numpy(has_n.astype(np.uint8)).cuda()
    b = kd.Builder(k, rc, first_seen_order=first_seen, table_slots_hint=1 << 14)
    span, tiles, rest = b.tile_plan(L)
    W = L - k + 1
    assert (span == 1 and rest == W) or (tiles * span + rest == W and tiles + rest < W)
    if (k, L) == (31, 101):
        assert (span, tiles, rest) == (14, 5, 1)
    if (k, L) == (63, 150):
        assert (span, tiles, rest) == (28, 3, 4) and b.tile_words(span) == 3
    for r0 in range(0, n, 1024):
        b.count_reads(packed, min(1024, n - r0), L, skip, first_read=r0)
    dg = b.finalize()
    ref = oracle.build_ascii(ascii_reads, k, rc)
    assert (dg.n_nodes, dg.n_edges) == (ref.n_nodes, ref.n_edges)
    if first_seen:
        assert np.array_equal(dg.edge_label.cpu().numpy(), ref.edge_label)
        assert np.array_equal(dg.edge_weight.cpu().numpy().view(np.uint32), ref.edge_weight)
        assert np.array_equal(dg.edge_src.cpu().numpy().view(np.uint64), ref.edge_src)
        assert np.array_equal(dg.edge_dst.cpu().numpy().view(np.uint64), ref.edge_dst)
    else:
        nw = dg.key_words
        ek = dg.edge_key.cpu().numpy().view(np.uint64).reshape(-1, nw)
        keys = [int(r[0]) if nw == 1 else (int(r[0]) << 64) | int(r[1]) for r in ek]
        got = list(zip([int_to_kmer(v, k) for v in keys], dg.edge_weight.cpu().numpy().view(np.uint32).tolist()))
        assert got == ref.multiset()
    b.close()
    # the host entry takes the same route
    from katome_amd.build import GpuGraph
    g, _ = GpuGraph.create_from_packed(pack_reads_ascii(clean).reshape(-1), n, L, skip=has_n.astype(np.uint8),
                                       reverse_complement=rc, k=k, first_seen_order=first_seen)
    assert g.multiset() == ref.multiset()


def test_build_and_stages_on_a_side_stream(oracle):
    """every entry takes the caller's stream (torch's current one): a whole build in the reference's numbering and the stages
    after it under a non-default stream, against the oracle index for index"""
    from katome_amd import device as kd
    n, L, k = 3000, 150, 31
    ascii_reads = oracle.synth_reads(0, n, L, 30000, 3e-3, 1)
    has_n = (ascii_reads == ord("N")).any(axis=1)
    clean = ascii_reads.copy()
    clean[clean == ord("N")] = ord("A")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        packed = torch.from_numpy(pack_reads_ascii(clean).reshape(-1).copy()).cuda()
        skip = torch.from_numpy(has_n.astype(np.uint8)).cuda()
        b = kd.Builder(k, True, first_seen_order=True, table_slots_hint=1 << 16)
        for r0 in range(0, n, 1024):
            b.count_reads(packed, min(1024, n - r0), L, skip, first_read=r0)
        assert b.table_count() >= 0
        b.finalize()
        b.remove_dead_paths()
        b.remove_weak_edges(2)
        dg = b.graph()
        ref = oracle.build_ascii(ascii_reads, k, True, stages="dw", remove_weak_edges=2)
        assert (dg.n_nodes, dg.n_edges) == (ref.n_nodes, ref.n_edges) and ref.n_edges > 0
        assert np.array_equal(dg.edge_label.cpu().numpy(), ref.edge_label)
        assert np.array_equal(dg.edge_weight.cpu().numpy().view(np.uint32), ref.edge_weight)
        assert np.array_equal(dg.edge_src.cpu().numpy().view(np.uint64), ref.edge_src)
        assert np.array_equal(dg.edge_dst.cpu().numpy().view(np.uint64), ref.edge_dst)
        b.close()
    side.synchronize()


def test_close_waits_for_the_views_of_the_graph(oracle):
    """Builder.close() with views of its arrays still alive: the library keeps the memory until the last view is gone, so
    a later build cannot be cut out of the same segments underneath them"""
    from katome_amd import device as kd
    n, L, k = 4000, 150, 31

    def build(seed):
        ascii_reads = oracle.synth_reads(seed, n, L, 40000, 2e-3, 0)
        packed = torch.from_numpy(pack_reads_ascii(ascii_reads).reshape(-1).copy()).cuda()
        b = kd.Builder(k, True, table_slots_hint=1 << 16)
        b.count_reads(packed, n, L, None)
        dg = b.finalize()
        b.close()                                  # put off: dg's arrays are views into the builder's memory
        return b, dg

    b1, g1 = build(1)
    assert b1._h and b1._close_pending and b1._views > 0
    keys = g1.edge_key.clone()
    labels = g1.edge_label.clone()
    others = [build(s) for s in (2, 3, 4)]
    torch.cuda.synchronize()
    assert torch.equal(g1.edge_key, keys) and torch.equal(g1.edge_label, labels)
    del g1, keys, labels
    assert not b1._h and b1._views == 0            # the last view took the builder with it
    builders = [b for b, _ in others]
    del others
    assert all(not b._h for b in builders)
