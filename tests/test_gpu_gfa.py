"""The unitig graph as GFA 1 (katome_dev_contigs_gfa, katome_dev_gfa_arrays, katome_gfa_*): the kernels on hand-made arrays against
the Python model of the format (tests/gfa_model.py), every malformed input refused, DeviceContigs.gfa() on the fixtures and on
by-key builds, the builder left as it was, and the host entries (file bytes, one GPU and three ranks, a path that cannot be made)."""
import json
import os

import numpy as np
import pytest

import gfa_model
from helpers import pack_reads_ascii

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


# ---- the kernels on hand-made arrays -----------------------------------------------------------------------------------------
def _seqs(rng, lengths):
    return ["".join(rng.choice(list("ACGT"), n)) for n in lengths]


def device_arrays(k, src, dst, weight, seqs, kmers=None, off=None, raw=None):
    """-> the arguments of kd.gfa_arrays after k and n_nodes"""
    parts = [gfa_model.compress_edge(s) for s in seqs]
    if off is None:
        off = np.zeros(len(parts) + 1, np.int64)
        off[1:] = np.cumsum([len(p) for p in parts])
    if raw is None:
        raw = b"".join(parts)
    if kmers is None:
        kmers = [len(s) - k + 1 for s in seqs]
    lab = torch.from_numpy(np.frombuffer(raw + b"\0" * (16 + (-len(raw)) % 4), np.uint8).copy()).cuda()
    u32 = lambda a: torch.from_numpy(np.array(a, np.uint32).view(np.int32).copy()).cuda()
    i64 = lambda a: torch.from_numpy(np.array(a, np.int64).copy()).cuda()
    return (i64(src), i64(dst), u32(weight), u32(kmers), i64(off), lab), len(raw)


def check_arrays(k, n_nodes, src, dst, weight, seqs):
    from katome_amd import device as kd
    args, label_bytes = device_arrays(k, src, dst, weight, seqs)
    g = kd.gfa_arrays(k, n_nodes, *args, label_bytes=label_bytes)
    kmers = [len(s) - k + 1 for s in seqs]
    want, seg, first = gfa_model.gfa_text(k, src, dst, weight, kmers, seqs)
    got = g.bytes()
    assert len(got) == g.text_bytes == len(want)
    assert got == want
    assert g.n_segments == len(seqs) and g.n_links == first[-1]
    assert g.segment_off.cpu().tolist() == seg and g.link_first.cpu().tolist() == first
    return g


def _case(name, k, rng):
    """-> (n_nodes, src, dst, weight, seqs)"""
    if name == "no_edges":
        return 3, [], [], [], []
    if name == "one_edge_no_link":
        return 2, [0], [1], [5], _seqs(rng, [k + 1])
    if name == "self_loop":
        return 1, [0], [0], [9], _seqs(rng, [k])
    if name == "every_pad":                        # a chain whose labels are k .. k + 9 bases long
        return 11, list(range(10)), list(range(1, 11)), [int(x) for x in rng.integers(1, 50, 10)], _seqs(rng, range(k, k + 10))
    if name == "hub":                              # 4 edges into vertex 4 and 4 out of it, listed in shuffled source order: 16 links
        src, dst = [0, 1, 2, 3, 4, 4, 4, 4], [4, 4, 4, 4, 5, 6, 7, 8]
        p = rng.permutation(8)
        return 9, [src[i] for i in p], [dst[i] for i in p], list(range(1, 9)), _seqs(rng, [int(x) for x in rng.integers(k, k + 30, 8)])
    if name == "long_then_tiny":                   # several tiles of bases, then 3000 labels of exactly k bases, a chain
        n = 3001
        return n + 1, list(range(n)), list(range(1, n + 1)), [1] * n, _seqs(rng, [70000] + [k] * 3000)
    if name == "many_segments":                    # names cross 10 / 100 / 1000; weights up to 2^32 - 1, KC up to 15 digits
        n = 1200
        lengths = [int(x) for x in rng.integers(k, k + 40, n)]
        lengths[1100] = 30000 + k - 1
        weight = [int(x) for x in rng.integers(1, 2 ** 32, n)]
        weight[0], weight[1100], weight[7] = 2 ** 32 - 1, 2 ** 32 - 1, 1
        assert len(str(weight[1100] * 30000)) == 15
        return 600, [int(x) for x in rng.integers(0, 600, n)], [int(x) for x in rng.integers(0, 600, n)], weight, _seqs(rng, lengths)
    if name == "big_hub":                          # 300 edges in, 300 out: 90 000 links, ranges longer than a workgroup
        src, dst = [1 + i for i in range(300)] + [0] * 300, [0] * 300 + [301 + i for i in range(300)]
        p = rng.permutation(600)
        return 601, [src[i] for i in p], [dst[i] for i in p], [int(x) for x in rng.integers(1, 1000, 600)], _seqs(rng, [k + (i % 5) for i in range(600)])
    raise KeyError(name)


@pytest.mark.parametrize("k", [3, 11])
@pytest.mark.parametrize("name", ["no_edges", "one_edge_no_link", "self_loop", "every_pad", "hub", "long_then_tiny", "many_segments", "big_hub"])
def test_kernels_on_hand_made_arrays(name, k):
    rng = np.random.default_rng(len(name) * 131 + k)
    n_nodes, src, dst, weight, seqs = _case(name, k, rng)
    g = check_arrays(k, n_nodes, src, dst, weight, seqs)
    want_links = {"no_edges": 0, "one_edge_no_link": 0, "self_loop": 1, "every_pad": 9, "hub": 16, "long_then_tiny": 3000, "big_hub": 90000}
    if name in want_links:
        assert g.n_links == want_links[name]
    if name == "hub":
        _, lks = gfa_model.parse(g.bytes())
        assert [(a, b) for a, b, _ in lks] == sorted((a, b) for a, b, _ in lks) and all(o == k - 1 for _, _, o in lks)


def test_malformed_input_is_refused():
    """each of them KATOME_E_ARG, with a message, before anything is read through it"""
    from katome_amd import device as kd
    from katome_amd.build import KatomePanic
    k, rng = 5, np.random.default_rng(5)
    seqs = _seqs(rng, [7, 9, 12])
    src, dst, weight = [0, 1, 2], [1, 2, 0], [1, 2, 3]
    good, label_bytes = device_arrays(k, src, dst, weight, seqs)
    assert kd.gfa_arrays(k, 3, *good, label_bytes=label_bytes).n_links == 3

    def refused(what, n_nodes=3, label_bytes=label_bytes, **kw):
        a = dict(src=src, dst=dst, weight=weight, seqs=seqs)
        a.update(kw)
        args, _ = device_arrays(k, **a)
        with pytest.raises(KatomePanic) as e:
            kd.gfa_arrays(k, n_nodes, *args, label_bytes=label_bytes)
        assert e.value.name == "E_ARG" and what in e.value.message, (what, e.value.message)

    refused("n_nodes", src=[0, 3, 2])                                     # edge_src >= n_nodes
    refused("n_nodes", dst=[1, 2, 2 ** 40])                               # edge_dst >= n_nodes
    refused("n_nodes", n_nodes=2)
    sizes = [len(gfa_model.compress_edge(s)) for s in seqs]
    total = sum(sizes)
    refused("offsets", off=[0, sizes[0], sizes[0] + sizes[1], total + 4])             # a label's end outside the labels
    refused("offsets", label_bytes=total - 1)
    refused("offsets", off=[0, sizes[0] + sizes[1], sizes[0], total])                 # offsets that go backwards
    refused("offsets", off=[0, sizes[0], sizes[0] + 1, total])                        # a label of one byte
    raw = bytearray(b"".join(gfa_model.compress_edge(s) for s in seqs))
    raw[sizes[0]] = 4
    refused("pad byte", raw=bytes(raw))                                               # pad byte > 3
    refused("shorter than k", seqs=[seqs[0], "ACGT", seqs[2]], kmers=[3, 1, 8])       # a label shorter than k bases
    refused("edge_kmers", kmers=[3, 5, 9])                                            # bases are not edge_kmers + k - 1
    refused("edge_kmers", kmers=[3, 2 ** 32 - 1, 8])


# ---- DeviceContigs.gfa() -----------------------------------------------------------------------------------------------------
def _host(dc):
    u = lambda t, dt: t.cpu().numpy().view(dt).tolist()
    return u(dc.edge_src, np.uint64), u(dc.edge_dst, np.uint64), u(dc.edge_weight, np.uint32), u(dc.edge_kmers, np.uint32), dc.sequences()


def check_contigs_gfa(dc, k):
    """gfa() of a shrink result against the model on the arrays copied from it -> (the text, its segments' sequences)"""
    src, dst, weight, kmers, seqs = _host(dc)
    g = dc.gfa()
    want, seg, first = gfa_model.gfa_text(k, src, dst, weight, kmers, seqs)
    got = g.bytes()
    assert got == want
    assert (g.n_segments, g.n_links, g.text_bytes) == (len(seqs), first[-1], len(want))
    assert g.segment_off.cpu().tolist() == seg and g.link_first.cpu().tolist() == first
    segments, lks = gfa_model.parse(got)
    assert [s[1] for s in segments] == dc.text("fasta").contigs()          # segment i is the record >katome_<i> of the unitig FASTA
    for a, b, overlap in lks:                                               # a link's two segments share their k - 1 end bases
        assert overlap == k - 1 and seqs[a][-(k - 1):] == seqs[b][:k - 1]
    del g
    return got, seqs


@pytest.fixture(scope="module")
def pinned(golden_dir):
    with open(os.path.join(golden_dir, "pinned.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("i", [0, 1, 2])
def test_fixtures(golden_dir, pinned, i):
    from katome_amd import device as kd
    from katome_amd.build import ingest_files, InputFileType
    path, k = os.path.join(golden_dir, pinned["fixtures"][i]), pinned["k"]
    r = ingest_files([path], InputFileType.Fastq, k)
    b = kd.Builder(k, False, first_seen_order=True)
    b.count_reads(torch.from_numpy(r["packed"].copy()).cuda(), r["n_reads"], r["fixed_len"])
    b.finalize()
    dc = b.shrink("exact")
    text, seqs = check_contigs_gfa(dc, k)
    assert text.count(b"\nS\t") == len(seqs) == pinned["shrink"]["counts"][i][1] == [1, 92, 233][i]
    del dc
    b.close()


N_READS, READ_LEN, GLEN = 2500, 110, 15000
_reads = {}


def synth(oracle, glen=GLEN):
    if glen not in _reads:
        ascii_reads = oracle.synth_reads(0, N_READS, READ_LEN, glen, 8e-3, 0)
        _reads[glen] = pack_reads_ascii(ascii_reads).reshape(-1).copy()
    return _reads[glen]


@pytest.mark.parametrize("k,rc", [(31, True), (40, False)])
def test_by_key_build_fast_shrink(oracle, k, rc):
    """a by-key build (k = 40: two-word keys) and the traversal-free shrink, whose edge_src is in no particular order"""
    from katome_amd import device as kd
    b = kd.Builder(k, rc)
    b.count_reads(torch.from_numpy(synth(oracle)).cuda(), N_READS, READ_LEN)
    b.finalize()
    dc = b.shrink("fast")
    text, seqs = check_contigs_gfa(dc, k)
    assert len(seqs) > 10 and text.count(b"\nL\t") > 10
    del dc
    b.close()


def test_builder_and_shrink_result_are_left_untouched(oracle):
    from katome_amd import device as kd
    b = kd.Builder(21, True, first_seen_order=True)
    b.count_reads(torch.from_numpy(synth(oracle)).cuda(), N_READS, READ_LEN)
    b.finalize()
    b.remove_dead_paths()
    dc = b.shrink()

    def arrays():
        dg = b.graph()
        return [dg.n_nodes, dg.n_edges, dc.n_nodes, dc.n_edges, dg.edge_age is None] + [x.cpu().numpy().copy() for x in (
            dg.edge_weight, dg.edge_src, dg.edge_dst, dg.edge_key, dg.edge_label, dg.node_key, dg.edge_age, dc.edge_src, dc.edge_dst, dc.edge_weight,
            dc.edge_kmers, dc.edge_label_off, dc.edge_label, dc.node_key) if x is not None]
    before = arrays()
    g = dc.gfa()
    assert g.n_segments == dc.n_edges > 10 and g.n_links > 10
    again = dc.gfa().bytes()                       # (the result is the builder's until the next call: the first one's views are stale now)
    after = arrays()
    assert before[:5] == after[:5]
    for x, y in zip(before[5:], after[5:]):
        assert np.array_equal(x, y)
    assert again == check_contigs_gfa(dc, 21)[0]
    del g, dc
    b.close()


# ---- the host entries ----------------------------------------------------------------------------------------------------------
def _staged_model(packed, n_reads, read_len, k, rc, thr, glen, stages, first_seen):
    """the same build, stages and shrink step by step on a Builder -> the model's text"""
    from katome_amd import device as kd
    b = kd.Builder(k, rc, first_seen_order=first_seen)
    b.count_reads(torch.from_numpy(packed).cuda(), n_reads, read_len)
    b.finalize()
    for st in stages:
        {"d": b.remove_dead_paths, "c": b.standardize_contigs, "w": lambda: b.remove_weak_edges(thr), "e": lambda: b.standardize_edges(glen, thr)}[st]()
    dc = b.shrink()
    src, dst, weight, kmers, seqs = _host(dc)
    del dc
    b.close()
    return gfa_model.gfa_text(k, src, dst, weight, kmers, seqs)


@pytest.mark.parametrize("n_devices", [1, 3])
def test_gfa_files(golden_dir, pinned, tmp_path, n_devices):
    """katome_gfa_files on a fixture with the stages "dcwced" and an output path (three ranks: thread ranks on one card)"""
    from katome_amd.build import GpuGraph, InputFileType, KatomePanic, ingest_files, set_global_k_sizes
    path, out = os.path.join(golden_dir, "data3.txt"), str(tmp_path / "graph.gfa")
    k, rc, thr, glen = 12, True, 1, 20000
    set_global_k_sizes(k)
    r = ingest_files([path], InputFileType.Fastq, k)
    want, seg, first = _staged_model(r["packed"].copy(), r["n_reads"], r["fixed_len"], k, rc, thr, glen, "dcwced", True)
    g = GpuGraph.gfa([path], InputFileType.Fastq, rc, thr, stages="dcwced", original_genome_length=glen, output_file=out, n_devices=n_devices,
                     ranks_share_device=n_devices > 1)
    assert g.n_segments == len(seg) > 10 and g.n_links == first[-1] > 10
    assert open(out, "rb").read() == g.text == want
    assert g.segment_off.tolist() == seg and g.link_first.tolist() == first
    assert g.read_bytes == pinned["read_bytes"]["values"][2] and g.k == k
    again = str(tmp_path / "again.gfa")
    g.save_to_file(again)                          # katome_gfa_save
    assert open(again, "rb").read() == want
    bad = str(tmp_path / "no_such_dir" / "graph.gfa")
    with pytest.raises(KatomePanic) as e:
        g.save_to_file(bad)
    assert e.value.name == "E_OPEN" and "couldn't create %s: entity not found" % bad in e.value.message
    if n_devices == 1:
        with pytest.raises(KatomePanic) as e:      # the file cannot be made: E_OPEN, and the result is handed back all the same
            GpuGraph.gfa([path], InputFileType.Fastq, rc, thr, stages="dcwced", original_genome_length=glen, output_file=bad)
        assert e.value.name == "E_OPEN" and "couldn't create %s: entity not found" % bad in e.value.message
        assert e.value.result is not None and e.value.result.text == want
        with pytest.raises(KatomePanic) as e:      # stage letters need the reference's numbering
            GpuGraph.gfa([path], InputFileType.Fastq, rc, thr, stages="d", first_seen_order=False)
        assert e.value.name == "E_ARG" and "FIRST_SEEN_ORDER" in e.value.message


@pytest.mark.parametrize("n_devices", [1, 3])
def test_gfa_packed(oracle, tmp_path, n_devices):
    """katome_gfa_packed on synthetic reads without stage letters: one GPU builds by packed key and shrinks in the fast form; three
    ranks build sharded in the reference's numbering, gather and shrink exactly"""
    from katome_amd.build import GpuGraph
    k, rc = 31, True
    packed, out = synth(oracle), str(tmp_path / "graph.gfa")
    want, seg, first = _staged_model(packed, N_READS, READ_LEN, k, rc, 0, 0, "", n_devices > 1)
    g = GpuGraph.gfa_from_packed(packed, N_READS, READ_LEN, reverse_complement=rc, stages="", output_file=out, k=k, n_devices=n_devices,
                                 ranks_share_device=n_devices > 1)
    assert g.n_segments == len(seg) > 10 and g.n_links == first[-1] > 10
    assert open(out, "rb").read() == g.text == want
    assert g.segment_off.tolist() == seg and g.link_first.tolist() == first
    assert g.read_bytes == N_READS * READ_LEN
