"""Collapsable::collapse (collapser.rs:25-273) on the device graph: the text kernel on hand-made arrays against a Python decode,
Builder.collapse() against the oracle's collapse on the fixtures, after the whole pipeline and on a by-key builder, the unitig text
of a shrink result, the host entry katome_assemble_* (file bytes, stats, read bytes; one GPU and three ranks), and the builder's
graph left as it was."""
import json
import os

import numpy as np
import pytest

from helpers import int_to_kmer, pack_reads_ascii

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WHOLE = 0x80000000


# ---- the text kernel on hand-made arrays ---------------------------------------------------------------------------------
def compress_edge(seq):
    """compress.rs:250-271: the pad byte, then the bases 2 bits each, first base in the top bits, zero padding"""
    pad = (4 - len(seq) % 4) % 4
    codes = ["ACGT".index(c) for c in seq] + [0] * pad
    return bytes([pad] + [codes[i] << 6 | codes[i + 1] << 4 | codes[i + 2] << 2 | codes[i + 3] for i in range(0, len(codes), 4)])


def py_contigs(labels, pieces, k):
    out = []
    for p in pieces:
        if p & WHOLE:
            out.append(labels[p & ~WHOLE])
        else:
            out[-1] += labels[p][k - 1:]
    return out


def py_text(contigs, layout):
    return "".join(contigs) if layout == "plain" else "".join(">katome_%d\n%s\n" % (i, c) for i, c in enumerate(contigs))


def run_kernel(labels, pieces, k, layout):
    """-> (contigs cut out of the text by the offsets and lengths, text[:text_bytes])"""
    from katome_amd import device as kd
    raw = [compress_edge(s) for s in labels]
    off = np.zeros(len(raw) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in raw])
    lab = torch.from_numpy(np.frombuffer(b"".join(raw) + b"\0" * 16, np.uint8).copy()).cuda()
    d_pieces = None if pieces is None else torch.from_numpy(np.array(pieces, np.uint32).view(np.int32).copy()).cuda()
    c_off, c_len, text, n = kd.pieces_text(lab, torch.from_numpy(off).cuda(), d_pieces, k, layout)
    assert text.numel() % 16 == 0 and text.numel() >= n
    text = bytes(text.cpu().numpy()[:n])
    return [text[o:o + ln].decode() for o, ln in zip(c_off.cpu().tolist(), c_len.cpu().tolist())], text.decode()


def _labels(rng, lengths):
    return ["".join(rng.choice(list("ACGT"), n)) for n in lengths]


def _case(name, k, rng):
    """-> (labels, pieces)"""
    if name == "every_pad":                       # labels of k .. k + 9 bases: all four pad values, whole and as remainders
        labels = _labels(rng, range(k, k + 10))
        pieces = [i | WHOLE for i in range(10)] + [0 | WHOLE] + list(range(10)) + [9 | WHOLE] + list(range(9, -1, -1))
    elif name == "single_whole":
        labels, pieces = _labels(rng, [k + 5]), [0 | WHOLE]
    elif name == "one_base_remainders":           # a whole piece and 40 remainders of one base (labels of exactly k bases)
        labels = _labels(rng, [k + 2] + [k] * 40)
        pieces = [0 | WHOLE] + list(range(1, 41))
    elif name == "long_then_tiny":                # crosses several output tiles; many pieces inside one lane's 16 bytes
        labels = _labels(rng, [70000 + k - 1] + [k] * 7)
        pieces = [3 | WHOLE, 0] + [int(x) for x in rng.integers(1, 8, 3000)]
    elif name == "many_contigs":                  # the header width changes at 10, 100 and 1000
        labels = _labels(rng, [int(x) for x in rng.integers(k, k + 40, 50)])
        pieces = []
        for _ in range(1200):
            pieces.append(int(rng.integers(50)) | WHOLE)
            pieces += [int(x) for x in rng.integers(0, 50, int(rng.integers(0, 3)))]
    else:
        raise KeyError(name)
    return labels, pieces


@pytest.mark.parametrize("layout", ["plain", "fasta"])
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("name", ["every_pad", "single_whole", "one_base_remainders", "long_then_tiny", "many_contigs"])
def test_text_kernel_on_hand_made_arrays(name, k, layout):
    rng = np.random.default_rng(len(name) * 31 + k)
    labels, pieces = _case(name, k, rng)
    want = py_contigs(labels, pieces, k)
    got, text = run_kernel(labels, pieces, k, layout)
    assert text == py_text(want, layout)
    assert got == want


@pytest.mark.parametrize("layout", ["plain", "fasta"])
def test_text_kernel_without_pieces(layout):
    """zero pieces; and no piece list at all: one whole piece per label (what the unitig text uses)"""
    from katome_amd import device as kd
    rng = np.random.default_rng(2)
    assert run_kernel(_labels(rng, [9, 12]), [], 5, layout) == ([], "")
    labels = _labels(rng, [int(x) for x in rng.integers(5, 300, 700)] + [20000])
    got, text = run_kernel(labels, None, 5, layout)
    assert got == labels and text == py_text(labels, layout)
    # a piece that names no label, and a first piece that begins no contig, are refused before anything is read through them
    from katome_amd.build import KatomePanic
    for bad in ([7 | WHOLE], [0]):
        with pytest.raises(KatomePanic):
            run_kernel(labels[:3], bad, 5, layout)
    assert kd.LAYOUTS == {"plain": 0, "fasta": 1}


# ---- Builder.collapse() ----------------------------------------------------------------------------------------------------
def restated_stats(lengths, genome_length):
    """stats/contigs.rs:31-89"""
    if not lengths:
        return (0, 0, 0, 0)
    c = sorted(lengths)
    total = sum(c)

    def n_metrics(tip):
        acc, last = 0, None
        for x in c:
            if acc >= tip:
                break
            last, acc = x, acc + x
        return last
    acc, l50 = 0, 0
    for i, x in enumerate(reversed(c)):
        if acc >= total // 2:
            break
        l50, acc = i + 1, acc + x
    return (n_metrics(total // 2), l50, n_metrics(int(0.1 * float(total))), n_metrics(genome_length // 2))


@pytest.fixture(scope="module")
def pinned(golden_dir):
    with open(os.path.join(golden_dir, "pinned.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("i", [0, 1, 2])
def test_fixtures(oracle, golden_dir, pinned, i):
    """tests/collapser.rs:32: [2, 92, 233] contigs, string for string and in order, and nothing left of the graph"""
    from katome_amd import device as kd
    from katome_amd.build import ingest_files, InputFileType
    path, k = os.path.join(golden_dir, pinned["fixtures"][i]), pinned["k"]
    r = ingest_files([path], InputFileType.Fastq, k)
    b = kd.Builder(k, False, first_seen_order=True)
    b.count_reads(torch.from_numpy(r["packed"].copy()).cuda(), r["n_reads"], r["fixed_len"])
    b.finalize()
    a = b.collapse()
    want = oracle.build_files([path], k, False, stages="C").collapsed
    assert a.contigs() == want
    assert a.n_contigs == len(want) == pinned["collapse"]["contigs"][i] == [2, 92, 233][i]
    assert (a.stats["nodes_left"], a.stats["edges_left"]) == (0, 0)
    assert a.n_pieces == a.stats["n_pieces"] >= a.n_contigs and b.last_collapse_host_ms >= 0
    fa = b.collapse("fasta")
    assert bytes(fa.text.cpu().numpy()).decode() == py_text(want, "fasta") and fa.contigs() == want
    del a, fa
    b.close()


SHAPES = [(31, True, 2, 15000), (21, False, 2, 15000), (12, True, 3, 4000), (8, True, 4, 1500), (40, True, 2, 20000)]
N_READS, READ_LEN = 2500, 110
_reads = {}


def synth(oracle, glen):
    if glen not in _reads:
        ascii_reads = oracle.synth_reads(0, N_READS, READ_LEN, glen, 8e-3, 0)
        _reads[glen] = (ascii_reads, pack_reads_ascii(ascii_reads).reshape(-1).copy())
    return _reads[glen]


def pipeline(oracle, k, rc, thr, glen):
    """ "dcwced" on the device -> the builder"""
    from katome_amd import device as kd
    b = kd.Builder(k, rc, first_seen_order=True)
    b.count_reads(torch.from_numpy(synth(oracle, glen)[1]).cuda(), N_READS, READ_LEN)
    b.finalize()
    b.remove_dead_paths()
    b.standardize_contigs()
    b.remove_weak_edges(thr)
    b.standardize_contigs()
    b.standardize_edges(glen, thr)
    b.remove_dead_paths()
    return b


@pytest.mark.parametrize("k,rc,thr,glen", SHAPES)
def test_whole_pipeline(oracle, k, rc, thr, glen):
    """every stage before collapse and collapse itself on the device graph against the oracle's all-CPU "dcwcedC": the contigs
    string for string and in order; Contigs::stats of the result against the restatement"""
    from katome_amd.build import KatomePanic, contig_stats
    oracle.set_genome_length(glen)
    want = oracle.build_ascii(synth(oracle, glen)[0], k, rc, remove_weak_edges=thr, stages="dcwcedC").collapsed
    assert len(want) > 10 and sum(map(len, want)) > 2000
    b = pipeline(oracle, k, rc, thr, glen)
    a = b.collapse()
    assert a.contigs() == want
    assert a.lengths() == [len(c) for c in want] and a.text_bytes == sum(map(len, want))
    assert (a.stats["nodes_left"], a.stats["edges_left"]) == (0, 0) and a.stats["n_contigs"] == len(want)
    assert contig_stats(a.lengths(), glen) == restated_stats([len(c) for c in want], glen) == a.contig_stats(glen)
    for zero in (0, 1):                            # original_genome_length / 2 == 0: the reference panics in n_metrics
        with pytest.raises(KatomePanic) as e:
            a.contig_stats(zero)
        assert e.value.status == -7 and "ng50" in str(e.value)
    del a
    b.close()


def _collapse_from_device_graph(oracle, dg, k):
    """(tests/test_gpu_prune.py) rebuild a PtGraph from the device arrays, edges added in ascending age, and run the oracle's collapse"""
    nw = dg.key_words
    ek = dg.edge_key.cpu().numpy().view(np.uint64).reshape(-1, nw)
    seqs = [int_to_kmer(int(x[0]) if nw == 1 else (int(x[0]) << 64) | int(x[1]), k) for x in ek]
    src = dg.edge_src.cpu().numpy().view(np.uint64).tolist()
    dst = dg.edge_dst.cpu().numpy().view(np.uint64).tolist()
    w = dg.edge_weight.cpu().numpy().view(np.uint32).tolist()
    age = dg.edge_age.cpu().numpy().view(np.uint32).tolist() if dg.edge_age is not None else list(range(dg.n_edges))
    order = sorted(range(dg.n_edges), key=lambda e: age[e])
    edges = [(src[e], dst[e], w[e], i + 1) for i, e in enumerate(order)]
    slots = [None] + [seqs[e] for e in order]
    return oracle.run_from_edges(dg.n_nodes, edges, "C", 0, k, slots).collapsed


@pytest.mark.parametrize("k,rc,glen", [(31, True, 15000), (21, False, 15000)])
def test_by_key_numbering(oracle, k, rc, glen):
    """a default-numbering builder has no ages: collapse() is the reference's collapse of THAT graph, edges in index order"""
    from katome_amd import device as kd
    b = kd.Builder(k, rc)
    b.count_reads(torch.from_numpy(synth(oracle, glen)[1]).cuda(), N_READS, READ_LEN)
    dg = b.finalize()
    assert dg.edge_age is None
    want = _collapse_from_device_graph(oracle, dg, k)
    assert len(want) > 10
    a = b.collapse()
    assert a.contigs() == want
    del a, dg
    b.close()


def test_unitig_text(oracle):
    """the text of a shrink result, fast and exact, one contig per merged edge, against the Python decode of the labels"""
    k, rc, thr, glen = SHAPES[0]
    b = pipeline(oracle, k, rc, thr, glen)
    for mode, layout in (("fast", "plain"), ("exact", "fasta")):
        dc = b.shrink(mode)
        want = dc.sequences()
        assert len(want) > 10
        t = dc.text(layout)
        assert t.contigs() == want and bytes(t.text.cpu().numpy()).decode() == py_text(want, layout)
        del t, dc
    b.close()


def test_builder_is_left_untouched(oracle):
    k, rc, thr, glen = SHAPES[2]
    b = pipeline(oracle, k, rc, thr, glen)

    def arrays():
        dg = b.graph()
        return [dg.n_nodes, dg.n_edges] + [x.cpu().numpy().copy() for x in (dg.edge_weight, dg.edge_src, dg.edge_dst, dg.edge_key, dg.edge_label,
                                                                           dg.node_key, dg.edge_age)]
    before = arrays()
    a = b.collapse()
    assert a.n_contigs > 10
    after = arrays()
    assert before[:2] == after[:2] and before[1] > 0
    for x, y in zip(before[2:], after[2:]):
        assert np.array_equal(x, y)
    del a
    b.close()


# ---- the host entries ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_devices", [1, 3])
def test_assemble_files(oracle, golden_dir, pinned, tmp_path, n_devices):
    """katome_assemble_files on the fixture with an output path: the file, the stats, the read bytes (three ranks: thread ranks on
    one card, as test_every_stage_after_a_sharded_build)"""
    from katome_amd.build import GpuGraph, InputFileType, KatomePanic, set_global_k_sizes
    path, out = os.path.join(golden_dir, "data3.txt"), str(tmp_path / "contigs.fa")
    k, rc, thr, glen = 12, True, 1, 20000
    set_global_k_sizes(k)
    oracle.set_genome_length(glen)
    want = oracle.build_files([path], k, rc, remove_weak_edges=thr, stages="dcwcedC").collapsed
    assert len(want) > 10 and sum(map(len, want)) > 2000
    a = GpuGraph.assemble([path], InputFileType.Fastq, rc, thr, glen, output_file=out, n_devices=n_devices, ranks_share_device=n_devices > 1)
    assert a.contigs == want
    assert open(out, "rb").read() == py_text(want, "fasta").encode() == a.fasta
    assert a.stats == restated_stats([len(c) for c in want], glen)
    assert a.read_bytes == pinned["read_bytes"]["values"][2]
    again = str(tmp_path / "again.fa")
    a.save_to_file(again)                          # katome_assembly_save
    assert open(again, "rb").read() == a.fasta
    with pytest.raises(KatomePanic) as e:
        a.save_to_file(str(tmp_path / "no_such_dir" / "contigs.fa"))
    assert e.value.status == -4 and "couldn't create" in str(e.value)


@pytest.mark.parametrize("n_devices", [1, 3])
def test_assemble_packed(oracle, tmp_path, n_devices):
    """the same through katome_assemble_packed: the synthetic reads of the pipeline test"""
    from katome_amd.build import GpuGraph, KatomePanic
    k, rc, thr, glen = SHAPES[0]
    ascii_reads, packed = synth(oracle, glen)
    oracle.set_genome_length(glen)
    want = oracle.build_ascii(ascii_reads, k, rc, remove_weak_edges=thr, stages="dcwcedC").collapsed
    assert len(want) > 10
    out = str(tmp_path / "contigs.fa")
    a = GpuGraph.assemble_from_packed(packed, N_READS, READ_LEN, reverse_complement=rc, minimal_weight_threshold=thr, original_genome_length=glen,
                                      output_file=out, k=k, n_devices=n_devices, ranks_share_device=n_devices > 1)
    assert a.contigs == want
    assert open(out, "rb").read() == py_text(want, "fasta").encode()
    assert a.stats == restated_stats([len(c) for c in want], glen)
    assert a.read_bytes == N_READS * READ_LEN and a.collapse_stats["n_contigs"] == len(want)
    if n_devices == 1:
        with pytest.raises(KatomePanic) as e:         # asm/mod.rs:62
            GpuGraph.assemble_from_packed(packed, N_READS, READ_LEN, reverse_complement=rc, minimal_weight_threshold=thr, original_genome_length=glen,
                                          output_file=str(tmp_path / "no_such_dir" / "contigs.fa"), k=k)
        assert e.value.status == -4 and "couldn't create" in str(e.value)
