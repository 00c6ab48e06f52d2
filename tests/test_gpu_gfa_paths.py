"""The GFA of the assembly (katome_dev_gfa_paths_arrays, katome_dev_collapse_gfa, katome_assemble_gfa_*): the path kernels on
hand-made arrays against the Python model (tests/gfa_paths_model.py) byte for byte, every malformed input refused,
Builder.collapse_gfa() on the fixtures and after the whole pipeline -- the paths follow L lines, their seams are real, they spell
the FASTA records and use every segment as often as it weighs --, a tandem repeat built on the GPU, and the host entries."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import gfa_model
import gfa_paths_model as model
from helpers import pack_reads_ascii

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WHOLE = model.WHOLE
GUARD = 64


# ---- the kernels on hand-made arrays -----------------------------------------------------------------------------------------
def _dev(a, dt):
    return torch.from_numpy(np.array(a, dt).view({np.uint32: np.int32, np.int64: np.int64}[dt]).copy()).cuda()


def run_arrays(src, dst, pieces, path_cap=None, text_cap=None):
    """the raw entry on buffers filled with 0xFF, with a guard behind each -> (text buffer, counts, line_off, contig, first_piece)"""
    from katome_amd import _lib
    from katome_amd.build import KatomePanic
    L = _lib.lib()
    d_src, d_dst, d_pieces = _dev(src, np.int64), _dev(dst, np.int64), _dev(pieces, np.uint32)
    p = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
    counts = (C.c_uint64 * 3)(7, 7, 7)
    args = (0, len(src), p(d_src), p(d_dst), p(d_pieces), len(pieces))
    rc = L.katome_dev_gfa_paths_arrays(*args, None, None, None, 0, None, 0, counts, None)
    if rc:
        assert list(counts) == [0, 0, 0]
        raise KatomePanic(rc, _lib.last_error())
    n_paths, n_bytes = counts[0], counts[2]
    path_cap = n_paths if path_cap is None else path_cap
    text_cap = (n_bytes + 15) // 16 * 16 if text_cap is None else text_cap
    ff = lambda n, dt: torch.full((n,), -1, dtype=dt, device="cuda")
    line_off, contig, first = ff(n_paths + 1 + GUARD, torch.int64), ff(n_paths + GUARD, torch.int64), ff(n_paths + 1 + GUARD, torch.int64)
    text = torch.full((max((n_bytes + 15) // 16 * 16, 16) + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    query = list(counts)
    rc = L.katome_dev_gfa_paths_arrays(*args, p(line_off), p(contig), p(first), path_cap, p(text), text_cap, counts, None)
    if rc:
        raise KatomePanic(rc, _lib.last_error())
    assert list(counts) == query
    return text.cpu().numpy(), dict(n_paths=counts[0], n_jumps=counts[1], text_bytes=counts[2]), line_off.cpu().tolist(), contig.cpu().tolist(), first.cpu().tolist()


def check_arrays(src, dst, pieces):
    want, want_off, want_contig, want_first, want_jumps = model.path_text(src, dst, pieces)
    text, counts, line_off, contig, first = run_arrays(src, dst, pieces)
    n, n_paths = len(want), len(want_contig)
    assert counts == dict(n_paths=n_paths, n_jumps=want_jumps, text_bytes=n)
    assert bytes(text[:n]) == want
    cap = (n + 15) // 16 * 16
    assert not text[n:cap].any()                                             # zeros up to the next multiple of 16
    assert (text[max(cap, 16):] == 0xFF).all() and len(text) == max(cap, 16) + GUARD      # ... and nothing behind it
    assert line_off[:n_paths + 1] == want_off and first[:n_paths + 1] == want_first and contig[:n_paths] == want_contig
    assert set(line_off[n_paths + 1:]) | set(first[n_paths + 1:]) | set(contig[n_paths:]) == {-1}
    return counts


def _case(name, rng):
    """-> (src, dst, pieces)"""
    if name == "zero_pieces":
        return [0, 1], [1, 2], []
    if name == "one_piece":
        return [0, 1], [1, 2], [1 | WHOLE]
    if name == "digits":                           # 1 200 edges in a chain, 1 200 contigs: segment and contig numbers cross 9/10, 99/100, 999/1000
        n = 1200
        pieces = []
        for c in range(n):
            pieces.append(c | WHOLE)
            for j in range(int(rng.integers(0, 3))):
                pieces.append(c + 1 + j if c + 1 + j < n and rng.random() < 0.8 else int(rng.integers(n)))
        return list(range(n)), list(range(1, n + 1)), pieces
    if name == "twelve_jumps":                     # edges that share no vertex: every piece after the first is a jump, runs .1 to .12
        return [2 * i for i in range(13)], [2 * i + 1 for i in range(13)], [5 | WHOLE, 0 | WHOLE] + list(range(1, 13)) + [3 | WHOLE]
    if name == "jump_on_last_piece":
        return [0, 1, 5], [1, 2, 6], [0 | WHOLE, 1, 0 | WHOLE, 1, 2]
    if name == "long_then_tiny":                   # one path of 6 000 pieces round a cycle of 1 000 edges (several tiles), then 3 000 one-piece paths
        n = 1000
        return list(range(n)), [(i + 1) % n for i in range(n)], [0 | WHOLE] + [i % n for i in range(1, 6000)] + [int(x) | WHOLE for x in rng.integers(0, n, 3000)]
    if name.startswith("random"):                  # a random walk that mostly follows the edges: short and long runs, jumps, many contigs
        n = int(rng.integers(50, 3000))
        n_nodes = max(2, n // 2)
        src, dst = rng.integers(0, n_nodes, n).tolist(), rng.integers(0, n_nodes, n).tolist()
        out_of = {}
        for e, v in enumerate(src):
            out_of.setdefault(v, []).append(e)
        pieces = [int(rng.integers(n)) | WHOLE]
        for _ in range(int(rng.integers(2000, 20000))):
            nxt = out_of.get(dst[pieces[-1] & ~WHOLE], [])
            if rng.random() < 0.05:
                pieces.append(int(rng.integers(n)) | WHOLE)
            elif nxt and rng.random() < 0.95:
                pieces.append(int(rng.choice(nxt)))
            else:
                pieces.append(int(rng.integers(n)))
        return src, dst, pieces
    raise KeyError(name)


@pytest.mark.parametrize("name", ["zero_pieces", "one_piece", "digits", "twelve_jumps", "jump_on_last_piece", "long_then_tiny", "random0", "random1", "random2"])
def test_kernels_on_hand_made_arrays(name):
    rng = np.random.default_rng(len(name) * 17 + ord(name[-1]))
    src, dst, pieces = _case(name, rng)
    counts = check_arrays(src, dst, pieces)
    if name == "zero_pieces":
        assert counts == dict(n_paths=0, n_jumps=0, text_bytes=0)
    if name == "digits":
        assert counts["n_paths"] - counts["n_jumps"] == 1200 and counts["n_jumps"] > 100
    if name == "twelve_jumps":
        text = model.path_text(src, dst, pieces)[0]
        assert counts["n_jumps"] == 12 and b"P\tkatome_1.10\t10+\t*\nP\tkatome_1.11\t11+\t*\nP\tkatome_1.12\t12+\t*\nP\tkatome_2\t3+" in text
    if name == "jump_on_last_piece":
        assert model.path_text(src, dst, pieces)[0].endswith(b"P\tkatome_1\t0+,1+\t*\nP\tkatome_1.1\t2+\t*\n") and counts["n_jumps"] == 1
    if name == "long_then_tiny":
        assert counts["n_paths"] == 3001 and counts["n_jumps"] == 0 and model.path_text(src, dst, pieces)[1][1] > 3 * 8192
    if name.startswith("random"):
        assert counts["n_jumps"] > 0


def test_binding_on_tensors():
    """device.gfa_paths_arrays, the same entry on torch tensors"""
    from katome_amd import device as kd
    src, dst, pieces = _case("digits", np.random.default_rng(1))
    want, want_off, want_contig, want_first, want_jumps = model.path_text(src, dst, pieces)
    text, counts, line_off, contig, first = kd.gfa_paths_arrays(_dev(src, np.int64), _dev(dst, np.int64), _dev(pieces, np.uint32))
    assert counts == dict(n_paths=len(want_contig), n_jumps=want_jumps, text_bytes=len(want)) and text.numel() % 16 == 0
    assert bytes(text.cpu().numpy()[:len(want)]) == want
    assert (line_off.cpu().tolist(), contig.cpu().tolist(), first.cpu().tolist()) == (want_off, want_contig, want_first)


def test_malformed_input_is_refused():
    """each of them KATOME_E_ARG, with a message, before anything is read through it"""
    from katome_amd import device as kd
    from katome_amd.build import KatomePanic
    src, dst = [0, 1, 2], [1, 2, 0]
    good = [0 | WHOLE, 1, 2, 1 | WHOLE]
    assert check_arrays(src, dst, good)["n_paths"] == 2

    def refused(what, pieces=good, **kw):
        with pytest.raises(KatomePanic) as e:
            run_arrays(src, dst, pieces, **kw)
        assert e.value.name == "E_ARG" and what in e.value.message, (what, e.value.message)

    refused("n_edges", [0 | WHOLE, 3])                                    # a piece id >= n_edges
    refused("n_edges", [0x7FFFFFFF | WHOLE])
    refused("n_edges", [0 | WHOLE, 1, 2, 0x7FFFFFFF])
    refused("first piece", [0, 1 | WHOLE])                                # a first piece without WHOLE
    refused("do not fit", text_cap=16)                                    # the text is 38 bytes
    refused("do not fit", path_cap=1)
    b = kd.Builder(5, False, first_seen_order=True)
    with pytest.raises(KatomePanic) as e:                                 # collapse_gfa() before collapse()
        b.collapse_gfa()
    assert e.value.name == "E_ARG" and "collapse_gfa: no collapse result" in e.value.message
    b.close()


# ---- Builder.collapse_gfa() ----------------------------------------------------------------------------------------------------
def py_fasta(contigs):
    return "".join(">katome_%d\n%s\n" % (i, c) for i, c in enumerate(contigs))


def check_collapse_gfa(b, k):
    """collapse("fasta"), shrink("exact") + gfa() and collapse_gfa() of one builder -> (the DeviceGfaPaths' host copy, the contigs)"""
    def graph_arrays():
        dg = b.graph()
        return [dg.n_nodes, dg.n_edges] + [x.cpu().numpy().copy() for x in (dg.edge_weight, dg.edge_src, dg.edge_dst, dg.edge_key, dg.edge_label,
                                                                           dg.node_key, dg.edge_age) if x is not None]
    fa = b.collapse("fasta")
    contigs, fasta = fa.contigs(), bytes(fa.text.cpu().numpy())
    dc = b.shrink("exact")
    unitigs = dc.gfa()
    hsl = unitigs.bytes()
    before = graph_arrays()
    g = b.collapse_gfa()
    # the builder's graph and the earlier results are as they were
    after = graph_arrays()
    assert before[:2] == after[:2] and all(np.array_equal(x, y) for x, y in zip(before[2:], after[2:]))
    assert unitigs.bytes() == hsl and bytes(fa.text.cpu().numpy()) == fasta and fa.contigs() == contigs
    # the H / S / L part is the unitig graph's GFA
    assert bytes(g.text.cpu().numpy()) == hsl and (g.n_segments, g.n_links, g.text_bytes) == (unitigs.n_segments, unitigs.n_links, len(hsl))
    assert g.segment_off.cpu().tolist() == unitigs.segment_off.cpu().tolist() and g.link_first.cpu().tolist() == unitigs.link_first.cpu().tolist()
    assert g.bytes() == hsl + bytes(g.path_text.cpu().numpy()) and g.path_bytes == g.path_text.numel()
    segments, lks = gfa_model.parse(hsl)
    linked = set((a, s) for a, s, _ in lks)
    seqs = [s[1] for s in segments]
    src, dst = dc.edge_src.cpu().tolist(), dc.edge_dst.cpu().tolist()
    paths = model.parse(bytes(g.path_text.cpu().numpy()))
    assert len(paths) == g.n_paths and g.path_contig.cpu().tolist() == [c for c, _, _ in paths]
    line_off, first = g.path_line_off.cpu().tolist(), g.path_first_piece.cpu().tolist()
    assert line_off[-1] == g.path_bytes and first[-1] == fa.stats["n_pieces"] and [y - x for x, y in zip(first, first[1:])] == [len(ids) for _, _, ids in paths]
    spelled, used = {}, [0] * len(seqs)
    for j, (c, r, ids) in enumerate(paths):
        assert all(pair in linked for pair in zip(ids, ids[1:]))            # every consecutive pair inside a P line is an L line
        if r:                                                              # a run boundary inside a contig: a real seam
            last = paths[j - 1]
            assert last[0] == c and last[1] == r - 1 and dst[last[2][-1]] != src[ids[0]]
        else:
            assert c == len(spelled)
        for n, i in enumerate(ids):
            used[i] += 1
            spelled[c] = spelled.get(c, "") + (seqs[i] if r == 0 and n == 0 else seqs[i][k - 1:])
    assert [spelled[c] for c in range(len(contigs))] == contigs and py_fasta(contigs).encode() == fasta
    assert used == [s[2]["ew"] for s in segments]                           # segment i occurs in the paths exactly ew_i times
    assert g.n_paths - len(contigs) == g.n_jumps <= fa.stats["simple_loops"]
    counts = (g.n_paths, g.n_jumps, len(contigs))
    del fa, dc, unitigs, g
    return counts


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
    n_paths, n_jumps, n_contigs = check_collapse_gfa(b, k)
    assert n_contigs == pinned["collapse"]["contigs"][i] == [2, 92, 233][i]
    b.close()


N_READS, READ_LEN, GLEN = 2500, 110, 15000
_reads = {}


def synth(oracle, glen=GLEN):
    if glen not in _reads:
        ascii_reads = oracle.synth_reads(0, N_READS, READ_LEN, glen, 8e-3, 0)
        _reads[glen] = pack_reads_ascii(ascii_reads).reshape(-1).copy()
    return _reads[glen]


def test_after_the_whole_pipeline(oracle):
    """a synthetic read set after "dcwced" """
    from katome_amd import device as kd
    k, rc, thr = 31, True, 2
    b = kd.Builder(k, rc, first_seen_order=True)
    b.count_reads(torch.from_numpy(synth(oracle)).cuda(), N_READS, READ_LEN)
    b.finalize()
    b.remove_dead_paths()
    b.standardize_contigs()
    b.remove_weak_edges(thr)
    b.standardize_contigs()
    b.standardize_edges(GLEN, thr)
    b.remove_dead_paths()
    n_paths, n_jumps, n_contigs = check_collapse_gfa(b, k)
    assert n_contigs > 10
    b.close()


def tandem_read():
    """X R R Y with |X| = |Y| = 15, |R| = 20"""
    rng = np.random.default_rng(7)
    x, r, y = ("".join(rng.choice(list("ACGT"), n)) for n in (15, 20, 15))
    return x + r + r + y


def test_tandem_repeat_built_on_the_gpu(oracle):
    """one read X R R Y, k = 7, first-seen order: the walk takes the repeat's simple loop, the first contig has a seam that is no
    (k - 1)-overlap, and is therefore two paths"""
    from katome_amd import device as kd
    k, read = 7, tandem_read()
    rows = np.frombuffer(read.encode(), np.uint8).reshape(1, -1)
    want = oracle.build_ascii(rows, k, False, stages="C").collapsed
    assert [len(c) for c in want] == [55, 21]
    b = kd.Builder(k, False, first_seen_order=True)
    b.count_reads(torch.from_numpy(pack_reads_ascii(rows).reshape(-1).copy()).cuda(), 1, len(read))
    b.finalize()
    assert check_collapse_gfa(b, k) == (3, 1, 2)
    a = b.collapse()
    assert a.contigs() == want and a.stats["simple_loops"] == 1
    g = b.collapse_gfa()
    assert [(c, r) for c, r, _ in model.parse(bytes(g.path_text.cpu().numpy()))] == [(0, 0), (0, 1), (1, 0)]
    del a, g
    b.close()


# ---- the host entries ----------------------------------------------------------------------------------------------------------
def check_host_result(a, g, k):
    """the two halves of one assemble_gfa agree: the paths spell the contigs from the S lines"""
    assert g.text[:g.text_bytes].startswith(b"H\tVN:Z:1.0\n") and g.path_text == g.text[g.text_bytes:] and len(g.path_text) == g.path_bytes
    segments, _ = gfa_model.parse(g.text[:g.text_bytes])
    seqs, spelled = [s[1] for s in segments], {}
    paths = model.parse(g.path_text)
    for c, r, ids in paths:
        for n, i in enumerate(ids):
            spelled[c] = spelled.get(c, "") + (seqs[i] if r == 0 and n == 0 else seqs[i][k - 1:])
    assert [spelled[c] for c in range(a.n_contigs)] == a.contigs
    assert (g.n_paths, g.n_jumps) == (len(paths), len(paths) - a.n_contigs) and g.n_segments == len(segments) and g.k == k
    assert g.path_contig.tolist() == [c for c, _, _ in paths] and g.path_line_off[-1] == g.path_bytes
    assert g.path_first_piece[-1] == a.collapse_stats["n_pieces"] == sum(len(ids) for _, _, ids in paths)


@pytest.mark.parametrize("n_devices", [1, 3])
def test_assemble_gfa_files(golden_dir, tmp_path, n_devices):
    """katome_assemble_gfa_files on a fixture (three ranks: thread ranks on one card): the two files, and katome_assemble_files' FASTA"""
    from katome_amd.build import GpuGraph, InputFileType, KatomePanic, set_global_k_sizes
    path = os.path.join(golden_dir, "data3.txt")
    k, rc, thr, glen = 12, True, 1, 20000
    set_global_k_sizes(k)
    fasta, gfa, plain = str(tmp_path / "contigs.fa"), str(tmp_path / "graph.gfa"), str(tmp_path / "plain.fa")
    share = dict(n_devices=n_devices, ranks_share_device=n_devices > 1)
    a, g = GpuGraph.assemble_gfa([path], InputFileType.Fastq, rc, thr, glen, fasta_file=fasta, gfa_file=gfa, **share)
    want = GpuGraph.assemble([path], InputFileType.Fastq, rc, thr, glen, output_file=plain, **share)
    assert a.n_contigs > 10 and a.contigs == want.contigs and a.stats == want.stats and a.read_bytes == want.read_bytes == g.read_bytes
    assert open(gfa, "rb").read() == g.text and len(g.text) == g.text_bytes + g.path_bytes
    assert open(fasta, "rb").read() == open(plain, "rb").read() == a.fasta
    check_host_result(a, g, k)
    again = str(tmp_path / "again.gfa")
    g.save_to_file(again)                          # katome_gfa_paths_save
    assert open(again, "rb").read() == g.text
    if n_devices == 1:
        bad = str(tmp_path / "no_such_dir" / "graph.gfa")
        with pytest.raises(KatomePanic) as e:      # the file cannot be made: E_OPEN, and both results are handed back all the same
            GpuGraph.assemble_gfa([path], InputFileType.Fastq, rc, thr, glen, gfa_file=bad)
        assert e.value.name == "E_OPEN" and "couldn't create %s: entity not found" % bad in e.value.message
        assert e.value.result[0].fasta == a.fasta and e.value.result[1].text == g.text
        with pytest.raises(KatomePanic) as e:
            GpuGraph.assemble_gfa([path], InputFileType.Fastq, rc, thr, glen, fasta_file=str(tmp_path / "no_such_dir" / "contigs.fa"), gfa_file=again)
        assert e.value.name == "E_OPEN" and "contigs.fa" in e.value.message and e.value.result[1].text == g.text
        assert open(again, "rb").read() == g.text


@pytest.mark.parametrize("n_devices", [1, 3])
def test_assemble_gfa_packed(oracle, tmp_path, n_devices):
    """the same through katome_assemble_gfa_packed on synthetic reads"""
    from katome_amd.build import GpuGraph
    k, rc, thr = 31, True, 2
    packed = synth(oracle)
    fasta, gfa, plain = str(tmp_path / "contigs.fa"), str(tmp_path / "graph.gfa"), str(tmp_path / "plain.fa")
    args = dict(reverse_complement=rc, minimal_weight_threshold=thr, original_genome_length=GLEN, k=k, n_devices=n_devices, ranks_share_device=n_devices > 1)
    a, g = GpuGraph.assemble_gfa_from_packed(packed, N_READS, READ_LEN, fasta_file=fasta, gfa_file=gfa, **args)
    want = GpuGraph.assemble_from_packed(packed, N_READS, READ_LEN, output_file=plain, **args)
    assert a.n_contigs > 10 and a.contigs == want.contigs and a.read_bytes == N_READS * READ_LEN
    assert open(gfa, "rb").read() == g.text
    assert open(fasta, "rb").read() == open(plain, "rb").read() == a.fasta
    check_host_result(a, g, k)
