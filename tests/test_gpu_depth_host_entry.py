"""katome_depth_paths (GpuGraph.depth): the graph built from read files as GpuGraph.create builds it, then every record of the query
files looked up, in file order and with nothing dropped -- per record against tests/depth_model.py on the graph create() returns."""
import ctypes as C

import pytest

import depth_model as dm
from helpers import revcomp_str

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

K = 21
N_READS, L, GENOME, ERR = 600, 80, 4000, 5e-3


@pytest.fixture(scope="module")
def files(oracle, tmp_path_factory):
    """a small FASTQ of synthetic reads; the query records as FASTA (one of them over several lines) and their FASTQ twin"""
    tmp = tmp_path_factory.mktemp("depth_files")
    rows = oracle.synth_reads(0, N_READS, L, GENOME, ERR, 0)
    reads = [bytes(r).decode() for r in rows]
    fq = tmp / "reads.fq"
    fq.write_text("".join("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)))
    records = [reads[0],                                                # written over several lines
               reads[3][:30] + "N" + reads[3][31:50] + "NN" + reads[3][52:],   # Ns: its other windows stay
               reads[4][:K - 1],                                        # shorter than k
               "",                                                      # empty
               revcomp_str(reads[5]),                                   # found on the other strand only (or by a reverse-complement build)
               reads[6][:K],                                            # exactly k
               reads[7].lower()[:40] + reads[7][40:]]                   # lower case is no base
    fa = tmp / "query.fa"
    fa.write_text("".join(">q%d some words\n%s" % (i, "".join(s[j:j + 37] + "\n" for j in range(0, len(s), 37))) for i, s in enumerate(records)))
    qfq = tmp / "query.fq"
    qfq.write_text("".join("@q%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(records)))
    return str(fq), str(fa), str(qfq), records


def _want(g, records, either):
    edges = dm.edge_dict(g.edge_key.tolist(), g.k, g.edge_weight.tolist())
    return dm.depth(edges, g.k, records, either)


def _check(d, want, hits):
    assert (d.n_records, d.n_windows, d.n_present, d.n_invalid, d.weight_sum, d.n_edges) == (
        want["n_seqs"], want["n_windows"], want["n_present"], want["n_invalid"], want["weight_sum"], want["n_edges"])
    for f in ("seq_present", "seq_invalid", "seq_sum", "seq_min", "seq_max"):
        assert getattr(d, f).tolist() == want[f], f
    if hits:
        assert d.edge_hits.tolist() == [want["edge_hits"].get(e, 0) for e in range(want["n_edges"])] and d.n_edges_hit == want["n_edges_hit"]
    else:
        assert d.edge_hits is None and d.n_edges_hit == 0


@pytest.mark.parametrize("rc,first_seen,stages,either", [(False, False, "", False), (False, False, "", True), (True, False, "", False),
                                                         (False, True, "", True), (True, True, "dw", False)])
@pytest.mark.parametrize("query", ["fasta", "fastq"])
def test_records_in_file_order_nothing_dropped(files, monkeypatch, query, rc, first_seen, stages, either):
    from katome_amd.build import GpuGraph, InputFileType, set_global_k_sizes
    fq, fa, qfq, records = files
    set_global_k_sizes(K)
    g, read_bytes = GpuGraph.create([fq], InputFileType.Fastq, rc, 2, first_seen_order=first_seen, stages=stages or None)
    want = _want(g, records, either)
    qfile, qft = (fa, InputFileType.Fasta) if query == "fasta" else (qfq, InputFileType.Fastq)
    d = GpuGraph.depth([fq], InputFileType.Fastq, rc, [qfile], qft, k=K, stages=stages, threshold=2, first_seen_order=first_seen, either_strand=either,
                       edge_hits=True)
    _check(d, want, True)
    assert d.read_bytes == read_bytes == N_READS * L and d.n_records == len(records)
    assert d.seq_present[2] == d.seq_present[3] == 0 and d.seq_invalid.tolist()[1] > 0 and d.seq_invalid.tolist()[6] == 40
    if not stages:
        assert d.seq_present[0] == len(records[0]) - K + 1 and d.seq_present[5] == 1
    # the same in batches of a few windows (a record at least per call): the arrays and the hits add up to the same
    monkeypatch.setenv("KATOME_DEPTH_BATCH_WINDOWS", "70")
    _check(GpuGraph.depth([fq], InputFileType.Fastq, rc, [qfile, qfile], qft, k=K, stages=stages, threshold=2, first_seen_order=first_seen,
                          either_strand=either, edge_hits=True), _want(g, records + records, either), True)
    monkeypatch.delenv("KATOME_DEPTH_BATCH_WINDOWS")
    _check(GpuGraph.depth([fq], InputFileType.Fastq, rc, [qfile], qft, k=K, stages=stages, threshold=2, first_seen_order=first_seen, either_strand=either),
           want, False)


def test_two_ranks_query_the_gathered_graph(files):
    from katome_amd.build import GpuGraph, InputFileType, set_global_k_sizes
    fq, fa, qfq, records = files
    set_global_k_sizes(K)
    g, _ = GpuGraph.create([fq], InputFileType.Fastq, True, 0, first_seen_order=True)
    d = GpuGraph.depth([fq], InputFileType.Fastq, True, [fa], InputFileType.Fasta, k=K, n_devices=2, ranks_share_device=True, edge_hits=True)
    _check(d, _want(g, records, False), True)


def test_refusals(files, tmp_path):
    from katome_amd import _lib
    from katome_amd.build import GpuGraph, InputFileType, KatomePanic, make_settings
    fq, fa, qfq, records = files

    def status(**kw):
        with pytest.raises(KatomePanic) as e:
            GpuGraph.depth([kw.pop("reads", fq)], InputFileType.Fastq, False, [kw.pop("q", fa)], kw.pop("qft", InputFileType.Fasta), k=K, **kw)
        return e.value.name, e.value.message
    name, msg = status(qft=InputFileType.BFCounter)
    assert name == "E_ARG" and "FASTA (0) or FASTQ (1)" in msg
    assert status(q=str(tmp_path / "missing.fa"))[0] == "E_PATH"              # the ingest's own status
    assert status(q=str(tmp_path))[0] == "E_IS_DIR"
    assert status(reads=str(tmp_path / "missing.fq"))[0] == "E_PATH"
    assert status(q=qfq)[0] == "E_PARSE"                                      # a FASTQ read as FASTA
    name, msg = status(stages="d", first_seen_order=False)
    assert name == "E_ARG" and "KATOME_FLAG_FIRST_SEEN_ORDER" in msg
    assert status(stages="x", first_seen_order=True)[0] == "E_ARG"
    L = _lib.lib()
    s = make_settings(K)
    paths = C.c_char_p * 1
    rp, qp, out = paths(fq.encode()), paths(fa.encode()), C.POINTER(_lib.Depth)()
    assert L.katome_depth_paths(C.byref(s), rp, 1, b"", 0, qp, 1, 0, 2, C.byref(out)) == -7 and "no per-window array" in _lib.last_error()     # WINDOWS
    assert L.katome_depth_paths(C.byref(s), rp, 1, b"", 0, qp, 1, 0, 8, C.byref(out)) == -7                                                     # an unknown bit
    assert L.katome_depth_paths(C.byref(s), rp, 1, b"", 0, qp, 1, 0, 0, None) == -7 and "null argument" in _lib.last_error()
    L.katome_depth_free(None)                                                                                                                    # (a no-op)
